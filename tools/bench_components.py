#!/usr/bin/env python3
"""Block-vector operator (bp5_apply_components) against NC scalar applications on the same mesh, in ONE process with alternating legs and HIP
events (the method of tools/bench_apply.py).

  (a) one bp5_apply_components on NC components              -- ONE pass over the metric planes and local_to_global
  (b) NC calls of bp5_apply on the atomic pencil kernel      -- the same arithmetic and scatter, the metric read NC times
  (c) NC calls of bp5_apply on the handle's default kernel   -- the deterministic block kernel on the bench bricks

usage: python tools/bench_components.py                       # bench mesh p = 4, NC = 1, 2, 3; then config-4 sizes p = 1..8, NC = 3
       python tools/bench_components.py --suite bench --cells 32 32 32 --rounds 3
Every application is a full vmult (zero-fill, cell kernel, combine pass where the kernel has one, Dirichlet copy).  Reported per leg: median /
min / max ms over the rounds, GDoF-components/s, and the achieved TB/s on the byte model 16 + 52 r / NC per DoF-component of leg (a) (legs
(b), (c): NC = 1 in the model, they read the metric per call).  --json FILE appends one JSON line per mesh."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bp5_pkg

pkg = bp5_pkg.load()
CONFIG_SIZES = {1: 367, 2: 184, 3: 122, 4: 92, 5: 73, 6: 61, 7: 52, 8: 46}            # bench.py: BASELINE config 4, ~5e7 DoFs per degree
BRICKS = {1: (8, 8, 8), 2: (8, 8, 4), 3: (8, 4, 4), 4: (4, 4, 4), 5: (6, 4, 2), 6: (4, 4, 2), 7: (4, 2, 2), 8: (8, 8, 8)}   # bench.py: default_cell_block
PENCIL_VARIANT = {1: 1, 3: 1}      # apply variant of the degree's DEFAULT pencil shape on a handle without cell blocks (p = 1, 3: variant 0 is the team kernel there)

ap = argparse.ArgumentParser()
ap.add_argument("--suite", choices=["bench", "config4", "all"], default="all")
ap.add_argument("--cells", type=int, nargs=3, default=None, help="override the mesh of every leg (quick runs)")
ap.add_argument("--degrees", type=int, nargs="+", default=list(range(1, 9)), help="degrees of the config-4 suite")
ap.add_argument("--quadrature", choices=["gauss", "gll"], default="gauss")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--json", default=None)
a = ap.parse_args()
quad = pkg.QUAD_GAUSS if a.quadrature == "gauss" else pkg.QUAD_GLL


def run(p, cells, ncs):
    mesh = pkg.BrickMesh(p, cells, h=1.0 / cells[0], cell_block=BRICKS[p], dof_numbering=1, cell_block_order=1)
    op = pkg.PoissonOperator(mesh, quad, pkg.COEF_STEP64)
    # the same cells in the same order and the same numbering, handed over WITHOUT the brick offsets: the library's pencil kernel, same planes
    plain = SimpleNamespace(**{k: v for k, v in vars(mesh).items() if k != "_h"})     # (views of the mesh's arrays; `mesh` outlives it)
    plain.cell_block_offsets = None
    op_pencil = pkg.PoissonOperator(plain, quad, pkg.COEF_STEP64)
    op_pencil.coef = op.coef
    op_pencil.mf_data.set_apply_variant(PENCIL_VARIANT.get(p, 0))
    n = mesh.n_owned
    r = mesh.n_cells * (p + 1) ** 3 / n
    nc_max = max(ncs)
    src, dst = op.initialize_block_vector(nc_max), op.initialize_block_vector(nc_max)
    src[:, :n] = torch.rand((nc_max, n), dtype=torch.float64, device="cuda") - 0.5
    rows = [(src[c, :n + mesh.n_ghost], dst[c, :n + mesh.n_ghost]) for c in range(nc_max)]    # the blocks as scalar vectors (16-byte aligned: ld is even)

    def components(nc):
        op.vmult(dst[:nc], src[:nc])

    def scalar(o):
        def f(nc):
            for s, d in rows[:nc]:
                o.vmult(d, s)
        return f
    legs = [(name, nc, fn) for nc in ncs for name, fn in (("a components", components), ("b pencil x NC", scalar(op_pencil)), ("c default x NC", scalar(op)))]
    times = {(name, nc): [] for name, nc, _ in legs}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for rnd in range(a.rounds + 1):                      # round 0 warms up
        for name, nc, fn in legs:
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(a.reps):
                fn(nc)
            ev[1].record()
            torch.cuda.synchronize()
            if rnd:
                times[(name, nc)].append(ev[0].elapsed_time(ev[1]) / a.reps)
    kernels = {}
    for name, o, blockvec in (("a components", op, True), ("b pencil x NC", op_pencil, False), ("c default x NC", op, False)):
        ctl = pkg.IterationNumberControl(1, 0.0)
        if blockvec:
            pkg.SolverCG(ctl).solve(o, op.initialize_block_vector(1), src[:1].clone(), pkg.DiagonalMatrix())
        else:
            o.mf_data.set_cg_fusion(False)
            pkg.SolverCG(ctl).solve(o, o.initialize_dof_vector(), rows[0][0].clone(), pkg.DiagonalMatrix())
        kernels[name] = ctl.apply_kernel
    print(f"p={p} cells={list(cells)} bricks={BRICKS[p]} dofs={n} r={r:.4f} quad={a.quadrature}  bytes/DoF-component: scalar {16 + 52 * r:.1f}, "
          + ", ".join(f"NC={nc} {16 + 52 * r / nc:.1f}" for nc in ncs))
    out = dict(p=p, cells=list(cells), dofs=int(n), r=r, quadrature=a.quadrature, rounds=a.rounds, reps=a.reps, kernels=kernels, legs=[])
    for name, nc, _ in legs:
        t = np.array(times[(name, nc)])
        med = float(np.median(t))
        model = 16 + 52 * r / (nc if name.startswith("a") else 1)
        gdofc, tbs = n * nc / med / 1e6, model * n * nc / med / 1e9
        print(f"  NC={nc} ({name}) {kernels[name]}: median {med:.3f} ms  min {t.min():.3f} max {t.max():.3f} ({len(t)} rounds x {a.reps})  "
              f"-> {gdofc:.2f} GDoF-components/s  {tbs:.2f} TB/s on {model:.1f} B")
        out["legs"].append(dict(leg=name, nc=nc, median_ms=med, min_ms=float(t.min()), max_ms=float(t.max()), gdof_components_per_s=gdofc, model_bytes=model, tb_per_s=tbs))
    for nc in ncs:
        m = {name: np.median(times[(name, nc)]) for name, k, _ in legs if k == nc}
        print(f"  NC={nc}: a / b = {m['a components'] / m['b pencil x NC']:.3f}   a / c = {m['a components'] / m['c default x NC']:.3f}   (time ratios; < 1: the block-vector kernel is faster)")
    if a.json:
        with open(a.json, "a") as f:
            f.write(json.dumps(out) + "\n")
    del op, op_pencil, src, dst, rows
    torch.cuda.empty_cache()


if a.suite in ("bench", "all"):
    run(4, tuple(a.cells) if a.cells else (116, 116, 120), [1, 2, 3])
if a.suite in ("config4", "all"):
    for p in a.degrees:
        run(p, tuple(a.cells) if a.cells else (CONFIG_SIZES[p],) * 3, [3])
