#!/usr/bin/env python3
"""Linear elasticity operator (bp5_elasticity_apply) against the three-component block-vector Laplacian (bp5_apply_components, NC = 3) on the
same cells, in ONE process with alternating legs and HIP events (the method of tools/bench_components.py).

  (a) one bp5_elasticity_apply                     -- ten planes, the components coupled at the quadrature points
  (b) one bp5_apply_components with NC = 3         -- the same gathers and atomics, six planes, no coupling (CEED BP6)

usage: python tools/bench_elasticity.py                       # bench mesh p = 4; then the config-4 sizes p = 1..8
       python tools/bench_elasticity.py --suite bench --cells 32 32 32 --rounds 3
Every application is a full vmult (per-block zero-fill, ONE cell kernel, Dirichlet copy).  Reported per leg: median (min - max) ms over the
rounds, GDoF-components/s and the achieved TB/s on the leg's byte model per DoF-component -- (a) 16 + 84 r / 3, (b) 16 + 52 r / 3, r = cell-local
entries per DoF -- and a / b beside the ratio of the two models.  --json FILE appends one JSON line per mesh."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bp5_pkg

pkg = bp5_pkg.load()
CONFIG_SIZES = {1: 367, 2: 184, 3: 122, 4: 92, 5: 73, 6: 61, 7: 52, 8: 46}            # bench.py: BASELINE config 4, ~5e7 DoFs per degree
BRICKS = {1: (8, 8, 8), 2: (8, 8, 4), 3: (8, 4, 4), 4: (4, 4, 4), 5: (6, 4, 2), 6: (4, 4, 2), 7: (4, 2, 2), 8: (8, 8, 8)}   # bench.py: default_cell_block

ap = argparse.ArgumentParser()
ap.add_argument("--suite", choices=["bench", "config4", "all"], default="all")
ap.add_argument("--cells", type=int, nargs=3, default=None, help="override the mesh of every leg (quick runs)")
ap.add_argument("--degrees", type=int, nargs="+", default=list(range(1, 9)), help="degrees of the config-4 suite")
ap.add_argument("--quadrature", choices=["gauss", "gll"], default="gauss")
ap.add_argument("--lam", type=float, default=0.5769)
ap.add_argument("--mu", type=float, default=0.3846)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--json", default=None)
a = ap.parse_args()
quad = pkg.QUAD_GAUSS if a.quadrature == "gauss" else pkg.QUAD_GLL


def run(p, cells):
    mesh = pkg.BrickMesh(p, cells, h=1.0 / cells[0], cell_block=BRICKS[p], dof_numbering=1, cell_block_order=1)
    el = pkg.ElasticityOperator(mesh, quad, pkg.COEF_STEP64, lam=a.lam, mu=a.mu)
    po = pkg.PoissonOperator(mesh, quad, pkg.COEF_STEP64)
    n = mesh.n_owned
    r = mesh.n_cells * (p + 1) ** 3 / n
    src, dst = el.initialize_block_vector(), el.initialize_block_vector()
    src[:, :n] = torch.rand((3, n), dtype=torch.float64, device="cuda") - 0.5
    legs = [("a elasticity", lambda: el.vmult(dst, src), 16 + 84 * r / 3), ("b components NC=3", lambda: po.vmult(dst, src), 16 + 52 * r / 3)]
    times = {name: [] for name, _, _ in legs}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for rnd in range(a.rounds + 1):                      # round 0 warms up
        for name, fn, _ in legs:
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(a.reps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(ev[0].elapsed_time(ev[1]) / a.reps)
    kernels = {}
    for name, o in (("a elasticity", el), ("b components NC=3", po)):
        ctl = pkg.IterationNumberControl(1, 0.0)
        pkg.SolverCG(ctl).solve(o, el.initialize_block_vector(), src.clone(), pkg.DiagonalMatrix())
        kernels[name] = ctl.apply_kernel
    print(f"p={p} cells={list(cells)} dofs={n} r={r:.4f} quad={a.quadrature}  bytes/DoF-component: elasticity {16 + 84 * r / 3:.1f}, components {16 + 52 * r / 3:.1f}")
    out = dict(p=p, cells=list(cells), dofs=int(n), r=r, quadrature=a.quadrature, rounds=a.rounds, reps=a.reps, kernels=kernels, legs=[])
    med = {}
    for name, _, model in legs:
        t = np.array(times[name])
        med[name] = float(np.median(t))
        gdofc, tbs = 3 * n / med[name] / 1e6, model * 3 * n / med[name] / 1e9
        print(f"  ({name}) {kernels[name]}: median {med[name]:.3f} ms ({t.min():.3f} - {t.max():.3f}; {len(t)} rounds x {a.reps})  "
              f"-> {gdofc:.2f} GDoF-components/s  {tbs:.2f} TB/s on {model:.1f} B")
        out["legs"].append(dict(leg=name, median_ms=med[name], min_ms=float(t.min()), max_ms=float(t.max()), gdof_components_per_s=gdofc, model_bytes=model, tb_per_s=tbs))
    ratio, model_ratio = med["a elasticity"] / med["b components NC=3"], (16 + 84 * r / 3) / (16 + 52 * r / 3)
    print(f"  a / b = {ratio:.3f}   byte-model ratio {model_ratio:.3f}")
    out["a_over_b"], out["model_ratio"] = ratio, model_ratio
    if a.json:
        with open(a.json, "a") as f:
            f.write(json.dumps(out) + "\n")
    del el, po, src, dst
    torch.cuda.empty_cache()


if a.suite in ("bench", "all"):
    run(4, tuple(a.cells) if a.cells else (116, 116, 120))
if a.suite in ("config4", "all"):
    for p in a.degrees:
        run(p, tuple(a.cells) if a.cells else (CONFIG_SIZES[p],) * 3)
