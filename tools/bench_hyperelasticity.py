#!/usr/bin/env python3
"""Neo-Hookean tangent and residual kernels (apply_pencil_hyperelasticity_kernel) beside the linear elasticity kernel
(apply_pencil_elasticity_kernel) at the same degree and size, in ONE process with alternating legs and HIP events (the method of
tools/bench_elasticity.py).

  (a) linear    ElasticityOperator.cell_loop over all cells              -- the kernel alone (accumulates), ten planes read
  (b) tangent   HyperelasticityOperator.cell_loop over all cells         -- the kernel alone (accumulates), ten geometry + ten state planes read
  (c) residual  HyperelasticityOperator.residual with do_zero_out=False  -- the kernel (ten planes read, ten written) + the three Dirichlet-zero launches

usage: python tools/bench_hyperelasticity.py                       # the config-4 sizes p = 1..8 (about 5e7 DoFs)
       python tools/bench_hyperelasticity.py --degrees 2 4 --cells 64 64 64 --rounds 5
Reported per leg: best and median (min - max) ms over the rounds, GDoF-components/s at the best time and the achieved TB/s on the leg's byte model
per DoF-component -- (a) 16 + 84 r / 3, (b) and (c) 16 + (4 + 160) r / 3, r = cell-local entries per DoF -- and b / a, c / a beside the ratio of the
models.  --json FILE appends one JSON line per mesh."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, nargs=3, default=None, help="override the mesh of every degree (quick runs)")
ap.add_argument("--degrees", type=int, nargs="+", default=list(range(1, 9)))
ap.add_argument("--quadrature", choices=["gauss", "gll"], default="gauss")
ap.add_argument("--lam", type=float, default=0.5769)
ap.add_argument("--mu", type=float, default=0.3846)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--json", default=None)
a = ap.parse_args()
quad = pkg.QUAD_GAUSS if a.quadrature == "gauss" else pkg.QUAD_GLL


def run(p, cells):
    mesh = pkg.BrickMesh(p, cells, h=1.0 / cells[0])
    op = pkg.HyperelasticityOperator(mesh, quad, pkg.COEF_STEP64, lam=a.lam, mu=a.mu)
    n = mesh.n_owned
    r = mesh.n_cells * (p + 1) ** 3 / n
    u, src, dst = op.initialize_block_vector(), op.initialize_block_vector(), op.initialize_block_vector()
    u[:, :n] = 0.01 / cells[0] * (torch.rand((3, n), dtype=torch.float64, device="cuda") - 0.5)      # |grad u| of a few percent: J > 0 everywhere
    src[:, :n] = torch.rand((3, n), dtype=torch.float64, device="cuda") - 0.5
    op.residual(dst, u)
    assert bool(torch.isfinite(op.state).all())
    op.do_zero_out = False
    m_lin, m_hyp = 16 + 84 * r / 3, 16 + 164 * r / 3
    legs = [("a linear", lambda: op.linear.cell_loop(src, dst), m_lin), ("b tangent", lambda: op.cell_loop(src, dst), m_hyp),
            ("c residual", lambda: op.residual(dst, u), m_hyp)]
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
    print(f"p={p} cells={list(cells)} dofs={n} r={r:.4f} quad={a.quadrature}  bytes/DoF-component: linear {m_lin:.1f}, tangent / residual {m_hyp:.1f}")
    out = dict(p=p, cells=list(cells), dofs=int(n), r=r, quadrature=a.quadrature, rounds=a.rounds, reps=a.reps, legs=[])
    best = {}
    for name, _, model in legs:
        t = np.array(times[name])
        best[name] = float(t.min())
        gdofc, tbs = 3 * n / best[name] / 1e6, model * 3 * n / best[name] / 1e9
        print(f"  ({name}) best {best[name]:.3f} ms, median {np.median(t):.3f} ({t.min():.3f} - {t.max():.3f}; {len(t)} rounds x {a.reps})  "
              f"-> {gdofc:.2f} GDoF-components/s  {tbs:.2f} TB/s on {model:.1f} B")
        out["legs"].append(dict(leg=name, best_ms=best[name], median_ms=float(np.median(t)), max_ms=float(t.max()), gdof_components_per_s=gdofc, model_bytes=model,
                                tb_per_s=tbs))
    out["tangent_over_linear"], out["residual_over_linear"] = best["b tangent"] / best["a linear"], best["c residual"] / best["a linear"]
    out["model_ratio"] = m_hyp / m_lin
    print(f"  tangent / linear = {out['tangent_over_linear']:.3f}   residual / linear = {out['residual_over_linear']:.3f}   byte-model ratio {out['model_ratio']:.3f}")
    if a.json:
        with open(a.json, "a") as f:
            f.write(json.dumps(out) + "\n")
    del op, u, src, dst
    torch.cuda.empty_cache()


for p in a.degrees:
    run(p, tuple(a.cells) if a.cells else (CONFIG_SIZES[p],) * 3)
