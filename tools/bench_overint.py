#!/usr/bin/env python3
"""Gauss(p+2) quadrature (BP5_QUAD_GAUSS_OVER: CEED BP3 and BP1 as CEED defines them) against the p + 1 operators on the same mesh, in ONE process
with alternating legs and HIP events (the method of tools/bench_mass.py).

  (a) PoissonOperator, Gauss(p+2)           apply_pencil_q_kernel
  (b) PoissonOperator, Gauss(p+1)           apply_pencil_kernel in the degree's default shape -- the same cells, order and numbering as (a)
  (c) PoissonOperator, Gauss(p+1)           the handle's default kernel on the brick mesh: the block kernel wherever these bricks have a plan
  (d) MassOperator, Gauss(p+2)              apply_pencil_mass_q_kernel
  (e) MassOperator, Gauss(p+1)              apply_pencil_mass_kernel

Legs (a), (b), (d), (e) get the cells of the brick mesh handed over WITHOUT brick offsets, so that each of them is a pencil kernel with an atomic
scatter; (c) is the project's best kernel for the BP5-class operator on that mesh.

usage: python tools/bench_overint.py                       # bench mesh p = 4; then config-4 sizes p = 1..8
       python tools/bench_overint.py --suite bench --cells 32 32 32 --rounds 3
Every application is a full vmult (zero-fill, cell kernel, combine pass where it has one, Dirichlet copy).  Reported per leg: median (min - max) ms
over the rounds, GDoF/s, and for (a) and (d) the achieved TB/s on their byte models 16 + 4r + 48 r_Q and 16 + 4r + 8 r_Q per DoF
(r = n_cells (p+1)^3 / N cell entries per DoF, r_Q = n_cells (p+2)^3 / N quadrature points per DoF).  --json FILE appends one JSON line per mesh."""
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
PENCIL_VARIANT = {1: 1, 3: 1}        # p = 1, 3 without cell blocks default to the x-row team kernel: variant 1 is apply_pencil_kernel in the default shape there

ap = argparse.ArgumentParser()
ap.add_argument("--suite", choices=["bench", "config4", "all"], default="all")
ap.add_argument("--cells", type=int, nargs=3, default=None, help="override the mesh of every leg (quick runs)")
ap.add_argument("--degrees", type=int, nargs="+", default=list(range(1, 9)), help="degrees of the config-4 suite")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--json", default=None)
a = ap.parse_args()


def kernel_of(op, b):
    """the operator kernel a solve on this handle launches (fusion off: the kernel vmult runs)"""
    ctl = pkg.IterationNumberControl(1, 0.0)
    op.mf_data.set_cg_fusion(False)
    pkg.SolverCG(ctl).solve(op, op.initialize_dof_vector(), b, pkg.DiagonalMatrix())
    op.mf_data.set_cg_fusion(True)
    return ctl.apply_kernel


def run(p, cells):
    mesh = pkg.BrickMesh(p, cells, h=1.0 / cells[0], cell_block=BRICKS[p], dof_numbering=1, cell_block_order=1)
    plain = SimpleNamespace(**{k: v for k, v in vars(mesh).items() if k != "_h"})         # (views of the mesh's arrays; `mesh` outlives it)
    plain.cell_block_offsets = None
    n = mesh.n_owned
    r, rq = mesh.n_cells * (p + 1) ** 3 / n, mesh.n_cells * (p + 2) ** 3 / n
    ops = {"a poisson p+2": pkg.PoissonOperator(plain, pkg.QUAD_GAUSS_OVER, pkg.COEF_STEP64),
           "b poisson p+1, pencil": pkg.PoissonOperator(plain, pkg.QUAD_GAUSS, pkg.COEF_STEP64),
           "c poisson p+1, default": pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_STEP64),
           "d mass p+2": pkg.MassOperator(plain, pkg.QUAD_GAUSS_OVER, pkg.COEF_STEP64),
           "e mass p+1, pencil": pkg.MassOperator(plain, pkg.QUAD_GAUSS, pkg.COEF_STEP64)}
    ops["b poisson p+1, pencil"].mf_data.set_apply_variant(PENCIL_VARIANT.get(p, 0))
    src, dst = ops["a poisson p+2"].initialize_dof_vector(), ops["a poisson p+2"].initialize_dof_vector()
    src[:n] = torch.rand(n, dtype=torch.float64, device="cuda") - 0.5
    times = {name: [] for name in ops}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for rnd in range(a.rounds + 1):                      # round 0 warms up
        for name, op in ops.items():
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(a.reps):
                op.vmult(dst, src)
            ev[1].record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(ev[0].elapsed_time(ev[1]) / a.reps)
    kernels = {name: kernel_of(op, src.clone()) for name, op in ops.items()}
    model = {"a poisson p+2": 16 + 4 * r + 48 * rq, "d mass p+2": 16 + 4 * r + 8 * rq}
    print(f"p={p} cells={list(cells)} bricks={BRICKS[p]} dofs={n} r={r:.4f} r_Q={rq:.4f} (Q/n)^3={(p + 2) ** 3 / (p + 1) ** 3:.3f}")
    out = dict(p=p, cells=list(cells), dofs=int(n), r=r, r_q=rq, rounds=a.rounds, reps=a.reps, kernels=kernels, legs=[])
    for name in ops:
        t = np.array(times[name])
        med = float(np.median(t))
        gdof = n / med / 1e6
        line = f"  ({name}) {kernels[name]}: median {med:.3f} ms ({t.min():.3f} - {t.max():.3f}; {len(t)} rounds x {a.reps})  -> {gdof:.2f} GDoF/s"
        leg = dict(leg=name, median_ms=med, min_ms=float(t.min()), max_ms=float(t.max()), gdof_per_s=gdof)
        if name in model:
            leg.update(model_bytes=model[name], tb_per_s=model[name] * n / med / 1e9)
            line += f"  {leg['tb_per_s']:.2f} TB/s on {model[name]:.1f} B/DoF"
        print(line)
        out["legs"].append(leg)
    m = {name[0]: float(np.median(times[name])) for name in ops}
    print(f"  time ratios: a / b = {m['a'] / m['b']:.3f}   a / c = {m['a'] / m['c']:.3f}   d / e = {m['d'] / m['e']:.3f}   d / a = {m['d'] / m['a']:.3f}", flush=True)
    if a.json:
        with open(a.json, "a") as f:
            f.write(json.dumps(out) + "\n")
    for op in ops.values():
        op.mf_data.close()
    del ops, src, dst
    torch.cuda.empty_cache()


if a.suite in ("bench", "all"):
    run(4, tuple(a.cells) if a.cells else (116, 116, 120))
if a.suite in ("config4", "all"):
    for p in a.degrees:
        run(p, tuple(a.cells) if a.cells else (CONFIG_SIZES[p],) * 3)
