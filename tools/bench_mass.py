#!/usr/bin/env python3
"""The mass operator (BP5_OP_MASS, pkg.MassOperator) against the other ways to apply an operator on the same mesh, in ONE process with
alternating legs and HIP events (the method of tools/bench_components.py).

  (a) MassOperator.vmult, the library's default kernel for the handle
  (b) the same operator on the other of its two kernels                    -- (a) block kernel: the pencil kernel, on the same cells handed over
                                                                              without brick offsets; (a) pencil kernel: variant 56, left out
                                                                              where these bricks have no block plan
  (c) PoissonOperator.vmult on the same mesh, its default kernel
  (d) HelmholtzOperator.vmult with planes 0-5 zero-filled                   -- the only native mass apply before BP5_OP_MASS existed

usage: python tools/bench_mass.py                       # bench mesh p = 4; then config-4 sizes p = 1..8
       python tools/bench_mass.py --suite bench --cells 32 32 32 --rounds 3
Every application is a full vmult (zero-fill where the kernel needs one, cell kernel, combine pass where it has one, Dirichlet copy).  Reported per
leg: median (min - max) ms over the rounds, GDoF/s, and for leg (a) the achieved TB/s on its own byte model: 16 + 4r + 8r per DoF on the pencil
kernel, 16 + 2r + 8r on the packed block kernel (r = cell entries per DoF).  --json FILE appends one JSON line per mesh."""
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


def kernel_of(op, b):
    """the operator kernel a solve on this handle launches (fusion off: the kernel vmult runs)"""
    ctl = pkg.IterationNumberControl(1, 0.0)
    op.mf_data.set_cg_fusion(False)
    pkg.SolverCG(ctl).solve(op, op.initialize_dof_vector(), b, pkg.DiagonalMatrix())
    op.mf_data.set_cg_fusion(True)
    return ctl.apply_kernel


def run(p, cells):
    mesh = pkg.BrickMesh(p, cells, h=1.0 / cells[0], cell_block=BRICKS[p], dof_numbering=1, cell_block_order=1)
    n = mesh.n_owned
    n3 = (p + 1) ** 3
    r = mesh.n_cells * n3 / n
    ops = {"a mass": pkg.MassOperator(mesh, quad, pkg.COEF_STEP64)}
    default = ops["a mass"].mf_data.get_apply_variant()
    if default == 56:   # the pencil kernel: the same cells in the same order and numbering, handed over WITHOUT the brick offsets (variant 0 = the library's choice)
        plain = SimpleNamespace(**{k: v for k, v in vars(mesh).items() if k != "_h"})     # (views of the mesh's arrays; `mesh` outlives it)
        plain.cell_block_offsets = None
        other = pkg.MassOperator(plain, quad, pkg.COEF_STEP64)
        ops["b mass, other kernel"] = other
    else:               # the block kernel, where the plan of these bricks allows it
        other = pkg.MassOperator(mesh, quad, pkg.COEF_STEP64)
        try:
            other.mf_data.set_apply_variant(56)
            other.vmult(other.initialize_dof_vector(), other.initialize_dof_vector() + 1.0)
            ops["b mass, other kernel"] = other
        except pkg.BP5Error as e:
            print(f"  (leg b left out: {e})")
            other.mf_data.close()
    ops["c poisson"] = pkg.PoissonOperator(mesh, quad, pkg.COEF_STEP64)
    helm = pkg.HelmholtzOperator(mesh, quad, pkg.COEF_STEP64)
    helm.coef[:6 * mesh.n_cells * n3] = 0.0                                   # planes 0-5 (plane-major): the Laplace part switched off
    ops["d helmholtz, planes 0-5 zero"] = helm
    src, dst = ops["a mass"].initialize_dof_vector(), ops["a mass"].initialize_dof_vector()
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
    model = {name: 16 + (2 if "block" in kernels[name] else 4) * r + 8 * r for name in ops if "mass" in name}
    print(f"p={p} cells={list(cells)} bricks={BRICKS[p]} dofs={n} r={r:.4f} quad={a.quadrature}")
    out = dict(p=p, cells=list(cells), dofs=int(n), r=r, quadrature=a.quadrature, rounds=a.rounds, reps=a.reps, kernels=kernels, legs=[])
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
    m = {name: float(np.median(times[name])) for name in ops}
    print("  time ratios: " + "   ".join(f"a / {name[0]} = {m['a mass'] / m[name]:.3f}" for name in ops if name != "a mass") + "   (< 1: leg a is faster)")
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
