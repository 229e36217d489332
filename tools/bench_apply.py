#!/usr/bin/env python3
"""A/B timing of operator-kernel variants in ONE process, interleaved rounds (guide rule 24).
usage: python tools/bench_apply.py --degree 4 --cells 116 116 116 --variants 0 1 2 3 4 5
The timing-only ablation variants (wrong results by construction: 20+mask, 40+mask, 60+mask, 80-99, ...) exist only in the separate
library: `make -C deal-and-ceed-on-gpu_amd/csrc timing` and run with BP5_LIB=deal-and-ceed-on-gpu_amd/libbp5_timing.so."""
import argparse, os, sys, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bp5_pkg
pkg = bp5_pkg.load()

ap = argparse.ArgumentParser()
ap.add_argument("--degree", type=int, default=4)
ap.add_argument("--cells", type=int, nargs=3, default=[116, 116, 116])
ap.add_argument("--variants", type=int, nargs="+", default=[0])
ap.add_argument("--quadrature", default="gauss")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--deform", type=float, default=0.0)
ap.add_argument("--cell-block", type=int, nargs=3, default=[0, 0, 0])
ap.add_argument("--numbering", type=int, default=0)
ap.add_argument("--block-order", type=int, default=0, help="1: parity-class-major cell order inside a block")
ap.add_argument("--geometry", choices=["merged6", "affine"], default="merged6")
ap.add_argument("--overwrite", action="store_true", help="time vmult with zero_dst=1 instead of the accumulating cell loop")
ap.add_argument("--operator", choices=["poisson", "helmholtz"], default="poisson", help="helmholtz: step-64's operator on the native fused kernel (seven planes)")
ap.add_argument("--metric-precision", choices=["float64", "float32"], nargs="+", default=["float64"],
                help="float32: metric planes stored as floats (4 B per plane entry in the byte formula); both: one operator each on the same mesh, "
                     "timed alternately in every round (same-process A/B)")
a = ap.parse_args()
if "float32" in a.metric_precision and (a.operator == "helmholtz" or a.geometry == "affine"):
    ap.error("--metric-precision float32 needs --operator poisson and --geometry merged6 (the Helmholtz operator and the affine mode keep double planes)")
a.metric_precision = list(dict.fromkeys(a.metric_precision))
default_run = a.metric_precision == ["float64"]         # the single-precision invocation prints what it always printed
p = a.degree
mesh = pkg.BrickMesh(p, a.cells, h=1.0 / a.cells[0], deform_amp=a.deform, cell_block=a.cell_block, dof_numbering=a.numbering, cell_block_order=a.block_order)
quad = pkg.QUAD_GAUSS if a.quadrature == "gauss" else pkg.QUAD_GLL
ops = {prec: pkg.HelmholtzOperator(mesh, quad, pkg.COEF_STEP64) if a.operator == "helmholtz" else
       pkg.PoissonOperator(mesh, quad, pkg.COEF_STEP64, geometry=pkg.GEOM_AFFINE if a.geometry == 'affine' else pkg.GEOM_MERGED6, metric_precision=prec)
       for prec in a.metric_precision}
n = mesh.n_owned
r = mesh.n_cells * (p + 1) ** 3 / n
B_ops = {prec: 16 + 4 * r + ((56 if a.operator == 'helmholtz' else 24 if prec == 'float32' else 48) if a.geometry == 'merged6' else 8) * r for prec in ops}
src = torch.rand(n, dtype=torch.float64, device="cuda") - 0.5
dst = next(iter(ops.values())).mf_data.initialize_dof_vector()
legs = [(prec, v) for v in a.variants for prec in ops]
times = {leg: [] for leg in legs}
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
for rnd in range(a.rounds + 1):
    for prec, v in legs:
        op = ops[prec]
        mf = op.mf_data
        mf.set_apply_variant(v)
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(a.reps):
            if a.overwrite:
                op.vmult(dst, src)
            else:
                mf.cell_loop(op.coef, src, dst)
        ev[1].record()
        torch.cuda.synchronize()
        if rnd:
            times[(prec, v)].append(ev[0].elapsed_time(ev[1]) / a.reps)
if default_run:
    print(f"p={p} cells={a.cells} dofs={n} r={r:.4f} B_op={B_ops['float64']:.1f} B/DoF quad={a.quadrature}")
else:
    print(f"p={p} cells={a.cells} dofs={n} r={r:.4f} quad={a.quadrature} B_op " + " ".join(f"{prec}={B:.1f}" for prec, B in B_ops.items()) + " B/DoF (index streams counted as 4 r)")
for prec, v in legs:
    t = np.array(times[(prec, v)])
    med, B_op = np.median(t), B_ops[prec]
    if default_run:
        print(f"variant {v}: median {med:.3f} ms  min {t.min():.3f} ms  -> {n / med / 1e6:.2f} GDoF/s  {B_op * n / med / 1e6:.0f} GB/s alg ({B_op * n / med / 1e6 / 80:.1f}% of 8 TB/s)")
        continue
    mf = ops[prec].mf_data
    mf.set_apply_variant(v)
    print(f"variant {v} {prec} (runs {mf.get_apply_variant()}): median {med:.3f} ms  min {t.min():.3f} max {t.max():.3f} ms ({len(t)} rounds x {a.reps})  -> {n / med / 1e6:.2f} GDoF/s  {B_op * n / med / 1e6:.0f} GB/s alg ({B_op * n / med / 1e6 / 80:.1f}% of 8 TB/s)")
if len(ops) == 2:
    for v in a.variants:
        m64, m32 = (np.median(times[(prec, v)]) for prec in ("float64", "float32"))
        print(f"variant {v}: float32 / float64 = {m32 / m64:.3f}")
