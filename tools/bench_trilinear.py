#!/usr/bin/env python3
"""The trilinear geometry mode (BP5_GEOM_TRILINEAR: the metric from the cells' vertices inside the operator kernel) against the stored planes on the
same straight-sided mesh, in ONE process with alternating legs and HIP events (the method of tools/bench_overint.py).

  (a) GEOM_TRILINEAR                        apply_pencil_trilinear_kernel
  (b) GEOM_MERGED6, pencil kernel           apply_pencil_kernel in the degree's default shape -- the same cells, order and numbering as (a)
  (c) GEOM_MERGED6, the handle's default    on the brick mesh: the block kernel wherever these bricks have a plan
  (d) GEOM_AFFINE on the undeformed twin    the kernel family of (a) without any per-point geometry: one scalar plane, six numbers per cell

The mesh is the generator's sine mesh with every cell's nodes moved onto the trilinear image of its eight vertices.  Legs (a), (b), (d) get the cells
of the brick mesh handed over WITHOUT brick offsets, so that each of them is a pencil-family kernel with an atomic scatter; (c) is the project's best
kernel for the operator on that mesh.

usage: python tools/bench_trilinear.py                       # bench mesh p = 4; then config-4 sizes p = 1..8
       python tools/bench_trilinear.py --suite config4 --degrees 4 --cells 32 32 32 --rounds 3
Every application is a full vmult (zero-fill, cell kernel, combine pass where it has one, Dirichlet copy).  Reported per leg: median (min - max) ms
over the rounds, GDoF/s, and the achieved TB/s of (a) on 16 + 4 r + 192 n_cells / N bytes per DoF and of (b) on 16 + 52 r
(r = n_cells (p+1)^3 / N cell entries per DoF).  --json FILE appends one JSON line per mesh."""
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
AMP = 0.04

ap = argparse.ArgumentParser()
ap.add_argument("--suite", choices=["bench", "config4", "all"], default="all")
ap.add_argument("--cells", type=int, nargs=3, default=None, help="override the mesh of every leg (quick runs)")
ap.add_argument("--degrees", type=int, nargs="+", default=list(range(1, 9)), help="degrees of the config-4 suite")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--json", default=None)
a = ap.parse_args()


def trilinearise(mesh, chunk=1 << 15):
    """every cell's nodes onto the trilinear image of its eight vertices, in place (mesh.coords is a view of the mesh's own array)"""
    p, n = mesh.degree, mesh.n
    nodes = pkg.shape_tables(p, pkg.QUAD_GAUSS)[0]
    F = np.stack([1.0 - nodes, nodes], axis=-1)
    W = np.einsum("kc,jb,ia->kjicba", F, F, F).reshape(n ** 3, 8)                      # node i + n (j + n k) from vertex a + 2 b + 4 c
    corner = np.array([i * p + n * (j * p + n * k * p) for k in (0, 1) for j in (0, 1) for i in (0, 1)])
    V = np.array(mesh.coords[mesh.l2g[:, corner].astype(np.int64)])                    # before any node moves (a vertex is its own image)
    for c0 in range(0, mesh.n_cells, chunk):
        mesh.coords[mesh.l2g[c0:c0 + chunk].ravel()] = np.matmul(W, V[c0:c0 + chunk]).reshape(-1, 3)


def kernel_of(op, b):
    """the operator kernel a solve on this handle launches (fusion off: the kernel vmult runs)"""
    ctl = pkg.IterationNumberControl(1, 0.0)
    op.mf_data.set_cg_fusion(False)
    pkg.SolverCG(ctl).solve(op, op.initialize_dof_vector(), b, pkg.DiagonalMatrix())
    op.mf_data.set_cg_fusion(True)
    return ctl.apply_kernel


def without_bricks(mesh):
    plain = SimpleNamespace(**{k: v for k, v in vars(mesh).items() if k != "_h"})      # (views of the mesh's arrays; `mesh` outlives it)
    plain.cell_block_offsets = None
    return plain


def run(p, cells):
    brick = dict(h=1.0 / cells[0], cell_block=BRICKS[p], dof_numbering=1, cell_block_order=1)
    mesh = pkg.BrickMesh(p, cells, deform_amp=AMP, **brick)
    trilinearise(mesh)
    flat = pkg.BrickMesh(p, cells, **brick)
    n = mesh.n_owned
    r = mesh.n_cells * (p + 1) ** 3 / n
    ops = {"a trilinear": pkg.PoissonOperator(without_bricks(mesh), pkg.QUAD_GAUSS, pkg.COEF_STEP64, geometry=pkg.GEOM_TRILINEAR),
           "b merged6, pencil": pkg.PoissonOperator(without_bricks(mesh), pkg.QUAD_GAUSS, pkg.COEF_STEP64),
           "c merged6, default": pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_STEP64),
           "d affine, undeformed": pkg.PoissonOperator(without_bricks(flat), pkg.QUAD_GAUSS, pkg.COEF_STEP64, geometry=pkg.GEOM_AFFINE)}
    ops["b merged6, pencil"].mf_data.set_apply_variant(PENCIL_VARIANT.get(p, 0))
    src, dst = ops["a trilinear"].initialize_dof_vector(), ops["a trilinear"].initialize_dof_vector()
    src[:n] = torch.rand(n, dtype=torch.float64, device="cuda") - 0.5
    # the two modes compute one operator: checked at the size that is timed
    ref = ops["b merged6, pencil"].initialize_dof_vector()
    ops["b merged6, pencil"].vmult(ref, src)
    ops["a trilinear"].vmult(dst, src)
    parity = float(torch.linalg.norm(dst - ref) / torch.linalg.norm(ref))
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
    model = {"a trilinear": 16 + 4 * r + 192.0 * mesh.n_cells / n, "b merged6, pencil": 16 + 52 * r}
    print(f"p={p} cells={list(cells)} bricks={BRICKS[p]} dofs={n} r={r:.4f} |A_tri s - A_merged6 s| / |A_merged6 s| = {parity:.2e}")
    out = dict(p=p, cells=list(cells), dofs=int(n), r=r, parity=parity, rounds=a.rounds, reps=a.reps, kernels=kernels, legs=[])
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
    print(f"  time ratios: a / b = {m['a'] / m['b']:.3f}   a / c = {m['a'] / m['c']:.3f}   a / d = {m['a'] / m['d']:.3f}", flush=True)
    if a.json:
        with open(a.json, "a") as f:
            f.write(json.dumps(out) + "\n")
    for op in ops.values():
        op.mf_data.close()
    del ops, src, dst, ref
    torch.cuda.empty_cache()


if a.suite in ("bench", "all"):
    run(4, tuple(a.cells) if a.cells else (116, 116, 120))
if a.suite in ("config4", "all"):
    for p in a.degrees:
        run(p, tuple(a.cells) if a.cells else (CONFIG_SIZES[p],) * 3)
