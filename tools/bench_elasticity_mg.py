#!/usr/bin/env python3
"""Elasticity solves: Jacobi-PCG against V-cycle-PCG (ElasticityPreconditionMG) to 1e-8 ||b||, in ONE process with alternating legs and HIP events
(bp5_cg_result.solve_ms), and the block Chebyshev step kernel against the scalar one.

  solves      per mesh: iterations and solve time of (a) SolverCG + the block inverse diagonal, (b) SolverCG + one V-cycle per iteration over
              make_elasticity_mg_hierarchy(op, h_levels="max"); and the ms of one preconditioner application by level: the V-cycle that starts
              at level l (torch events around --reps applications) minus the one that starts at level l + 1
  step kernel chebyshev_step_kernel on three blocks in one launch (gridDim.y = 3) against the same kernel on a scalar vector (gridDim.y = 1) of about
              the same total length: a degree-1 polynomial with given bounds is ONE launch of the step kernel (x = D^-1 src / theta: 24 bytes per entry) and
              no operator application; alternating legs, GB/s of each and their ratio

usage: python tools/bench_elasticity_mg.py                    # p = 4 on 16^3 and 32^3, p = 2 on 32^3 and 64^3 (8e5 ... 6.4e6 three-component DoFs)
       python tools/bench_elasticity_mg.py --meshes 4:8 --rounds 2     # quick run
--json FILE appends one JSON line per mesh and one for the step kernel."""
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
ap = argparse.ArgumentParser()
ap.add_argument("--meshes", nargs="+", default=["4:16", "4:32", "2:32", "2:64"], help="degree:cells per direction")
ap.add_argument("--lam", type=float, default=0.5769)
ap.add_argument("--mu", type=float, default=0.3846)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--step-cells", type=int, default=64, help="cells per direction of the p = 2 mesh of the step-kernel comparison")
ap.add_argument("--json", default=None)
a = ap.parse_args()


def emit(rec):
    if a.json:
        with open(a.json, "a") as f:
            f.write(json.dumps(rec) + "\n")


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def solves(p, nc):
    cells = (nc, nc, nc)
    op = pkg.ElasticityOperator(pkg.BrickMesh(p, cells, h=1.0 / nc), pkg.QUAD_GAUSS, pkg.COEF_STEP64, lam=a.lam, mu=a.mu)
    n = op.mf_data.n_local
    ops = pkg.make_elasticity_mg_hierarchy(op, h_levels="max")
    mg = pkg.ElasticityPreconditionMG(ops)
    inv = op.compute_diagonal(invert=True)
    b, x = op.initialize_block_vector(), op.initialize_block_vector()
    base = op.assemble_rhs()[:n]
    i = torch.arange(n, dtype=torch.float64, device=base.device)
    b[0, :n], b[1, :n], b[2, :n] = base * (0.3 * torch.sin(0.37 * i)), base * (0.2 * torch.cos(0.11 * i)), -base
    tol = 1e-8 * float(b[:, :n].norm())
    legs = [("jacobi", pkg.DiagonalMatrix(inv)), ("v-cycle", mg)]
    ms, its = {k: [] for k, _ in legs}, {}
    for rnd in range(a.rounds + 1):                      # round 0 warms up
        for name, pre in legs:
            ctl = pkg.SolverControl(20000, tol)
            # the diagonal solve enqueues every iteration up to max_steps unless the host looks at the stop flag: every 10 iterations here;
            # a solve with a callback preconditioner looks by itself (two iterations behind)
            pkg.SolverCG(ctl, check_every=10 if name == "jacobi" else 0).solve(op, x, b, pre)
            its[name] = ctl.last_step()
            if rnd:
                ms[name].append(ctl.solve_ms)
    print(f"p={p} cells={list(cells)} three-component dofs={3 * int(op.mf_data.mesh.n_global_dofs)} levels={[(o.mf_data.mesh.degree, tuple(o.mf_data.mesh.cells)) for o in ops]}")
    rec = dict(p=p, cells=list(cells), dofs3=3 * int(op.mf_data.mesh.n_global_dofs), rounds=a.rounds, legs=[], levels=[])
    for name, _ in legs:
        t = np.array(ms[name])
        print(f"  ({name}) {its[name]} iterations, solve median {np.median(t):.3f} ms ({t.min():.3f} - {t.max():.3f}), {np.median(t) / max(its[name], 1):.4f} ms per iteration")
        rec["legs"].append(dict(leg=name, iterations=its[name], median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max())))
    print(f"  jacobi / v-cycle: iterations {its['jacobi'] / max(its['v-cycle'], 1):.1f}, time {np.median(ms['jacobi']) / np.median(ms['v-cycle']):.2f}"
          f"  (jacobi's time holds up to 9 iterations past its stop: at most {100.0 * 9 / max(its['jacobi'], 1):.1f} % too long)")
    # one preconditioner application by level: the cycle from level l minus the cycle from level l + 1
    info = mg.level_info()
    below = []
    for l in range(len(ops)):
        sub = mg if l == 0 else pkg.ElasticityPreconditionMG(ops[l:])
        s, d = ops[l].initialize_block_vector(), ops[l].initialize_block_vector()
        s[:, :ops[l].mf_data.n_local] = 1.0
        sub.vmult(d, s)
        below.append(min(timed(lambda: sub.vmult(d, s), a.reps) for _ in range(a.rounds)))
        if l:
            sub.clear()
    for l, o in enumerate(ops):
        own = below[l] - (below[l + 1] if l + 1 < len(ops) else 0.0)
        print(f"  level {l}: degree {info[l]['degree']} cells {info[l]['cells']} dofs3 {3 * info[l]['n_owned']}  cycle from here {below[l]:.3f} ms, this level {own:.3f} ms")
        rec["levels"].append(dict(level=l, degree=info[l]["degree"], cells=info[l]["cells"], dofs3=3 * info[l]["n_owned"], cycle_ms=below[l], level_ms=own))
    emit(rec)
    mg.clear()


def step_kernel():
    nc = a.step_cells
    el = pkg.ElasticityOperator(pkg.BrickMesh(2, (nc, nc, nc), h=1.0 / nc), pkg.QUAD_GAUSS, pkg.COEF_ONE, lam=a.lam, mu=a.mu)
    n = el.mf_data.n_local
    side = round((3 * n) ** (1.0 / 3.0)) - 1
    po = pkg.PoissonOperator(pkg.BrickMesh(1, (side, side, side), h=1.0 / side), pkg.QUAD_GAUSS, pkg.COEF_ONE)
    ns = po.mf_data.n_local
    dg_b, dg_s = el.initialize_block_vector(), po.initialize_dof_vector()
    dg_b.fill_(0.5)
    dg_s.fill_(0.5)
    data = lambda d: pkg.PreconditionChebyshev.AdditionalData(degree=1, max_eigenvalue=2.0, min_eigenvalue=0.1, preconditioner=pkg.DiagonalMatrix(d))
    cb = pkg.ElasticityPreconditionChebyshev().initialize(el, data(dg_b))
    cs = pkg.PreconditionChebyshev().initialize(po, data(dg_s))
    sb, db = el.initialize_block_vector(), el.initialize_block_vector()
    ss, ds = po.initialize_dof_vector(), po.initialize_dof_vector()
    legs = [("block (3 x %d)" % n, lambda: cb.vmult(db, sb), 24.0 * 3 * n), ("scalar (%d)" % ns, lambda: cs.vmult(ds, ss), 24.0 * ns)]
    gbs = {k: [] for k, _, _ in legs}
    for rnd in range(a.rounds + 3):
        for name, fn, nbytes in legs:
            t = timed(fn, 20)
            if rnd:
                gbs[name].append(nbytes / t / 1e6)
    print("Chebyshev step kernel, FORM 0 with a diagonal (24 B per entry), 20 launches per sample:")
    rec = dict(step_kernel=True, legs=[])
    med = []
    for name, _, _ in legs:
        g = np.array(gbs[name])
        med.append(float(np.median(g)))
        print(f"  {name}: median {np.median(g):.0f} GB/s ({g.min():.0f} - {g.max():.0f}; {len(g)} samples)")
        rec["legs"].append(dict(leg=name, median_gbs=float(np.median(g)), min_gbs=float(g.min()), max_gbs=float(g.max())))
    print(f"  block / scalar bytes per second: {med[0] / med[1]:.3f}")
    rec["block_over_scalar"] = med[0] / med[1]
    emit(rec)


for spec in a.meshes:
    p, nc = (int(v) for v in spec.split(":"))
    solves(p, nc)
step_kernel()
