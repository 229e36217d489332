"""Chebyshev preconditioner on the bench's p = 4 mesh (116 x 116 x 120 cells, 1.04e8 DoFs, cell bricks 4x4x4, block kernel, step-64 kappa):

  setup   time of PreconditionChebyshev.initialize (8-step CG-Lanczos estimate + allocation)
  vmult   time per Chebyshev vmult at degree 2 / 4 / 6 and of one operator application alone (HIP events), then 30 iterations of merged CG.
          The driver runs this leg under `rocprofv3 --kernel-trace --stats` (when rocprofv3 is on the PATH) and reads the kernel statistics of
          that one run: chebyshev_step_kernel per form and cgm_update_kernel per mode, with the achieved bandwidth on their algorithmic bytes
          (step: 24 / 48 / 40 B per DoF for the first / three-term / second step with a diagonal; update: 40 B in mode 1 -- p, r, v read, p, r
          written -- and 56 B in mode 2, x read and written as well)
  solve   iterations and time to solution (tolerance 1e-8 ||b||: 1e-10 is not reached at 1e8 DoFs in double precision) of Chebyshev(2/4/6)-PCG,
          Jacobi-PCG (SolverCG + diagonal) and Jacobi merged CG (SolverCGFullMerge + diagonal)

Driver (default): runs every leg in a fresh child process under `timeout -k 10 <limit>` and stops at the first leg that fails; one JSON
line per leg on stdout, all of them in <out>/bench_chebyshev.json.
  python tools/bench_chebyshev.py [--cells 116 116 120] [--legs vmult] [--out bench_out]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = {"setup": 150, "vmult": 240, "solve": 420}


def _problem(cells):
    import bp5_pkg
    pkg = bp5_pkg.load()
    mesh = pkg.BrickMesh(4, cells, h=1.0 / cells[0], cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1)
    op = pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_STEP64)
    inv = op.compute_diagonal(invert=True)
    return pkg, mesh, op, inv


def _timed(torch, fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def leg(name, cells):
    import torch
    pkg, mesh, op, inv = _problem(cells)
    Cheb = pkg.PreconditionChebyshev
    n = mesh.n_owned
    out = {"leg": name, "cells": list(cells), "n_dofs": int(mesh.n_global_dofs), "apply_kernel": op.mf_data.get_apply_variant()}
    data = lambda k: Cheb.AdditionalData(degree=k, smoothing_range=20.0, preconditioner=pkg.DiagonalMatrix(inv))
    if name == "setup":
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ch = Cheb().initialize(op, data(4))
            times.append((time.perf_counter() - t0) * 1e3)
        out.update(setup_ms=times, estimate=ch.estimated_eigenvalues())
    elif name == "vmult":
        b = op.assemble_rhs()
        dst = op.initialize_dof_vector()
        reps = 20
        out["apply_ms"] = _timed(torch, lambda: op.vmult(dst, b), reps)
        for k in (2, 4, 6):
            ch = Cheb().initialize(op, data(k))
            out[f"vmult_deg{k}_ms"] = _timed(torch, lambda: ch.vmult(dst, b), reps)
        ctl = pkg.IterationNumberControl(30, 0.0)
        x = op.initialize_dof_vector()
        pkg.SolverCGFullMerge(ctl).solve(op, x, b, pkg.DiagonalMatrix())
        out["merged_cg_ms_per_iteration"] = ctl.solve_ms / 30
    elif name == "solve":
        b = op.assemble_rhs()
        tol = 1e-8 * float(torch.linalg.norm(b[:n]))
        rows = {}
        for label, solver, P in [("jacobi_pcg", pkg.SolverCG, pkg.DiagonalMatrix(inv)), ("jacobi_merged_cg", pkg.SolverCGFullMerge, pkg.DiagonalMatrix(inv)),
                                 ("chebyshev2_pcg", pkg.SolverCG, 2), ("chebyshev4_pcg", pkg.SolverCG, 4), ("chebyshev6_pcg", pkg.SolverCG, 6)]:
            if isinstance(P, int):
                P = Cheb().initialize(op, data(P))
            ctl = pkg.IterationNumberControl(6000, tol)
            x = op.initialize_dof_vector()
            solver(ctl).solve(op, x, b, P)
            rows[label] = dict(iterations=ctl.last_step(), solve_ms=ctl.solve_ms, residual=ctl.last_value(), converged=ctl.last_value() <= tol)
        out["solves"] = rows
    return out


STEP_BYTES = {0: 24, 1: 48, 2: 40, 3: 40}    # chebyshev_step_kernel<FORM, diag = true, ...>: bytes per owned DoF
UPDATE_BYTES = {1: 40, 2: 56}                # cgm_update_kernel<MODE, ...>


def kernel_rows(stats_csv, n_dofs):
    """chebyshev_step_kernel and cgm_update_kernel rows of a rocprofv3 kernel_stats.csv: calls, average time, achieved TB/s"""
    import csv
    import re
    rows = {}
    for r in csv.DictReader(open(stats_csv)):
        name, avg = r["Name"], float(r["AverageNs"]) * 1e-9
        m = re.search(r"chebyshev_step_kernel<(\d), (true|false)", name)
        if m and m.group(2) == "true":
            nb = STEP_BYTES[int(m.group(1))]
            rows[f"chebyshev_step_kernel<{m.group(1)}>"] = dict(calls=int(r["Calls"]), avg_us=avg * 1e6, bytes_per_dof=nb, TBps=nb * n_dofs / avg / 1e12)
        m = re.search(r"cgm_update_kernel<(\d),", name)
        if m and int(m.group(1)) in UPDATE_BYTES:
            nb = UPDATE_BYTES[int(m.group(1))]
            rows[f"cgm_update_kernel<{m.group(1)}>"] = dict(calls=int(r["Calls"]), avg_us=avg * 1e6, bytes_per_dof=nb, TBps=nb * n_dofs / avg / 1e12)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=sorted(LEGS), help="run one leg in this process (the driver's child)")
    ap.add_argument("--cells", type=int, nargs=3, default=[116, 116, 120])
    ap.add_argument("--legs", nargs="+", choices=sorted(LEGS), default=list(LEGS), help="the driver's legs (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out"))
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(leg(args.leg, tuple(args.cells))), flush=True)
        return 0
    os.makedirs(args.out, exist_ok=True)
    results = []
    prof_dir = os.path.join(os.path.abspath(args.out), "bench_chebyshev_prof")
    for name, limit in ((k, v) for k, v in LEGS.items() if k in args.legs):
        leg_cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--cells"] + [str(c) for c in args.cells]
        profiled = name == "vmult" and shutil.which("rocprofv3") is not None
        if profiled:   # kernel statistics only: no counter collection, no other tracing
            leg_cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof_dir, "-o", "vmult", "--"] + leg_cmd
        p = subprocess.run(["timeout", "-k", "10", str(limit)] + leg_cmd, capture_output=True, text=True)
        line = next((l for l in reversed(p.stdout.splitlines()) if l.startswith("{")), None)
        if p.returncode != 0 or line is None:
            print(json.dumps({"leg": name, "exit": p.returncode, "tail": (p.stdout + p.stderr)[-2000:]}), flush=True)
            return p.returncode or 1
        row = json.loads(line)
        if profiled:
            stats = [os.path.join(d, f) for d, _, fs in os.walk(prof_dir) for f in fs if f.endswith("kernel_stats.csv")]
            row["kernel_stats"] = kernel_rows(stats[0], row["n_dofs"]) if stats else "no kernel_stats.csv written"
        print(json.dumps(row), flush=True)
        results.append(row)
        with open(os.path.join(args.out, "bench_chebyshev.json"), "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
