"""p-multigrid preconditioner (PreconditionMG: V-cycle, Chebyshev smoothers, Chebyshev coarse solver) on the bench's p = 4 mesh
(116 x 116 x 120 cells, 1.04e8 DoFs, cell bricks 4x4x4, block kernel, step-64 kappa); hierarchy p = 4, 2, 1 on the same cells:

  setup   time of make_mg_hierarchy + PreconditionMG (diagonals, CG-Lanczos estimates, transfers) and the per-level bounds
  cycle   time per V-cycle and per level (the V-cycle of the hierarchy from level l on, minus the one from level l + 1 on), one operator
          application per level, one prolongation and one restriction.  The driver runs this leg under `rocprofv3 --kernel-trace --stats`
          (when rocprofv3 is on the PATH) and reads the kernel statistics of the fine transfer (4 -> 2): mg_prolongate_kernel,
          mg_restrict_kernel (residual form) and mg_combine_kernel, with the achieved bandwidth on their algorithmic bytes (index streams
          included; bytes per fine DoF in the row)
  solve   iterations and time to solution (tolerance 1e-8 ||b||) of MG-PCG for coarse Chebyshev degrees 30 and 60 (default)

With --h-levels N | max (the hybrid hierarchy: the p-levels, then up to N geometric levels at degree 1 on 2:1 coarser meshes,
make_mg_hierarchy(h_levels=...)) the same legs run on that hierarchy, and
  setup   also reports each level's cells
  cycle   also times the first geometric transfer and reads mg_geo_prolongate_kernel / mg_geo_restrict_kernel from the kernel statistics
  solve   runs coarse degrees 10, 20, 30 and 60 on the hybrid hierarchy, and the p-only default (coarse degree 60) beside them
--metric-precision float32: the level operators keep their metric planes as floats (make_mg_hierarchy(metric_precision="float32")); the
outer CG of the solve leg runs on the FP64 fine operator; `apply_bytes_per_dof_p<k>` (cycle leg: the unfused application's algorithmic
bytes, 16 + 6 e r with e = 4 or 8 bytes per plane entry, index streams not counted) follows the precision.
--degree sets the fine degree (default 4), e.g. --degree 1 --cells 256 256 256 --h-levels max against --h-levels 0 (one level).

Driver (default): runs every leg in a fresh child process under `timeout -k 10 <limit>` and stops at the first leg that fails; one JSON
line per leg on stdout, all of them in <out>/bench_multigrid.json.
  python tools/bench_multigrid.py [--cells 116 116 120] [--degree 4] [--h-levels N|max] [--out bench_out]
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
LEGS = {"setup": 240, "cycle": 300, "solve": 420}


def _hierarchy(pkg, cells, degree=4, h_levels=None, metric_precision=None):
    """(outer operator, level operators): the same list unless metric_precision makes level 0 a float32 twin of the outer operator"""
    mesh = pkg.BrickMesh(degree, cells, h=1.0 / cells[0], cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1)
    op = pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_STEP64)
    kw = {} if h_levels is None else dict(h_levels=h_levels)
    if metric_precision is not None:
        kw["metric_precision"] = metric_precision
    ops = pkg.make_mg_hierarchy(op, **kw)
    for o in [op] + ops:
        o.mf_data.set_apply_variant(56)
    return op, ops


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


def transfer_bytes(nf, nc, n_cells, n_fine, n_coarse):
    """algorithmic bytes of one fine-level transfer (index streams included): prolongation, residual restriction, combine pass"""
    f3, c3, words = nf ** 3, nc ** 3, (nf ** 3 + 31) // 32
    return {"mg_prolongate_kernel": 16 * n_fine + n_cells * (4 * f3 + 4 * words + 4 * c3) + 8 * n_coarse,
            "mg_restrict_kernel": 24 * n_fine + n_cells * (4 * f3 + 8 * c3),
            "mg_combine_kernel": n_cells * 12 * c3 + 12 * n_coarse}


def geo_transfer_bytes(n, n_cells, n_fine, n_coarse):
    """the same for a geometric transfer at degree n - 1 (per fine cell: parent word, index stream, writer mask, slots; the parents' index
    lists counted once per coarse cell)"""
    n3, words = n ** 3, (n ** 3 + 31) // 32
    return {"mg_geo_prolongate_kernel": 16 * n_fine + n_cells * (4 + 4 * n3 + 4 * words) + (n_cells // 8) * 4 * n3 + 8 * n_coarse,
            "mg_geo_restrict_kernel": 24 * n_fine + n_cells * (4 + 4 * n3 + 8 * n3),
            "mg_combine_kernel": n_cells * 12 * n3 + 12 * n_coarse}


def leg(name, cells, degree=4, h_levels=None, metric_precision=None):
    import torch
    import bp5_pkg
    pkg = bp5_pkg.load()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outer, ops = _hierarchy(pkg, cells, degree, h_levels, metric_precision)
    fine = ops[0]
    n = fine.mf_data.n_owned
    out = {"leg": name, "cells": list(cells), "n_dofs": int(fine.mf_data.mesh.n_global_dofs), "degrees": [o.mf_data.mesh.degree for o in ops],
           "level_dofs": [int(o.mf_data.mesh.n_global_dofs) for o in ops]}
    if metric_precision is not None:
        out["metric_precision"] = metric_precision
    if h_levels is not None:
        out.update(h_levels=h_levels, level_cells=[list(o.mf_data.mesh.cells) for o in ops])
    if name == "setup":
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        mg = pkg.PreconditionMG(ops)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        out.update(hierarchy_ms=(t1 - t0) * 1e3, mg_setup_ms=(t2 - t1) * 1e3, levels=mg.level_info())
    elif name == "cycle":
        b = fine.assemble_rhs()
        mgs = [pkg.PreconditionMG(ops[l:]) for l in range(len(ops))]
        reps = 10
        cyc = []
        for l, mg in enumerate(mgs):
            src = ops[l].initialize_dof_vector()
            src[:ops[l].mf_data.n_owned] = 1.0
            ops[l].mf_data.set_constrained_values(0.0, src)
            dst = ops[l].initialize_dof_vector()
            cyc.append(_timed(torch, lambda: mg.vmult(dst, src), reps))
            out[f"apply_ms_p{ops[l].mf_data.mesh.degree}"] = _timed(torch, lambda: ops[l].vmult(dst, src), reps)
            ml = ops[l].mf_data.mesh
            out[f"apply_bytes_per_dof_p{ml.degree}"] = 16 + 6 * (4 if metric_precision == "float32" else 8) * ml.n_cells * (ml.degree + 1) ** 3 / ops[l].mf_data.n_owned
        out["v_cycle_ms"] = cyc[0]
        out["level_ms"] = [cyc[l] - (cyc[l + 1] if l + 1 < len(cyc) else 0.0) for l in range(len(cyc))]
        if len(ops) > 1 and not mgs[0].transfers[0].geometric:
            tr = mgs[0].transfers[0]
            nf_, nc_ = ops[0].mf_data.mesh.degree + 1, ops[1].mf_data.mesh.degree + 1
            xf, xc = fine.initialize_dof_vector(), ops[1].initialize_dof_vector()
            out["prolongate_ms"] = _timed(torch, lambda: tr.prolongate_and_add(xf, xc), reps)
            out["restrict_ms"] = _timed(torch, lambda: tr.restrict_and_add(xc, b), reps)
            out["transfer_bytes"] = transfer_bytes(nf_, nc_, fine.mf_data.mesh.n_cells, n, ops[1].mf_data.n_owned)
            out["transfer_pair"] = [nf_, nc_]
        geo = [l for l, t in enumerate(mgs[0].transfers) if t.geometric]
        if geo:   # the finest geometric transfer
            l = geo[0]
            tr, fo, co = mgs[0].transfers[l], ops[l], ops[l + 1]
            xf, xc, bf = fo.initialize_dof_vector(), co.initialize_dof_vector(), fo.initialize_dof_vector()
            bf[:fo.mf_data.n_owned] = 1.0
            out["geo_level"] = l
            out["geo_prolongate_ms"] = _timed(torch, lambda: tr.prolongate_and_add(xf, xc), reps)
            out["geo_restrict_ms"] = _timed(torch, lambda: tr.restrict_and_add(xc, bf), reps)
            out["geo_transfer_bytes"] = geo_transfer_bytes(fo.mf_data.mesh.degree + 1, fo.mf_data.mesh.n_cells, fo.mf_data.n_owned, co.mf_data.n_owned)
            out["geo_n_fine_dofs"] = int(fo.mf_data.mesh.n_global_dofs)
    elif name == "solve":
        b = fine.assemble_rhs()
        tol = 1e-8 * float(torch.linalg.norm(b[:n]))
        rows = {}
        runs = [("mg_pcg_coarse%d", c, ops) for c in ((30, 60) if h_levels is None else (10, 20, 30, 60))]
        if h_levels is not None:   # the p-only default beside the hybrid rows
            runs.append(("p_only_mg_pcg_coarse%d", 60, ops[:len(pkg.mg_coarse_degrees(degree))]))
        for key, cdeg, lops in runs:
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            mg = pkg.PreconditionMG(lops, pkg.PreconditionMG.AdditionalData(coarse_degree=cdeg))
            torch.cuda.synchronize()
            setup_ms = (time.perf_counter() - t1) * 1e3
            for rep in range(2):
                ctl = pkg.SolverControl(500, tol)
                x = fine.initialize_dof_vector()
                pkg.SolverCG(ctl).solve(outer, x, b, mg)
            rows[key % cdeg] = dict(n_levels=len(lops), iterations=ctl.last_step(), solve_ms=ctl.solve_ms, setup_ms=setup_ms, residual=ctl.last_value(),
                                                converged=ctl.last_value() <= tol, ms_per_iteration=ctl.solve_ms / max(ctl.last_step(), 1),
                                                solution_l2=outer.l2_norm_solution(x))
            mg.clear()
        out["solves"] = rows
    return out


def kernel_rows(stats_csv, legrow):
    """the fine transfer's kernels (mg_*<5, 3...>, combine on the p = 2 level) of a rocprofv3 kernel_stats.csv: calls, average time, TB/s;
    with h-levels also the geometric kernels (mg_geo_*: every level's launches averaged)"""
    import csv
    nbytes = legrow.get("transfer_bytes", {})
    n_f = legrow["n_dofs"]
    rows = {}
    for r in csv.DictReader(open(stats_csv)):
        name, avg = r["Name"], float(r["AverageNs"]) * 1e-9
        for k, nb in legrow.get("geo_transfer_bytes", {}).items():
            if k.startswith("mg_geo_") and k in name:
                key = name[name.index(k):].split("(")[0].replace(" ", "")
                rows[key] = dict(calls=int(r["Calls"]), avg_us=avg * 1e6, bytes_per_fine_dof_finest=nb / legrow["geo_n_fine_dofs"],
                                 note="every geometric level's launches averaged (no bandwidth: the levels differ in size); geo_*_ms time the finest")
        for k, nb in nbytes.items():
            fine_one = (f"<{legrow['transfer_pair'][0]}, {legrow['transfer_pair'][1]}" in name) if k != "mg_combine_kernel" else True
            if k in name and fine_one:
                key = k + ("<5,3,true>" if k == "mg_restrict_kernel" and "true" in name else "<5,3,false>" if k == "mg_restrict_kernel" else
                           "<5,3>" if k == "mg_prolongate_kernel" else ("<true>" if "true" in name else "<false>"))
                rows[key] = dict(calls=int(r["Calls"]), avg_us=avg * 1e6, bytes_per_fine_dof=nb / n_f, TBps=nb / avg / 1e12,
                                 note="combine rows: every level's launches averaged" if k == "mg_combine_kernel" else "")
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=sorted(LEGS), help="run one leg in this process (the driver's child)")
    ap.add_argument("--cells", type=int, nargs=3, default=[116, 116, 120])
    ap.add_argument("--degree", type=int, default=4)
    ap.add_argument("--h-levels", default=None, help="N or max: the hybrid hierarchy (default: the p-levels only, today's legs)")
    ap.add_argument("--metric-precision", choices=["float64", "float32"], default=None, help="float32: level operators with float metric planes under the FP64 outer CG")
    ap.add_argument("--legs", nargs="+", choices=sorted(LEGS), default=list(LEGS), help="the driver's legs (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out"))
    args = ap.parse_args()
    h_levels = None if args.h_levels is None else (args.h_levels if args.h_levels == "max" else int(args.h_levels))
    if args.leg:
        print(json.dumps(leg(args.leg, tuple(args.cells), args.degree, h_levels, args.metric_precision)), flush=True)
        return 0
    os.makedirs(args.out, exist_ok=True)
    results = []
    prof_dir = os.path.join(os.path.abspath(args.out), "bench_multigrid_prof")
    for name, limit in ((k, v) for k, v in LEGS.items() if k in args.legs):
        leg_cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--degree", str(args.degree), "--cells"] + [str(c) for c in args.cells]
        if h_levels is not None:
            leg_cmd += ["--h-levels", str(h_levels)]
        if args.metric_precision is not None:
            leg_cmd += ["--metric-precision", args.metric_precision]
        profiled = name == "cycle" and shutil.which("rocprofv3") is not None
        if profiled:   # kernel statistics only: no counter collection, no other tracing
            leg_cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof_dir, "-o", "cycle", "--"] + leg_cmd
        p = subprocess.run(["timeout", "-k", "10", str(limit)] + leg_cmd, capture_output=True, text=True)
        line = next((l for l in reversed(p.stdout.splitlines()) if l.startswith("{")), None)
        if p.returncode != 0 or line is None:
            print(json.dumps({"leg": name, "exit": p.returncode, "tail": (p.stdout + p.stderr)[-2000:]}), flush=True)
            return p.returncode or 1
        row = json.loads(line)
        if profiled:
            stats = [os.path.join(d, f) for d, _, fs in os.walk(prof_dir) for f in fs if f.endswith("kernel_stats.csv")]
            row["kernel_stats"] = kernel_rows(stats[0], row) if stats else "no kernel_stats.csv written"
        print(json.dumps(row), flush=True)
        results.append(row)
        tag = ("" if h_levels is None else f"_p{args.degree}_h{h_levels}") + ("" if args.metric_precision is None else f"_{args.metric_precision}")
        with open(os.path.join(args.out, f"bench_multigrid{tag}.json"), "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
