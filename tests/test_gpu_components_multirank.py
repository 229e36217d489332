"""Block vectors on N ranks: N PROCESSES ON ONE GPU (the loopback build of tests/test_gpu_multirank_loopback.py: lagging transfers whose
receive buffers are poisoned with NaN until the message has landed) against tests/components_ref.py on the UNDIVIDED problem.  The worker
(tests/loopback/worker_components.py) goes through the Python mirror only, so the dispatch of PoissonOperator.vmult / SolverCG.solve on
PoissonOperator.distributed is what is tested, down to the exchange of the block vector between different ranks: first, middle and last rank,
ragged slabs, one message per neighbour and direction.

Both fixed-iteration references have their noise drift pinned below 1e-13 in tests/test_components_cpu.py (config 1 at every component
count; p = 4 (4,4,4) with the inverse diagonal), two decades under the 1e-11 they are compared to."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import components_ref as R
from test_components_cpu import diag_case
from test_gpu_multirank_loopback import ROOT, _rel, _run_ranks, _stop_tolerance

pytestmark = pytest.mark.gpu
pkg = bp5_pkg.load()
WORKER = os.path.join(ROOT, "tests", "loopback", "worker_components.py")
TOL_OP, TOL_CG = 1e-13, 1e-11
ITERS = 10
_cache = {}


def _config1(nc):
    """config 1 (p = 2, 8^3 cells, kappa = 1): problem, right-hand sides, operator result and the 10-iteration stacked solve; once per process"""
    if "pr" not in _cache:
        pr = O.Problem(2, (8, 8, 8), O.QUAD_GAUSS)
        _cache["pr"] = (pr, pr.rhs())
    pr, b = _cache["pr"]
    if nc not in _cache:
        B = R.rhs_blocks(b, nc)
        S = np.stack([O.deterministic_src(pr.mesh.n_dofs, seed=21 + c) for c in range(nc)])
        ref = dict(B=B, A=R.vmult(pr, S), cg=R.cg(pr.vmult, B, ITERS))
        for a in (ref["B"], ref["A"], ref["cg"][0]):
            a.setflags(write=False)
        _cache[nc] = ref
    return pr, _cache[nc]


def _union(tmp_path, world, n_dofs):
    ranks = [np.load(os.path.join(str(tmp_path), f"rank{r}.npz")) for r in range(world)]
    keys = [k for k in ranks[0].files if k[0] in "Ax"]
    full = {k: np.full((ranks[0][k].shape[0], n_dofs), np.nan) for k in keys}
    owner = np.full(n_dofs, -1)
    for r, z in enumerate(ranks):
        gid = z["gid"].astype(np.int64)
        assert (owner[gid] == -1).all()                                       # every DoF owned by exactly one rank
        owner[gid] = r
        for k in keys:
            full[k][:, gid] = z[k]
    assert (owner >= 0).all() and not any(np.isnan(v).any() for v in full.values())
    assert int(ranks[0]["n_ghost"]) == 0 and all(int(z["n_ghost"]) > 0 for z in ranks[1:])   # every rank but the first reads ghosts
    return ranks, full


def _one_rank_solve(mesh, coefficient, B, max_iter, tol, inv=None):
    """the same solve on ONE rank (the product library, this process): (iterations, residual)"""
    import torch
    op = pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, coefficient)
    b = op.initialize_block_vector(B.shape[0])
    b[:, :B.shape[1]] = torch.from_numpy(np.array(B)).cuda()        # (a copy: the cached references are read-only)
    x = op.initialize_block_vector(B.shape[0])
    ctl = pkg.SolverControl(max_iter, tol) if tol > 0.0 else pkg.IterationNumberControl(max_iter, 0.0)
    pkg.SolverCG(ctl).solve(op, x, b, pkg.DiagonalMatrix(torch.from_numpy(inv).cuda()) if inv is not None else pkg.DiagonalMatrix())
    out = ctl.last_step(), ctl.last_value()
    op.mf_data.close()
    return out


def _check_fixed_iterations(ranks, full, nc, overlaps, A_ref, cg_ref, one_rank_its, kernel):
    for mode in (0, 1, 2):
        errs = [_rel(full[f"A{mode}_{nc}"][c], A_ref[c]) for c in range(nc)]
        print(f"{nc} components, overlap {mode}: vmult, per component", " ".join(f"{e:.2e}" for e in errs))
        assert max(errs) < TOL_OP, (nc, mode, errs)
    xr, k, res = cg_ref
    for mode in overlaps:
        errs = [_rel(full[f"x{mode}_{nc}"][c], xr[c]) for c in range(nc)]
        print(f"{nc} components, overlap {mode}: {ITERS} iterations, per component", " ".join(f"{e:.2e}" for e in errs),
              f"residual {float(ranks[0][f'res{mode}_{nc}']):.10e} (numpy {res:.10e})")
        assert max(errs) < TOL_CG, (nc, mode, errs)
        its = [int(z[f"its{mode}_{nc}"]) for z in ranks]
        residuals = [float(z[f"res{mode}_{nc}"]) for z in ranks]
        assert its == [k] * len(ranks) and k == ITERS == one_rank_its                 # every rank, the oracle and the one-rank run
        assert residuals == [residuals[0]] * len(ranks)                                 # every rank sees the same all-reduced residual
        assert abs(residuals[0] - res) <= 1e-10 * res
        want = {0: 1, 1: 3, 2: 1}[mode]                                                 # (auto: slabs this small run unsplit)
        assert all(int(z[f"sched{mode}_{nc}"]) == want for z in ranks)
        assert all(str(z[f"kernel{mode}_{nc}"]).startswith(kernel) for z in ranks)


@pytest.mark.parametrize("world,delay_us", [(2, 400), (3, 250)])
def test_config1_on_ranks_matches_the_undivided_problem(tmp_path, world, delay_us):
    """p = 2, 8^3 cells, kappa = 1; 3 and 8 components in one run of the ranks; three ranks: ragged slabs (8 layers), a middle rank with two
    neighbours.  Two ranks: plus one solve that stops on a tolerance."""
    components = (3, 8)
    pr, ref3 = _config1(3)
    args = [2, 8, 8, 8, 0.0, pkg.COEF_ONE, ",".join(str(c) for c in components), ITERS, 0, "0,1"]
    stop = None
    if world == 2:
        # a tolerance half way (geometrically) between two consecutive record lows of the STACKED system's own residual history: rounding
        # cannot move the stopping iteration (the rule of _stop_tolerance, handed the stacked operator and right-hand side)
        B3 = ref3["B"]
        stacked = SimpleNamespace(vmult=R.stacked(pr.vmult, 3), rhs=lambda: B3.reshape(-1))
        k_stop, stop_tol = _stop_tolerance(stacked)
        stop = (k_stop, stop_tol)
        args.append(repr(stop_tol))
    _run_ranks(world, args, str(tmp_path), worker=WORKER, delay_us=delay_us)
    ranks, full = _union(tmp_path, world, pr.mesh.n_dofs)
    mesh1 = pkg.BrickMesh(2, (8, 8, 8))
    for nc in components:
        _, ref = _config1(nc)
        its1, _ = _one_rank_solve(mesh1, pkg.COEF_ONE, ref["B"], ITERS, 0.0)
        _check_fixed_iterations(ranks, full, nc, (0, 1), ref["A"], ref["cg"], its1, "apply_pencil_components_kernel<2,false,")
    if stop:
        k_stop, stop_tol = stop
        x_stop, k_ref, _ = R.cg(pr.vmult, ref3["B"], 400, tol=stop_tol)
        its1, res1 = _one_rank_solve(mesh1, pkg.COEF_ONE, ref3["B"], 400, stop_tol)
        assert k_ref == k_stop == its1 and res1 <= stop_tol
        for mode in (0, 1):
            its = [int(z[f"its_stop{mode}"]) for z in ranks]
            print(f"tolerance stop, overlap {mode}: iterations {its} (numpy {k_ref}, one rank {its1}), tolerance {stop_tol:.6e}")
            assert its == [k_ref] * world, (mode, its, k_ref)
            assert all(float(z[f"res_stop{mode}"]) <= stop_tol for z in ranks)
            assert len({float(z[f"res_stop{mode}"]) for z in ranks}) == 1
            assert max(_rel(full[f"x_stop{mode}"][c], x_stop[c]) for c in range(3)) < 1e-10       # (the bound of the scalar tolerance-stop test)


def test_preconditioned_p4_on_two_ranks_with_the_overlap_forced_on(tmp_path):
    """p = 4, (4,4,4), deformed, step-64 kappa, inverse diagonal assembled across the ranks, 3 components, three-phase schedule, lagging
    transfers: the workgroup-barrier family of the kernel behind the exchange"""
    nc = 3
    pr, B, inv = diag_case(nc)
    S = np.stack([O.deterministic_src(pr.mesh.n_dofs, seed=21 + c) for c in range(nc)])
    _run_ranks(2, [4, 4, 4, 4, 0.04, pkg.COEF_STEP64, str(nc), ITERS, 1, "1"], str(tmp_path), worker=WORKER, delay_us=300)
    ranks, full = _union(tmp_path, 2, pr.mesh.n_dofs)
    its1, _ = _one_rank_solve(pkg.BrickMesh(4, (4, 4, 4), deform_amp=0.04), pkg.COEF_STEP64, B, ITERS, 0.0, inv=inv)
    _check_fixed_iterations(ranks, full, nc, (1,), R.vmult(pr, S), R.cg(pr.vmult, B, ITERS, inv_diag=inv), its1, "apply_pencil_components_kernel<4,false,")
