"""The mass operator (BP5_OP_MASS) on 2 ranks as processes on ONE GPU (the loopback build of test_gpu_multirank_loopback.py, every transfer
lagging behind its stream, receive buffers poisoned with NaN), with the one-rank run beside them: the distributed application against the numpy
reference of tests/mass_ref.py on the undivided mesh, ten Jacobi-CG iterations with both solvers against numpy, and a tolerance stop whose count
and residual are the same on every rank and equal to the one-rank run's."""
import os

import numpy as np
import pytest

import bp5_oracle as O
import mass_ref as M
from test_gpu_multirank_loopback import ROOT, _rel, _run_ranks

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "loopback", "worker_mass.py")
ITERATIONS = 10


def _union(ranks, key, nd):
    full = np.full(nd, np.nan)
    for z in ranks:
        full[z["gid"].astype(np.int64)] = z[key]
    assert not np.isnan(full).any()
    return full


def _stop(A, b, inv, k_min=8, k_max=40):
    """the rule of _stop_tolerance (tests/test_gpu_multirank_loopback.py) with the inverse diagonal"""
    hist = []
    O.cg_plain(A, b, k_max, diag=inv, history=hist)
    res = [float(np.linalg.norm(b))] + hist
    for k in range(k_min, k_max + 1):
        low = min(res[:k])
        if res[k] < 0.92 * low:
            return k, float(np.sqrt(res[k] * low))
    raise AssertionError("no clear record low in the reference's residual history")


@pytest.mark.parametrize("world,p,cells,block,numbering,variant,overlap,delay_us", [
    (2, 4, (4, 4, 6), (0, 0, 0), 0, 0, 1, 250),   # lexicographic cells, mass pencil kernel, overlap forced on: the three-phase schedule of the atomic kernels
    (2, 2, (8, 8, 8), (4, 4, 4), 1, 56, 2, 400),  # bricks, the mass build of the block kernel; the automatic schedule (ghost rows combined first)
    (2, 2, (8, 8, 8), (4, 4, 4), 1, 56, 1, 400),  # ... boundary-first: the ghost-touching bricks run first, the exchange under the interior bricks
    (2, 2, (8, 8, 8), (4, 4, 4), 1, 56, 0, 0),    # ... unsplit
])
def test_mass_operator_across_ranks_matches_one_rank_and_numpy(tmp_path, world, p, cells, block, numbering, variant, overlap, delay_us):
    pr = M.Problem(p, cells, deform_amp=0.05, rho=O.kappa_step64)
    nd = pr.mesh.n_dofs
    b_ref, inv_ref = pr.rhs(), 1.0 / pr.diagonal()
    k_stop, stop_tol = _stop(pr.vmult, b_ref, inv_ref)
    runs = {}
    for w in (1, world):
        out = tmp_path / f"w{w}"
        out.mkdir()
        _run_ranks(w, [p, *cells, *block, numbering, variant, overlap, ITERATIONS, repr(stop_tol)], str(out), worker=WORKER, delay_us=delay_us if w > 1 else 0)
        runs[w] = [np.load(os.path.join(str(out), f"rank{r}.npz")) for r in range(w)]
    one, many = runs[1], runs[world]
    assert all(int(z["n_ghost"]) > 0 for z in many[1:])
    s = O.deterministic_src(nd, seed=47)
    for ranks in (one, many):
        assert _rel(_union(ranks, "vmult", nd), pr.vmult(s)) <= 1e-13
        assert _rel(_union(ranks, "inv_diag", nd), inv_ref) <= 1e-13
        assert _rel(_union(ranks, "b", nd), b_ref) <= 1e-13
    for name, solver in (("plain", O.cg_plain), ("merged", O.cg_merged)):
        x_ref, k, res = solver(pr.vmult, b_ref, ITERATIONS, diag=inv_ref)
        for ranks in (one, many):
            e = _rel(_union(ranks, f"x_{name}", nd), x_ref)
            print(f"world {len(ranks)} {name}: {e:.2e} kernel {str(ranks[0]['kernel_x_' + name])} schedule {int(ranks[0]['sched_x_' + name])}")
            assert e <= 1e-11 and all(int(z[f"its_x_{name}"]) == k for z in ranks)
        _, k_tol, _ = solver(pr.vmult, b_ref, 200, tol=stop_tol, diag=inv_ref)
        its = {int(z[f"its_xtol_{name}"]) for z in one + many}
        assert its == {k_tol} and (name != "plain" or k_tol == k_stop), (its, k_tol, k_stop)
        ref_res = float(one[0][f"res_xtol_{name}"])
        assert all(float(z[f"res_xtol_{name}"]) == float(many[0][f"res_xtol_{name}"]) for z in many)       # one all-reduced value on every rank
        assert abs(float(many[0][f"res_xtol_{name}"]) - ref_res) <= 1e-9 * ref_res
        x = _union(many, f"xtol_{name}", nd)
        assert np.linalg.norm(pr.vmult(x) - b_ref) <= stop_tol
        if variant == 56:   # the block kernel; the plain solver takes d.h from its write-out, the merged one only without a preconditioner vector
            assert all(str(z[f"kernel_x_{name}"]).startswith(f"apply_block_kernel<{p},false,") for z in one + many)
            assert all(int(z[f"fused_x_{name}"]) == (1 if name == "plain" else 0) for z in one + many)
        else:
            assert all(str(z[f"kernel_x_{name}"]).startswith("apply_pencil_mass_kernel<") and int(z[f"fused_x_{name}"]) == 0 for z in one + many)
