"""The Gauss(p+2) operators (BP5_QUAD_GAUSS_OVER) on 2 ranks as processes on ONE GPU (the loopback build of test_gpu_multirank_loopback.py, every
transfer lagging behind its stream, receive buffers poisoned with NaN), with the one-rank run beside them: one distributed application in each
overlap mode against the numpy reference of tests/overint_ref.py on the undivided mesh, and ten Jacobi-CG iterations with both solvers whose count
and residual are the same on both ranks and equal to the one-rank run's.  No new exchange code: the schedules are the atomic kernels'."""
import os

import numpy as np
import pytest

import bp5_oracle as O
import overint_ref as R
from test_gpu_multirank_loopback import ROOT, _rel, _run_ranks

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "loopback", "worker_overint.py")
ITERATIONS = 10


def _union(ranks, key, nd):
    full = np.full(nd, np.nan)
    for z in ranks:
        full[z["gid"].astype(np.int64)] = z[key]
    assert not np.isnan(full).any()
    return full


@pytest.mark.parametrize("p,cells,kernel", [(2, (4, 4, 6), "apply_pencil_q_kernel<2,1,16,4,true>"), (4, (3, 3, 4), "apply_pencil_q_kernel<4,4,36,1,true>")])
def test_over_integrated_operators_across_ranks_match_one_rank_and_numpy(tmp_path, p, cells, kernel):
    world = 2
    pr = R.Problem(p, cells, deform_amp=0.05, kappa=O.kappa_step64)
    prm = R.Problem(p, cells, deform_amp=0.05, kappa=O.kappa_step64, mass=True, mesh=pr.mesh)
    nd = pr.mesh.n_dofs
    b_ref, inv_ref = pr.rhs(), 1.0 / pr.diagonal()
    runs = {}
    for w in (1, world):
        out = tmp_path / f"w{w}"
        out.mkdir()
        _run_ranks(w, [p, *cells, ITERATIONS], str(out), worker=WORKER, delay_us=300 if w > 1 else 0)
        runs[w] = [np.load(os.path.join(str(out), f"rank{r}.npz")) for r in range(w)]
    one, many = runs[1], runs[world]
    assert all(int(z["n_ghost"]) > 0 for z in many[1:])
    s = O.deterministic_src(nd, seed=47)
    want, want_mass = pr.vmult(s), prm.vmult(s)
    for ranks in (one, many):
        for overlap in (0, 1, 2):
            e = _rel(_union(ranks, f"vmult_{overlap}", nd), want)
            print(f"p={p} world {len(ranks)} overlap {overlap}: {e:.2e}")
            assert e <= 1e-13
        assert _rel(_union(ranks, "mass_vmult", nd), want_mass) <= 1e-13
        assert _rel(_union(ranks, "inv_diag", nd), inv_ref) <= 1e-13
        assert _rel(_union(ranks, "b", nd), b_ref) <= 1e-13
    for name, solver in (("plain", O.cg_plain), ("merged", O.cg_merged)):
        x_ref, k, res = solver(pr.vmult, b_ref, ITERATIONS, diag=inv_ref)
        for ranks in (one, many):
            e = _rel(_union(ranks, f"x_{name}", nd), x_ref)
            print(f"p={p} world {len(ranks)} {name}: {e:.2e} kernel {str(ranks[0]['kernel_' + name])} schedule {int(ranks[0]['sched_' + name])}")
            assert e <= 1e-11 and all(int(z[f"its_{name}"]) == k == ITERATIONS for z in ranks)
            assert all(str(z[f"kernel_{name}"]) == kernel and int(z[f"fused_{name}"]) == 0 for z in ranks)
        assert all(float(z[f"res_{name}"]) == float(many[0][f"res_{name}"]) for z in many)               # one all-reduced value on every rank
        ref_res = float(one[0][f"res_{name}"])
        assert abs(float(many[0][f"res_{name}"]) - ref_res) <= 1e-9 * ref_res and abs(ref_res - res) <= 1e-9 * res
        assert all(int(z[f"sched_{name}"]) == 3 for z in many) and int(one[0][f"sched_{name}"]) == 0       # overlap on: the three-phase schedule
