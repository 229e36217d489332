"""PreconditionChebyshev and the preconditioned CG on 1, 2 and 3 ranks as processes on ONE GPU (the loopback build of
test_gpu_multirank_loopback.py, every transfer lagging behind its stream): the all-reduced estimate equals the one-rank estimate, the
union of the ranks' results matches numpy on the undivided mesh, the iteration count of a tolerance stop is the one-rank count."""
import os

import numpy as np
import pytest

import bp5_oracle as O
import chebyshev_ref as R
from test_gpu_multirank_loopback import ROOT, _rel, _run_ranks

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "loopback", "worker_chebyshev.py")


def _union(ranks, key, nd):
    full = np.full(nd, np.nan)
    for z in ranks:
        full[z["gid"].astype(np.int64)] = z[key]
    assert not np.isnan(full).any()
    return full


@pytest.mark.parametrize("world,cells,block,delay_us", [
    (2, (8, 8, 12), (4, 4, 4), 400),   # block kernel, two slabs
    (3, (8, 4, 13), (4, 4, 2), 250),   # first / middle / last rank, ragged slabs
])
def test_chebyshev_across_ranks_matches_one_rank_and_numpy(tmp_path, world, cells, block, delay_us):
    p, iters = 4, 10
    pr = O.Problem(p, cells, O.QUAD_GAUSS, deform_amp=0.05, kappa=O.kappa_step64)
    nd = pr.mesh.n_dofs
    b_ref = pr.rhs()
    tol = float(1e-9 * np.linalg.norm(b_ref))
    runs = {}
    for w in (1, world):
        out = tmp_path / f"w{w}"
        out.mkdir()
        _run_ranks(w, [p, *cells, *block, 1, 56, iters, repr(tol)], str(out), worker=WORKER, delay_us=delay_us if w > 1 else 0)
        runs[w] = [np.load(os.path.join(str(out), f"rank{r}.npz")) for r in range(w)]
    one, many = runs[1], runs[world]
    assert all(int(z["n_ghost"]) > 0 for z in many[1:])                  # the ranks really exchange halos
    # estimate: every rank the same; equal to one rank to 1e-12 and to numpy's CG-Lanczos on the undivided mesh to 1e-10
    inv_ref = 1.0 / O.operator_diagonal(pr.mesh, pr.coef, pr.N, pr.D)
    lo, hi, k = R.lanczos_estimate(pr.vmult, inv_ref, R.start_vector(np.arange(nd), pr.mesh.constrained), 8)
    for key in ("min_est", "max_est", "min_used", "max_used"):
        ref = float(one[0]["est_" + key])
        for z in many:
            assert abs(float(z["est_" + key]) - ref) <= 1e-12 * abs(ref), (key, float(z["est_" + key]), ref)
    assert all(int(z["est_cg_its"]) == k for z in one + many)
    assert abs(float(many[0]["est_min_est"]) - lo) <= 1e-10 * lo and abs(float(many[0]["est_max_est"]) - hi) <= 1e-10 * hi
    mu, Mu = R.bounds(lo, hi, 20.0)
    assert _rel(_union(many, "inv", nd), inv_ref) < 1e-13
    # vmult / step
    s, x0 = O.deterministic_src(nd, seed=31), O.deterministic_src(nd, seed=32)
    assert _rel(_union(many, "vmult", nd), R.vmult(pr.vmult, inv_ref, s, mu, Mu, 4)) < 1e-11
    assert _rel(_union(many, "step", nd), R.step(pr.vmult, inv_ref, x0, s, mu, Mu, 4)) < 1e-11
    # Chebyshev-PCG at a fixed iteration count, native and through the callbacks
    x_ref, _, _ = R.pcg(pr.vmult, lambda g: R.vmult(pr.vmult, inv_ref, g, mu, Mu, 4), b_ref, iters)
    for key in ("x_native", "x_callback"):
        assert _rel(_union(many, key, nd), x_ref) < 1e-10, key
    # tolerance stop: the one-rank iteration count (at most one off), the same on every rank, for check_every 0 and 1
    k1 = int(one[0]["its_tol0"])
    for z in many:
        assert int(z["its_tol0"]) == int(z["its_tol1"]) == int(many[0]["its_tol0"])
    assert abs(int(many[0]["its_tol0"]) - k1) <= 1
    x_tol, k_ref, _ = R.pcg(pr.vmult, lambda g: R.vmult(pr.vmult, inv_ref, g, mu, Mu, 4), b_ref, 500, tol=tol)
    assert abs(k_ref - k1) <= 1
    assert _rel(_union(many, "x_tol0", nd), x_tol) < 1e-8
    assert np.array_equal(_union(many, "x_tol0", nd), _union(many, "x_tol1", nd))
