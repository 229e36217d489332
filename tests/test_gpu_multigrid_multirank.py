"""PreconditionMG on 1, 2 and 3 ranks as processes on ONE GPU (the loopback build of test_gpu_multirank_loopback.py, every transfer lagging
behind its stream): the per-level estimates equal the one-rank ones, the iteration count of MG-PCG is the one-rank count, and the union of
the ranks' V-cycle and solution matches numpy on the undivided mesh."""
import os

import numpy as np
import pytest

import bp5_oracle as O
import chebyshev_ref as R
import multigrid_ref as G
from test_gpu_multirank_loopback import ROOT, _rel, _run_ranks

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "loopback", "worker_multigrid.py")


def _union(ranks, key, nd):
    full = np.full(nd, np.nan)
    for z in ranks:
        full[z["gid"].astype(np.int64)] = z[key]
    assert not np.isnan(full).any()
    return full


@pytest.mark.parametrize("world,p,cells,block,delay_us", [
    (2, 4, (6, 6, 8), (4, 4, 4), 400),   # block kernel, two slabs
    (3, 2, (8, 4, 13), (4, 4, 2), 250),  # first / middle / last rank, ragged slabs
])
def test_multigrid_across_ranks_matches_one_rank_and_numpy(tmp_path, world, p, cells, block, delay_us):
    runs = {}
    for w in (1, world):
        out = tmp_path / f"w{w}"
        out.mkdir()
        _run_ranks(w, [p, *cells, *block, 1, 56, "1e-8"], str(out), worker=WORKER, delay_us=delay_us if w > 1 else 0)
        runs[w] = [np.load(os.path.join(str(out), f"rank{r}.npz")) for r in range(w)]
    one, many = runs[1], runs[world]
    assert all(int(z["n_ghost"][0]) > 0 and int(z["n_ghost"][-1]) > 0 for z in many[1:])   # fine and coarse levels exchange halos
    n_levels = len(G.degrees(p))
    for lev in range(n_levels):
        for key in ("min_est", "max_est", "min_used", "max_used"):
            ref = float(one[0][f"l{lev}_{key}"])
            for z in many:
                assert abs(float(z[f"l{lev}_{key}"]) - ref) <= 1e-12 * abs(ref), (lev, key, float(z[f"l{lev}_{key}"]), ref)
        assert all(int(z[f"l{lev}_cg_its"]) == int(one[0][f"l{lev}_cg_its"]) for z in many)
    assert all(int(z["its"]) == int(one[0]["its"]) for z in many)
    V = G.VCycle(p, cells, deform_amp=0.05, kappa=O.kappa_step64)
    A = V.levels[0]
    nd = A.pr.mesh.n_dofs
    s = O.deterministic_src(nd, A.pr.mesh.constrained, seed=43)
    assert _rel(_union(many, "vcycle", nd), V.vmult(s)) < 1e-11
    b = A.pr.rhs()
    x_ref, k_ref, _ = R.pcg(A.A, V.vmult, b, 200, tol=1e-8 * np.linalg.norm(b))
    assert abs(int(many[0]["its"]) - k_ref) <= 1
    assert _rel(_union(many, "x", nd), x_ref) < 1e-7
