"""PreconditionMG on the hybrid hierarchy (p-levels, then geometric h-levels at degree 1) on 1, 2 and 3 ranks as processes on ONE GPU (the
loopback build of test_gpu_multirank_loopback.py, every transfer lagging behind its stream): the per-level estimates equal the one-rank
ones, the iteration count of MG-PCG is the one-rank count, and the union of the ranks' V-cycle and solution matches numpy on the undivided
mesh."""
import os

import numpy as np
import pytest

import bp5_oracle as O
import chebyshev_ref as R
import hmg_ref as H
from test_gpu_multirank_loopback import ROOT, _rel, _run_ranks

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "loopback", "worker_hybrid_multigrid.py")
COARSE = 10


def _union(ranks, key, nd):
    full = np.full(nd, np.nan)
    for z in ranks:
        full[z["gid"].astype(np.int64)] = z[key]
    assert not np.isnan(full).any()
    return full


@pytest.mark.parametrize("world,p,cells,block,numbering,variant,delay_us", [
    (2, 2, (8, 8, 8), (4, 4, 4), 1, 56, 400),   # block kernel, two slabs: p = 2, 1 on 8^3, then p = 1 on 4^3
    (3, 1, (8, 8, 12), (0, 0, 0), 0, 0, 250),   # first / middle / last rank: 12 -> 6 layers (4 -> 2 per rank), min_cells 4 stops there
])
def test_hybrid_multigrid_across_ranks_matches_one_rank_and_numpy(tmp_path, world, p, cells, block, numbering, variant, delay_us):
    runs = {}
    for w in (1, world):
        out = tmp_path / f"w{w}"
        out.mkdir()
        _run_ranks(w, [p, *cells, *block, numbering, variant, "1e-8", "max", COARSE], str(out), worker=WORKER, delay_us=delay_us if w > 1 else 0)
        runs[w] = [np.load(os.path.join(str(out), f"rank{r}.npz")) for r in range(w)]
    one, many = runs[1], runs[world]
    V = H.HybridVCycle(p, cells, deform_amp=0.05, kappa=O.kappa_step64, coarse_degree=COARSE)
    spec = [(q, c) for q, c, _ in V.spec]
    assert len(spec) > len(H.hierarchy(p, cells, h_levels=0))                                   # there are h-levels
    for z in one + many:
        assert [(int(q), tuple(int(x) for x in c)) for q, c in zip(z["degrees"], z["cells"])] == spec
    assert all(int(z["n_ghost"][0]) > 0 and int(z["n_ghost"][-1]) > 0 for z in many[1:])   # fine and coarsest levels exchange halos
    for lev in range(len(spec)):
        for key in ("min_est", "max_est", "min_used", "max_used"):
            ref = float(one[0][f"l{lev}_{key}"])
            for z in many:
                assert abs(float(z[f"l{lev}_{key}"]) - ref) <= 1e-12 * abs(ref), (lev, key, float(z[f"l{lev}_{key}"]), ref)
        assert all(int(z[f"l{lev}_cg_its"]) == int(one[0][f"l{lev}_cg_its"]) for z in many)
    assert all(int(z["its"]) == int(one[0]["its"]) for z in many)
    A = V.levels[0]
    nd = A.pr.mesh.n_dofs
    s = O.deterministic_src(nd, A.pr.mesh.constrained, seed=43)
    assert _rel(_union(many, "vcycle", nd), V.vmult(s)) < 1e-11
    b = A.pr.rhs()
    x_ref, k_ref, _ = R.pcg(A.A, V.vmult, b, 200, tol=1e-8 * np.linalg.norm(b))
    assert abs(int(many[0]["its"]) - k_ref) <= 1
    assert _rel(_union(many, "x", nd), x_ref) < 1e-7
