"""FP32 metric planes (bp5_mf_set_metric_precision) on 2 ranks as processes on ONE GPU (the loopback build of
test_gpu_multirank_loopback.py, every transfer lagging behind its stream): the distributed application of the FP32-plane operator against the
oracle on the planes read back from the library, and the mixed-precision MG-PCG (outer operator FP64, every level on float planes) against
the one-rank count and the numpy solution.  The pattern of tests/test_gpu_hybrid_multigrid_multirank.py."""
import os

import numpy as np
import pytest

import bp5_oracle as O
import chebyshev_ref as R
import f32_metric_ref as F
import hmg_ref as H
from test_gpu_multirank_loopback import ROOT, _rel, _run_ranks

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "loopback", "worker_f32_metric.py")
COARSE = 10


def _union(ranks, key, nd):
    full = np.full(nd, np.nan)
    for z in ranks:
        full[z["gid"].astype(np.int64)] = z[key]
    assert not np.isnan(full).any()
    return full


def _planes(ranks, lev, n_cells):
    """the level's planes of all ranks in the oracle's lexicographic cell order"""
    n3 = ranks[0][f"planes{lev}"].shape[2]
    full = np.full((6, n_cells, n3), np.nan)
    for z in ranks:
        full[:, z[f"cell_lex{lev}"].astype(np.int64)] = z[f"planes{lev}"]
    assert not np.isnan(full).any()
    return full


@pytest.mark.parametrize("world,p,cells,block,numbering,variant,h_levels,delay_us", [
    (2, 2, (8, 8, 8), (4, 4, 4), 1, 56, "max", 400),   # block kernel on float planes, two slabs with ghost rows: p = 2, 1 on 8^3, then p = 1 on 4^3
    (2, 4, (4, 4, 6), (0, 0, 0), 0, 0, 0, 250),        # lexicographic cells, pencil kernel on float planes (3-phase schedule): p = 4, 2, 1
])
def test_f32_metric_across_ranks_matches_one_rank_and_numpy(tmp_path, world, p, cells, block, numbering, variant, h_levels, delay_us):
    runs = {}
    for w in (1, world):
        out = tmp_path / f"w{w}"
        out.mkdir()
        _run_ranks(w, [p, *cells, *block, numbering, variant, "1e-10", h_levels, COARSE], str(out), worker=WORKER, delay_us=delay_us if w > 1 else 0)
        runs[w] = [np.load(os.path.join(str(out), f"rank{r}.npz")) for r in range(w)]
    one, many = runs[1], runs[world]
    spec = H.hierarchy(p, cells, h_levels)
    for z in one + many:
        assert [(int(q), tuple(int(x) for x in c)) for q, c in zip(z["degrees"], z["cells"])] == [(q, c) for q, c, _ in spec]
        assert all(str(s) == "float32" for s in z["precision"])
    assert all(int(z["n_ghost"][0]) > 0 for z in many[1:])
    planes = [_planes(many, lev, int(np.prod(c))) for lev, (_, c, _) in enumerate(spec)]
    for lev in range(len(spec)):                                                    # the planes do not depend on the partition
        assert np.array_equal(planes[lev], _planes(one, lev, planes[lev].shape[1]))
        assert np.array_equal(planes[lev], planes[lev].astype(np.float32).astype(np.float64))
    V = F.VCycle(p, cells, deform_amp=0.05, kappa=O.kappa_step64, h_levels=h_levels, planes=planes, coarse_degree=COARSE)
    A32 = V.levels[0]
    nd = A32.pr.mesh.n_dofs
    # bp5_apply_distributed on float planes, summed through global_ids, against the oracle on the read-back planes
    s = O.deterministic_src(nd, A32.pr.mesh.constrained, seed=43)
    assert _rel(_union(many, "vmult", nd), A32.A(s)) <= 1e-13
    # mixed-precision MG-PCG: level bounds and count of the one-rank run, count and solution of numpy (outer operator: FP64 planes)
    for lev, L in enumerate(V.levels):
        for key in ("min_est", "max_est", "min_used", "max_used"):
            ref = float(one[0][f"l{lev}_{key}"])
            assert abs(ref - getattr(L, key)) <= 1e-10 * abs(getattr(L, key)), (lev, key, ref, getattr(L, key))
            for z in many:
                assert abs(float(z[f"l{lev}_{key}"]) - ref) <= 1e-12 * abs(ref), (lev, key, float(z[f"l{lev}_{key}"]), ref)
        assert all(int(z[f"l{lev}_cg_its"]) == int(one[0][f"l{lev}_cg_its"]) == L.cg_its for z in many)
    assert all(int(z["its"]) == int(one[0]["its"]) for z in many)
    pr64 = O.Problem(p, cells, O.QUAD_GAUSS, deform_amp=0.05, kappa=O.kappa_step64)
    b = pr64.rhs()
    tol = 1e-10 * np.linalg.norm(b)
    x_ref, k_ref, _ = R.pcg(pr64.vmult, V.vmult, b, 200, tol=tol)
    assert abs(int(many[0]["its"]) - k_ref) <= 1, (int(many[0]["its"]), k_ref)
    x = _union(many, "x", nd)
    assert _rel(x, x_ref) < 1e-7
    assert np.linalg.norm(b - pr64.vmult(x)) <= tol                                # the residual, recomputed with the FP64 operator
