"""CPU checks of the numpy reference of FP32 metric planes (tests/f32_metric_ref.py) that the GPU tests of bp5_mf_set_metric_precision compare
against -- the V-cycle on rounded planes is symmetric and costs MG-PCG no iteration -- and the argument validation of the new entry points
that needs no device."""
import ctypes as C

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import chebyshev_ref as R
import f32_metric_ref as F
import multigrid_ref as G

pkg = bp5_pkg.load()
CASES = [(2, (8, 8, 8)), (4, (6, 6, 6)), (3, (6, 4, 6))]      # all deformed 0.05, step-64 kappa, tolerance 1e-10 ||b||
_cache = {}


def _cycles(p, cells):
    if (p, cells) not in _cache:
        _cache[(p, cells)] = (G.VCycle(p, cells, deform_amp=0.05, kappa=O.kappa_step64), F.VCycle(p, cells, deform_amp=0.05, kappa=O.kappa_step64))
    return _cache[(p, cells)]


def test_rounded_planes_are_floats_and_half_an_ulp_away():
    pr = O.Problem(4, (2, 2, 2), deform_amp=0.05, kappa=O.kappa_step64)
    r = F.round_planes(pr.coef)
    assert np.array_equal(r, r.astype(np.float32).astype(np.float64))
    assert (np.abs(r - pr.coef) <= 2.0 ** -24 * np.abs(pr.coef)).all()
    L = F.Level(4, (2, 2, 2), 1.0, O.QUAD_GAUSS, 0.05, O.kappa_step64, 4, 20.0, 10)
    assert np.array_equal(L.pr.coef, r) and np.array_equal(L.coef64, pr.coef)
    # planes handed in are used as they are, and the diagonal follows them
    L2 = F.Level(4, (2, 2, 2), 1.0, O.QUAD_GAUSS, 0.05, O.kappa_step64, 4, 20.0, 10, planes=2.0 * r)
    assert np.allclose(L2.inv[~np.isin(np.arange(L2.inv.size), pr.mesh.constrained)] * 2.0, L.inv[~np.isin(np.arange(L.inv.size), pr.mesh.constrained)], rtol=1e-14)


@pytest.mark.parametrize("p,cells", CASES)
def test_v_cycle_on_rounded_planes_is_symmetric(p, cells):
    _, V32 = _cycles(p, cells)
    m = V32.levels[0].pr.mesh
    rng = np.random.default_rng(3)
    u, v = rng.uniform(-1, 1, m.n_dofs), rng.uniform(-1, 1, m.n_dofs)
    c = m.constrained.astype(np.int64)
    u[c] = v[c] = 0.0
    Vu, Vv = V32.vmult(u), V32.vmult(v)
    assert abs(u @ Vv - v @ Vu) <= 1e-12 * abs(u @ Vu)


@pytest.mark.parametrize("p,cells,count", [(2, (8, 8, 8), 7), (4, (6, 6, 6), 7), (3, (6, 4, 6), 8)])
def test_mg_pcg_count_equals_the_fp64_levels_count(p, cells, count):
    """outer operator FP64 either way: rounded level planes cost no iteration (7/7, 7/7, 8/8)"""
    V64, V32 = _cycles(p, cells)
    A = V64.levels[0]
    b = A.pr.rhs()
    tol = 1e-10 * np.linalg.norm(b)
    x64, k64, _ = R.pcg(A.A, V64.vmult, b, 100, tol=tol)
    x32, k32, _ = R.pcg(A.A, V32.vmult, b, 100, tol=tol)
    assert k64 == k32 == count, (k64, k32)
    assert np.linalg.norm(b - A.A(x32)) <= tol
    # the rounded operator is an O(1e-8) perturbation of the FP64 one
    u = O.deterministic_src(A.pr.mesh.n_dofs, A.pr.mesh.constrained, seed=5)
    d = np.linalg.norm(V32.levels[0].A(u) - A.A(u)) / np.linalg.norm(A.A(u))
    assert 1e-10 < d < 1e-7, d


def test_metric_precision_entry_points_validate_their_arguments_without_a_gpu():
    """a NULL handle and an unknown value are refused before anything touches a device (status codes, no crash)"""
    L = pkg.lib()
    null = C.c_void_p()
    assert L.bp5_mf_set_metric_precision(null, 1) == 1
    assert b"null" in L.bp5_last_error().lower()
    assert L.bp5_mf_set_metric_precision(null, 0) == 1
    assert L.bp5_mf_set_metric_precision(null, 7) == 1
    v = C.c_int(-1)
    assert L.bp5_mf_get_metric_precision(null, C.byref(v)) == 1 and v.value == -1
    with pytest.raises(pkg.BP5Error):
        pkg.MatrixFree().set_metric_precision("float32")        # no handle yet
    text = open(bp5_pkg.ROOT + "/include/bp5.h").read()
    assert "BP5_METRIC_F64 = 0, BP5_METRIC_F32 = 1" in text
    assert pkg.MatrixFree.METRIC_PRECISION == {"float64": 0, "float32": 1}
