"""Gauss(p+2) quadrature (BP5_QUAD_GAUSS_OVER; CEED BP1 / BP3) without a GPU: the library's rectangular tables, the numpy reference of
tests/overint_ref.py pinned against quantities that do not come from it, the noise drift of every fixed-iteration CG reference
tests/test_gpu_overint.py compares against, and the refusals that need no handle."""
import os
import re

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import mass_ref as M
import overint_ref as R

pkg = bp5_pkg.load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMP = 0.04
_cache = {}


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def problem(p, cells, amp=0.0, kappa=O.kappa_none, mass=False, dirichlet=True, extra=1, h=1.0):
    key = (p, cells, amp, kappa, mass, dirichlet, extra, h)
    if key not in _cache:
        _cache[key] = R.Problem(p, cells, h=h, deform_amp=amp, kappa=kappa, mass=mass, dirichlet=dirichlet, extra=extra)
    return _cache[key]


# ------------------------------------------------------------------ the CG references of the GPU tests (computed once, shared, never changed)
CG_ITERATIONS = 10
SOLVERS = {"plain": O.cg_plain, "merged": O.cg_merged}


def config1_case():
    """BASELINE config 1's geometry (p = 2, 8^3 cells), deformed, kappa = 1, b_i = int phi_i, no preconditioner"""
    pr = problem(2, (8, 8, 8), AMP)
    return pr, pr.rhs(), None


def step64_case():
    """p = 4, 4^3 deformed cells, step-64's coefficient, Jacobi"""
    pr = problem(4, (4, 4, 4), AMP, O.kappa_step64)
    return pr, pr.rhs(), 1.0 / pr.diagonal()


def mass_case():
    """the mass operator at p = 2 on 4^3 deformed cells, rho = step-64's coefficient, Jacobi (the Dirichlet identity rows sit far from the mass
    spectrum: the inverse diagonal is part of the case)"""
    pr = problem(2, (4, 4, 4), AMP, O.kappa_step64, mass=True)
    return pr, pr.rhs(), 1.0 / pr.diagonal()


CG_CASES = {"config1": config1_case, "step64": step64_case, "mass": mass_case}


def cg_reference(case, solver):
    key = ("cg", case, solver)
    if key not in _cache:
        pr, b, inv = CG_CASES[case]()
        x, k, res = SOLVERS[solver](pr.vmult, b, CG_ITERATIONS, diag=inv)
        x.setflags(write=False)
        _cache[key] = (x, k, res)
    return _cache[key]


# ------------------------------------------------------------------ 1. the library's tables
@pytest.mark.parametrize("p", range(1, 9))
def test_library_tables(p):
    n, Q = p + 1, p + 2
    assert pkg.quadrature_points_1d(p, pkg.QUAD_GAUSS_OVER) == Q and pkg.quadrature_points_1d(p, 0) == n and pkg.quadrature_points_1d(p, 1) == n
    nodes, pts, w, N, D = pkg.shape_tables(p, pkg.QUAD_GAUSS_OVER)
    assert nodes.shape == (n,) and pts.shape == (Q,) and w.shape == (Q,) and N.shape == (Q, n) and D.shape == (Q, n)
    for got, want in zip((nodes, pts, w, N, D), R.tables(p)):
        assert np.allclose(got, want, atol=1e-13, rtol=1e-13)
    # the bitwise (anti)symmetry the kernels rely on: they read half of each table
    assert np.array_equal(N, N[::-1, ::-1]) and np.array_equal(D, -D[::-1, ::-1])
    assert abs(w.sum() - 1.0) <= 1e-15
    for k in range(2 * p + 4):                                           # Gauss(p+2) is exact up to degree 2 (p + 2) - 1 = 2 p + 3
        assert abs(w @ pts ** k - 1.0 / (k + 1)) <= 1e-14, (p, k)
    assert np.allclose(N.sum(axis=1), 1.0, atol=1e-14) and np.allclose(D.sum(axis=1), 0.0, atol=1e-12)
    # the square tables are what they were
    for quad in (0, 1):
        for got, want in zip(pkg.shape_tables(p, quad), O.shape_tables(p, quad)):
            assert got.shape == want.shape and np.allclose(got, want, atol=1e-13, rtol=1e-13)


def test_unknown_ids_stay_refused():
    L = pkg.lib()
    for quad in (3, 7, -1):
        assert L.bp5_shape_tables(3, quad, None, None, None, None, None) == 1 and b"quadrature" in L.bp5_last_error()
        with pytest.raises(pkg.BP5Error) as e:
            pkg.quadrature_points_1d(3, quad)
        assert e.value.status == 1 and "quadrature" in str(e.value)
        with pytest.raises(pkg.BP5Error) as e:
            pkg.shape_tables(3, quad)
        assert e.value.status == 1 and "quadrature" in str(e.value)
    for p in (0, 9):
        with pytest.raises(pkg.BP5Error) as e:
            pkg.quadrature_points_1d(p, pkg.QUAD_GAUSS_OVER)
        assert e.value.status == 1 and "degree" in str(e.value)
    assert L.bp5_quadrature_points_1d(3, 2, None) == 1


# ------------------------------------------------------------------ 2. the reference, pinned outside itself
@pytest.mark.parametrize("p,cells", [(1, (3, 2, 2)), (2, (3, 2, 2)), (4, (3, 2, 2)), (8, (2, 1, 1))])
def test_affine_cells_give_the_p_plus_1_operator(p, cells):
    """undeformed mesh, kappa = 1: both quadratures integrate the cell matrices exactly (Poisson: degree 2p per variable; mass: 2p)"""
    src = O.deterministic_src(problem(p, cells).mesh.n_dofs, seed=3)
    a = rel(problem(p, cells).vmult(src), O.Problem(p, cells, O.QUAD_GAUSS).vmult(src))
    b = rel(problem(p, cells, mass=True).vmult(src), M.Problem(p, cells, O.QUAD_GAUSS).vmult(src))
    print(f"p={p} {cells}: Poisson {a:.2e}, mass {b:.2e}")
    assert a <= 1e-13 and b <= 1e-13


@pytest.mark.parametrize("p,cells,kappa", [(1, (3, 2, 2), O.kappa_step64), (2, (3, 2, 2), O.kappa_none), (4, (3, 2, 2), O.kappa_none), (8, (2, 1, 1), O.kappa_none)])
def test_deformed_cells_do_not(p, cells, kappa):
    """deform_amp = 0.04: the two quadratures give different operators (p = 1: the sine deformation vanishes at every vertex of (3, 2, 2), so
    the variable coefficient tells them apart)"""
    src = O.deterministic_src(problem(p, cells).mesh.n_dofs, seed=3)
    out = []
    for mass in (False, True):
        over, square = problem(p, cells, AMP, kappa, mass=mass), problem(p, cells, AMP, kappa, mass=mass, extra=0)
        out.append(rel(over.apply_cells(src), square.apply_cells(src)))
    print(f"p={p} {cells}: Poisson {out[0]:.2e}, mass {out[1]:.2e}")
    assert min(out) > 1e-3
    # ... and extra = 0 IS the oracle's operator
    kap = "kappa" if kappa is O.kappa_step64 else None
    ref = O.Problem(p, cells, O.QUAD_GAUSS, deform_amp=AMP, kappa=kappa)
    assert rel(problem(p, cells, AMP, kappa, extra=0).vmult(src), ref.vmult(src)) <= 1e-13, kap


@pytest.mark.parametrize("p,cells,kappa", [(1, (3, 2, 2), O.kappa_step64), (2, (3, 2, 2), O.kappa_none), (3, (2, 2, 1), O.kappa_step64), (4, (2, 1, 1), O.kappa_step64)])
def test_sum_factorised_apply_is_the_dense_element_matrix(p, cells, kappa):
    """per cell of a deformed mesh: O.element_matrix (already rectangular) / the dense mass matrix, applied and summed through l2g; and the
    diagonals are the diagonals of those matrices"""
    for mass in (False, True):
        pr = problem(p, cells, AMP, kappa, mass=mass)
        m = pr.mesh
        src = O.deterministic_src(m.n_dofs, seed=4)
        want, dwant = np.zeros(m.n_dofs), np.zeros(m.n_dofs)
        for c in range(m.n_cells):
            A = R.mass_element_matrix(pr.coef[c], pr.N) if mass else O.element_matrix(pr.coef[:, c], pr.N, pr.D)
            assert np.abs(A - A.T).max() <= 1e-13 * np.abs(A).max()
            idx = m.l2g[c].astype(np.int64)
            np.add.at(want, idx, A @ src[idx])
            np.add.at(dwant, idx, np.diag(A))
        assert rel(pr.apply_cells(src), want) <= 1e-13
        dwant[m.constrained.astype(np.int64)] = 1.0
        assert rel(pr.diagonal(), dwant) <= 1e-13


@pytest.mark.parametrize("p,cells", [(2, (3, 2, 2)), (4, (3, 2, 2))])
def test_symmetry_null_space_and_volume(p, cells):
    for mass in (False, True):
        pr = problem(p, cells, AMP, O.kappa_step64, mass=mass, dirichlet=False)
        n = pr.mesh.n_dofs
        u, v = O.deterministic_src(n, seed=5), O.deterministic_src(n, seed=6)
        Au, Av = pr.apply_cells(u), pr.apply_cells(v)
        assert abs(v @ Au - u @ Av) <= 1e-13 * abs(v @ Au)
        assert u @ Au > 0.0
    one = np.ones(n)
    lap = problem(p, cells, AMP, O.kappa_step64, dirichlet=False)
    assert np.linalg.norm(lap.apply_cells(one)) <= 1e-12 * np.linalg.norm(lap.apply_cells(u))      # constants: the null space without a boundary condition
    # 1^T M 1 is the volume: h^3 per cell on the undeformed mesh; the deformation keeps the boundary, and Gauss(p+2) integrates det J (degree 3p - 1
    # per variable) exactly while 3p - 1 <= 2p + 3, i.e. up to p = 4
    vol = problem(p, cells, mass=True, dirichlet=False, h=0.5)
    assert abs(one @ vol.apply_cells(one) - 0.125 * float(np.prod(cells))) <= 1e-13 * float(np.prod(cells))
    vol = problem(p, cells, AMP, mass=True, dirichlet=False)
    assert abs(one @ vol.apply_cells(one) - float(np.prod(cells))) <= 1e-13 * float(np.prod(cells))


# ------------------------------------------------------------------ 3. noise drift of the fixed-iteration CG references
@pytest.mark.parametrize("solver", sorted(SOLVERS))
@pytest.mark.parametrize("case", sorted(CG_CASES))
def test_cg_references_do_not_amplify_rounding(case, solver):
    """a relative perturbation of 1e-16 per operator application moves the 10-iteration solution by less than 1e-13: the 1e-11 bound of the GPU
    comparison is two orders above what rounding can do to these references"""
    pr, b, inv = CG_CASES[case]()
    drift = R.noise_drift(pr.vmult, b, CG_ITERATIONS, inv_diag=inv, solver=SOLVERS[solver])
    x, k, res = cg_reference(case, solver)
    print(f"{case} / {solver}: drift {drift:.2e}, residual after {k} iterations {res:.3e} (|b| = {np.linalg.norm(b):.3e})")
    assert k == CG_ITERATIONS and drift < 1e-13 and res > 1e-8 * np.linalg.norm(b)


# ------------------------------------------------------------------ 4. the feature's public names
def test_public_names():
    from deal_and_ceed_on_gpu_amd import _lib
    assert _lib.QUAD_GAUSS_OVER == 2 and pkg.QUAD_GAUSS_OVER == 2
    assert "bp5_quadrature_points_1d" in pkg.HEADER_SYMBOLS and hasattr(pkg.lib(), "bp5_quadrature_points_1d")
    text = open(os.path.join(ROOT, "include", "bp5.h")).read()
    assert re.search(r"BP5_QUAD_GAUSS_OVER\s*=\s*2\b", text)
