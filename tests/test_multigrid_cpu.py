"""CPU checks of the p-multigrid numpy reference (tests/multigrid_ref.py) that the GPU tests of PreconditionMG compare against: the 1-D
interpolation matrix, the transpose built from weighted cell contributions, and the MG-PCG iteration counts (the acceptance band of the
GPU counts)."""
import numpy as np
import pytest

import bp5_oracle as O
import chebyshev_ref as R
import multigrid_ref as G

PAIRS = [(2, 1), (3, 1), (4, 2), (5, 2), (6, 3), (7, 3), (8, 4)]


def test_hierarchy_degrees():
    assert G.degrees(8) == [8, 4, 2, 1]
    assert G.degrees(7) == [7, 3, 1]
    assert G.degrees(6) == [6, 3, 1]
    assert G.degrees(1) == [1]


@pytest.mark.parametrize("pf,pc", PAIRS)
def test_interpolation_matrix_reproduces_coarse_polynomials(pf, pc):
    M = G.lagrange_matrix(pf, pc)
    xf, _ = O.gll_01(pf + 1)
    xc, _ = O.gll_01(pc + 1)
    assert np.array_equal(M[0], np.eye(pc + 1)[0]) and np.array_equal(M[-1], np.eye(pc + 1)[-1])
    for k in range(pc + 1):
        assert np.abs(M @ xc ** k - xf ** k).max() < 1e-14
    assert np.abs(M.sum(axis=1) - 1.0).max() < 1e-14
    # the columns are the coarse Lagrange polynomials: the oracle's tables of degree pc, evaluated at the fine nodes
    N, _ = O.lagrange_tables(xc, xf)
    assert np.abs(M - N).max() < 1e-13


def _cell_wise(mesh_f, mesh_c, M, rf=None, ec=None):
    """restriction from weighted cell contributions (w = 1 / cells holding the DoF) and prolongation cell by cell, writer = first cell"""
    nf, nc = M.shape
    l2g_f, l2g_c = mesh_f.l2g.astype(np.int64), mesh_c.l2g.astype(np.int64)
    count = np.bincount(l2g_f.ravel(), minlength=mesh_f.n_dofs).astype(float)
    bnd_c = np.zeros(mesh_c.n_dofs, dtype=bool)
    bnd_c[mesh_c.constrained.astype(np.int64)] = True
    out_r = np.zeros(mesh_c.n_dofs)
    out_p = np.full(mesh_f.n_dofs, np.nan)
    for c in range(mesh_f.n_cells):
        if rf is not None:
            v = ((rf / count)[l2g_f[c]]).reshape(nf, nf, nf)
            out_r[l2g_c[c]] += np.einsum("ka,jb,ic,kji->abc", M, M, M, v).ravel()
        if ec is not None:
            u = np.where(bnd_c, 0.0, ec)[l2g_c[c]].reshape(nc, nc, nc)
            y = np.einsum("ka,jb,ic,abc->kji", M, M, M, u).ravel()
            first = np.isnan(out_p[l2g_f[c]])
            out_p[l2g_f[c][first]] = y[first]
    out_r[bnd_c] = 0.0
    return out_r, out_p


@pytest.mark.parametrize("pf,cells", [(2, (3, 2, 4)), (4, (2, 3, 2)), (5, (2, 2, 3)), (8, (1, 2, 2))])
def test_weighted_cell_transpose_equals_assembled_transpose(pf, cells):
    pc = G.coarse_degree(pf)
    T = G.Transfer(cells, pf, pc)
    mf, mc = O.BrickMesh(pf, cells), O.BrickMesh(pc, cells)
    nf, nc = mf.n_dofs, mc.n_dofs
    # assembled P Z_c, column by column
    P = np.stack([T.prolongate(np.eye(nc)[j]) for j in range(nc)], axis=1)
    Z = np.ones(nc)
    Z[mc.constrained.astype(np.int64)] = 0.0
    assert np.abs(P - P * Z[None, :]).max() == 0.0
    rng = np.random.default_rng(5)
    rf, ec = rng.uniform(-1, 1, nf), rng.uniform(-1, 1, nc)
    r_cells, p_cells = _cell_wise(mf, mc, T.M, rf=rf, ec=ec)
    assert np.abs(r_cells - P.T @ rf).max() < 1e-13 * np.abs(rf).sum()
    assert np.abs(T.restrict(rf) - P.T @ rf).max() < 1e-13 * np.abs(rf).sum()
    assert np.abs(p_cells - P @ ec).max() < 1e-13
    # adjoint: <R r, e> = <r, P e>
    assert abs(T.restrict(rf) @ ec - rf @ T.prolongate(ec)) < 1e-12 * np.abs(rf).sum()
    # prolongation reproduces a coarse field exactly when it is a polynomial of degree pc per direction that vanishes on the boundary
    if pc >= 2:
        def f(X):
            return X[:, 0] * (cells[0] - X[:, 0]) * X[:, 1] * (cells[1] - X[:, 1]) * X[:, 2] * (cells[2] - X[:, 2])
        assert np.abs(T.prolongate(f(mc.coords)) - f(mf.coords)).max() < 1e-12


@pytest.mark.parametrize("p,cells", [(2, (4, 4, 4)), (4, (3, 3, 3)), (6, (3, 3, 3)), (2, (8, 8, 8)), (4, (6, 6, 6))])
def test_numpy_mg_pcg_iteration_count_is_flat(p, cells):
    V = G.VCycle(p, cells, deform_amp=0.05, kappa=O.kappa_step64)
    A = V.levels[0]
    b = A.pr.rhs()
    tol = 1e-8 * np.linalg.norm(b)
    x, k, res = R.pcg(A.A, V.vmult, b, 100, tol=tol)
    assert res <= tol
    assert 4 <= k <= 9, k
    r = b - A.A(x)
    assert np.linalg.norm(r) <= 1.01 * tol
    # against Chebyshev(4)-PCG on the same mesh: far more iterations
    if p == 4 and cells == (6, 6, 6):
        lo, hi, _ = R.lanczos_estimate(A.A, A.inv, R.start_vector(np.arange(A.pr.mesh.n_dofs), A.pr.mesh.constrained), 8)
        mu, Mu = R.bounds(lo, hi, 20.0)
        _, kc, _ = R.pcg(A.A, lambda g: R.vmult(A.A, A.inv, g, mu, Mu, 4), b, 500, tol=tol)
        assert kc >= 3 * k, (kc, k)


def test_v_cycle_is_symmetric():
    V = G.VCycle(4, (2, 2, 3), deform_amp=0.05, kappa=O.kappa_step64)
    n = V.levels[0].pr.mesh.n_dofs
    rng = np.random.default_rng(3)
    u, v = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    c = V.levels[0].pr.mesh.constrained.astype(np.int64)
    u[c] = v[c] = 0.0
    assert abs(u @ V.vmult(v) - v @ V.vmult(u)) < 1e-12 * abs(u @ V.vmult(u))


@pytest.mark.parametrize("pf,cells", [(4, (3, 2, 1)), (2, (1, 3, 2))])
def test_direction_sweeps_equal_the_assembled_kronecker_product(pf, cells):
    """Transfer applies P = Pz x Py x Px one direction at a time (the full-size GPU tests rely on it at 1.4e8 DoFs): against np.kron"""
    T = G.Transfer(cells, pf)
    Px, Py, Pz = T.P1
    P = np.kron(Pz, np.kron(Py, Px))
    rng = np.random.default_rng(9)
    ec, rf = rng.uniform(-1, 1, P.shape[1]), rng.uniform(-1, 1, P.shape[0])
    z = np.where(T.boundary_c, 0.0, 1.0)
    assert np.abs(T.prolongate(ec) - P @ (z * ec)).max() < 1e-14
    assert np.abs(T.restrict(rf) - z * (P.T @ rf)).max() < 1e-13


@pytest.mark.parametrize("p,quad,amp", [(2, 0, 0.05), (3, 1, 0.0), (4, 0, 0.04)])
def test_helmholtz_problem_is_the_oracle_helmholtz_operator(p, quad, amp):
    """HelmholtzProblem (the Helmholtz levels of the multigrid reference): vmult is O.apply_helmholtz_cells with the Dirichlet rows of
    PoissonOperator.vmult, and its diagonal is (A e_g)_g"""
    cells = (2, 2, 1)
    pr = G.HelmholtzProblem(p, cells, quad, h=0.5, deform_amp=amp)
    m = pr.mesh
    s = O.deterministic_src(m.n_dofs, seed=3)
    ref = O.apply_helmholtz_cells(m, pr.N, pr.D, pr.w, s)
    c = m.constrained.astype(np.int64)
    ref[c] = s[c]
    assert np.linalg.norm(pr.vmult(s) - ref) < 1e-13 * np.linalg.norm(ref)
    d_ref = np.array([pr.vmult(np.eye(1, m.n_dofs, g).ravel())[g] for g in range(m.n_dofs)])
    assert np.abs(pr.diagonal() - d_ref).max() < 1e-13 * np.abs(d_ref).max()
    # the mass term is there: the Poisson diagonal is smaller on every free row
    free = np.ones(m.n_dofs, bool)
    free[c] = False
    po, d_po = G.problem("poisson", p, cells, quad, h=0.5, deform_amp=amp)
    assert (d_ref[free] > d_po[free]).all()


def test_helmholtz_v_cycle_is_symmetric_and_converges():
    V = G.VCycle(4, (3, 3, 3), deform_amp=0.05, kappa=O.kappa_step64, operator="helmholtz")
    assert all(isinstance(L.pr, G.HelmholtzProblem) for L in V.levels)
    A = V.levels[0]
    n = A.pr.mesh.n_dofs
    rng = np.random.default_rng(4)
    u, v = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    c = A.pr.mesh.constrained.astype(np.int64)
    u[c] = v[c] = 0.0
    assert abs(u @ V.vmult(v) - v @ V.vmult(u)) < 1e-12 * abs(u @ V.vmult(u))
    b = A.pr.rhs()
    tol = 1e-8 * np.linalg.norm(b)
    x, k, res = R.pcg(A.A, V.vmult, b, 100, tol=tol)
    assert res <= tol and 3 <= k <= 9, k
    assert np.linalg.norm(b - A.A(x)) <= 1.01 * tol
