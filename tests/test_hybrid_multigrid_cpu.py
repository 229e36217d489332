"""CPU checks of the geometric (h) multigrid transfer and the hybrid p-then-h hierarchy: the 1-D matrices M_s, the numpy prolongation and
its cell-wise weighted transpose (tests/hmg_ref.py), the host parent map bp5_mesh_parent_cells on every cell order the generator emits and
its refusals, BrickMesh.coarsen, and the numpy MG-PCG iteration counts the GPU tests compare against."""
import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import chebyshev_ref as R
import hmg_ref as H

pkg = bp5_pkg.load()
AMP = 0.05


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_geometric_matrices_reproduce_polynomials(p):
    x, _ = O.gll_01(p + 1)
    for s, M in enumerate(H.geometric_matrices(p)):
        assert np.abs(M.sum(axis=1) - 1.0).max() < 1e-14
        for k in range(p + 1):
            assert np.abs(M @ x ** k - (0.5 * x + 0.5 * s) ** k).max() < 1e-14
    M0, M1 = H.geometric_matrices(p)
    assert np.array_equal(M0[0], np.eye(p + 1)[0]) and np.array_equal(M1[-1], np.eye(p + 1)[-1])
    assert np.array_equal(M0[-1], M1[0])                     # the node at the middle of the parent, seen from both children
    if p % 2 == 0:
        assert np.array_equal(M0[-1], np.eye(p + 1)[p // 2])


@pytest.mark.parametrize("p,cells_c", [(1, (3, 2, 2)), (2, (2, 3, 2)), (3, (2, 2, 1)), (4, (1, 2, 2))])
def test_prolongation_interpolates_degree_p_polynomials(p, cells_c):
    mc, mf = O.BrickMesh(p, cells_c, h=2.0), O.BrickMesh(p, tuple(2 * c for c in cells_c), h=1.0)
    T = H.GeometricTransfer(cells_c, p)

    def f(X):   # degree p in every direction
        return (1.0 + X[:, 0]) ** p * (0.5 - X[:, 1]) ** p + X[:, 2] ** p * X[:, 0] - 0.25 * X[:, 1]

    Px, Py, Pz = T.P1
    u = f(mc.coords).reshape(T.shape_c)
    got = np.einsum("xa,yb,zc,cba->zyx", Px, Py, Pz, u, optimize=True).ravel()
    assert np.abs(got - f(mf.coords)).max() < 1e-12 * np.abs(f(mf.coords)).max()
    if p >= 2:   # with the coarse Dirichlet DoFs zeroed: a polynomial that vanishes on the boundary
        L = [2.0 * c for c in cells_c]

        def g(X):
            return np.prod([X[:, d] * (L[d] - X[:, d]) for d in range(3)], axis=0)

        assert np.abs(T.prolongate(g(mc.coords)) - g(mf.coords)).max() < 1e-12


@pytest.mark.parametrize("p,cells_c", [(1, (3, 2, 2)), (2, (2, 2, 3)), (4, (1, 2, 2))])
def test_weighted_cell_transpose_equals_assembled_transpose(p, cells_c):
    cells_f = tuple(2 * c for c in cells_c)
    mf, mc = O.BrickMesh(p, cells_f, h=1.0), O.BrickMesh(p, cells_c, h=2.0)
    T = H.GeometricTransfer(cells_c, p)
    nf, nc = mf.n_dofs, mc.n_dofs
    P = np.stack([T.prolongate(np.eye(nc)[j]) for j in range(nc)], axis=1)
    bnd_c = np.zeros(nc, dtype=bool)
    bnd_c[mc.constrained.astype(np.int64)] = True
    assert np.abs(P[:, bnd_c]).max() == 0.0
    # cell-wise: w = 1 / cells holding the fine DoF; parent and child from the cells' first corners
    l2g_f, l2g_c = mf.l2g.astype(np.int64), mc.l2g.astype(np.int64)
    NXf, NYf = p * cells_f[0] + 1, p * cells_f[1] + 1
    NXc, NYc = p * cells_c[0] + 1, p * cells_c[1] + 1
    first_c = {int(l2g_c[c, 0]): c for c in range(mc.n_cells)}
    Ms = H.geometric_matrices(p)
    count = np.bincount(l2g_f.ravel(), minlength=nf).astype(float)
    rng = np.random.default_rng(7)
    rf, ec = rng.uniform(-1, 1, nf), rng.uniform(-1, 1, nc)
    out_r = np.zeros(nc)
    out_p = np.full(nf, np.nan)
    n = p + 1
    for c in range(mf.n_cells):
        g0 = int(l2g_f[c, 0])
        x, y, z = (g0 % NXf) // p, (g0 // NXf % NYf) // p, (g0 // (NXf * NYf)) // p
        par = first_c[p * (x // 2) + NXc * (p * (y // 2) + NYc * p * (z // 2))]
        Mx, My, Mz = Ms[x & 1], Ms[y & 1], Ms[z & 1]
        v = ((rf / count)[l2g_f[c]]).reshape(n, n, n)
        out_r[l2g_c[par]] += np.einsum("ka,jb,ic,kji->abc", Mz, My, Mx, v).ravel()
        u = np.where(bnd_c, 0.0, ec)[l2g_c[par]].reshape(n, n, n)
        yv = np.einsum("ka,jb,ic,abc->kji", Mz, My, Mx, u).ravel()
        first = np.isnan(out_p[l2g_f[c]])
        out_p[l2g_f[c][first]] = yv[first]
    out_r[bnd_c] = 0.0
    assert np.abs(out_r - P.T @ rf).max() < 1e-13 * np.abs(rf).sum()
    assert np.abs(T.restrict(rf) - P.T @ rf).max() < 1e-13 * np.abs(rf).sum()
    assert np.abs(out_p - P @ ec).max() < 1e-13
    assert abs(T.restrict(rf) @ ec - rf @ T.prolongate(ec)) < 1e-12 * np.abs(rf).sum()


def _xyz(m):
    """global cell coordinates of a BrickMesh's local cells, from the lexicographic global id of each cell's first corner"""
    NX, NY = m.view.global_dofs_per_dir[0], m.view.global_dofs_per_dir[1]
    g = m.global_ids[m.l2g[:, 0].astype(np.int64)].astype(np.int64)
    return np.stack([g % NX, g // NX % NY, g // (NX * NY)], axis=1) // m.degree


def _check_parent_map(fine, coarse):
    parent, child = fine.parent_cells(coarse)
    assert parent.dtype == np.uint32 and child.dtype == np.uint8 and parent.shape == child.shape == (fine.n_cells,)
    xf, xc = _xyz(fine), _xyz(coarse)
    assert np.array_equal(xc[parent.astype(np.int64)], xf // 2)
    assert np.array_equal(child, (xf[:, 0] & 1) | (xf[:, 1] & 1) << 1 | (xf[:, 2] & 1) << 2)
    # every coarse cell: 8 distinct children
    codes = np.zeros((coarse.n_cells, 8), dtype=int)
    np.add.at(codes, (parent.astype(np.int64), child.astype(np.int64)), 1)
    assert (codes == 1).all()


ORDERS = {"lex": {}, "bricks": dict(cell_block=(4, 2, 2)), "bricks_block_major": dict(cell_block=(2, 4, 2), dof_numbering=1),
          "class_major": dict(cell_block=(4, 4, 2), dof_numbering=1, cell_block_order=1), "interiors_first": dict(dof_numbering=2)}


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("p", [1, 2])
def test_parent_cells_on_every_cell_order(order, p):
    fine = pkg.BrickMesh(p, (8, 6, 10), deform_amp=AMP, **ORDERS[order])
    coarse = fine.coarsen(min_cells=2)
    assert coarse.cells == (4, 3, 5) and coarse.h == 2.0 and coarse.degree == p and coarse.cell_block == fine.cell_block
    _check_parent_map(fine, coarse)


@pytest.mark.parametrize("n_ranks,cells,order", [(2, (8, 6, 8), "lex"), (2, (8, 8, 8), "class_major"), (3, (8, 8, 12), "lex"),
                                                 (3, (8, 8, 12), "bricks_block_major")])
def test_parent_cells_on_several_ranks(n_ranks, cells, order):
    for r in range(n_ranks):
        fine = pkg.BrickMesh(1, cells, rank=r, n_ranks=n_ranks, **ORDERS[order])
        mesh = fine
        layers = [cells[2]]
        while True:
            coarse = mesh.coarsen(min_cells=1)
            if coarse is None:
                break
            _check_parent_map(mesh, coarse)
            layers.append(coarse.cells[2])
            mesh = coarse
        if n_ranks == 3:
            assert layers == [12, 6, 3]


def test_coarsen_stops_where_the_rules_say():
    assert pkg.BrickMesh(1, (16, 16, 16)).coarsen().cells == (8, 8, 8)
    assert pkg.BrickMesh(1, (8, 8, 8)).coarsen().cells == (4, 4, 4)
    assert pkg.BrickMesh(1, (4, 8, 8)).coarsen() is None                    # 2 < min_cells
    assert pkg.BrickMesh(1, (4, 8, 8)).coarsen(min_cells=2).cells == (2, 4, 4)
    assert pkg.BrickMesh(1, (8, 9, 8)).coarsen() is None                    # odd
    assert pkg.BrickMesh(1, (116, 116, 120)).coarsen().coarsen().cells == (29, 29, 30)
    assert pkg.BrickMesh(1, (116, 116, 120)).coarsen().coarsen().coarsen() is None
    assert pkg.BrickMesh(1, (8, 8, 120), rank=0, n_ranks=8).coarsen() is None   # 15 layers per rank: the slabs do not nest
    assert pkg.BrickMesh(1, (8, 8, 20), rank=0, n_ranks=8).coarsen() is None
    assert pkg.BrickMesh(1, (8, 8, 32), rank=0, n_ranks=8).coarsen().cells == (4, 4, 16)
    for cells, R_ in [((16, 16, 16), 1), ((8, 9, 8), 1), ((8, 8, 120), 8), ((8, 8, 32), 8)]:
        c = H.coarsen(cells, 4, R_)
        m = pkg.BrickMesh(1, cells, rank=0, n_ranks=R_).coarsen()
        assert (c is None and m is None) or c == m.cells


def _refused(fine, coarse, word):
    with pytest.raises(pkg.BP5Error) as e:
        fine.parent_cells(coarse)
    assert e.value.status == 1 and word in str(e.value), str(e.value)


def test_parent_cells_refuses_meshes_that_are_not_a_2_to_1_pair():
    fine = pkg.BrickMesh(1, (8, 8, 8), deform_amp=AMP)
    _refused(fine, pkg.BrickMesh(1, (4, 4, 3), h=2.0, deform_amp=AMP), "twice")             # odd / not half
    _refused(pkg.BrickMesh(1, (8, 8, 7), deform_amp=AMP), pkg.BrickMesh(1, (4, 4, 3), h=2.0, deform_amp=AMP), "twice")
    _refused(fine, pkg.BrickMesh(1, (4, 4, 4), h=1.0, deform_amp=AMP), "size")              # h not doubled
    _refused(fine, pkg.BrickMesh(2, (4, 4, 4), h=2.0, deform_amp=AMP), "degree")
    _refused(fine, pkg.BrickMesh(1, (4, 4, 4), h=2.0, deform_amp=0.0), "deformation")
    _refused(fine, pkg.BrickMesh(1, (4, 4, 4), h=2.0, deform_amp=AMP, rank=0, n_ranks=2), "rank")
    # 20 layers on 8 ranks: rank 2 owns fine layers 5..7, whose parents are split between coarse ranks
    for r in (0, 2):
        _refused(pkg.BrickMesh(1, (4, 4, 20), rank=r, n_ranks=8), pkg.BrickMesh(1, (2, 2, 10), h=2.0, rank=r, n_ranks=8), "slab")
    assert fine.parent_cells(pkg.BrickMesh(1, (4, 4, 4), h=2.0, deform_amp=AMP))[0].shape == (512,)


def _count(V, max_it=300):
    A = V.levels[0]
    b = A.pr.rhs()
    tol = 1e-8 * np.linalg.norm(b)
    x, k, res = R.pcg(A.A, V.vmult, b, max_it, tol=tol)
    assert res <= tol
    return k


COARSE = 10   # a coarse Chebyshev degree at which the p-only count visibly grows with the mesh


def test_hierarchy_spec():
    assert [(q, c) for q, c, _ in H.hierarchy(4, (116, 116, 120))] == [(4, (116, 116, 120)), (2, (116, 116, 120)), (1, (116, 116, 120)),
                                                                        (1, (58, 58, 60)), (1, (29, 29, 30))]
    assert [c for _, c, _ in H.hierarchy(1, (32, 32, 32))] == [(32, 32, 32), (16, 16, 16), (8, 8, 8), (4, 4, 4)]
    assert [h for _, _, h in H.hierarchy(1, (32, 32, 32))] == [1.0, 2.0, 4.0, 8.0]
    assert len(H.hierarchy(1, (32, 32, 32), h_levels=1)) == 2 and len(H.hierarchy(2, (8, 8, 8), h_levels=0)) == 2


@pytest.mark.parametrize("p,sizes", [(2, (8, 16)), (1, (8, 16, 32))])
def test_numpy_hybrid_mg_pcg_iteration_count_is_flat(p, sizes):
    hyb, ponly = [], []
    for n in sizes:
        hyb.append(_count(H.HybridVCycle(p, (n, n, n), deform_amp=AMP, kappa=O.kappa_step64, coarse_degree=COARSE)))
        if n <= 16:
            ponly.append(_count(H.HybridVCycle(p, (n, n, n), deform_amp=AMP, kappa=O.kappa_step64, coarse_degree=COARSE, h_levels=0)))
    assert all(5 <= k <= 7 for k in hyb) and max(hyb) - min(hyb) <= 1, hyb
    assert all(k >= 2 * max(hyb) for k in ponly[-1:]), (ponly, hyb)   # p-only: a fixed coarse polynomial against an h^-2 condition number
    if p == 2:
        assert ponly[1] >= ponly[0] + 3, ponly


def test_hybrid_v_cycle_is_symmetric():
    V = H.HybridVCycle(2, (4, 4, 4), deform_amp=AMP, kappa=O.kappa_step64, min_cells=2)
    assert [(q, c) for q, c, _ in V.spec] == [(2, (4, 4, 4)), (1, (4, 4, 4)), (1, (2, 2, 2))]
    n = V.levels[0].pr.mesh.n_dofs
    rng = np.random.default_rng(3)
    u, v = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    c = V.levels[0].pr.mesh.constrained.astype(np.int64)
    u[c] = v[c] = 0.0
    assert abs(u @ V.vmult(v) - v @ V.vmult(u)) < 1e-12 * abs(u @ V.vmult(u))


def test_geometric_sweeps_equal_the_assembled_kronecker_product():
    T = H.GeometricTransfer((2, 1, 3), 2)
    Px, Py, Pz = T.P1
    P = np.kron(Pz, np.kron(Py, Px))
    rng = np.random.default_rng(10)
    ec, rf = rng.uniform(-1, 1, P.shape[1]), rng.uniform(-1, 1, P.shape[0])
    z = np.where(T.boundary_c, 0.0, 1.0)
    assert np.abs(T.prolongate(ec) - P @ (z * ec)).max() < 1e-14
    assert np.abs(T.restrict(rf) - z * (P.T @ rf)).max() < 1e-13


def test_hybrid_helmholtz_levels_carry_the_mass_term_of_their_mesh():
    """operator="helmholtz": every level, p and h, is step-64's Helmholtz operator on its own mesh (cell size 2^k h: the mass term scales
    as h^3, the gradient term as h), and the hybrid MG-PCG converges in a few iterations"""
    import multigrid_ref as G
    V = H.HybridVCycle(2, (8, 8, 8), deform_amp=AMP, kappa=O.kappa_step64, coarse_degree=10, operator="helmholtz")
    assert [(q, c) for q, c, _ in V.spec] == [(2, (8, 8, 8)), (1, (8, 8, 8)), (1, (4, 4, 4))]
    for (q, c, h), L in zip(V.spec, V.levels):
        ref = G.HelmholtzProblem(q, c, h=h, deform_amp=AMP)
        s = O.deterministic_src(ref.mesh.n_dofs, ref.mesh.constrained, seed=5)
        assert np.linalg.norm(L.A(s) - ref.vmult(s)) < 1e-13 * np.linalg.norm(ref.vmult(s))
        assert np.array_equal(L.inv, 1.0 / ref.diagonal())
    A = V.levels[0]
    b = A.pr.rhs()
    tol = 1e-8 * np.linalg.norm(b)
    x, k, res = R.pcg(A.A, V.vmult, b, 100, tol=tol)
    assert res <= tol and k <= 12, k
