"""PreconditionChebyshev and PreconditionMG on the setups they accept besides the Poisson operator on a conforming, six-plane,
generator-numbered BrickMesh, each against the numpy references (tests/chebyshev_ref.py, tests/multigrid_ref.py, tests/hmg_ref.py on the
oracle's operators): partly filled last workgroups of the transfer kernels, the affine geometry mode, the Helmholtz operator,
interior-first and external numberings, hanging-node meshes (Chebyshev only: the multigrid transfers refuse them)."""
from types import SimpleNamespace

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import chebyshev_ref as R
import hmg_ref as H
import multigrid_ref as G

pkg = bp5_pkg.load()
pytestmark = pytest.mark.gpu
Cheb = pkg.PreconditionChebyshev
AMP = 0.05
COARSE = 10
BRICKS = dict(cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1)


def _t():
    import torch
    return torch


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _perm(op):
    m = op.mf_data.mesh
    return m.global_ids[:m.n_owned].astype(np.int64)


def _dev(v_lex, op):
    torch = _t()
    x = op.initialize_dof_vector()
    x[:op.mf_data.n_owned] = torch.from_numpy(np.ascontiguousarray(v_lex[_perm(op)])).to(x.device)
    return x


def _lex(x, op, n):
    out = np.zeros(n)
    out[_perm(op)] = x[:op.mf_data.n_owned].cpu().numpy()
    return out


def _op(mesh, **kw):
    return pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_STEP64, **kw)


def _check_transfer(fine, coarse, T, geometric, seed):
    """prolongate_and_add / restrict_and_add against the numpy transfer T: 1e-13, Dirichlet rows unchanged, adjoint"""
    nf, nc = int(fine.mf_data.mesh.n_global_dofs), int(coarse.mf_data.mesh.n_global_dofs)
    rng = np.random.default_rng(seed)
    ec, x0, rf, b0 = rng.uniform(-1, 1, nc), rng.uniform(-1, 1, nf), rng.uniform(-1, 1, nf), rng.uniform(-1, 1, nc)
    tr = pkg.MGTwoLevelTransfer(fine, coarse, geometric=geometric)
    x = _dev(x0, fine)
    tr.prolongate_and_add(x, _dev(ec, coarse))
    b = _dev(b0, coarse)
    tr.restrict_and_add(b, _dev(rf, fine))
    tr.clear()
    pe, got = _lex(x, fine, nf) - x0, _lex(b, coarse, nc)
    assert _rel(pe, T.prolongate(ec)) < 1e-13
    bc = T.boundary_c
    assert np.array_equal(got[bc], b0[bc])
    assert _rel(got[~bc] - b0[~bc], T.restrict(rf)[~bc]) < 1e-13
    lhs, rhs = (got - b0) @ np.where(bc, 0.0, ec), rf @ pe
    assert abs(lhs - rhs) <= 1e-13 * np.abs(rf).sum() * np.abs(ec).max() * 8
    return pe, got - b0


def _v_cycle(mg, op0, V, seed=41):
    n = V.levels[0].pr.mesh.n_dofs
    s = O.deterministic_src(n, V.levels[0].pr.mesh.constrained, seed=seed)
    dst = op0.initialize_dof_vector()
    dst.fill_(float("nan"))
    mg.vmult(dst, _dev(s, op0))
    return _lex(dst, op0, n), V.vmult(s)


def _check_levels(mg, V):
    for d, L in zip(mg.level_info(), V.levels):
        assert d["degree"] == L.pr.mesh.p and d["cg_its"] == L.cg_its and d["chebyshev_degree"] == L.degree
        for k in ("min_est", "max_est", "min_used", "max_used"):
            assert abs(d[k] - getattr(L, k)) <= 1e-10 * abs(getattr(L, k)), (k, d[k], getattr(L, k))


# ---------------------------------------------------------------------------------------------------- partly filled last workgroups
# MgShape<NF, NC>::CPB cells per transfer workgroup: 2 for p 4 -> 2 (125 fine nodes per cell), 32 for geometric p = 1 (8).  Geometric
# p = 4 has CPB 2 too, but its fine mesh has 8 cells per coarse cell: an even count, so its last workgroup is always full.

def test_p4_to_p2_transfer_and_v_cycle_with_an_odd_cell_count():
    cells = (3, 3, 3)                                                # 27 cells: the last workgroup holds one
    ops = pkg.make_mg_hierarchy(_op(pkg.BrickMesh(4, cells, deform_amp=AMP)))
    _check_transfer(ops[0], ops[1], G.Transfer(cells, 4, 2), False, seed=1)
    mg = pkg.PreconditionMG(ops, pkg.PreconditionMG.AdditionalData(coarse_degree=COARSE))
    got, ref = _v_cycle(mg, ops[0], G.VCycle(4, cells, deform_amp=AMP, kappa=O.kappa_step64, coarse_degree=COARSE))
    assert _rel(got, ref) < 1e-11
    mg.clear()


def test_geometric_p1_transfer_and_v_cycle_with_a_partial_last_workgroup():
    cells_c, cells = (3, 2, 3), (6, 4, 6)                            # 144 fine cells = 4 x 32 + 16
    assert np.prod(cells) % 32 == 16
    ops = pkg.make_mg_hierarchy(_op(pkg.BrickMesh(1, cells, deform_amp=AMP)), h_levels="max", min_cells=1)
    assert [o.mf_data.mesh.cells for o in ops] == [cells, cells_c]
    _check_transfer(ops[0], ops[1], H.GeometricTransfer(cells_c, 1), True, seed=2)
    mg = pkg.PreconditionMG(ops, pkg.PreconditionMG.AdditionalData(coarse_degree=COARSE))
    V = H.HybridVCycle(1, cells, deform_amp=AMP, kappa=O.kappa_step64, min_cells=1, coarse_degree=COARSE)
    got, ref = _v_cycle(mg, ops[0], V)
    assert _rel(got, ref) < 1e-11
    mg.clear()


# ---------------------------------------------------------------------------------------------------- affine geometry mode (coef NULL)
@pytest.mark.parametrize("p,variant,kw", [(4, 10, {}), (4, 56, BRICKS), (2, 0, {})])
def test_chebyshev_on_the_affine_geometry_mode(p, variant, kw):
    """bp5_chebyshev_create without a metric (BP5_GEOM_AFFINE): the CG-Lanczos estimate, vmult / step at fixed bounds and Chebyshev-PCG
    at a fixed iteration count against numpy"""
    torch = _t()
    cells = (8, 5, 4) if kw else (4, 3, 3)
    pr = O.Problem(p, cells, 0, h=0.25, kappa=O.kappa_step64)
    mesh = pkg.BrickMesh(p, cells, h=0.25, **kw)
    op = _op(mesh, geometry=pkg.GEOM_AFFINE)
    op.mf_data.set_apply_variant(variant)
    assert op.coef is None
    perm = mesh.global_ids.astype(np.int64)

    def A(v):                                                        # the oracle operator in the mesh's own numbering
        full = np.zeros(v.size)
        full[perm] = v
        return pr.vmult(full)[perm]

    inv = op.compute_diagonal(invert=True)
    inv_ref = (1.0 / O.operator_diagonal(pr.mesh, pr.coef, pr.N, pr.D))[perm]
    assert _rel(inv.cpu().numpy(), inv_ref) < 1e-13
    ch = Cheb().initialize(op, Cheb.AdditionalData(degree=4, smoothing_range=20.0, preconditioner=pkg.DiagonalMatrix(inv)))
    e = ch.estimated_eigenvalues()
    lo, hi, k = R.lanczos_estimate(A, inv_ref, R.start_vector(mesh.global_ids, mesh.constrained), 8)
    mu, Mu = R.bounds(lo, hi, 20.0)
    assert e["cg_its"] == k
    for key, val in (("min_est", lo), ("max_est", hi), ("min_used", mu), ("max_used", Mu)):
        assert abs(e[key] - val) <= 1e-10 * val, (key, e[key], val)
    n = mesh.n_owned
    src, x0 = O.deterministic_src(n, seed=5), O.deterministic_src(n, seed=6)
    fixed = Cheb().initialize(op, Cheb.AdditionalData(degree=3, max_eigenvalue=2.1, min_eigenvalue=0.15, preconditioner=pkg.DiagonalMatrix(inv)))
    s = op.initialize_dof_vector()
    s[:n] = torch.from_numpy(src)
    d = op.initialize_dof_vector()
    d.fill_(7.0)
    fixed.vmult(d, s)
    assert _rel(d.cpu().numpy(), R.vmult(A, inv_ref, src, 0.15, 2.1, 3)) < 1e-12
    x = op.initialize_dof_vector()
    x[:n] = torch.from_numpy(x0)
    fixed.step(x, s)
    assert _rel(x.cpu().numpy(), R.step(A, inv_ref, x0, src, 0.15, 2.1, 3)) < 1e-12
    b = op.assemble_rhs()
    x = op.initialize_dof_vector()
    ctl = pkg.IterationNumberControl(12, 0.0)
    pkg.SolverCG(ctl).solve(op, x, b, ch)
    xr, kr, res = R.pcg(A, lambda g: R.vmult(A, inv_ref, g, mu, Mu, 4), pr.rhs()[perm], 12)
    assert ctl.last_step() == kr == 12
    assert _rel(x.cpu().numpy(), xr) < 1e-11
    assert abs(ctl.last_value() - res) <= 1e-9 * res


@pytest.mark.parametrize("p,cells,kw,variant,h_levels", [(2, (8, 8, 8), {}, None, 0), (2, (8, 8, 8), {}, None, "max"),
                                                         (4, (4, 3, 4), {}, 10, 0), (4, (8, 8, 8), BRICKS, 56, "max"),
                                                         (6, (2, 2, 3), {}, None, 0)])
def test_affine_mg_hierarchy_matches_numpy_and_the_six_plane_hierarchy(p, cells, kw, variant, h_levels):
    """make_mg_hierarchy of an affine-mode operator gives affine-mode levels (no metric array: coef None), bp5_mg_create takes them
    without one, and the V-cycle is numpy's (p-only and hybrid) at 1e-11 and the six-plane hierarchy's at 1e-12.  The fine level runs
    the team (10) or block (56) kernel at p = 4"""
    outs = []
    for geometry in (pkg.GEOM_AFFINE, pkg.GEOM_MERGED6):
        fine = _op(pkg.BrickMesh(p, cells, **kw), geometry=geometry)
        if variant is not None:
            fine.mf_data.set_apply_variant(variant)
        ops = pkg.make_mg_hierarchy(fine, h_levels=h_levels)
        assert all((o.coef is None) == (geometry == pkg.GEOM_AFFINE) for o in ops)
        assert all(o.geometry == geometry for o in ops)
        mg = pkg.PreconditionMG(ops, pkg.PreconditionMG.AdditionalData(coarse_degree=COARSE))
        V = H.HybridVCycle(p, cells, kappa=O.kappa_step64, h_levels=h_levels, coarse_degree=COARSE)
        assert [(d["degree"], d["cells"]) for d in mg.level_info()] == [(q, c) for q, c, _ in V.spec]
        got, ref = _v_cycle(mg, ops[0], V)
        if geometry == pkg.GEOM_AFFINE:
            _check_levels(mg, V)
            assert _rel(got, ref) < 1e-11
        outs.append(got)
        mg.clear()
    assert _rel(outs[0], outs[1]) < 1e-12


# ---------------------------------------------------------------------------------------------------- Helmholtz operator
def test_chebyshev_estimate_and_pcg_on_the_helmholtz_operator():
    p, cells = 3, (3, 3, 2)
    hp = G.HelmholtzProblem(p, cells, 0, h=0.25, deform_amp=0.04)
    mesh = pkg.BrickMesh(p, cells, h=0.25, deform_amp=0.04)
    op = pkg.HelmholtzOperator(mesh, 0, pkg.COEF_STEP64)
    inv = op.compute_diagonal(invert=True)
    inv_ref = 1.0 / hp.diagonal()
    assert _rel(inv.cpu().numpy(), inv_ref) < 1e-13
    ch = Cheb().initialize(op, Cheb.AdditionalData(degree=4, smoothing_range=20.0, eig_cg_n_iterations=10, preconditioner=pkg.DiagonalMatrix(inv)))
    e = ch.estimated_eigenvalues()
    lo, hi, k = R.lanczos_estimate(hp.vmult, inv_ref, R.start_vector(mesh.global_ids, mesh.constrained), 10)
    mu, Mu = R.bounds(lo, hi, 20.0)
    assert e["cg_its"] == k
    for key, val in (("min_est", lo), ("max_est", hi), ("min_used", mu), ("max_used", Mu)):
        assert abs(e[key] - val) <= 1e-10 * val, (key, e[key], val)
    b = op.assemble_rhs()
    x = op.initialize_dof_vector()
    ctl = pkg.IterationNumberControl(12, 0.0)
    pkg.SolverCG(ctl).solve(op, x, b, ch)
    xr, kr, res = R.pcg(hp.vmult, lambda g: R.vmult(hp.vmult, inv_ref, g, mu, Mu, 4), hp.rhs(), 12)
    assert ctl.last_step() == kr == 12
    assert _rel(x.cpu().numpy(), xr) < 1e-11
    assert abs(ctl.last_value() - res) <= 1e-9 * res


@pytest.mark.parametrize("p,cells,h_levels", [(4, (4, 4, 4), 0), (2, (8, 8, 8), "max")])
def test_helmholtz_mg_hierarchy_matches_numpy(p, cells, h_levels):
    """make_mg_hierarchy(HelmholtzOperator) yields Helmholtz levels (seven planes: the mass term on every p- and h-level); their bounds,
    the V-cycle and the MG-PCG count and solution are numpy's"""
    torch = _t()
    fine = pkg.HelmholtzOperator(pkg.BrickMesh(p, cells, deform_amp=AMP), pkg.QUAD_GAUSS, pkg.COEF_STEP64)
    ops = pkg.make_mg_hierarchy(fine, h_levels=h_levels)
    assert all(type(o) is pkg.HelmholtzOperator for o in ops)
    assert all(o.mf_data.coef_size() == 7 * o.mf_data.mesh.n_cells * (o.mf_data.mesh.degree + 1) ** 3 for o in ops)
    mg = pkg.PreconditionMG(ops, pkg.PreconditionMG.AdditionalData(coarse_degree=COARSE))
    V = H.HybridVCycle(p, cells, deform_amp=AMP, kappa=O.kappa_step64, h_levels=h_levels, coarse_degree=COARSE, operator="helmholtz")
    assert [(d["degree"], d["cells"]) for d in mg.level_info()] == [(q, c) for q, c, _ in V.spec]
    _check_levels(mg, V)
    got, ref = _v_cycle(mg, ops[0], V)
    assert _rel(got, ref) < 1e-11
    b = fine.assemble_rhs()
    x = fine.initialize_dof_vector()
    ctl = pkg.SolverControl(100, 1e-8 * float(torch.linalg.norm(b[:fine.mf_data.n_owned])))
    pkg.SolverCG(ctl).solve(fine, x, b, mg)
    A = V.levels[0]
    b_ref = A.pr.rhs()
    x_ref, k_ref, _ = R.pcg(A.A, V.vmult, b_ref, 100, tol=1e-8 * np.linalg.norm(b_ref))
    assert abs(ctl.last_step() - k_ref) <= 1, (ctl.last_step(), k_ref)
    assert _rel(_lex(x, fine, A.pr.mesh.n_dofs), x_ref) < 1e-7
    mg.clear()


# ---------------------------------------------------------------------------------------------------- other numberings
def test_interior_first_numbering_gives_the_lexicographic_transfers_and_v_cycle():
    """dof_numbering = 2 (the DoFs inside a cell first, cell by cell): p 4 -> 2 and geometric p = 1 transfers and the hybrid V-cycle give
    the lexicographic mesh's results"""
    cells = (3, 3, 3)
    res = []
    for numbering in (0, 2):
        f, c = _op(pkg.BrickMesh(4, cells, deform_amp=AMP, dof_numbering=numbering)), _op(pkg.BrickMesh(2, cells, deform_amp=AMP, dof_numbering=numbering))
        assert f.mf_data.mesh.dof_numbering == numbering
        res.append(_check_transfer(f, c, G.Transfer(cells, 4, 2), False, seed=7))
        f = _op(pkg.BrickMesh(1, (6, 4, 6), deform_amp=AMP, dof_numbering=numbering))
        c = _op(f.mf_data.mesh.coarsen(min_cells=1))
        res.append(_check_transfer(f, c, H.GeometricTransfer((3, 2, 3), 1), True, seed=8))
        ops = pkg.make_mg_hierarchy(_op(pkg.BrickMesh(2, (8, 8, 8), deform_amp=AMP, dof_numbering=numbering)), h_levels="max")
        assert [o.mf_data.mesh.dof_numbering for o in ops] == [numbering] * 3
        mg = pkg.PreconditionMG(ops, pkg.PreconditionMG.AdditionalData(coarse_degree=COARSE))
        got, ref = _v_cycle(mg, ops[0], H.HybridVCycle(2, (8, 8, 8), deform_amp=AMP, kappa=O.kappa_step64, coarse_degree=COARSE))
        assert _rel(got, ref) < 1e-11
        res.append((got,))
        mg.clear()
    for a, b in zip(res[:3], res[3:]):
        for u, v in zip(a, b):
            assert _rel(v, u) < 1e-12


def _external(p, cells, h, cperm, rng):
    """the oracle's mesh handed over as an external mesh: cells in the order cperm (new cell k = old cell cperm[k]), DoFs in a random
    numbering; global_ids give the oracle's (lexicographic) id of every DoF"""
    om = O.BrickMesh(p, cells, h=h, deform_amp=AMP)
    new_of_old = rng.permutation(om.n_dofs).astype(np.int64)
    old_of_new = np.argsort(new_of_old)
    n = om.n_dofs
    return SimpleNamespace(degree=p, n=p + 1, cells=tuple(cells), n_cells=om.n_cells, n_interior_cells=om.n_cells, n_owned=n, n_ghost=0,
                           n_local=n, n_global_dofs=n, l2g=new_of_old[om.l2g.astype(np.int64)[cperm]].astype(np.uint32),
                           coords=np.ascontiguousarray(om.coords[old_of_new]), global_ids=old_of_new.astype(np.uint64),
                           constrained=np.sort(new_of_old[om.constrained.astype(np.int64)]).astype(np.uint32), n_neighbors=0,
                           neighbor_rank=np.zeros(0, np.int32), send_offsets=np.zeros(1, np.uint32), send_indices=np.zeros(0, np.uint32),
                           recv_offsets=np.zeros(1, np.uint32), cell_block_offsets=None, rank=0, n_ranks=1, h=h, deform_amp=AMP)


def _attach_parent_map(fine, coarse, cperm_f, cperm_c):
    """parent_cells of the randomly ordered 2:1 pair (what BrickMesh.parent_cells gives for the generator's meshes), by hand: the
    lexicographic parent and child position of every fine cell, through both cell permutations"""
    n0, n1, _ = fine.cells
    old = np.asarray(cperm_f, np.int64)
    cx, cy, cz = old % n0, (old // n0) % n1, old // (n0 * n1)
    parent_old = cx // 2 + (n0 // 2) * (cy // 2 + (n1 // 2) * (cz // 2))
    new_of_old_c = np.argsort(cperm_c)
    parent = new_of_old_c[parent_old].astype(np.uint32)
    child = ((cx % 2) | (cy % 2) << 1 | (cz % 2) << 2).astype(np.uint8)
    fine.parent_cells = lambda c: (parent, child)


def test_externally_numbered_meshes_give_the_numpy_transfers_and_v_cycle():
    """random cell order and random DoF numbering on every level (the p-levels share their cell order, which the p-transfer needs; the
    h-level has its own, linked by the parent map): the transfers' writer masks and slot tables come from such l2g arrays too"""
    rng = np.random.default_rng(12)
    cells, cells_c = (4, 4, 4), (2, 2, 2)
    cperm = rng.permutation(64)
    cperm_c = rng.permutation(8)
    meshes = [_external(2, cells, 1.0, cperm, rng), _external(1, cells, 1.0, cperm, rng), _external(1, cells_c, 2.0, cperm_c, rng)]
    _attach_parent_map(meshes[1], meshes[2], cperm, cperm_c)
    ops = [_op(m) for m in meshes]
    _check_transfer(ops[0], ops[1], G.Transfer(cells, 2, 1), False, seed=13)
    _check_transfer(ops[1], ops[2], H.GeometricTransfer(cells_c, 1), True, seed=14)
    mg = pkg.PreconditionMG(ops, pkg.PreconditionMG.AdditionalData(coarse_degree=COARSE))
    V = H.HybridVCycle(2, cells, deform_amp=AMP, kappa=O.kappa_step64, min_cells=2, coarse_degree=COARSE)
    assert [(d["degree"], d["cells"]) for d in mg.level_info()] == [(q, c) for q, c, _ in V.spec]
    _check_levels(mg, V)
    got, ref = _v_cycle(mg, ops[0], V)
    assert _rel(got, ref) < 1e-11
    mg.clear()


# ---------------------------------------------------------------------------------------------------- hanging nodes (Chebyshev)
def _hanging_mesh(kind):
    if kind == "planar":
        return O.HangingBrickMesh(2, 2, 2, 1, 3, H=1.0, deform_amp=0.03)
    r = np.zeros((2, 2, 3), bool)                                    # staircase: one, two, three constrained faces and edges
    r[0, 0, 0] = r[0, 0, 1] = r[0, 1, 0] = r[1, 0, 0] = r[1, 1, 2] = True
    return O.RefinedBrickMesh(2, (3, 2, 2), r, H=0.5, deform_amp=0.03)


@pytest.mark.parametrize("kind", ["planar", "general"])
@pytest.mark.parametrize("variant", [90, 56])
def test_chebyshev_pcg_on_hanging_node_meshes(kind, variant):
    """Chebyshev(4)-PCG with the Jacobi inner preconditioner, 10 iterations, on a hanging-node handle: the pencil kernel (90) on the mesh
    as generated, the block kernel (56) on it in cell groups and block-major numbering; against chebyshev_ref on the oracle's hanging
    operator (estimate and iterate)"""
    from test_gpu_parity import _hanging_namespace, _with_cell_blocks
    m = _hanging_mesh(kind)
    _, _, w, N, D = O.shape_tables(m.p, 0)
    coef = O.merged_metric(m, N, D, w, O.kappa_step64)

    def A(s):
        return O.vmult(m, coef, N, D, s)

    inv_ref = 1.0 / O.operator_diagonal(m, coef, N, D)
    if variant == 90:
        ns, old_of_new = _hanging_namespace(m), np.arange(m.n_dofs)
    else:
        ns, new_of_old = _with_cell_blocks(m, 4)
        old_of_new = np.argsort(new_of_old)
    ns.global_ids = old_of_new.astype(np.uint64)                    # the Lanczos start vector follows the oracle's DoF ids
    op = _op(ns)
    op.mf_data.set_apply_variant(variant)
    inv = op.compute_diagonal(invert=True)
    assert _rel(inv.cpu().numpy(), inv_ref[old_of_new]) < 1e-13
    ch = Cheb().initialize(op, Cheb.AdditionalData(degree=4, smoothing_range=20.0, preconditioner=pkg.DiagonalMatrix(inv)))
    e = ch.estimated_eigenvalues()
    lo, hi, k = R.lanczos_estimate(A, inv_ref, R.start_vector(np.arange(m.n_dofs), m.constrained), 8)
    mu, Mu = R.bounds(lo, hi, 20.0)
    assert e["cg_its"] == k and abs(e["max_est"] - hi) <= 1e-10 * hi and abs(e["min_est"] - lo) <= 1e-10 * lo, (e, lo, hi)
    b = op.assemble_rhs()
    x = op.initialize_dof_vector()
    ctl = pkg.IterationNumberControl(10, 0.0)
    pkg.SolverCG(ctl).solve(op, x, b, ch)
    xr, kr, res = R.pcg(A, lambda g: R.vmult(A, inv_ref, g, mu, Mu, 4), O.assemble_rhs(m), 10)
    assert ctl.last_step() == kr == 10
    assert _rel(x.cpu().numpy(), xr[old_of_new]) < 1e-11
    assert abs(ctl.last_value() - res) <= 1e-9 * res
