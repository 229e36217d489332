"""Geometric (h) multigrid transfers and PreconditionMG on the hybrid hierarchy (p-levels, then h-levels at degree 1) on the MI355X against
the numpy reference (tests/hmg_ref.py on the oracle's operator), in each mesh's local numbering through global_ids."""
import ctypes as C

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import chebyshev_ref as R
import hmg_ref as H

pkg = bp5_pkg.load()
pytestmark = pytest.mark.gpu
AMP = 0.05
COARSE = 10   # the coarse Chebyshev degree at which the p-only count grows with the mesh (test_hybrid_multigrid_cpu.py)
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


def _op(mesh):
    return pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_STEP64)


def _pair(p, cells_c, **kw):
    fine = _op(pkg.BrickMesh(p, tuple(2 * c for c in cells_c), deform_amp=AMP, **kw))
    coarse = _op(fine.mf_data.mesh.coarsen(min_cells=1))
    assert coarse.mf_data.mesh.cells == tuple(cells_c)
    return fine, coarse


def _transfer_results(fine, coarse, seed):
    nf, nc = int(fine.mf_data.mesh.n_global_dofs), int(coarse.mf_data.mesh.n_global_dofs)
    rng = np.random.default_rng(seed)
    ec, x0, rf, b0 = rng.uniform(-1, 1, nc), rng.uniform(-1, 1, nf), rng.uniform(-1, 1, nf), rng.uniform(-1, 1, nc)
    tr = pkg.MGTwoLevelTransfer(fine, coarse, geometric=True)
    x = _dev(x0, fine)
    tr.prolongate_and_add(x, _dev(ec, coarse))
    b = _dev(b0, coarse)
    tr.restrict_and_add(b, _dev(rf, fine))
    tr.clear()
    return ec, x0, rf, b0, _lex(x, fine, nf) - x0, _lex(b, coarse, nc)


@pytest.mark.parametrize("p,cells_c", [(1, (3, 2, 4)), (2, (2, 3, 2)), (3, (2, 2, 3)), (4, (2, 1, 2))])
def test_geometric_transfer_matches_numpy_and_is_adjoint(p, cells_c):
    fine, coarse = _pair(p, cells_c)
    T = H.GeometricTransfer(cells_c, p)
    ec, x0, rf, b0, pe, got = _transfer_results(fine, coarse, seed=p)
    assert _rel(pe, T.prolongate(ec)) < 1e-13
    bc = T.boundary_c
    ref = T.restrict(rf)
    assert np.array_equal(got[bc], b0[bc])                        # Dirichlet rows unchanged
    assert _rel(got[~bc] - b0[~bc], ref[~bc]) < 1e-13
    lhs, rhs = (got - b0) @ np.where(bc, 0.0, ec), rf @ pe
    assert abs(lhs - rhs) <= 1e-13 * np.abs(rf).sum() * np.abs(ec).max() * 8


@pytest.mark.parametrize("kw", [BRICKS, dict(cell_block=(4, 2, 4)), dict(cell_block=(4, 4, 2), dof_numbering=1)])
def test_brick_and_class_major_meshes_give_the_lexicographic_transfer(kw):
    cells_c = (3, 2, 4)
    lex = _transfer_results(*_pair(1, cells_c), seed=11)
    brk = _transfer_results(*_pair(1, cells_c, **kw), seed=11)
    for a, b in zip(lex, brk):
        assert _rel(b, a) < 1e-14 if np.linalg.norm(a) else np.array_equal(a, b)


def _hybrid(p, cells, h_levels="max", **kw):
    ops = pkg.make_mg_hierarchy(_op(pkg.BrickMesh(p, cells, deform_amp=AMP, **{k: v for k, v in kw.items() if k != "variant"})),
                                h_levels=h_levels)
    if "variant" in kw:
        for o in ops:
            o.mf_data.set_apply_variant(kw["variant"])
    return ops


def test_make_mg_hierarchy_h_levels():
    assert [o.mf_data.mesh.degree for o in _hybrid(4, (8, 8, 8), h_levels=0)] == [4, 2, 1]            # the default: p-levels only
    assert [o.mf_data.mesh.degree for o in pkg.make_mg_hierarchy(_op(pkg.BrickMesh(4, (8, 8, 8))))] == [4, 2, 1]
    ops = _hybrid(2, (16, 16, 16))
    assert [(o.mf_data.mesh.degree, o.mf_data.mesh.cells, o.mf_data.mesh.h) for o in ops] == \
        [(2, (16, 16, 16), 1.0), (1, (16, 16, 16), 1.0), (1, (8, 8, 8), 2.0), (1, (4, 4, 4), 4.0)]
    assert len(_hybrid(1, (16, 16, 16), h_levels=1)) == 2
    assert len(_hybrid(1, (16, 16, 16), h_levels=5)) == 3
    with pytest.raises(pkg.BP5Error):
        pkg.make_mg_hierarchy(_op(pkg.BrickMesh(1, (8, 8, 8))), h_levels="all")


@pytest.mark.parametrize("p,cells", [(1, (8, 8, 8)), (2, (8, 8, 8)), (3, (8, 8, 8)), (4, (8, 8, 8))])
def test_hybrid_v_cycle_and_level_bounds_match_numpy(p, cells):
    ops = _hybrid(p, cells)
    mg = pkg.PreconditionMG(ops, pkg.PreconditionMG.AdditionalData(coarse_degree=COARSE))
    V = H.HybridVCycle(p, cells, deform_amp=AMP, kappa=O.kappa_step64, coarse_degree=COARSE)
    info = mg.level_info()
    assert [(d["degree"], d["cells"]) for d in info] == [(q, c) for q, c, _ in V.spec]
    assert [t.geometric for t in mg.transfers] == [q == r for (q, _, _), (r, _, _) in zip(V.spec[:-1], V.spec[1:])]
    for d, L in zip(info, V.levels):
        assert d["cg_its"] == L.cg_its and d["chebyshev_degree"] == L.degree
        for k in ("min_est", "max_est", "min_used", "max_used"):
            assert abs(d[k] - getattr(L, k)) <= 1e-10 * abs(getattr(L, k)), (k, d[k], getattr(L, k))
    n = V.levels[0].pr.mesh.n_dofs
    s = O.deterministic_src(n, V.levels[0].pr.mesh.constrained, seed=41)
    dst = ops[0].initialize_dof_vector()
    dst.fill_(float("nan"))
    mg.vmult(dst, _dev(s, ops[0]))
    assert _rel(_lex(dst, ops[0], n), V.vmult(s)) < 1e-11
    mg.clear()


def _solve(ops, mg, tol_rel=1e-8, b=None):
    b = ops[0].assemble_rhs() if b is None else b
    tol = tol_rel * float(_t().linalg.norm(b[:ops[0].mf_data.n_owned]))
    x = ops[0].initialize_dof_vector()
    ctl = pkg.SolverControl(300, tol)
    pkg.SolverCG(ctl).solve(ops[0], x, b, mg)
    return x, ctl


@pytest.mark.parametrize("p,cells", [(1, (16, 16, 16)), (2, (8, 8, 8)), (4, (8, 8, 8))])
def test_hybrid_mg_pcg_converges_in_the_numpy_count(p, cells):
    ops = _hybrid(p, cells)
    assert len(ops) > len(pkg.mg_coarse_degrees(p))          # p = 1 too: real levels below the fine mesh
    mg = pkg.PreconditionMG(ops, pkg.PreconditionMG.AdditionalData(coarse_degree=COARSE))
    x, ctl = _solve(ops, mg)
    V = H.HybridVCycle(p, cells, deform_amp=AMP, kappa=O.kappa_step64, coarse_degree=COARSE)
    A = V.levels[0]
    b = A.pr.rhs()
    x_ref, k_ref, _ = R.pcg(A.A, V.vmult, b, 300, tol=1e-8 * np.linalg.norm(b))
    assert abs(ctl.last_step() - k_ref) <= 1, (ctl.last_step(), k_ref)
    assert ctl.last_value() <= ctl.tolerance
    assert _rel(_lex(x, ops[0], A.pr.mesh.n_dofs), x_ref) < 1e-7
    mg.clear()


def test_hybrid_count_is_flat_where_the_p_only_count_grows():
    counts = {}
    for n in (8, 16):
        for h in ("max", 0):
            ops = _hybrid(2, (n, n, n), h_levels=h)
            mg = pkg.PreconditionMG(ops, pkg.PreconditionMG.AdditionalData(coarse_degree=COARSE))
            counts[n, h] = _solve(ops, mg)[1].last_step()
            mg.clear()
    assert abs(counts[16, "max"] - counts[8, "max"]) <= 1, counts
    assert counts[16, 0] >= counts[8, 0] + 3 and counts[16, 0] > counts[16, "max"] + 3, counts


def test_two_hybrid_solves_are_bitwise_identical():
    ops = _hybrid(4, (8, 8, 8), variant=56, **BRICKS)
    mg = pkg.PreconditionMG(ops, pkg.PreconditionMG.AdditionalData(coarse_degree=COARSE))
    b = ops[0].assemble_rhs()
    x1, c1 = _solve(ops, mg, b=b)
    x2, c2 = _solve(ops, mg, b=b)
    assert c1.last_step() == c2.last_step()
    assert _t().equal(x1, x2)
    mg.clear()


def _create(fine, coarse, parent, child):
    h = C.c_void_p()
    st = pkg.lib().bp5_mg_transfer_create_geometric(fine.mf_data.handle, coarse.mf_data.handle, np.ascontiguousarray(parent, np.uint32).ctypes.data,
                                                    np.ascontiguousarray(child, np.uint8).ctypes.data, C.byref(h))
    msg = pkg.lib().bp5_last_error().decode()
    if st == 0:
        pkg.lib().bp5_mg_transfer_destroy(h)
    return st, msg


def test_refusals():
    fine, coarse = _pair(1, (2, 2, 2))
    parent, child = fine.mf_data.mesh.parent_cells(coarse.mf_data.mesh)
    assert _create(fine, coarse, parent, child)[0] == 0
    bad = parent.copy()
    bad[3] = coarse.mf_data.mesh.n_cells                    # not a local coarse cell
    st, msg = _create(fine, coarse, bad, child)
    assert st == 1 and "local coarse cell" in msg, msg
    ch = child.copy()
    ch[np.nonzero(parent == 0)[0][:2]] = 5                  # two children of one code
    st, msg = _create(fine, coarse, parent, ch)
    assert st == 1 and "child" in msg, msg
    # two children of the same code in different parents swapped: counts fine, corners wrong
    k0 = np.nonzero((parent == 0) & (child == 0))[0][0]
    k1 = np.nonzero((parent == 1) & (child == 0))[0][0]
    sw = parent.copy()
    sw[k0], sw[k1] = parent[k1], parent[k0]
    st, msg = _create(fine, coarse, sw, child)
    assert st == 1 and "corner" in msg, msg
    # a coarse mesh of other coordinates: the parent map fits the cells, not the geometry
    other = _op(pkg.BrickMesh(1, (2, 2, 2), h=2.5, deform_amp=AMP))
    st, msg = _create(fine, other, parent, child)
    assert st == 1 and "corner" in msg, msg
    # degree 5
    f5 = _op(pkg.BrickMesh(5, (2, 2, 2)))
    c5 = _op(f5.mf_data.mesh.coarsen(min_cells=1))
    with pytest.raises(pkg.BP5Error) as e:
        pkg.MGTwoLevelTransfer(f5, c5, geometric=True)
    assert e.value.status == 1 and "1..4" in str(e.value)
    # the p-transfer still refuses equal degrees
    with pytest.raises(pkg.BP5Error):
        pkg.MGTwoLevelTransfer(fine, coarse)


def test_hanging_node_handle_is_refused():
    from types import SimpleNamespace

    def ns(m):
        return SimpleNamespace(degree=m.p, n=m.n, n_cells=m.n_cells, n_interior_cells=m.n_cells, n_owned=m.n_dofs, n_ghost=0, n_local=m.n_dofs,
                               n_global_dofs=m.n_dofs, l2g=m.l2g, coords=m.coords, constrained=m.constrained, n_neighbors=0,
                               neighbor_rank=np.zeros(0, np.int32), send_offsets=np.zeros(1, np.uint32), send_indices=np.zeros(0, np.uint32),
                               recv_offsets=np.zeros(1, np.uint32), cell_block_offsets=None, constraint_mask=m.constraint_mask, rank=0, n_ranks=1)
    fine = pkg.PoissonOperator(ns(O.HangingBrickMesh(1, 2, 2, 1, 3)), pkg.QUAD_GAUSS)
    coarse = _op(pkg.BrickMesh(1, (1, 1, 1)))
    n = fine.mf_data.mesh.n_cells
    st, msg = _create(fine, coarse, np.zeros(n, np.uint32), np.arange(n, dtype=np.uint8) % 8)
    assert st == 1 and "hanging" in msg, msg


def test_facade_example_with_h_levels_matches_the_python_solve():
    """examples/bp5_multigrid with its last argument h_levels: the facade's PreconditionMG takes the parent maps of the equal-degree pairs
    from bp5_mesh_parent_cells and reports the iteration count, the level bounds and the solution norm of the Python solve"""
    import os
    import subprocess
    torch = _t()
    exe = os.path.join(bp5_pkg.ROOT, "examples", "bp5_multigrid")
    txt = subprocess.run([exe, "2", "8", "8", "8", "0.05", "1e-8", "1", "2"], capture_output=True, text=True, timeout=300, check=True).stdout
    got = {l.split()[0]: l.split()[1:] for l in txt.splitlines() if l.strip()}
    ops = pkg.make_mg_hierarchy(pkg.PoissonOperator(pkg.BrickMesh(2, (8, 8, 8), deform_amp=0.05), pkg.QUAD_GAUSS, pkg.COEF_STEP64), h_levels=2)
    assert [o.mf_data.mesh.cells for o in ops] == [(8, 8, 8), (8, 8, 8), (4, 4, 4)]
    mg = pkg.PreconditionMG(ops)
    x, ctl = _solve(ops, mg)
    assert int(got["iterations"][0]) == ctl.last_step()
    for lev, d in enumerate(mg.level_info()):
        row = got[f"level{lev}"]
        assert int(row[0]) == d["degree"] and int(row[1]) == d["n_owned"]
        assert abs(float(row[3]) - d["max_used"]) <= 1e-12 * d["max_used"]
    assert f"level{len(ops)}" not in got
    xn = float(torch.linalg.norm(x[:ops[0].mf_data.n_owned]))
    assert abs(float(got["solution_norm"][0]) - xn) <= 1e-10 * xn, (got, xn)
    mg.clear()
