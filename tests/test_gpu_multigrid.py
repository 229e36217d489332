"""PreconditionMG (p-multigrid V-cycle with Chebyshev smoothers) and its transfer on the MI355X against the numpy reference
(tests/multigrid_ref.py on the oracle's operator), in each mesh's local numbering through global_ids."""
import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import chebyshev_ref as R
import multigrid_ref as G

pkg = bp5_pkg.load()
pytestmark = pytest.mark.gpu
AMP = 0.05


def _t():
    import torch
    return torch


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _hierarchy(p, cells, quad=pkg.QUAD_GAUSS, block=None, variant=None):
    """GPU operators fine to coarse on one mesh family (lexicographic, or brick-ordered block-major with the block kernel)"""
    kw = dict(deform_amp=AMP)
    if block is not None:
        kw.update(cell_block=block, dof_numbering=1, cell_block_order=1)
    fine = pkg.PoissonOperator(pkg.BrickMesh(p, cells, **kw), quad, pkg.COEF_STEP64)
    ops = pkg.make_mg_hierarchy(fine)
    if variant is not None:
        for o in ops:
            o.mf_data.set_apply_variant(variant)
    return ops


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


@pytest.mark.parametrize("p,quad", [(2, 0), (3, 1), (4, 0), (4, 1), (5, 0), (6, 1), (7, 0), (8, 0), (8, 1)])
def test_transfer_matches_numpy_and_is_adjoint(p, quad):
    cells = (3, 2, 4) if p <= 4 else (2, 2, 3)
    ops = _hierarchy(p, cells, quad)
    fine, coarse = ops[0], ops[1]
    T = G.Transfer(cells, p)
    nf, nc = int(fine.mf_data.mesh.n_global_dofs), int(coarse.mf_data.mesh.n_global_dofs)
    tr = pkg.MGTwoLevelTransfer(fine, coarse)
    rng = np.random.default_rng(p)
    ec, x0 = rng.uniform(-1, 1, nc), rng.uniform(-1, 1, nf)      # non-zero on the boundary too: Dirichlet DoFs count as 0
    rf, b0 = rng.uniform(-1, 1, nf), rng.uniform(-1, 1, nc)
    x = _dev(x0, fine)
    tr.prolongate_and_add(x, _dev(ec, coarse))
    pe = _lex(x, fine, nf) - x0
    assert _rel(pe, T.prolongate(ec)) < 1e-13
    b = _dev(b0, coarse)
    tr.restrict_and_add(b, _dev(rf, fine))
    got = _lex(b, coarse, nc)
    ref = T.restrict(rf)
    bc = T.boundary_c
    assert np.array_equal(got[bc], b0[bc])                        # Dirichlet rows unchanged
    assert _rel(got[~bc] - b0[~bc], ref[~bc]) < 1e-13
    # <R r, e> = <r, P e> with the device's own results
    lhs, rhs = (got - b0) @ np.where(bc, 0.0, ec), rf @ pe
    assert abs(lhs - rhs) <= 1e-13 * np.abs(rf).sum() * np.abs(ec).max() * 8
    tr.clear()


def _vcycle_case(p, cells, quad=pkg.QUAD_GAUSS, **kw):
    ops = _hierarchy(p, cells, quad, **kw)
    mg = pkg.PreconditionMG(ops)
    V = G.VCycle(p, cells, quad, deform_amp=AMP, kappa=O.kappa_step64)
    return ops, mg, V


@pytest.mark.parametrize("p,quad", [(2, 0), (3, 0), (4, 0), (4, 1), (5, 1), (6, 0), (7, 1), (8, 0)])
def test_v_cycle_and_level_bounds_match_numpy(p, quad):
    cells = (3, 3, 2) if p <= 5 else (2, 2, 2)
    ops, mg, V = _vcycle_case(p, cells, quad)
    info = mg.level_info()
    assert [d["degree"] for d in info] == G.degrees(p)
    for d, L in zip(info, V.levels):
        assert d["cg_its"] == L.cg_its and d["chebyshev_degree"] == L.degree
        for k in ("min_est", "max_est", "min_used", "max_used"):
            assert abs(d[k] - getattr(L, k)) <= 1e-10 * abs(getattr(L, k)), (k, d[k], getattr(L, k))
    n = V.levels[0].pr.mesh.n_dofs
    s = O.deterministic_src(n, V.levels[0].pr.mesh.constrained, seed=41)
    dst = ops[0].initialize_dof_vector()
    dst.fill_(float("nan"))                                       # prior content is ignored
    mg.vmult(dst, _dev(s, ops[0]))
    assert _rel(_lex(dst, ops[0], n), V.vmult(s)) < 1e-11
    mg.clear()


def _solve(ops, mg, tol_rel=1e-8, b=None):
    b = ops[0].assemble_rhs() if b is None else b
    tol = tol_rel * float(_t().linalg.norm(b[:ops[0].mf_data.n_owned]))
    x = ops[0].initialize_dof_vector()
    ctl = pkg.SolverControl(200, tol)
    pkg.SolverCG(ctl).solve(ops[0], x, b, mg)
    return x, ctl


@pytest.mark.parametrize("p,cells", [(2, (8, 8, 8)), (4, (6, 6, 6)), (6, (4, 4, 4)), (8, (3, 3, 3))])
def test_mg_pcg_converges_in_the_numpy_count(p, cells):
    ops, mg, V = _vcycle_case(p, cells)
    x, ctl = _solve(ops, mg)
    A = V.levels[0]
    b = A.pr.rhs()
    tol = 1e-8 * np.linalg.norm(b)
    x_ref, k_ref, _ = R.pcg(A.A, V.vmult, b, 200, tol=tol)
    assert abs(ctl.last_step() - k_ref) <= 1, (ctl.last_step(), k_ref)
    assert ctl.last_value() <= ctl.tolerance
    n = A.pr.mesh.n_dofs
    assert _rel(_lex(x, ops[0], n), x_ref) < 1e-7
    # against Chebyshev(4)-PCG on the same operator
    inv = ops[0].compute_diagonal(invert=True)
    ch = pkg.PreconditionChebyshev().initialize(ops[0], pkg.PreconditionChebyshev.AdditionalData(
        degree=4, smoothing_range=20.0, preconditioner=pkg.DiagonalMatrix(inv)))
    _, ctl_c = _solve(ops, ch)
    assert ctl_c.last_step() >= 2 * ctl.last_step(), (ctl_c.last_step(), ctl.last_step())
    mg.clear()


def test_two_solves_are_bitwise_identical():
    """on the block kernel (owner stores, no atomics) every level's operator is bitwise reproducible, and so are the transfers"""
    ops, mg, _ = _vcycle_case(4, (5, 4, 6), block=(4, 4, 4), variant=56)
    b = ops[0].assemble_rhs()                                    # (assembled once: the right-hand side sums atomically)
    x1, c1 = _solve(ops, mg, b=b)
    x2, c2 = _solve(ops, mg, b=b)
    assert c1.last_step() == c2.last_step()
    assert _t().equal(x1, x2)
    mg.clear()


def test_block_ordered_mesh_gives_the_lexicographic_result():
    p, cells = 4, (6, 5, 7)
    ops_l, mg_l, _ = _vcycle_case(p, cells)
    ops_b, mg_b, _ = _vcycle_case(p, cells, block=(4, 4, 4), variant=56)
    n = int(ops_l[0].mf_data.mesh.n_global_dofs)
    s = O.deterministic_src(n, O.BrickMesh(p, cells).constrained, seed=42)
    outs = []
    for ops, mg in ((ops_l, mg_l), (ops_b, mg_b)):
        d = ops[0].initialize_dof_vector()
        mg.vmult(d, _dev(s, ops[0]))
        outs.append(_lex(d, ops[0], n))
    assert _rel(outs[1], outs[0]) < 1e-12
    xl, cl = _solve(ops_l, mg_l)
    xb, cb = _solve(ops_b, mg_b)
    assert cl.last_step() == cb.last_step()
    assert _rel(_lex(xb, ops_b[0], n), _lex(xl, ops_l[0], n)) < 1e-10
    mg_l.clear()
    mg_b.clear()


def test_hanging_node_handle_is_refused():
    from types import SimpleNamespace

    def ns(m):
        return SimpleNamespace(degree=m.p, n=m.n, n_cells=m.n_cells, n_interior_cells=m.n_cells, n_owned=m.n_dofs, n_ghost=0, n_local=m.n_dofs,
                               n_global_dofs=m.n_dofs, l2g=m.l2g, coords=m.coords, constrained=m.constrained, n_neighbors=0,
                               neighbor_rank=np.zeros(0, np.int32), send_offsets=np.zeros(1, np.uint32), send_indices=np.zeros(0, np.uint32),
                               recv_offsets=np.zeros(1, np.uint32), cell_block_offsets=None, constraint_mask=m.constraint_mask, rank=0, n_ranks=1)
    fine = pkg.PoissonOperator(ns(O.HangingBrickMesh(2, 2, 2, 1, 3)), pkg.QUAD_GAUSS)
    coarse = pkg.PoissonOperator(ns(O.HangingBrickMesh(1, 2, 2, 1, 3)), pkg.QUAD_GAUSS)
    with pytest.raises(pkg.BP5Error) as e:
        pkg.MGTwoLevelTransfer(fine, coarse)
    assert e.value.status == 1 and "hanging" in str(e.value)


def test_mismatched_levels_are_refused():
    a = pkg.PoissonOperator(pkg.BrickMesh(4, (3, 3, 3)), pkg.QUAD_GAUSS)
    b = pkg.PoissonOperator(pkg.BrickMesh(1, (3, 3, 3)), pkg.QUAD_GAUSS)       # degree 1 is not 4 // 2
    c = pkg.PoissonOperator(pkg.BrickMesh(2, (3, 3, 4)), pkg.QUAD_GAUSS)       # other cells
    for coarse in (b, c):
        with pytest.raises(pkg.BP5Error) as e:
            pkg.MGTwoLevelTransfer(a, coarse)
        assert e.value.status == 1


def test_facade_example_matches_the_python_solve():
    """examples/bp5_multigrid (step-37's solve on the C++ facade: the level operators, PreconditionMG, SolverCG) reports the iteration
    count, the level bounds and the solution norm of the Python solve of the same problem."""
    import os
    import subprocess
    torch = _t()
    exe = os.path.join(bp5_pkg.ROOT, "examples", "bp5_multigrid")
    txt = subprocess.run([exe, "4", "5", "4", "4", "0.05", "1e-8"], capture_output=True, text=True, timeout=300, check=True).stdout
    got = {l.split()[0]: l.split()[1:] for l in txt.splitlines() if l.strip()}
    ops = pkg.make_mg_hierarchy(pkg.PoissonOperator(pkg.BrickMesh(4, (5, 4, 4), deform_amp=0.05), pkg.QUAD_GAUSS, pkg.COEF_STEP64))
    mg = pkg.PreconditionMG(ops)
    x, ctl = _solve(ops, mg)
    assert int(got["iterations"][0]) == ctl.last_step()
    for lev, d in enumerate(mg.level_info()):
        row = got[f"level{lev}"]
        assert int(row[0]) == d["degree"] and int(row[1]) == d["n_owned"]
        assert abs(float(row[3]) - d["max_used"]) <= 1e-12 * d["max_used"]
    xn = float(torch.linalg.norm(x[:ops[0].mf_data.n_owned]))
    assert abs(float(got["solution_norm"][0]) - xn) <= 1e-10 * xn, (got, xn)
    mg.clear()
