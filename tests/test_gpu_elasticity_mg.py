"""The elasticity preconditioners on the GPU (bp5_mg_transfer_*_components, bp5_elasticity_chebyshev_create, bp5_elasticity_mg_create,
bp5_cg_solve_elasticity_preconditioned; ElasticityPreconditionChebyshev, ElasticityPreconditionMG) against the numpy composition
tests/elasticity_mg_ref.py, which tests/test_elasticity_mg_cpu.py pins and whose comparisons it shows to be stable.  The block-vector transfers
are compared BITWISE with the scalar entry points block by block; everything that contains the operator (atomic scatter) to the project's
tolerances: 1e-12 Chebyshev, 1e-11 V-cycle, 1e-10 bounds, 1e-7 solutions of tolerance-stopped solves.  Lexicographic one-rank meshes: the
library's numbering is the oracle's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import chebyshev_ref as CR
import elasticity_mg_ref as M
import elasticity_ref as E
import hmg_ref as H
import multigrid_ref as G
import stream_harness as SH
from stream_harness import SENTINEL

pytestmark = pytest.mark.gpu
pkg = bp5_pkg.load()
AMP = M.AMP
TOL_BOUNDS, TOL_CHEB, TOL_MG, TOL_CG, TOL_SOLVE = 1e-10, 1e-12, 1e-11, 1e-11, 1e-7
EXTRA = 66
_cache = {}


def _t():
    import torch
    return torch


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def ld_of(n):
    return n + (n & 1) + EXTRA


def block(values, n, pad=SENTINEL):
    """(rows, ld) tensor, ld = n rounded up to even + 66: the rows hold `values`, the padding `pad`"""
    torch = _t()
    values = np.asarray(values, dtype=np.float64)
    t = torch.full((values.shape[0], ld_of(n)), pad, dtype=torch.float64, device="cuda:0")
    t[:, :n] = torch.from_numpy(np.array(values[:, :n])).to("cuda:0")          # (a copy: the references are read-only arrays)
    return t


def padding_is(t, n, value=SENTINEL):
    pad = t[:, n:].cpu().numpy()
    return pad.size > 0 and bool((pad == value).all())


def _operator(p, cells, quad=0, lame=0, free=False):
    key = ("op", p, cells, quad, lame, free)
    if key not in _cache:
        mesh = pkg.BrickMesh(p, cells, deform_amp=AMP)
        if free:
            mesh.constrained = np.zeros(0, np.uint32)
        _cache[key] = pkg.ElasticityOperator(mesh, quad, pkg.COEF_STEP64, lam=E.LAME[lame][0], mu=E.LAME[lame][1])
    return _cache[key]


def _inverse_diagonal(op, pad=float("nan")):
    """the block inverse diagonal in a padded (3, ld) tensor (bp5_elasticity_compute_diagonal leaves the padding alone)"""
    n = op.mf_data.n_local
    d = block(np.zeros((3, n)), n, pad)
    pkg.lib().bp5_elasticity_compute_diagonal(op.mf_data.handle, ptr(op.coef), op.lam, op.mu, d.shape[1], ptr(d), 1)
    return d


# ------------------------------------------------------------------ 1. transfers on block vectors
TRANSFERS = ([("p", p, (3, 2, 2) if p <= 4 else (2, 2, 2)) for p in range(2, 9)] + [("h", 1, (4, 4, 4)), ("h", 2, (4, 4, 4))]
             + [("h", 3, (2, 2, 2)), ("h", 4, (2, 2, 2))])        # (one coarse cell: 8 and 27 interior coarse DoFs)


def _transfer(kind, p, cells):
    """(fine operator, coarse operator, MGTwoLevelTransfer, numpy transfer); scalar Poisson handles: the transfer handles are scalar ones"""
    if kind == "p":
        fine = pkg.PoissonOperator(pkg.BrickMesh(p, cells, deform_amp=AMP), pkg.QUAD_GAUSS)
        coarse = pkg.PoissonOperator(pkg.BrickMesh(G.coarse_degree(p), cells, deform_amp=AMP), pkg.QUAD_GAUSS)
        return fine, coarse, pkg.MGTwoLevelTransfer(fine, coarse), G.Transfer(cells, p)
    mesh = pkg.BrickMesh(p, cells, deform_amp=AMP)
    fine, coarse = pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS), pkg.PoissonOperator(mesh.coarsen(1), pkg.QUAD_GAUSS)    # (min_cells = 1: a one-cell coarse mesh is fine)
    return fine, coarse, pkg.MGTwoLevelTransfer(fine, coarse, geometric=True), H.GeometricTransfer(tuple(c // 2 for c in cells), p)


@pytest.mark.parametrize("kind,p,cells", TRANSFERS)
def test_block_transfers_give_the_bits_of_the_scalar_entries(kind, p, cells):
    """The scalar and the block entries launch ONE kernel set (a scalar call is n_components = 1), so the ncomp = 1 leg compares a kernel with itself:
    it pins the entry points' plumbing (slots, leading dimensions, padding).  What the test proves about the kernels is the ncomp = 3 leg -- the
    component loop gives every block the bits of a one-component launch on it -- and the numpy, Dirichlet-row and adjointness assertions."""
    torch = _t()
    fine, coarse, tr, T = _transfer(kind, p, cells)
    nf, nc = fine.mf_data.n_local, coarse.mf_data.n_local
    rng = np.random.default_rng(100 + p)
    ec, x0 = rng.uniform(-1, 1, (3, nc)), rng.uniform(-1, 1, (3, nf))      # non-zero on the boundary too: coarse Dirichlet DoFs count as 0
    rf, b0 = rng.uniform(-1, 1, (3, nf)), rng.uniform(-1, 1, (3, nc))
    bc = T.boundary_c
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0")
    # the scalar entries, block by block
    pro, res = [], []
    for c in range(3):
        x = dev(x0[c])
        tr.prolongate_and_add(x, dev(ec[c]))
        pro.append(x)
        b = dev(b0[c])
        tr.restrict_and_add(b, dev(rf[c]))
        res.append(b)
    for ncomp in (1, 3):
        x, e = block(x0[:ncomp], nf), block(ec[:ncomp], nc)
        tr.prolongate_and_add_components(x, e)
        b, r = block(b0[:ncomp], nc), block(rf[:ncomp], nf)
        tr.restrict_and_add_components(b, r)
        for c in range(ncomp):
            assert torch.equal(x[c, :nf], pro[c]), ("prolongate", ncomp, c)
            assert torch.equal(b[c, :nc], res[c]), ("restrict", ncomp, c)
        for t, n, v in ((x, nf, x0), (e, nc, ec), (b, nc, b0), (r, nf, rf)):
            assert padding_is(t, n), "padding touched"
            if t is e or t is r:
                assert np.array_equal(t[:, :n].cpu().numpy(), v[:ncomp])          # sources unchanged
    got_p, got_r = x[:, :nf].cpu().numpy() - x0, b[:, :nc].cpu().numpy()
    # numpy, the scalar contract on the Dirichlet rows, and <R r, e> = <r, P e> with the device's own results
    BT = M.BlockTransfer(T)
    assert rel(got_p, BT.prolongate(ec)) < 1e-13
    assert np.array_equal(got_r[:, bc], b0[:, bc])
    assert rel(got_r[:, ~bc] - b0[:, ~bc], BT.restrict(rf)[:, ~bc]) < 1e-13
    lhs, rhs = np.sum((got_r - b0) * np.where(bc, 0.0, ec)), np.sum(rf * got_p)
    assert abs(lhs - rhs) <= 1e-13 * np.abs(rf).sum() * np.abs(ec).max() * 8
    tr.clear()


# p-transfer meshes whose cell count is no multiple of the cells per workgroup (MgShape::CPB = 9 / 4 / 2 at p = 2 / 3 / 4): (3, 1, 1) is three cells
# in a workgroup with room for nine, for four, and a second half-empty one -- the `c < n_cells` guards of the preloaded-index kernels, with one
# component and with three.  On (3, 1, 1) every coarse DoF of p = 2, 3 (coarse degree 1) lies on the boundary, so P e and the free rows of R r are
# empty there and those cases can only show exact zeros; (3, 3, 2) at p = 3 (18 cells, the fifth workgroup half empty) adds a partial
# workgroup with interior coarse DoFs.  p = 2 has one in TRANSFERS already ((3, 2, 2): 12 cells), p = 4 has 5 interior coarse DoFs on (3, 1, 1).
PARTIAL = [(2, (3, 1, 1)), (3, (3, 1, 1)), (4, (3, 1, 1)), (3, (3, 3, 2))]


@pytest.mark.parametrize("p,cells", PARTIAL)
def test_transfers_on_a_partly_empty_last_workgroup_match_numpy(p, cells):
    torch = _t()
    fine, coarse, tr, T = _transfer("p", p, cells)
    nf, nc = fine.mf_data.n_local, coarse.mf_data.n_local
    assert fine.mf_data.mesh.n_cells == int(np.prod(cells)) and int(np.prod(cells)) % {2: 9, 3: 4, 4: 2}[p] != 0
    rng = np.random.default_rng(300 + p)
    ec, x0, rf, b0 = rng.uniform(-1, 1, (3, nc)), rng.uniform(-1, 1, (3, nf)), rng.uniform(-1, 1, (3, nf)), rng.uniform(-1, 1, (3, nc))
    bc = T.boundary_c
    BT = M.BlockTransfer(T)
    ref_p, ref_r = BT.prolongate(ec), BT.restrict(rf)

    def check(got_x, got_b, rows):
        """1e-13 relative to the numpy transfer as in the test above; where the reference is empty or exactly zero, exactly that"""
        got_p, free = got_x - x0[rows], got_b[:, ~bc] - b0[rows][:, ~bc]
        if np.any(ref_p[rows]):
            assert rel(got_p, ref_p[rows]) < 1e-13
        else:
            assert not np.any(got_p)
        if np.any(ref_r[rows][:, ~bc]):
            assert rel(free, ref_r[rows][:, ~bc]) < 1e-13
        else:
            assert not np.any(free)
        assert np.array_equal(got_b[:, bc], b0[rows][:, bc])

    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0")
    for c in range(3):                                         # the scalar entries
        x, b = dev(x0[c]), dev(b0[c])
        tr.prolongate_and_add(x, dev(ec[c]))
        tr.restrict_and_add(b, dev(rf[c]))
        check(x.cpu().numpy()[None], b.cpu().numpy()[None], slice(c, c + 1))
    for ncomp in (1, 3):                                       # the block entries
        x, e, b, r = block(x0[:ncomp], nf), block(ec[:ncomp], nc), block(b0[:ncomp], nc), block(rf[:ncomp], nf)
        tr.prolongate_and_add_components(x, e)
        tr.restrict_and_add_components(b, r)
        check(x[:, :nf].cpu().numpy(), b[:, :nc].cpu().numpy(), slice(0, ncomp))
        for t, n in ((x, nf), (e, nc), (b, nc), (r, nf)):
            assert padding_is(t, n), "padding touched"
    tr.clear()


def test_block_transfer_layout_refusals_write_nothing():
    torch = _t()
    L = pkg.lib()
    fine, coarse, tr, _ = _transfer("p", 2, (3, 2, 2))
    nf, nc = fine.mf_data.n_local, coarse.mf_data.n_local
    xf, xc = block(np.ones((3, nf)), nf), block(np.ones((3, nc)), nc)
    ldf, ldc = xf.shape[1], xc.shape[1]
    keep_f, keep_c = xf.clone(), xc.clone()
    small_f = (nf - 1) - ((nf - 1) & 1)
    cases = [((0, ldf, ptr(xf), ldc, ptr(xc)), "n_components"), ((9, ldf, ptr(xf), ldc, ptr(xc)), "n_components"), ((3, ldf + 1, ptr(xf), ldc, ptr(xc)), "even"),
             ((3, ldf, ptr(xf), ldc + 1, ptr(xc)), "even"), ((3, small_f, ptr(xf), ldc, ptr(xc)), "ld <"), ((3, ldf, ptr(xf), 2, ptr(xc)), "ld <"),
             ((3, ldf, C.c_void_p(xf.data_ptr() + 8), ldc, ptr(xc)), "aligned"), ((3, ldf, ptr(xf), ldc, C.c_void_p(xc.data_ptr() + 8)), "aligned"),
             ((3, ldf, None, ldc, ptr(xc)), "null"), ((3, ldf, ptr(xf), ldc, None), "null")]
    for (ncomp, lf, pf, lc, pc), word in cases:
        for st in (L.bp5_mg_transfer_prolongate_add_components(tr.handle, ncomp, lf, pf, lc, pc), L.bp5_mg_transfer_restrict_add_components(tr.handle, ncomp, lc, pc, lf, pf)):
            assert st == 1 and word in L.bp5_last_error().decode(), (ncomp, lf, lc, word, st, L.bp5_last_error().decode())
    torch.cuda.synchronize()
    assert torch.equal(xf, keep_f) and torch.equal(xc, keep_c)
    # the Python mirror: component counts that differ
    with pytest.raises(pkg.BP5Error) as e:
        tr.prolongate_and_add_components(xf, xc[:2])
    assert e.value.status == 1
    tr.clear()


# ------------------------------------------------------------------ 2. Chebyshev
@pytest.mark.parametrize("p,degree,block_diagonal", M.CHEBYSHEV_CASES)
def test_chebyshev_bounds_vmult_and_step_match_numpy(p, degree, block_diagonal):
    Lv, src, x0 = M.chebyshev_case(p, degree, block_diagonal)
    op = _operator(p, M.CHEBYSHEV_CELLS)
    n = op.mf_data.n_local
    inv = _inverse_diagonal(op) if block_diagonal else None
    if inv is not None:
        assert max(rel(inv[c, :n].cpu().numpy(), Lv.inv[c]) for c in range(3)) <= 1e-13
    ch = pkg.ElasticityPreconditionChebyshev().initialize(op, pkg.ElasticityPreconditionChebyshev.AdditionalData(
        degree=degree, smoothing_range=20.0, eig_cg_n_iterations=8, preconditioner=pkg.DiagonalMatrix(inv) if inv is not None else None), ld=ld_of(n))
    e = ch.estimated_eigenvalues()
    print(f"p = {p}, degree {degree}, block diagonal {block_diagonal}: estimate {e}, numpy [{Lv.min_est}, {Lv.max_est}] in {Lv.cg_its} steps")
    assert e["cg_its"] == Lv.cg_its
    for k in ("min_est", "max_est", "min_used", "max_used"):
        assert abs(e[k] - getattr(Lv, k)) <= TOL_BOUNDS * abs(getattr(Lv, k)), (k, e[k], getattr(Lv, k))
    s = block(src, n)
    dst = block(np.full((3, n), np.nan), n)                              # prior content is ignored
    ch.vmult(dst, s)
    want = CR.vmult(Lv.A, Lv.inv, src, e["min_used"], e["max_used"], degree)
    err_v = rel(dst[:, :n].cpu().numpy(), want)
    dst = block(x0, n)
    ch.step(dst, s)
    want = CR.step(Lv.A, Lv.inv, x0, src, e["min_used"], e["max_used"], degree)
    err_s = rel(dst[:, :n].cpu().numpy(), want)
    print(f"  vmult error {err_v:.2e}, step error {err_s:.2e}")
    assert err_v <= TOL_CHEB and err_s <= TOL_CHEB
    assert padding_is(dst, n) and padding_is(s, n) and np.array_equal(s[:, :n].cpu().numpy(), src)
    ch.clear()


# ------------------------------------------------------------------ 3. V-cycle
def _hierarchy(name):
    p, cells, quad, lame, h_levels, min_cells = M.VCYCLE_CASES[name]
    fine = pkg.ElasticityOperator(pkg.BrickMesh(p, cells, deform_amp=AMP), quad, pkg.COEF_STEP64, lam=E.LAME[lame][0], mu=E.LAME[lame][1])
    return pkg.make_elasticity_mg_hierarchy(fine, h_levels=h_levels, min_cells=min_cells)


def _check_level_info(info, V):
    assert [(d["degree"], d["cells"]) for d in info] == [(q, c) for q, c, _ in V.spec]
    for lev, (d, Lv) in enumerate(zip(info, V.levels)):
        assert d["n_owned"] == Lv.pr.mesh.n_dofs and d["cg_its"] == Lv.cg_its and d["chebyshev_degree"] == Lv.degree, (lev, d, Lv.cg_its)
        for k in ("min_est", "max_est", "min_used", "max_used"):
            assert abs(d[k] - getattr(Lv, k)) <= TOL_BOUNDS * abs(getattr(Lv, k)), (lev, k, d[k], getattr(Lv, k))


@pytest.mark.parametrize("name", sorted(M.VCYCLE_CASES))
def test_v_cycle_and_level_info_match_numpy(name):
    V, s = M.vcycle_case(name)
    ops = _hierarchy(name)
    assert all(isinstance(o, pkg.ElasticityOperator) and (o.lam, o.mu) == (ops[0].lam, ops[0].mu) for o in ops)
    n = ops[0].mf_data.n_local
    mg = pkg.ElasticityPreconditionMG(ops, ld=ld_of(n))
    _check_level_info(mg.level_info(), V)
    src = block(s, n)
    dst = block(np.full((3, n), np.nan), n)
    mg.vmult(dst, src)
    err = rel(dst[:, :n].cpu().numpy(), V.vmult(s))
    print(f"{name}: V-cycle error {err:.2e}")
    assert err <= TOL_MG
    assert padding_is(dst, n) and padding_is(src, n) and np.array_equal(src[:, :n].cpu().numpy(), s)
    mg.clear()


# ------------------------------------------------------------------ 4. the solve
def _solve(op, b, pre, tol, max_iter=400, check_every=0, pad=True):
    n = op.mf_data.n_local
    bt = block(b, n, 0.0) if pad else op.initialize_block_vector()
    if not pad:
        bt[:, :n] = _t().from_numpy(np.ascontiguousarray(b)).to("cuda:0")
    x = block(np.full((3, n), np.nan), n) if pad else op.initialize_block_vector()
    ctl = pkg.SolverControl(max_iter, tol)
    pkg.SolverCG(ctl, check_every=check_every).solve(op, x, bt, pre)
    if pad:
        assert padding_is(x, n)
    return x[:, :n].cpu().numpy(), ctl


@pytest.mark.parametrize("name", sorted(M.SOLVE_CASES))
def test_preconditioned_cg_converges_in_the_numpy_count(name):
    V, b = M.solve_case(name)
    p, cells = M.SOLVE_CASES[name]
    L0 = V.levels[0]
    op = _operator(p, cells)
    n = op.mf_data.n_local
    tol = 1e-8 * np.linalg.norm(b)
    ops = pkg.make_elasticity_mg_hierarchy(op)
    mg = pkg.ElasticityPreconditionMG(ops, ld=ld_of(n))
    x, ctl = _solve(op, b, mg, tol)
    x_ref, k_ref, _ = M.pcg(L0.pr.vmult, V.vmult, b, 400, tol=tol)
    inv = _inverse_diagonal(op)
    _, ctl_j = _solve(op, b, pkg.DiagonalMatrix(inv), tol, max_iter=2000)
    print(f"{name}: V-cycle-PCG {ctl.last_step()} iterations (numpy {k_ref}), error {rel(x, x_ref):.2e}; Jacobi-PCG {ctl_j.last_step()}")
    assert abs(ctl.last_step() - k_ref) <= 1 and ctl.last_value() <= tol
    assert rel(x, x_ref) < TOL_SOLVE
    assert 5 * ctl.last_step() <= ctl_j.last_step()
    # Chebyshev(4)-PCG, checked the same way against its numpy twin
    Lc = M.Level(p, cells, 1.0, O.QUAD_GAUSS, AMP, O.kappa_step64, E.LAME[0][0], E.LAME[0][1], 4, 20.0, 8)
    ch = pkg.ElasticityPreconditionChebyshev().initialize(op, pkg.ElasticityPreconditionChebyshev.AdditionalData(
        degree=4, smoothing_range=20.0, eig_cg_n_iterations=8, preconditioner=pkg.DiagonalMatrix(inv)))
    assert ch.ld == ld_of(n)
    xc, ctl_c = _solve(op, b, ch, tol, check_every=3)
    xc_ref, kc_ref, _ = M.pcg(L0.pr.vmult, Lc.vmult, b, 400, tol=tol)
    print(f"{name}: Chebyshev(4)-PCG {ctl_c.last_step()} iterations (numpy {kc_ref}), error {rel(xc, xc_ref):.2e}")
    assert abs(ctl_c.last_step() - kc_ref) <= 1 and ctl_c.last_value() <= tol and rel(xc, xc_ref) < TOL_SOLVE
    assert ctl.last_step() < ctl_c.last_step() < ctl_j.last_step()
    mg.clear()
    ch.clear()


def test_preconditioned_cg_edges_a_python_callback_and_the_merged_variant():
    from deal_and_ceed_on_gpu_amd import _lib
    torch = _t()
    L = pkg.lib()
    pr, b, inv, its = E.cg_case("p4")                                   # the fixed-iteration case whose drift tests/test_elasticity_cpu.py asserts
    op = _operator(4, (4, 4, 4))
    n, h = op.mf_data.n_local, op.mf_data.handle
    ops = pkg.make_elasticity_mg_hierarchy(op)
    mg = pkg.ElasticityPreconditionMG(ops, ld=ld_of(n))
    # b = 0: no iteration, x exactly 0; max_iter = 0: x = 0 and the initial residual reported; the padding kept either way
    x, ctl = _solve(op, np.zeros_like(b), mg, 0.0, max_iter=10)
    assert ctl.last_step() == 0 and not x.any() and ctl.last_value() == 0.0
    x, ctl = _solve(op, b, mg, 0.0, max_iter=0)
    assert ctl.last_step() == 0 and not x.any() and abs(ctl.last_value() - np.linalg.norm(b)) <= 1e-13 * np.linalg.norm(b)
    # a plain Python object as preconditioner through the C entry: z = D^-1 g on torch views of the library's vectors -- Jacobi-PCG, which
    # the numpy reference of bp5_cg_solve_elasticity states
    ld = ld_of(n)
    inv_t = block(inv, n, 1.0)
    calls = []

    class Jacobi:
        def vmult(self, dst, src):
            calls.append(1)
            torch.mul(inv_t[:, :n], src[:, :n], out=dst[:, :n])

    from deal_and_ceed_on_gpu_amd.matrix_free import _DeviceArray

    def view(p):
        return torch.as_tensor(_DeviceArray(p, 3 * ld), device="cuda:0").view(3, ld)
    P, failure = Jacobi(), []

    def callback(_ctx, dst, src):
        try:
            P.vmult(view(dst), view(src))
            return 0
        except Exception as e:      # noqa: BLE001
            failure.append(e)
            return 1
    cb = _lib.VMULT_FN(callback)
    bt, xt = block(b, n, 0.0), block(np.full((3, n), np.nan), n)
    for check_every in (0, 2):
        prm, res = _lib.CGParams(_lib.CG_PLAIN, its, 0.0, check_every, 0), _lib.CGResult()
        xt[:, :n] = float("nan")
        st = L.bp5_cg_solve_elasticity_preconditioned(h, ptr(op.coef), op.lam, op.mu, ld, C.cast(cb, C.c_void_p), None, ptr(bt), ptr(xt), C.byref(prm), C.byref(res))
        assert st == 0 and not failure, (st, L.bp5_last_error().decode(), failure)
        xr, k, rr = E.cg(pr.vmult, b, its, inv_diag=inv)
        err = max(rel(xt[c, :n].cpu().numpy(), xr[c]) for c in range(3))
        print(f"Python callback, check_every {check_every}: {res.iterations} iterations, error {err:.2e}, {len(calls)} preconditioner calls")
        assert res.iterations == k == its and err <= TOL_CG and abs(res.residual - rr) <= 1e-10 * rr and padding_is(xt, n)
    assert len(calls) >= its
    # the merged variant is known and not offered
    xt.fill_(0.0)
    prm = _lib.CGParams(_lib.CG_MERGED, 3, 0.0, 0, 0)
    st = L.bp5_cg_solve_elasticity_preconditioned(h, ptr(op.coef), op.lam, op.mu, ld, C.cast(L.bp5_mg_vmult, C.c_void_p), mg.handle, ptr(bt), ptr(xt), C.byref(prm), C.byref(res))
    msg = L.bp5_last_error().decode()
    torch.cuda.synchronize()
    assert st == 5 and "BP5_CG_MERGED" in msg and "elasticity" in msg and float(xt.abs().max()) == 0.0
    # vectors of another ld than the preconditioner's are the Python mirror's to refuse
    with pytest.raises(pkg.BP5Error) as e:
        pkg.SolverCG(pkg.SolverControl(3, 0.0)).solve(op, op.initialize_block_vector(), op.initialize_block_vector(), mg)
    assert e.value.status == 1 and "ld" in str(e.value)
    mg.clear()


# ------------------------------------------------------------------ 5. refusals
def test_every_refusal_names_its_reason_and_writes_nothing():
    from types import SimpleNamespace
    from deal_and_ceed_on_gpu_amd import _lib
    torch = _t()
    L = pkg.lib()
    mesh = pkg.BrickMesh(2, (3, 2, 2))

    def ns(m):
        return SimpleNamespace(degree=m.p, n=m.n, n_cells=m.n_cells, n_interior_cells=m.n_cells, n_owned=m.n_dofs, n_ghost=0, n_local=m.n_dofs,
                               n_global_dofs=m.n_dofs, l2g=m.l2g, coords=m.coords, constrained=m.constrained, n_neighbors=0,
                               neighbor_rank=np.zeros(0, np.int32), send_offsets=np.zeros(1, np.uint32), send_indices=np.zeros(0, np.uint32),
                               recv_offsets=np.zeros(1, np.uint32), cell_block_offsets=None, constraint_mask=m.constraint_mask, rank=0, n_ranks=1)
    comm = pkg.Communicator(0, 1)
    cases = [(pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS_OVER), "BP5_QUAD_GAUSS_OVER"), (pkg.HelmholtzOperator(mesh, 0), "Helmholtz"), (pkg.MassOperator(mesh, 0), "mass"),
             (pkg.PoissonOperator(ns(O.HangingBrickMesh(2, 2, 2, 1, 3)), 0), "hanging"), (pkg.PoissonOperator(mesh, 0, geometry=pkg.GEOM_AFFINE), "affine"),
             (pkg.PoissonOperator(mesh, 0, metric_precision="float32"), "FP32"),
             (pkg.PoissonOperator(pkg.BrickMesh(2, (3, 2, 4), rank=1, n_ranks=2), 0, comm=comm), "communicator")]
    prm, res = _lib.CGParams(_lib.CG_PLAIN, 3, 0.0, 0, 0), _lib.CGResult()
    cheb = _lib.ChebyshevParams(4, 20.0, 8, 0.0, 0.0, None)
    mgp = _lib.MGParams()
    L.bp5_mg_params_default(C.byref(mgp))
    never = _lib.VMULT_FN(lambda ctx, d, s: 1)

    def three_creates(h, coef, ld, x, b, lam=1.0, mu=1.0):
        """the Chebyshev create, the one-level multigrid create and the preconditioned solve on one handle: (statuses, last message, handles)"""
        out_c, out_m = C.c_void_p(), C.c_void_p()
        mfs, coefs = (C.c_void_p * 1)(h.value), (C.c_void_p * 1)(coef.data_ptr())
        st = [L.bp5_elasticity_chebyshev_create(h, ptr(coef), lam, mu, ld, None, C.byref(cheb), C.byref(out_c))]
        msgs = [L.bp5_last_error().decode()]
        st.append(L.bp5_elasticity_mg_create(1, mfs, coefs, lam, mu, ld, None, C.byref(mgp), C.byref(out_m)))
        msgs.append(L.bp5_last_error().decode())
        st.append(L.bp5_cg_solve_elasticity_preconditioned(h, ptr(coef), lam, mu, ld, C.cast(never, C.c_void_p), None, ptr(b), ptr(x), C.byref(prm), C.byref(res)))
        msgs.append(L.bp5_last_error().decode())
        return st, msgs, (out_c, out_m)

    for op, word in cases:
        x, b = op.initialize_block_vector(3), op.initialize_block_vector(3)
        b.fill_(1.0)
        coef = torch.zeros(16, dtype=torch.float64, device="cuda:0")     # never read: every call below is refused before any launch
        st, msgs, outs = three_creates(op.mf_data.handle, coef, x.shape[1], x, b)
        assert st == [5, 5, 5] and all(word in m and "elasticity" in m for m in msgs), (word, st, msgs)
        assert not outs[0].value and not outs[1].value
        torch.cuda.synchronize()
        assert float(x.abs().max()) == 0.0 and float(coef.abs().max()) == 0.0
    comm.close()
    # what needs a good handle: the layout against the handle, the parameters, a level without Dirichlet DoFs, levels on different streams
    op = _operator(2, (3, 2, 2))
    n, h = op.mf_data.n_local, op.mf_data.handle
    x, b = op.initialize_block_vector(), op.initialize_block_vector()
    b.fill_(1.0)
    ld = x.shape[1]
    small = (n - 1) - ((n - 1) & 1)
    for kw, word in ((dict(ld=small), "ld <"), (dict(ld=ld + 1), "even"), (dict(mu=0.0), "mu"), (dict(lam=-1.0), "bulk"), (dict(lam=float("nan")), "finite")):
        st, msgs, outs = three_creates(h, op.coef, kw.pop("ld", ld), x, b, **kw)
        assert st == [1, 1, 1] and all(word in m and "elasticity" in m for m in msgs), (word, st, msgs)
    free = _operator(2, (3, 2, 2), free=True)
    out = C.c_void_p()
    st = L.bp5_elasticity_mg_create(1, (C.c_void_p * 1)(free.mf_data.handle.value), (C.c_void_p * 1)(free.coef.data_ptr()), 1.0, 1.0, ld, None, C.byref(mgp), C.byref(out))
    msg = L.bp5_last_error().decode()
    assert st == 5 and "Dirichlet" in msg and "elasticity" in msg and not out.value, (st, msg)
    with torch.cuda.stream(SH.side_stream()):
        other = pkg.ElasticityOperator(pkg.BrickMesh(1, (3, 2, 2), deform_amp=AMP), 0, pkg.COEF_STEP64, lam=op.lam, mu=op.mu)
    assert other.mf_data.stream != op.mf_data.stream
    two = (C.c_void_p * 2)(h.value, other.mf_data.handle.value)
    st = L.bp5_elasticity_mg_create(2, two, (C.c_void_p * 2)(op.coef.data_ptr(), other.coef.data_ptr()), op.lam, op.mu, ld, (C.c_void_p * 1)(None), C.byref(mgp), C.byref(out))
    msg = L.bp5_last_error().decode()
    assert st == 1 and "stream" in msg and "elasticity" in msg and not out.value, (st, msg)
    with pytest.raises(pkg.BP5Error) as e:
        pkg.ElasticityPreconditionMG([op, other])
    assert e.value.status == 1 and "stream" in str(e.value)
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0
    # the refusals the existing classes pin stay what they were
    for fn in (lambda: pkg.PreconditionChebyshev().initialize(op), lambda: pkg.PreconditionMG([op]),
               lambda: pkg.SolverCG(pkg.IterationNumberControl(3, 0.0)).solve(op, x, b, pkg.PreconditionChebyshev()),
               lambda: pkg.SolverCGFullMerge(pkg.IterationNumberControl(3, 0.0)).solve(op, x, b, pkg.DiagonalMatrix())):
        with pytest.raises(pkg.BP5Error) as e:
            fn()
        assert e.value.status == 5, str(e.value)
    assert float(x.abs().max()) == 0.0


# ------------------------------------------------------------------ 6. stream ordering
def test_every_new_entry_point_on_a_busy_non_blocking_side_stream():
    """tests/stream_harness.py's protocol: the handles sit on a non-blocking side stream that is held busy, the inputs are produced behind the hold,
    the outputs are consumed on the stream without a host synchronisation.  The creates and the solve are host-synchronous (run once plainly and
    once with the null stream held as well), the transfers and the applications asynchronous (the warmed call returns while the hold lasts)."""
    torch = _t()
    name = "p2_gll"
    V, s = M.vcycle_case(name)
    p, cells, quad, lame, _, _ = M.VCYCLE_CASES[name]
    S = SH.side_stream()
    with torch.cuda.stream(S):
        fine = pkg.ElasticityOperator(pkg.BrickMesh(p, cells, deform_amp=AMP), quad, pkg.COEF_STEP64, lam=E.LAME[lame][0], mu=E.LAME[lame][1])
        ops = pkg.make_elasticity_mg_hierarchy(fine)
        torch.cuda.synchronize()
    assert all(o.mf_data.stream == S.cuda_stream for o in ops)
    L0, L1 = V.levels[0], V.levels[1]
    nf, nc = fine.mf_data.n_local, ops[1].mf_data.n_local
    ld = ld_of(nf)

    def pair(values, n, pad=SENTINEL):
        """(working tensor, staging tensor with the good values)"""
        with torch.cuda.stream(S):
            g = block(values, n, pad)
            return torch.empty_like(g), g

    def protocol(inputs, outputs, call, check, asynchronous):
        for second in (False, True):
            got, value = SH.run(S, inputs, outputs, call, asynchronous=asynchronous and second, hold_null=(not asynchronous) and second,
                                scale=1.0 if asynchronous and second else 2.0)
            check([g.cpu().numpy() for g in got], value)

    # the transfers on block vectors
    rng = np.random.default_rng(5)
    ec, x0, rf, b0 = rng.uniform(-1, 1, (3, nc)), rng.uniform(-1, 1, (3, nf)), rng.uniform(-1, 1, (3, nf)), rng.uniform(-1, 1, (3, nc))
    BT = V.transfers[0]
    bc = BT.T.boundary_c
    with torch.cuda.stream(S):
        tr = pkg.MGTwoLevelTransfer(fine, ops[1])
    e_w, e_g = pair(ec, nc)
    x_w, x_g = pair(x0, nf)
    r_w, r_g = pair(rf, nf)
    b_w, b_g = pair(b0, nc)

    def check_p(got, _):
        assert rel(got[0][:, :nf] - x0, BT.prolongate(ec)) < 1e-13 and (got[0][:, nf:] == SENTINEL).all()

    def check_r(got, _):
        assert rel(got[0][:, :nc][:, ~bc] - b0[:, ~bc], BT.restrict(rf)[:, ~bc]) < 1e-13 and (got[0][:, nc:] == SENTINEL).all()
    protocol([(e_w, e_g)], [(x_w, x_g)], lambda: tr.prolongate_and_add_components(x_w, e_w), check_p, True)
    protocol([(r_w, r_g)], [(b_w, b_g)], lambda: tr.restrict_and_add_components(b_w, r_w), check_r, True)
    # bp5_elasticity_chebyshev_create with the inverse diagonal produced behind the hold, then vmult and step
    d_w, d_g = pair(L0.inv, nf, float("nan"))
    data = pkg.ElasticityPreconditionChebyshev.AdditionalData(degree=4, smoothing_range=20.0, eig_cg_n_iterations=10, preconditioner=pkg.DiagonalMatrix(d_w))
    made = []

    def check_create(_, ch):
        e = ch.estimated_eigenvalues()
        made.append(ch)
        assert e["cg_its"] == L0.cg_its and abs(e["max_est"] - L0.max_est) <= TOL_BOUNDS * L0.max_est and abs(e["min_est"] - L0.min_est) <= TOL_BOUNDS * L0.min_est, e
    protocol([(d_w, d_g)], [], lambda: pkg.ElasticityPreconditionChebyshev().initialize(fine, data), check_create, False)
    ch = made[-1]
    s_w, s_g = pair(s, nf)
    dst, nan_pre = pair(np.full((3, nf), np.nan), nf)
    _, x0_g = pair(x0, nf)
    e = ch.estimated_eigenvalues()

    def close_to(want, tol):
        def check(got, _):
            assert np.isfinite(got[0][:, :nf]).all() and rel(got[0][:, :nf], want) <= tol and (got[0][:, nf:] == SENTINEL).all()
        return check
    protocol([(s_w, s_g), (d_w, d_g)], [(dst, nan_pre)], lambda: ch.vmult(dst, s_w), close_to(CR.vmult(L0.A, L0.inv, s, e["min_used"], e["max_used"], 4), TOL_CHEB), True)
    protocol([(s_w, s_g), (d_w, d_g)], [(dst, x0_g)], lambda: ch.step(dst, s_w), close_to(CR.step(L0.A, L0.inv, x0, s, e["min_used"], e["max_used"], 4), TOL_CHEB), True)
    # bp5_elasticity_mg_create (its estimates run on the held stream), then the V-cycle and the preconditioned solve
    mgs = []

    def check_mg(_, mg):
        mgs.append(mg)
        _check_level_info(mg.level_info(), V)
    protocol([], [], lambda: pkg.ElasticityPreconditionMG(ops, ld=ld), check_mg, False)
    mg = mgs[-1]
    protocol([(s_w, s_g)], [(dst, nan_pre)], lambda: mg.vmult(dst, s_w), close_to(V.vmult(s), TOL_MG), True)
    b = M.rhs(L0.pr)
    tol = 1e-8 * np.linalg.norm(b)
    xr, k_ref, _ = M.pcg(L0.pr.vmult, V.vmult, b, 200, tol=tol)
    rhs_w, rhs_g = pair(b, nf, 0.0)
    ctls = []

    def solve():
        ctls.append(pkg.SolverControl(200, tol))
        pkg.SolverCG(ctls[-1]).solve(fine, dst, rhs_w, mg)

    def check_solve(got, _):
        assert abs(ctls[-1].last_step() - k_ref) <= 1 and ctls[-1].last_value() <= tol and rel(got[0][:, :nf], xr) < TOL_SOLVE and (got[0][:, nf:] == SENTINEL).all()
    protocol([(rhs_w, rhs_g)], [(dst, nan_pre)], solve, check_solve, False)
    for m in mgs:
        m.clear()
    for c in made:
        c.clear()
    tr.clear()


# ------------------------------------------------------------------ 7. the example
def test_example_reproduces_the_python_solve():
    """examples/bp5_elasticity_mg (the C ABI alone): iteration count, level bounds and solution norm of the Python solve of the same problem"""
    exe = os.path.join(bp5_pkg.ROOT, "examples", "bp5_elasticity_mg")
    lam, mu = E.LAME[0]
    txt = subprocess.run([exe, "4", "4", "3", "3", "0.04", repr(lam), repr(mu), "1e-8"], capture_output=True, text=True, timeout=300, check=True).stdout
    got = {l.split()[0]: l.split()[1:] for l in txt.splitlines() if l.strip()}
    op = pkg.ElasticityOperator(pkg.BrickMesh(4, (4, 3, 3), deform_amp=0.04), pkg.QUAD_GAUSS, pkg.COEF_STEP64, lam=lam, mu=mu)
    n = op.mf_data.n_local
    mg = pkg.ElasticityPreconditionMG(pkg.make_elasticity_mg_hierarchy(op))
    b, x = op.initialize_block_vector(), op.initialize_block_vector()
    b[2, :n] = -op.assemble_rhs()
    ctl = pkg.SolverControl(500, 1e-8 * float(b[2, :n].norm()))
    pkg.SolverCG(ctl).solve(op, x, b, mg)
    print(txt, ctl.last_step())
    assert int(got["iterations"][0]) == ctl.last_step() and 0 < ctl.last_step() <= 15
    for lev, d in enumerate(mg.level_info()):
        row = got[f"level{lev}"]
        assert int(row[0]) == d["degree"] and int(row[1]) == d["n_owned"]
        assert abs(float(row[3]) - d["max_used"]) <= 1e-12 * d["max_used"]
    xn = float(_t().linalg.norm(x[:, :n]))
    assert abs(float(got["solution_norm"][0]) - xn) <= 1e-10 * xn, (got, xn)
    mg.clear()
