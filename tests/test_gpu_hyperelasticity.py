"""Finite-strain neo-Hookean hyperelasticity on the GPU (bp5_hyperelasticity_*, bp5_cg_solve_hyperelasticity, bp5_hyperelasticity_newton;
HyperelasticityOperator, NewtonSolver) against the numpy statement tests/hyperelasticity_ref.py, which tests/test_hyperelasticity_cpu.py pins
(finite differences, linear limit, symmetry, objectivity, homogeneous stretch) and whose fixed cases it shows to be stable.  The kernels scatter
with atomics: results are compared to tolerances, never bitwise.
  TOL_OP  1e-13: the tangent -- the apply-parity tolerance of tests/test_gpu_elasticity.py (same arithmetic depth).  The residual and the state:
          the larger of that number and 10 x the reference's own change under a relative 1e-16 perturbation of u
          (hyperelasticity_ref.input_noise_drift, per case and quantity; tests/test_hyperelasticity_cpu.py::test_parity_references_under_input_noise
          prints both: 1e-13 governs except for ln J from p = 6).
  TOL_CG  1e-11: fixed-iteration CG; the references stay two decades below it under operator noise (the CPU test asserts that)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import elasticity_mg_ref as M
import elasticity_ref as E
import hyperelasticity_ref as H

pytestmark = pytest.mark.gpu
pkg = bp5_pkg.load()
TOL_OP = 1e-13
TOL_CG = 1e-11
SENTINEL = -7.25e30
AMP = 0.04
LAME = E.LAME
_cache = {}


def _t():
    import torch
    return torch


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def errors(got, ref):
    return [rel(got[c], ref[c]) for c in range(3)]


def block(values, n_local, pad_value=float("nan"), extra=66):
    """(3, ld) tensor, ld = n_local rounded up to even + extra (even); rows hold `values`, the padding pad_value"""
    torch = _t()
    values = np.asarray(values)
    ld = n_local + (n_local & 1) + extra
    t = torch.full((values.shape[0], ld), pad_value, dtype=torch.float64, device="cuda:0")
    t[:, :n_local] = torch.from_numpy(np.array(values[:, :n_local])).to("cuda:0")
    return t


def check_padding(t, n_local, value):
    pad = t[:, n_local:].cpu().numpy()
    assert pad.size and (np.isnan(pad).all() if np.isnan(value) else (pad == value).all())


def workgroup_cells(p):
    """cells of one workgroup of the degree's default pencil launch (csrc/bp5_device.hpp: DefaultPencil)"""
    tw, lpc, tpb = (1, (p + 1) ** 2, 4) if p <= 3 else (4, (p + 1) ** 2, 1)
    return (64 * tw // lpc) * tpb


def parity_cells(p):
    return (5, 4, 4) if p <= 2 else (11, 2, 1)


def _reference(p, quad, cells, lame=0):
    """problem, displacement (non-zero on the Dirichlet set), tangent source, and the reference residual / state / tangent: once, read-only"""
    key = ("ref", p, quad, cells, lame)
    if key not in _cache:
        pr = H.Problem(p, cells, quad, deform_amp=AMP, kappa=O.kappa_step64, lam=LAME[lame][0], mu=LAME[lame][1])
        u = H.smooth_displacement(pr, 0.2)
        v = np.stack([O.deterministic_src(pr.mesh.n_dofs, seed=60 + c) for c in range(3)])
        out = dict(pr=pr, u=u, v=v, r_cells=pr.residual_cells(u), state=pr.state(u), t_cells=pr.tangent_cells(u, v),
                   tol=tuple(max(TOL_OP, 10.0 * d) for d in H.input_noise_drift(pr, u)))      # (residual, state B, ln J)
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def _operator(p, quad, cells, lame=0):
    key = ("op", p, quad, cells, lame)
    if key not in _cache:
        _cache[key] = pkg.HyperelasticityOperator(pkg.BrickMesh(p, cells, deform_amp=AMP), quad, pkg.COEF_STEP64, lam=LAME[lame][0], mu=LAME[lame][1])
    return _cache[key]


# ------------------------------------------------------------------ 1. parity: residual, state, tangent, cell ranges, accumulate, Dirichlet, padding
@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("p", range(1, 9))
def test_residual_state_and_tangent_match_numpy(p, quad):
    torch = _t()
    cells = parity_cells(p)
    ref = _reference(p, quad, cells)
    pr, u, v = ref["pr"], ref["u"], ref["v"]
    op = _operator(p, quad, cells)
    n, n_cells, cst = op.mf_data.n_local, pr.mesh.n_cells, pr.constrained
    assert n == pr.mesh.n_dofs and n_cells > workgroup_cells(p) and n_cells % workgroup_cells(p) != 0
    assert np.abs(u[:, cst]).max() > 0 and 0.19 < H.max_grad(pr, u) < 0.21
    sz = C.c_size_t()
    assert pkg.lib().bp5_hyperelasticity_state_size(op.mf_data.handle, C.byref(sz)) == 0 and sz.value == 10 * n_cells * (p + 1) ** 3 == op.state.numel()
    # ---- residual, overwrite: NaN-filled r, NaN source padding, a sentinel behind r; the state
    ut, vt = block(u, n), block(v, n)
    r = block(np.full((3, n), np.nan), n, pad_value=SENTINEL)
    op.state.fill_(float("nan"))
    op.residual(r, ut)
    got = r[:, :n].cpu().numpy()
    want = np.array(ref["r_cells"])
    want[:, cst] = 0.0
    e_r = errors(got, want)
    assert not got[:, cst].any()                                            # exact zeros on the Dirichlet rows of every block
    check_padding(r, n, SENTINEL)
    check_padding(ut, n, float("nan"))
    st, st_ref = op.state.cpu().numpy().reshape(10, -1), pr.to_device_layout(ref["state"]).reshape(10, -1)
    assert not np.isnan(st).any()
    e_b = np.abs(st[:9] - st_ref[:9]).max() / np.abs(st_ref[:9]).max()
    e_j = np.abs(st[9] - st_ref[9]).max() / np.abs(st_ref[9]).max()
    print(f"p={p} quad={quad} cells={cells}: residual {max(e_r):.2e}, state B {e_b:.2e}, ln J {e_j:.2e}", end="")
    tol_r, tol_b, tol_j = ref["tol"]
    assert max(e_r) <= tol_r and e_b <= tol_b and e_j <= tol_j, (e_r, e_b, e_j, ref["tol"])
    # ---- tangent at that state, overwrite
    d = block(np.full((3, n), np.nan), n, pad_value=SENTINEL)
    op.vmult(d, vt)
    got = d[:, :n].cpu().numpy()
    want = np.array(ref["t_cells"])
    want[:, cst] = v[:, cst]
    e_t = errors(got, want)
    print(f", tangent {max(e_t):.2e}", end="")
    assert max(e_t) <= TOL_OP, e_t
    assert np.array_equal(got[:, cst], v[:, cst])                           # the Dirichlet copy
    check_padding(d, n, SENTINEL)
    check_padding(vt, n, float("nan"))
    # ---- accumulate (zero_dst = 0) onto a non-zero dst: residual (Dirichlet rows 0) and tangent (Dirichlet rows copied)
    pre = np.random.default_rng(5).uniform(-1, 1, (3, n))
    op.do_zero_out = False
    try:
        r = block(pre, n, pad_value=SENTINEL)
        op.residual(r, ut)
        d = block(pre, n, pad_value=SENTINEL)
        op.vmult(d, vt)
    finally:
        op.do_zero_out = True
    want = pre + ref["r_cells"]
    want[:, cst] = 0.0
    e_ra = errors(r[:, :n].cpu().numpy(), want)
    want = pre + ref["t_cells"]
    want[:, cst] = v[:, cst]
    e_ta = errors(d[:, :n].cpu().numpy(), want)
    print(f", accumulate {max(e_ra):.2e} / {max(e_ta):.2e}", end="")
    assert max(e_ra) <= tol_r and max(e_ta) <= TOL_OP, (e_ra, e_ta)
    assert not r[:, :n].cpu().numpy()[:, cst].any()
    check_padding(r, n, SENTINEL)
    check_padding(d, n, SENTINEL)
    # ---- two ragged cell ranges, then an empty one
    for c0, c1 in ((1, n_cells - 1), (0, workgroup_cells(p) + 1)):
        d = block(pre, n, pad_value=SENTINEL)
        op.cell_loop(vt, d, c0, c1)
        want = pr.tangent_cells(u, v, (c0, c1), dst=pre.copy())
        e_c = errors(d[:, :n].cpu().numpy(), want)
        print(f", cells [{c0}, {c1}) {max(e_c):.2e}", end="")
        assert max(e_c) <= TOL_OP, e_c
        check_padding(d, n, SENTINEL)
    before = d.clone()
    op.cell_loop(vt, d, 2, 2)
    assert torch.equal(torch.nan_to_num(d), torch.nan_to_num(before))
    print()
    # ---- the kernel a solve reports
    ctl = pkg.IterationNumberControl(1, 0.0)
    b = block(v, n, pad_value=0.0, extra=0)
    pkg.SolverCG(ctl).solve(op, op.initialize_block_vector(), b, None)
    tw, lpc, tpb = (1, (p + 1) ** 2, 4) if p <= 3 else (4, (p + 1) ** 2, 1)
    assert ctl.last_step() == 1 and not ctl.dot_products_fused
    assert ctl.apply_kernel.startswith("apply_pencil_hyperelasticity_kernel<") and ctl.apply_kernel == \
        f"apply_pencil_hyperelasticity_kernel<{p},{'true' if quad else 'false'},{tw},{lpc},{tpb},tangent>", ctl.apply_kernel


def test_second_lame_pair_and_the_state_of_a_fresh_operator():
    """the nearly incompressible pair (lambda = 10, mu = 1); a fresh operator holds the state of u = 0: its vmult is the linear operator's"""
    p, quad, cells = 2, 0, (5, 4, 4)
    ref = _reference(p, quad, cells, 1)
    pr, u, v = ref["pr"], ref["u"], ref["v"]
    op = pkg.HyperelasticityOperator(pkg.BrickMesh(p, cells, deform_amp=AMP), quad, pkg.COEF_STEP64, lam=LAME[1][0], mu=LAME[1][1])
    n, cst = op.mf_data.n_local, pr.constrained
    vt = block(v, n)
    d = block(np.full((3, n), np.nan), n, pad_value=SENTINEL)
    op.vmult(d, vt)
    e_lin = errors(d[:, :n].cpu().numpy(), pr.vmult(v))
    r = block(np.full((3, n), np.nan), n, pad_value=SENTINEL)
    op.residual(r, block(u, n))
    want = np.array(ref["r_cells"])
    want[:, cst] = 0.0
    e_r = errors(r[:, :n].cpu().numpy(), want)
    op.vmult(d, vt)
    want = np.array(ref["t_cells"])
    want[:, cst] = v[:, cst]
    e_t = errors(d[:, :n].cpu().numpy(), want)
    print(f"lame {LAME[1]}: linear limit {max(e_lin):.2e}, residual {max(e_r):.2e}, tangent {max(e_t):.2e}")
    assert max(e_lin) <= TOL_OP and max(e_r) <= ref["tol"][0] and max(e_t) <= TOL_OP


def test_a_point_with_negative_determinant_gives_nan_not_a_trap():
    """J <= 0 at a quadrature point: NaN in the state and in r (documented in bp5.h); the call itself succeeds"""
    p, quad, cells = 2, 0, (5, 4, 4)
    pr = _reference(p, quad, cells)["pr"]
    op = _operator(p, quad, cells)
    n = op.mf_data.n_local
    u = -1.5 * pr.mesh.coords.T                                             # F = -0.5 I: J < 0 everywhere
    r = block(np.zeros((3, n)), n, pad_value=SENTINEL)
    op.residual(r, block(u, n))
    got = r[:, :n].cpu().numpy()
    free = np.setdiff1d(np.arange(n), pr.constrained)
    assert np.isnan(got[:, free]).all() and not got[:, pr.constrained].any() and np.isnan(op.state.cpu().numpy()).all()
    check_padding(r, n, SENTINEL)
    op.residual(r, block(np.zeros((3, n)), n))                               # (leave the cached operator with a finite state)


# ------------------------------------------------------------------ 2. CG on the tangent
def _cg_setup(name):
    pr, u, b, its = H.cg_case(name)
    op = _operator(pr.mesh.p, 0, pr.mesh.cells)
    n = op.mf_data.n_local
    r = op.initialize_block_vector()
    ut = op.initialize_block_vector()
    ut[:, :n] = _t().from_numpy(np.array(u)).to("cuda:0")
    op.residual(r, ut)                                                       # the state of u
    return pr, u, b, its, op


def _cg(op, b, pre, max_iter, tol=0.0, check_every=0):
    n = op.mf_data.n_local
    bt, x = op.initialize_block_vector(), op.initialize_block_vector()
    bt[:, :n] = _t().from_numpy(np.array(b)).to("cuda:0")
    x[:, :n] = float("nan")
    ctl = pkg.SolverControl(max_iter, tol) if tol else pkg.IterationNumberControl(max_iter, 0.0)
    pkg.SolverCG(ctl, check_every=check_every).solve(op, x, bt, pre)
    return x[:, :n].cpu().numpy(), ctl


@pytest.mark.parametrize("name", ["p2", "p4"])
def test_cg_on_the_tangent_with_identity_chebyshev_and_v_cycle(name):
    """fixed iteration counts against elasticity_ref.cg / elasticity_mg_ref.pcg on the reference tangent, the preconditioners those of the LINEAR
    operator (numpy twins: elasticity_mg_ref.Level / VCycle); then the iteration counts to 1e-8 ||b||"""
    pr, u, b, its, op = _cg_setup(name)
    p, cells = pr.mesh.p, pr.mesh.cells
    A = lambda w: pr.tangent(u, w)        # noqa: E731
    inv = op.linear.compute_diagonal(invert=True)
    ch = pkg.ElasticityPreconditionChebyshev().initialize(op.linear, pkg.ElasticityPreconditionChebyshev.AdditionalData(
        degree=4, smoothing_range=20.0, eig_cg_n_iterations=8, preconditioner=pkg.DiagonalMatrix(inv)))
    mg = pkg.ElasticityPreconditionMG(pkg.make_elasticity_mg_hierarchy(op.linear))
    Lc = M.Level(p, cells, 1.0, O.QUAD_GAUSS, AMP, O.kappa_step64, LAME[0][0], LAME[0][1], 4, 20.0, 8)
    V = M.VCycle(p, cells)
    tol = 1e-8 * np.linalg.norm(b)
    counts = {}
    for label, pre, P in (("identity", None, None), ("chebyshev", ch, Lc.vmult), ("v-cycle", mg, V.vmult)):
        xr, k, rr = E.cg(A, b, its) if P is None else M.pcg(A, P, b, its)
        x, ctl = _cg(op, b, pre, its)
        e = errors(x, xr)
        print(f"{name} {label}: {ctl.last_step()} iterations, per-block error {e}, residual {ctl.last_value():.6e} (numpy {rr:.6e})", end="")
        assert ctl.last_step() == k == its and max(e) <= TOL_CG and abs(ctl.last_value() - rr) <= 1e-8 * rr
        assert ctl.apply_kernel.startswith("apply_pencil_hyperelasticity_kernel<") and not ctl.dot_products_fused
        _, kr, _ = E.cg(A, b, 2000, tol=tol) if P is None else M.pcg(A, P, b, 400, tol=tol)
        _, ctl = _cg(op, b, pre, 2000, tol=tol, check_every=3 if label == "chebyshev" else 0)
        counts[label] = ctl.last_step()
        print(f"; to 1e-8: {ctl.last_step()} (numpy {kr})")
        # (the preconditioned solves take a few steps: the count of the numpy twin +- 1, as tests/test_gpu_elasticity_mg.py; the unpreconditioned one
        # takes hundreds, over which CG loses orthogonality to rounding and the step at which ||g|| crosses the tolerance moves by a few: 5 %)
        assert abs(ctl.last_step() - kr) <= (1 if P is not None else 0.05 * kr) and ctl.last_value() <= tol
    assert counts["v-cycle"] < counts["chebyshev"] < counts["identity"], counts
    ch.clear()
    mg.clear()


# ------------------------------------------------------------------ 3. Newton
def _newton(backtracking, preconditioned):
    pr, f, u_ref, info = H.newton_case(backtracking)
    prm = H.BACKTRACK_PARAMS if backtracking else H.NEWTON_PARAMS
    op = pkg.HyperelasticityOperator(pkg.BrickMesh(H.NEWTON_P, H.NEWTON_CELLS, deform_amp=AMP), pkg.QUAD_GAUSS, pkg.COEF_STEP64, lam=LAME[0][0], mu=LAME[0][1])
    n = op.mf_data.n_local
    ft = block(f, n, pad_value=SENTINEL)
    ut = block(np.zeros((3, n)), n, pad_value=SENTINEL)
    mg = pkg.ElasticityPreconditionMG(pkg.make_elasticity_mg_hierarchy(op.linear), ld=ut.shape[1]) if preconditioned else None
    solver = pkg.NewtonSolver(pkg.SolverControl(prm["max_newton"], prm["abs_tol"]), pkg.SolverControl(prm["cg_max_iter"], 0.0), rel_tol=prm["rel_tol"],
                              cg_rel_tol=prm["cg_rel_tol"], max_backtracks=prm["max_backtracks"])
    status = 0
    try:
        solver.solve(op, ut, ft, mg)
    except pkg.BP5Error as e:
        status = e.status
    check_padding(ut, n, SENTINEL)
    check_padding(ft, n, SENTINEL)
    if mg is not None:
        mg.clear()
    return pr, u_ref, info, op, solver, status, ut[:, :n].cpu().numpy()


@pytest.mark.parametrize("preconditioned", [False, True])
def test_newton_converges_as_the_reference(preconditioned):
    """the clamped block under body force: the Newton iteration count of the reference, every history entry within 1e-6 relative until below
    1e-10 ||r_0||, the final u within 1e-8 relative -- without a preconditioner and with the V-cycle of the linear operator (the tangent solves run
    to 1e-12 ||r||, so the Newton iterates do not depend on the preconditioner beyond that)"""
    pr, u_ref, info, op, solver, status, u = _newton(False, preconditioned)
    print(f"preconditioned={preconditioned}: status {status}, {solver.newton_iterations} steps, {solver.total_cg_iterations} CG iterations "
          f"(numpy {info['total_cg_iterations']} without preconditioner), history {solver.residual_history}")
    assert status == 0 and info["status"] == "ok"
    assert solver.newton_iterations == info["newton_iterations"] and solver.backtracks == info["backtracks"] == 0
    hist, hist_ref = solver.residual_history, info["history"]
    assert len(hist) == len(hist_ref)
    for k, (a, b) in enumerate(zip(hist, hist_ref)):
        if b >= 1e-10 * hist_ref[0]:
            assert abs(a - b) <= 1e-6 * b, (k, a, b)
    assert hist[-1] <= 1e-10 * hist[0]
    e = rel(u, u_ref)
    print(f"  final u: {e:.2e}")
    assert e <= 1e-8
    if preconditioned:
        assert solver.total_cg_iterations < info["total_cg_iterations"] / 5
    # the state belongs to the accepted iterate: the tangent is the reference's at u_ref
    n = op.mf_data.n_local
    v = np.stack([O.deterministic_src(n, seed=60 + c) for c in range(3)])
    d = block(np.full((3, n), np.nan), n, pad_value=SENTINEL)
    op.vmult(d, block(v, n))
    assert max(errors(d[:, :n].cpu().numpy(), pr.tangent(u_ref, v))) <= 1e-8


def test_newton_backtracks_as_the_reference():
    """20 x the load, cut off after three steps: the same number of halvings, the same status, the same history"""
    pr, u_ref, info, op, solver, status, u = _newton(True, False)
    print(f"status {status} (numpy {info['status']}), {solver.newton_iterations} steps, {solver.backtracks} backtracks (numpy {info['backtracks']}), "
          f"history {solver.residual_history} (numpy {info['history']})")
    assert info["backtracks"] >= 1
    assert status == {"ok": 0, "no_convergence": 7, "breakdown": 6}[info["status"]]
    assert solver.backtracks == info["backtracks"] and solver.newton_iterations == info["newton_iterations"]
    for a, b in zip(solver.residual_history, info["history"]):
        assert abs(a - b) <= 1e-6 * b, (a, b)
    assert rel(u, u_ref) <= 1e-8


# ------------------------------------------------------------------ 4. refusals
def test_refusals_name_hyperelasticity_and_write_nothing():
    from deal_and_ceed_on_gpu_amd import _lib
    torch = _t()
    L = pkg.lib()
    mesh = pkg.BrickMesh(2, (3, 2, 2))
    comm = pkg.Communicator(0, 1)

    def ns(m):      # a hanging-node mesh of the oracle as the mesh object MatrixFree.reinit reads
        from types import SimpleNamespace
        return SimpleNamespace(degree=m.p, n=m.n, n_cells=m.n_cells, n_interior_cells=m.n_cells, n_owned=m.n_dofs, n_ghost=0, n_local=m.n_dofs,
                               n_global_dofs=m.n_dofs, l2g=m.l2g, coords=m.coords, constrained=m.constrained, n_neighbors=0,
                               neighbor_rank=np.zeros(0, np.int32), send_offsets=np.zeros(1, np.uint32), send_indices=np.zeros(0, np.uint32),
                               recv_offsets=np.zeros(1, np.uint32), cell_block_offsets=None, constraint_mask=m.constraint_mask, rank=0, n_ranks=1)
    cases = [(pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS_OVER), "BP5_QUAD_GAUSS_OVER"), (pkg.HelmholtzOperator(mesh, 0), "Helmholtz"), (pkg.MassOperator(mesh, 0), "mass"),
             (pkg.PoissonOperator(ns(O.HangingBrickMesh(2, 2, 2, 1, 3)), 0), "hanging"),
             (pkg.PoissonOperator(mesh, 0, geometry=pkg.GEOM_AFFINE), "affine"), (pkg.PoissonOperator(mesh, 0, geometry=pkg.GEOM_TRILINEAR), "trilinear"),
             (pkg.PoissonOperator(mesh, 0, metric_precision="float32"), "FP32"),
             (pkg.PoissonOperator(pkg.BrickMesh(2, (3, 2, 4), rank=1, n_ranks=2), 0, comm=comm), "communicator")]
    prm, res = _lib.CGParams(_lib.CG_PLAIN, 3, 0.0, 0, 0), _lib.CGResult()
    nprm, nres = _lib.NewtonParams(3, 0.0, 1e-8, prm, 1e-8, 2), _lib.NewtonResult()

    def all_calls(h, cp, sp, lam, mu, ld, bp, xp, n=None):
        calls = [L.bp5_hyperelasticity_residual(h, cp, sp, lam, mu, ld, bp, xp, 1), L.bp5_hyperelasticity_apply(h, cp, sp, lam, mu, ld, bp, xp, 1),
                 L.bp5_hyperelasticity_apply_cells(h, cp, sp, lam, mu, ld, bp, xp, 0, 1),
                 L.bp5_cg_solve_hyperelasticity(h, cp, sp, lam, mu, ld, None, None, bp, xp, C.byref(prm), C.byref(res)),
                 L.bp5_hyperelasticity_newton(h, cp, sp, lam, mu, ld, None, None, bp, xp, C.byref(nprm), C.byref(nres))]
        if n is not None:
            calls.append(L.bp5_hyperelasticity_state_size(h, C.byref(n)))
        return calls, L.bp5_last_error().decode()
    for op, word in cases:
        h = op.mf_data.handle
        x, b = op.initialize_block_vector(3), op.initialize_block_vector(3)
        b.fill_(1.0)
        ld = x.shape[1]
        coef, state = torch.zeros(16, dtype=torch.float64, device="cuda:0"), torch.zeros(16, dtype=torch.float64, device="cuda:0")   # never read or written
        n = C.c_size_t(7)
        calls, msg = all_calls(h, ptr(coef), ptr(state), 1.0, 1.0, ld, ptr(b), ptr(x), n)
        assert calls == [5] * 6 and word in msg and "hyperelasticity" in msg, (word, calls, msg)
        calls, msg = all_calls(h, ptr(coef), None, 1.0, 1.0, ld, ptr(b), ptr(x))                        # a null state: a layout error whatever the handle is
        assert calls == [1] * 5 and "state" in msg and "hyperelasticity" in msg, (word, calls, msg)
        calls, msg = all_calls(h, None, ptr(state), 1.0, 1.0, ld, ptr(b), ptr(x))
        assert calls == [1] * 5 and "null" in msg and "hyperelasticity" in msg, (word, calls, msg)
        torch.cuda.synchronize()
        assert float(x.abs().max()) == 0.0 and float((b - 1.0).abs().max()) == 0.0 and n.value == 7 and float(state.abs().max()) == 0.0
    comm.close()
    # arguments that need a good handle
    op = _operator(2, 0, (5, 4, 4))
    nl, h = op.mf_data.n_local, op.mf_data.handle
    x, b = op.initialize_block_vector(), op.initialize_block_vector()
    b.fill_(1.0)
    ld = x.shape[1]
    state0 = op.state.clone()
    small = (nl - 1) - ((nl - 1) & 1)
    for (lam, mu, ldv, bb, xx), word in (((1.0, 1.0, small, b, x), "ld <"), ((1.0, 1.0, ld, x, x[1:]), "overlap"), ((1.0, 0.0, ld, b, x), "mu"),
                                         ((-1.0, 1.0, ld, b, x), "bulk"), ((float("nan"), 1.0, ld, b, x), "finite"), ((1.0, 1.0, ld + 1, b, x), "even")):
        calls, msg = all_calls(h, ptr(op.coef), ptr(op.state), lam, mu, ldv, ptr(bb), ptr(xx))
        assert calls == [1] * 5 and word in msg and "hyperelasticity" in msg, (word, calls, msg)
    st = L.bp5_hyperelasticity_apply_cells(h, ptr(op.coef), ptr(op.state), 1.0, 1.0, ld, ptr(b), ptr(x), 3, 999)
    assert st == 1 and "hyperelasticity" in L.bp5_last_error().decode()
    merged = _lib.CGParams(_lib.CG_MERGED, 3, 0.0, 0, 0)
    st = L.bp5_cg_solve_hyperelasticity(h, ptr(op.coef), ptr(op.state), 1.0, 1.0, ld, None, None, ptr(b), ptr(x), C.byref(merged), C.byref(res))
    msg = L.bp5_last_error().decode()
    assert st == 5 and "BP5_CG_MERGED" in msg and "hyperelasticity" in msg
    bad = _lib.NewtonParams(-1, 0.0, 1e-8, prm, 1e-8, 2)
    st = L.bp5_hyperelasticity_newton(h, ptr(op.coef), ptr(op.state), 1.0, 1.0, ld, None, None, ptr(b), ptr(x), C.byref(bad), C.byref(nres))
    assert st == 1 and "hyperelasticity" in L.bp5_last_error().decode()
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0 and float((b - 1.0).abs().max()) == 0.0 and torch.equal(torch.nan_to_num(op.state), torch.nan_to_num(state0))
    # the Python mirror
    ctl = pkg.IterationNumberControl(3, 0.0)
    for fn, status in ((lambda: pkg.SolverCGFullMerge(ctl).solve(op, x, b, None), 5), (lambda: pkg.SolverCG(ctl).solve(op, x, b, pkg.DiagonalMatrix()), 5),
                       (lambda: pkg.PreconditionChebyshev().initialize(op), 5), (lambda: pkg.PreconditionMG([op]), 5),
                       (lambda: pkg.NewtonSolver(ctl, ctl).solve(op.linear, x, b), 1)):
        with pytest.raises(pkg.BP5Error) as e:
            fn()
        assert e.value.status == status, str(e.value)
    assert float(x.abs().max()) == 0.0


# ------------------------------------------------------------------ 5. the neighbours' bits
def test_other_operators_of_the_mesh_keep_their_results():
    """A Poisson block-kernel vmult (deterministic: bitwise) and an ElasticityOperator.vmult (atomics: TOL_OP against its own first result and the
    reference) before and after hyperelastic calls on the same mesh -- the Poisson handle itself serving them with arrays of their own"""
    torch = _t()
    L = pkg.lib()
    p, cells = 4, (6, 5, 5)
    mesh = pkg.BrickMesh(p, cells, deform_amp=AMP, cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1)
    po = pkg.PoissonOperator(mesh, 0, pkg.COEF_STEP64)
    po.mf_data.set_apply_variant(56)
    el = pkg.ElasticityOperator(mesh, 0, pkg.COEF_STEP64, lam=LAME[0][0], mu=LAME[0][1])
    n, h = po.mf_data.n_local, po.mf_data.handle
    s = torch.from_numpy(O.deterministic_src(n, seed=9)).to("cuda:0")
    s3 = el.initialize_block_vector()
    for c in range(3):
        s3[c, :n] = torch.from_numpy(O.deterministic_src(n, seed=20 + c)).to("cuda:0")

    def others():
        d = po.initialize_dof_vector()
        po.vmult(d, s)
        d3 = el.initialize_block_vector()
        el.vmult(d3, s3)
        return d, d3
    before = others()
    sz = C.c_size_t()
    assert L.bp5_elasticity_coef_size(h, C.byref(sz)) == 0
    coef = torch.empty(sz.value, dtype=torch.float64, device="cuda:0")
    assert L.bp5_hyperelasticity_state_size(h, C.byref(sz)) == 0
    state = torch.empty(sz.value, dtype=torch.float64, device="cuda:0")
    u, r, t = el.initialize_block_vector(), el.initialize_block_vector(), el.initialize_block_vector()
    u[:, :n] = 0.01 * s3[:, :n]
    ld = u.shape[1]
    lam, mu = LAME[0]
    assert L.bp5_elasticity_compute_metric(h, ptr(coef)) == 0
    assert L.bp5_hyperelasticity_residual(h, ptr(coef), ptr(state), lam, mu, ld, ptr(u), ptr(r), 1) == 0
    assert L.bp5_hyperelasticity_apply(h, ptr(coef), ptr(state), lam, mu, ld, ptr(s3), ptr(t), 1) == 0
    assert float(r.abs().max()) > 0 and float(t.abs().max()) > 0 and bool(torch.isfinite(state).all())
    from deal_and_ceed_on_gpu_amd import _lib
    prm, res = _lib.CGParams(_lib.CG_PLAIN, 3, 0.0, 0, 0), _lib.CGResult()
    assert L.bp5_cg_solve_hyperelasticity(h, ptr(coef), ptr(state), lam, mu, ld, None, None, ptr(r), ptr(t), C.byref(prm), C.byref(res)) == 0 and res.iterations == 3
    after = others()
    assert torch.equal(before[0], after[0])
    e = errors(after[1][:, :n].cpu().numpy(), before[1][:, :n].cpu().numpy())
    print(f"elasticity vmult before / after: {max(e):.2e}")
    assert max(e) <= TOL_OP


# ------------------------------------------------------------------ 6. the example
def test_example_prints_a_converging_history():
    """examples/bp5_hyperelasticity (the C ABI alone) on the Newton case: the residual history of the Python solve"""
    exe = os.path.join(bp5_pkg.ROOT, "examples", "bp5_hyperelasticity")
    pr, f, u_ref, info = H.newton_case()
    txt = subprocess.run([exe, str(H.NEWTON_P), *[str(c) for c in H.NEWTON_CELLS], repr(AMP), repr(LAME[0][0]), repr(LAME[0][1]), repr(H.NEWTON_LOAD)],
                         capture_output=True, text=True, timeout=300, check=True).stdout
    print(txt)
    hist = [float(l.split()[2]) for l in txt.splitlines() if l.startswith("newton_step")]
    got = {l.split()[0]: l.split()[1] for l in txt.splitlines() if l.strip() and not l.startswith("newton_step")}
    assert int(got["newton_iterations"]) == info["newton_iterations"] and int(got["backtracks"]) == 0 and got["status"] == "0"
    assert len(hist) == len(info["history"]) and all(b < a for a, b in zip(hist, hist[1:]))
    for a, b in zip(hist, info["history"]):
        if b >= 1e-10 * info["history"][0]:
            assert abs(a - b) <= 1e-6 * b, (a, b)
