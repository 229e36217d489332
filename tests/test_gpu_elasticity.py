"""Linear elasticity on the GPU (bp5_elasticity_*, bp5_cg_solve_elasticity; ElasticityOperator): the ten planes, the coupled three-component
operator at every degree and both quadratures against the numpy statement (tests/elasticity_ref.py, pinned by tests/test_elasticity_cpu.py), the
rigid-body null space, the coupling that separates it from CEED BP6, the three diagonals, the solve, every refusal, the bits of the scalar paths
of a handle that also serves elasticity, and the example.  The kernel scatters with atomics: results are compared to the project's tolerances
(1e-13 operator, 1e-11 CG), never bitwise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import elasticity_ref as R

pytestmark = pytest.mark.gpu
pkg = bp5_pkg.load()
TOL_OP = 1e-13     # one operator application (rounding + atomic summation order)
TOL_CG = 1e-11     # CG solution vector at a fixed iteration count
SENTINEL = -7.25e30
AMP = 0.04
LAME = R.LAME
_cache = {}
# the name bp5_cg_result.apply_kernel reports, per (degree, GLL): the degree's default pencil shape
KERNEL = {
    (1, 0): "apply_pencil_elasticity_kernel<1,false,1,4,4>", (1, 1): "apply_pencil_elasticity_kernel<1,true,1,4,4>",
    (2, 0): "apply_pencil_elasticity_kernel<2,false,1,9,4>", (2, 1): "apply_pencil_elasticity_kernel<2,true,1,9,4>",
    (3, 0): "apply_pencil_elasticity_kernel<3,false,1,16,4>", (3, 1): "apply_pencil_elasticity_kernel<3,true,1,16,4>",
    (4, 0): "apply_pencil_elasticity_kernel<4,false,4,25,1>", (4, 1): "apply_pencil_elasticity_kernel<4,true,4,25,1>",
    (5, 0): "apply_pencil_elasticity_kernel<5,false,4,36,1>", (5, 1): "apply_pencil_elasticity_kernel<5,true,4,36,1>",
    (6, 0): "apply_pencil_elasticity_kernel<6,false,4,49,1>", (6, 1): "apply_pencil_elasticity_kernel<6,true,4,49,1>",
    (7, 0): "apply_pencil_elasticity_kernel<7,false,4,64,1>", (7, 1): "apply_pencil_elasticity_kernel<7,true,4,64,1>",
    (8, 0): "apply_pencil_elasticity_kernel<8,false,4,81,1>", (8, 1): "apply_pencil_elasticity_kernel<8,true,4,81,1>",
}


def _t():
    import torch
    return torch


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def launch_shape(p, n_cells):
    """(cells per team, teams, workgroups) of the degree's default pencil launch (csrc/bp5_device.hpp: DefaultPencil)"""
    tw, lpc, tpb = (1, (p + 1) ** 2, 4) if p <= 3 else (4, (p + 1) ** 2, 1)
    cpt = 64 * tw // lpc
    teams = -(-n_cells // cpt)
    return cpt, teams, -(-teams // tpb)


def _problem(p, quad, cells, lame=0, free=False):
    """reference problem, a three-block source (non-zero on the boundary) and its vmult -- computed once, never changed"""
    key = (p, quad, cells, lame, free)
    if key not in _cache:
        pr = R.Problem(p, cells, quad, deform_amp=AMP, kappa=O.kappa_step64, lam=LAME[lame][0], mu=LAME[lame][1], free=free)
        src = np.stack([O.deterministic_src(pr.mesh.n_dofs, seed=60 + c) for c in range(3)])
        ref = pr.vmult(src)
        for a in (src, ref):
            a.setflags(write=False)
        _cache[key] = (pr, src, ref)
    return _cache[key]


def _operator(p, quad, cells, lame=0, free=False, amp=AMP, coefficient=None):
    key = ("op", p, quad, cells, lame, free, amp, coefficient)
    if key not in _cache:
        mesh = pkg.BrickMesh(p, cells, deform_amp=amp)
        if free:
            mesh.constrained = np.zeros(0, np.uint32)          # no Dirichlet DoFs: the rigid-body modes are the null space
        _cache[key] = pkg.ElasticityOperator(mesh, quad, pkg.COEF_STEP64 if coefficient is None else coefficient, lam=LAME[lame][0], mu=LAME[lame][1])
    return _cache[key]


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


def errors(got, ref):
    return [rel(got[c], ref[c]) for c in range(3)]


# ------------------------------------------------------------------ 1. planes
@pytest.mark.parametrize("p", [1, 2, 4, 8])
@pytest.mark.parametrize("quad", [0, 1])
def test_planes(p, quad):
    """the ten planes against the reference K, kappa JxW through the numpy restatement of coef_off; the size"""
    cells = (3, 2, 2)
    pr, _, _ = _problem(p, quad, cells)
    op = _operator(p, quad, cells)
    n = C.c_size_t()
    assert pkg.lib().bp5_elasticity_coef_size(op.mf_data.handle, C.byref(n)) == 0
    assert n.value == 10 * pr.mesh.n_cells * (p + 1) ** 3 == op.coef.numel()
    got, want = op.coef.cpu().numpy().reshape(10, -1), R.planes_device_layout(pr).reshape(10, -1)
    e_k = np.abs(got[:9] - want[:9]).max() / np.abs(want[:9]).max()          # the nine entries of K share one scale (the inverse mixes them)
    e_s = np.abs(got[9] - want[9]).max() / np.abs(want[9]).max()
    print(f"p={p} quad={quad}: K {e_k:.2e}, kappa JxW {e_s:.2e}")
    assert e_k <= 1e-13 and e_s <= 1e-13, (e_k, e_s)


# ------------------------------------------------------------------ 2. operator parity
@pytest.mark.parametrize("cells,lame", [((3, 2, 2), 0), ((3, 2, 2), 1), ((13, 1, 1), 1)])
@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("p", range(1, 9))
def test_operator_parity(p, quad, cells, lame):
    """(13, 1, 1) ends in a partly filled team at every degree"""
    torch = _t()
    pr, src, ref = _problem(p, quad, cells, lame)
    op = _operator(p, quad, cells, lame)
    n, n_cells = op.mf_data.n_local, pr.mesh.n_cells
    assert n == pr.mesh.n_dofs
    if cells == (13, 1, 1):
        assert n_cells % launch_shape(p, n_cells)[0] != 0
    cst = pr.constrained
    # overwrite: NaN-filled dst, NaN source padding, a sentinel behind dst
    s = block(src, n)
    d = block(np.full((3, n), np.nan), n, pad_value=SENTINEL)
    assert d.shape[1] == n + (n & 1) + 66
    op.vmult(d, s)
    got = d[:, :n].cpu().numpy()
    assert not np.isnan(got).any()
    check_padding(d, n, SENTINEL)
    check_padding(s, n, float("nan"))
    e = errors(got, ref)
    print(f"p={p} quad={quad} cells={cells} lame={LAME[lame]}: vmult {max(e):.2e}", end="")
    assert max(e) <= TOL_OP, e
    assert np.array_equal(got[:, cst], src[:, cst])
    # accumulate (dst += A src, Dirichlet rows copied)
    pre = np.random.default_rng(5).uniform(-1, 1, (3, n))
    d = block(pre, n, pad_value=SENTINEL)
    op.do_zero_out = False
    try:
        op.vmult(d, s)
    finally:
        op.do_zero_out = True
    want = pre + pr.apply_cells(src)
    want[:, cst] = src[:, cst]
    e = errors(d[:, :n].cpu().numpy(), want)
    print(f", accumulate {max(e):.2e}", end="")
    assert max(e) <= TOL_OP, e
    check_padding(d, n, SENTINEL)
    # a ragged cell range, then an empty one
    c0, c1 = 1, n_cells - 1
    d = block(pre, n, pad_value=SENTINEL)
    op.cell_loop(s, d, c0, c1)
    want = pr.apply_cells(src, (c0, c1), dst=pre.copy())
    e = errors(d[:, :n].cpu().numpy(), want)
    print(f", cells [{c0}, {c1}) {max(e):.2e}")
    assert max(e) <= TOL_OP, e
    before = d.clone()
    op.cell_loop(s, d, 2, 2)
    assert torch.equal(torch.nan_to_num(d), torch.nan_to_num(before))
    check_padding(d, n, SENTINEL)
    # the kernel a solve reports
    ctl = pkg.IterationNumberControl(1, 0.0)
    b = block(src, n, pad_value=0.0, extra=0)
    pkg.SolverCG(ctl).solve(op, op.initialize_block_vector(), b, pkg.DiagonalMatrix())
    assert ctl.last_step() == 1 and ctl.apply_kernel == KERNEL[p, quad] and not ctl.dot_products_fused, ctl.apply_kernel


# ------------------------------------------------------------------ 3. one cell; many workgroups
@pytest.mark.parametrize("p,quad", [(1, 0), (2, 1), (4, 0), (8, 0)])
def test_one_cell(p, quad):
    pr, src, _ = _problem(p, quad, (1, 1, 1), 1)
    op = _operator(p, quad, (1, 1, 1), 1)
    n = op.mf_data.n_local
    s, d = block(src, n), block(np.zeros((3, n)), n, pad_value=SENTINEL)
    op.cell_loop(s, d)
    e = errors(d[:, :n].cpu().numpy(), pr.apply_cells(src))
    print(f"one cell p={p} quad={quad}: {max(e):.2e}")
    assert max(e) <= TOL_OP, e
    check_padding(d, n, SENTINEL)


MANY_WORKGROUPS = {2: ((5, 5, 11), 10), 4: ((7, 5, 3), 11)}     # degree -> (cells, workgroups): wave-local barrier family, workgroup barrier


@pytest.mark.parametrize("p", sorted(MANY_WORKGROUPS))
def test_many_workgroups(p):
    """the XCD remap blk = (blockIdx.x & 7) teams_per_xcd + (blockIdx.x >> 3) with teams_per_xcd > 1, idle trailing workgroups and a partly
    filled last team"""
    cells, expected = MANY_WORKGROUPS[p]
    n_cells = cells[0] * cells[1] * cells[2]
    cpt, teams, workgroups = launch_shape(p, n_cells)
    assert workgroups == expected >= 9 and workgroups % 8 != 0 and n_cells % cpt != 0, (cpt, teams, workgroups)
    pr, src, ref = _problem(p, 0, cells)
    op = _operator(p, 0, cells)
    n = op.mf_data.n_local
    s, d = block(src, n), block(np.full((3, n), np.nan), n, pad_value=SENTINEL)
    op.vmult(d, s)
    e = errors(d[:, :n].cpu().numpy(), ref)
    print(f"p={p} cells={cells} workgroups={workgroups}: {max(e):.2e}")
    assert max(e) <= TOL_OP, e
    check_padding(d, n, SENTINEL)


# ------------------------------------------------------------------ 4. rigid-body modes
@pytest.mark.parametrize("p,quad", [(2, 0), (3, 1), (4, 0), (5, 0)])
def test_rigid_body_modes_are_in_the_null_space(p, quad):
    """A handle without Dirichlet DoFs: translations and rotations u = omega x X, scaled to max |u| = 1 like the constant vector of the Poisson
    null-space test (tests/test_gpu_parity.py::test_full_size_properties), are annihilated to that test's bound -- 1e-11 times the largest
    operator coefficient times (p+1)^3; here the coefficient is (lambda + 2 mu) max kappa JxW |K[0][:]|^2, the elasticity counterpart of the
    merged metric's plane 0.  ||A u|| / ||A w|| for a deterministic w of the same norm is printed and held to the same 1e-11 (p+1)^3."""
    cells, lame = (3, 2, 2), 1
    pr, _, _ = _problem(p, quad, cells, lame, free=True)
    op = _operator(p, quad, cells, lame, free=True)
    assert op.mf_data.mesh.constrained.size == 0
    n = op.mf_data.n_local
    scale = (pr.lam + 2 * pr.mu) * float((pr.s * np.sum(pr.K[:, :, 0, :] ** 2, axis=-1)).max())
    bound = 1e-11 * (p + 1) ** 3
    w = pr.source(3)
    for m, u in enumerate(pr.rigid_body_modes()):
        u = u / np.abs(u).max()
        wm = w * (np.linalg.norm(u) / np.linalg.norm(w))
        du, dw = block(np.full((3, n), np.nan), n), block(np.full((3, n), np.nan), n)
        op.vmult(du, block(u, n))
        op.vmult(dw, block(wm, n))
        Au, Aw = du[:, :n].cpu().numpy(), dw[:, :n].cpu().numpy()
        ratio = np.linalg.norm(Au) / np.linalg.norm(Aw)
        print(f"p={p} quad={quad} mode {m}: max |A u| {np.abs(Au).max():.2e} (bound {bound * scale:.2e}), |A u| / |A w| {ratio:.2e}")
        assert np.abs(Au).max() < bound * scale and ratio < bound, (m, np.abs(Au).max(), ratio)


# ------------------------------------------------------------------ 5. coupling
@pytest.mark.parametrize("p,quad", [(2, 0), (4, 1)])
def test_a_source_in_one_component_reaches_the_others(p, quad):
    cells, lame = (3, 2, 2), 1
    pr, src, _ = _problem(p, quad, cells, lame)
    op = _operator(p, quad, cells, lame)
    n = op.mf_data.n_local
    one = np.array(src)
    one[1:] = 0.0
    ref = pr.vmult(one)
    d = block(np.full((3, n), np.nan), n, pad_value=SENTINEL)
    op.vmult(d, block(one, n))
    got = d[:, :n].cpu().numpy()
    e = errors(got, ref)
    print(f"p={p} quad={quad}: {e}, block norms {[float(np.linalg.norm(g)) for g in got]}")
    assert max(e) <= TOL_OP, e
    assert np.linalg.norm(got[1]) > 0.05 * np.linalg.norm(got[0]) and np.linalg.norm(got[2]) > 0.05 * np.linalg.norm(got[0])


# ------------------------------------------------------------------ 6. diagonal
@pytest.mark.parametrize("p,quad,lame", [(1, 0, 0), (2, 1, 1), (3, 0, 1), (4, 0, 0), (4, 1, 1), (6, 0, 1), (8, 0, 0)])
def test_diagonal(p, quad, lame):
    cells = (3, 2, 2)
    pr, _, _ = _problem(p, quad, cells, lame)
    op = _operator(p, quad, cells, lame)
    n = op.mf_data.n_local
    ref = pr.diagonal()
    d, inv = op.compute_diagonal(), op.compute_diagonal(invert=True)
    e, ei = errors(d[:, :n].cpu().numpy(), ref), errors(inv[:, :n].cpu().numpy(), 1.0 / ref)
    print(f"p={p} quad={quad} lame={LAME[lame]}: diagonal {max(e):.2e}, inverted {max(ei):.2e}")
    assert max(e) <= 1e-13 and max(ei) <= 1e-13, (e, ei)
    assert float(d[:, n:].abs().max() if d.shape[1] > n else 0.0) == 0.0
    assert not np.allclose(ref[0], ref[1], rtol=1e-3)         # the diagonals differ per component: three blocks, not one


# ------------------------------------------------------------------ 7. CG
def _solve(op, B, max_iter, tol=0.0, inv=None, check_every=0, extra=0):
    n = op.mf_data.n_local
    b = block(B, n, pad_value=0.0, extra=extra)
    x = block(np.full((3, n), np.nan), n, pad_value=SENTINEL, extra=extra) if extra else op.initialize_block_vector()
    di = block(inv, n, pad_value=float("nan"), extra=extra) if inv is not None else None
    ctl = pkg.IterationNumberControl(max_iter, tol)
    pkg.SolverCG(ctl, check_every=check_every).solve(op, x, b, pkg.DiagonalMatrix(di))
    if extra:
        check_padding(x, n, SENTINEL)
    return x[:, :n].cpu().numpy(), ctl


def _cg_operator(name):
    pr, b, inv, its = R.cg_case(name)
    op = _operator(pr.mesh.p, 0, pr.mesh.cells)
    return pr, b, inv, its, op


@pytest.mark.parametrize("name", ["p2", "p4"])
def test_cg_fixed_iterations_with_the_block_inverse_diagonal(name):
    pr, b, inv, its, op = _cg_operator(name)
    xr, k, res = R.cg(pr.vmult, b, its, inv_diag=inv)
    x, ctl = _solve(op, b, its, inv=inv, extra=66)
    e = errors(x, xr)
    print(f"{name}: {ctl.last_step()} iterations, per-block error {e}, residual {ctl.last_value():.12e} (reference {res:.12e})")
    assert ctl.last_step() == k == its and max(e) <= TOL_CG and abs(ctl.last_value() - res) <= 1e-10 * res
    assert ctl.apply_kernel == KERNEL[pr.mesh.p, 0] and not ctl.dot_products_fused
    # the device inverse diagonal is the one the reference used
    assert max(errors(op.compute_diagonal(invert=True)[:, :pr.mesh.n_dofs].cpu().numpy(), inv)) <= 1e-13


@pytest.mark.parametrize("check_every", [0, 3])
def test_cg_tolerance_stop(check_every):
    pr, b, inv, _, op = _cg_operator("p2")
    tol = 1e-8 * np.linalg.norm(b)
    xr, k, _ = R.cg(pr.vmult, b, 2000, tol=tol, inv_diag=inv)
    x, ctl = _solve(op, b, 2000, tol=tol, inv=inv, check_every=check_every)
    true_res = np.linalg.norm(b - pr.vmult(x))
    print(f"check_every={check_every}: iterations {ctl.last_step()} (numpy {k}), recomputed FP64 residual {true_res:.3e}, tolerance {tol:.3e}")
    assert ctl.last_step() == k and ctl.last_value() <= tol and true_res <= tol * (1 + 1e-6)


def test_cg_edges():
    """b = 0: no iteration, x exactly 0, the padding kept; max_iter = 0: x = 0 and the initial residual reported"""
    pr, b, inv, _, op = _cg_operator("p2")
    x, ctl = _solve(op, np.zeros_like(b), 10, inv=inv, extra=66)
    assert ctl.last_step() == 0 and not x.any() and ctl.last_value() == 0.0
    x, ctl = _solve(op, b, 0, inv=inv, extra=66)
    assert ctl.last_step() == 0 and not x.any() and abs(ctl.last_value() - np.linalg.norm(b)) <= 1e-13 * np.linalg.norm(b)
    # NULL == identity (the drift of this reference: tests/test_elasticity_cpu.py::test_identity_preconditioned_reference_is_stable_under_operator_noise)
    assert R.IDENTITY_CASE == "p2"
    x, ctl = _solve(op, b, R.IDENTITY_ITERATIONS)
    xr, k, res = R.cg(pr.vmult, b, R.IDENTITY_ITERATIONS)
    assert ctl.last_step() == k == R.IDENTITY_ITERATIONS and max(errors(x, xr)) <= TOL_CG


# ------------------------------------------------------------------ 8. refusals
def _raw(op_handle, coef, lam, mu, ld, s, d):
    L = pkg.lib()
    st = L.bp5_elasticity_apply(op_handle, C.c_void_p(coef.data_ptr()), lam, mu, ld, C.c_void_p(s.data_ptr()), C.c_void_p(d.data_ptr()), 1)
    return st, L.bp5_last_error().decode()


def test_unsupported_handles_are_refused_with_their_reason():
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
    cases = [(pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS_OVER), "BP5_QUAD_GAUSS_OVER"),
             (pkg.HelmholtzOperator(mesh, 0), "Helmholtz"),
             (pkg.MassOperator(mesh, 0), "mass"),
             (pkg.PoissonOperator(ns(O.HangingBrickMesh(2, 2, 2, 1, 3)), 0), "hanging"),
             (pkg.PoissonOperator(mesh, 0, geometry=pkg.GEOM_AFFINE), "affine"),
             (pkg.PoissonOperator(mesh, 0, metric_precision="float32"), "FP32"),
             (pkg.PoissonOperator(pkg.BrickMesh(2, (3, 2, 4), rank=1, n_ranks=2), 0, comm=comm), "communicator")]
    prm, res = _lib.CGParams(_lib.CG_PLAIN, 3, 0.0, 0, 0), _lib.CGResult()
    for op, word in cases:
        h = op.mf_data.handle
        x, b = op.initialize_block_vector(3), op.initialize_block_vector(3)
        b.fill_(1.0)
        ld = x.shape[1]
        coef = torch.zeros(16, dtype=torch.float64, device="cuda:0")     # never read: every call below is refused before any launch
        cp, xp, bp = C.c_void_p(coef.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(b.data_ptr())
        n = C.c_size_t(7)
        calls = [L.bp5_elasticity_coef_size(h, C.byref(n)), L.bp5_elasticity_compute_metric(h, cp), L.bp5_elasticity_apply(h, cp, 1.0, 1.0, ld, bp, xp, 1),
                 L.bp5_elasticity_apply_cells(h, cp, 1.0, 1.0, ld, bp, xp, 0, 1), L.bp5_elasticity_compute_diagonal(h, cp, 1.0, 1.0, ld, xp, 0),
                 L.bp5_cg_solve_elasticity(h, cp, 1.0, 1.0, ld, None, bp, xp, C.byref(prm), C.byref(res))]
        msg = L.bp5_last_error().decode()
        assert calls == [5] * 6 and word in msg and "elasticity" in msg, (word, calls, msg)
        # a null pointer is a layout error, named as such whatever the handle is
        nulls = [L.bp5_elasticity_compute_metric(h, None), L.bp5_elasticity_apply(h, None, 1.0, 1.0, ld, bp, xp, 1),
                 L.bp5_elasticity_apply_cells(h, None, 1.0, 1.0, ld, bp, xp, 0, 1), L.bp5_elasticity_compute_diagonal(h, None, 1.0, 1.0, ld, xp, 0),
                 L.bp5_cg_solve_elasticity(h, None, 1.0, 1.0, ld, None, bp, xp, C.byref(prm), C.byref(res)), L.bp5_elasticity_coef_size(h, None)]
        assert nulls == [1] * 6 and "null" in L.bp5_last_error().decode(), (word, nulls)
        torch.cuda.synchronize()
        assert float(x.abs().max()) == 0.0 and n.value == 7 and float(coef.abs().max()) == 0.0        # refused before any launch
    comm.close()
    # a rank-local slab with ghosts and no communicator is fine
    slab = pkg.ElasticityOperator(pkg.BrickMesh(2, (3, 2, 4), rank=1, n_ranks=2), 0, lam=1.0, mu=1.0)
    assert slab.mf_data.n_ghost > 0
    x, b = slab.initialize_block_vector(), slab.initialize_block_vector()
    slab.vmult(x, b)


def test_invalid_arguments_that_need_a_handle_and_the_merged_variant():
    from deal_and_ceed_on_gpu_amd import _lib
    L = pkg.lib()
    op = _operator(2, 0, (3, 2, 2))
    n, h = op.mf_data.n_local, op.mf_data.handle
    x, b = op.initialize_block_vector(), op.initialize_block_vector()
    b.fill_(1.0)
    ld = x.shape[1]
    small = (n - 1) - ((n - 1) & 1)                                          # even and < n_local
    for args, word in (((1.0, 1.0, small, b, x), "ld <"), ((1.0, 1.0, ld, x, x[1:]), "overlap"), ((1.0, 0.0, ld, b, x), "mu"),
                       ((-1.0, 1.0, ld, b, x), "bulk"), ((float("nan"), 1.0, ld, b, x), "finite"), ((1.0, 1.0, ld + 1, b, x), "even")):
        st, msg = _raw(h, op.coef, *args)
        assert st == 1 and word in msg and "elasticity" in msg, (args[:3], st, msg)
    st = L.bp5_elasticity_apply_cells(h, C.c_void_p(op.coef.data_ptr()), 1.0, 1.0, ld, C.c_void_p(b.data_ptr()), C.c_void_p(x.data_ptr()), 3, 99)
    assert st == 1 and "elasticity" in L.bp5_last_error().decode()
    prm, res = _lib.CGParams(_lib.CG_MERGED, 3, 0.0, 0, 0), _lib.CGResult()
    st = L.bp5_cg_solve_elasticity(h, C.c_void_p(op.coef.data_ptr()), 1.0, 1.0, ld, None, C.c_void_p(b.data_ptr()), C.c_void_p(x.data_ptr()), C.byref(prm), C.byref(res))
    msg = L.bp5_last_error().decode()
    assert st == 5 and "BP5_CG_MERGED" in msg and "elasticity" in msg
    # an inverse diagonal that is x, or starts inside it
    prm = _lib.CGParams(_lib.CG_PLAIN, 3, 0.0, 0, 0)
    big = _t().zeros((4, ld), dtype=_t().float64, device="cuda:0")
    for dg, xx in ((x, x), (big[1:], big[:3])):
        st = L.bp5_cg_solve_elasticity(h, C.c_void_p(op.coef.data_ptr()), 1.0, 1.0, ld, C.c_void_p(dg.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(xx.data_ptr()),
                                       C.byref(prm), C.byref(res))
        msg = L.bp5_last_error().decode()
        assert st == 1 and "inv_diag" in msg and "elasticity" in msg, (st, msg)
    _t().cuda.synchronize()
    assert float(x.abs().max()) == 0.0
    # the Python mirror
    for fn in (lambda: pkg.SolverCGFullMerge(pkg.IterationNumberControl(3, 0.0)).solve(op, x, b, pkg.DiagonalMatrix()),
               lambda: pkg.SolverCGFullMerge(pkg.IterationNumberControl(3, 0.0)).solve(op, x, b, pkg.PreconditionChebyshev()),
               lambda: pkg.PreconditionChebyshev().initialize(op), lambda: pkg.PreconditionMG([op]),
               lambda: pkg.SolverCG(pkg.IterationNumberControl(3, 0.0)).solve(op, x, b, pkg.PreconditionChebyshev())):
        with pytest.raises(pkg.BP5Error) as e:
            fn()
        assert e.value.status == 5, str(e.value)
    assert float(x.abs().max()) == 0.0


# ------------------------------------------------------------------ 9. the neighbours' bits
def test_scalar_paths_of_a_handle_keep_their_bits():
    """A scalar Poisson handle's block-kernel vmult and a five-iteration SolverCG solve are bit for bit identical before and after
    bp5_elasticity_compute_metric, an application, the diagonals and a solve ON THE SAME HANDLE (its plane count stays uncommitted by them)"""
    from deal_and_ceed_on_gpu_amd import _lib
    torch = _t()
    L = pkg.lib()
    p, cells = 4, (6, 5, 5)
    op = pkg.PoissonOperator(pkg.BrickMesh(p, cells, deform_amp=AMP, cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1), 0, pkg.COEF_STEP64)
    op.mf_data.set_apply_variant(56)
    n, h = op.mf_data.n_local, op.mf_data.handle
    s = torch.from_numpy(O.deterministic_src(n, seed=9)).to("cuda:0")
    op.mf_data.set_constrained_values(0.0, s)
    rhs = op.assemble_rhs()                                  # once: the load vector is assembled with atomics

    def scalar():
        d = op.initialize_dof_vector()
        op.vmult(d, s)
        x = op.initialize_dof_vector()
        ctl = pkg.IterationNumberControl(5, 0.0)
        pkg.SolverCG(ctl).solve(op, x, rhs, pkg.DiagonalMatrix())
        assert ctl.apply_kernel.startswith("apply_block_kernel<4,false,"), ctl.apply_kernel
        return d, x, ctl.last_value()

    before = scalar()
    nd = C.c_size_t()
    assert L.bp5_elasticity_coef_size(h, C.byref(nd)) == 0
    coef = torch.empty(nd.value, dtype=torch.float64, device="cuda:0")
    x, b, dg = op.initialize_block_vector(3), op.initialize_block_vector(3), op.initialize_block_vector(3)
    b[:, :n] = s
    ld = x.shape[1]
    cp = lambda t: C.c_void_p(t.data_ptr())
    lam, mu = LAME[0]
    assert L.bp5_elasticity_compute_metric(h, cp(coef)) == 0
    assert L.bp5_elasticity_apply(h, cp(coef), lam, mu, ld, cp(b), cp(x), 1) == 0
    assert float(x.abs().max()) > 0
    assert L.bp5_elasticity_compute_diagonal(h, cp(coef), lam, mu, ld, cp(dg), 1) == 0
    prm, res = _lib.CGParams(_lib.CG_PLAIN, 4, 0.0, 0, 0), _lib.CGResult()
    assert L.bp5_cg_solve_elasticity(h, cp(coef), lam, mu, ld, cp(dg), cp(b), cp(x), C.byref(prm), C.byref(res)) == 0
    assert res.iterations == 4 and res.apply_kernel.decode() == KERNEL[4, 0]
    after = scalar()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]) and before[2] == after[2]
    # ... and the handle still sizes its own array as before (six planes)
    sz = C.c_size_t()
    assert L.bp5_mf_coef_size(h, C.byref(sz)) == 0 and sz.value == op.coef.numel()


def test_a_fresh_handle_stays_uncommitted():
    """bp5_elasticity_coef_size and bp5_elasticity_compute_metric on a handle that has sized nothing yet leave its plane count open:
    bp5_mf_set_operator, which refuses a change of the plane count once an array has been sized or filled, still takes the seven-plane class, and
    bp5_mf_coef_size then reports seven planes; set back, the handle serves bp5_apply on six"""
    torch = _t()
    L = pkg.lib()
    p, cells = 2, (3, 2, 2)
    mf = pkg.MatrixFree().reinit(pkg.BrickMesh(p, cells, deform_amp=AMP), pkg.QUAD_GAUSS, pkg.COEF_STEP64)
    h, per_plane = mf.handle, 12 * (p + 1) ** 3
    nd = C.c_size_t()
    assert L.bp5_elasticity_coef_size(h, C.byref(nd)) == 0 and nd.value == 10 * per_plane
    coef = torch.empty(nd.value, dtype=torch.float64, device="cuda:0")
    assert L.bp5_elasticity_compute_metric(h, C.c_void_p(coef.data_ptr())) == 0
    pr, _, _ = _problem(p, 0, cells)
    assert np.abs(coef.cpu().numpy() - R.planes_device_layout(pr)).max() <= 1e-13 * np.abs(R.planes_device_layout(pr)).max()
    mf.set_operator(pkg.OP_HELMHOLTZ)                          # refused (BP5_ERR_INVALID) had the calls above committed a plane count
    assert mf.coef_size() == 7 * per_plane
    # the committed handle refuses the change, which is what the line above would have met
    with pytest.raises(pkg.BP5Error) as e:
        mf.set_operator(pkg.OP_POISSON)
    assert e.value.status == 1
    # a second fresh handle: elasticity first, then the scalar operator on its own six planes
    op_el = pkg.ElasticityOperator(pkg.BrickMesh(p, cells, deform_amp=AMP), pkg.QUAD_GAUSS, pkg.COEF_STEP64, lam=LAME[0][0], mu=LAME[0][1])
    m2 = op_el.mf_data
    assert m2.coef_size() == 6 * per_plane
    c6 = m2.evaluate_coefficients()
    po = O.Problem(p, cells, O.QUAD_GAUSS, deform_amp=AMP, kappa=O.kappa_step64)
    s = O.deterministic_src(po.mesh.n_dofs, seed=3)
    d = torch.full((m2.n_local,), float("nan"), dtype=torch.float64, device="cuda:0")
    assert L.bp5_apply(m2.handle, C.c_void_p(c6.data_ptr()), C.c_void_p(torch.from_numpy(s).to("cuda:0").data_ptr()), C.c_void_p(d.data_ptr()), 1) == 0
    assert rel(d.cpu().numpy(), po.vmult(s)) <= TOL_OP


# ------------------------------------------------------------------ 10. the example
def test_example_reproduces_the_python_solve():
    """examples/bp5_elasticity (the C ABI alone): iteration count and per-component L2 norms of the Python solve of the same problem"""
    exe = os.path.join(bp5_pkg.ROOT, "examples", "bp5_elasticity")
    lam, mu = LAME[0]
    txt = subprocess.run([exe, "2", "6", "5", "4", "0.04", repr(lam), repr(mu), "1e-8"], capture_output=True, text=True, timeout=300, check=True).stdout
    got = {l.split()[0]: l.split()[1] for l in txt.splitlines() if l.strip()}
    op = pkg.ElasticityOperator(pkg.BrickMesh(2, (6, 5, 4), deform_amp=0.04), pkg.QUAD_GAUSS, pkg.COEF_STEP64, lam=lam, mu=mu)
    n = op.mf_data.n_local
    b, x = op.initialize_block_vector(), op.initialize_block_vector()
    b[2, :n] = -op.assemble_rhs()
    ctl = pkg.SolverControl(10000, 1e-8 * float(b[2, :n].norm()))
    pkg.SolverCG(ctl).solve(op, x, b, pkg.DiagonalMatrix(op.compute_diagonal(invert=True)))
    norms = [op.l2_norm_solution(x[c]) for c in range(3)]
    print(txt, ctl.last_step(), norms)
    assert int(got["iterations"]) == ctl.last_step() > 10 and got["apply_kernel"] == KERNEL[2, 0]
    for c in range(3):
        assert norms[c] > 0 and abs(float(got[f"l2_norm_{c}"]) - norms[c]) <= 1e-10 * norms[c], (c, got, norms)
