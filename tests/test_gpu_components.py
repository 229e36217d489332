"""Block vectors on the GPU (bp5_apply_components, bp5_cg_solve_components; CEED BP6): the n_components operator against the oracle per
component (O.vmult) and against the scalar entry points on every block, the stacked CG against its numpy statement (tests/components_ref.py:
O.cg_plain on concat(A v_c)), the refusals, the Python mirror and the facade example.  Every component count the header offers (1 ... 8) at
every degree; many workgroups at every degree; the CG where its grid is capped by the partial-sum row; the solver's edges.  The multi-component
kernel scatters with atomics: results are compared to the project's tolerances (1e-13 operator, 1e-11 CG), never bitwise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import components_ref as R
from test_components_cpu import (CAPPED_CELLS, CAPPED_ITERATIONS, EDGES, SEQUENCE, SEQUENCE_CELLS, SEQUENCE_ITERATIONS, capped_case, diag_case,
                                 sequence_case, zero_block_case)

pytestmark = pytest.mark.gpu
pkg = bp5_pkg.load()
TOL_OP = 1e-13     # one operator application (rounding + atomic summation order)
TOL_CG = 1e-11     # CG solution vector at a fixed iteration count
SENTINEL = -7.25e30
N_BLOCKS = 8       # BP5_MAX_COMPONENTS: every count the header offers
_cache = {}


def _t():
    import torch
    return torch


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _cells(p):
    return (3, 3, 2) if p <= 4 else (3, 2, 1)          # a partial last team at every degree (18 cells: 16 per team at p = 1, 7 at p = 2, ...)


def _problem(p, quad, cells=None, amp=0.04):
    """oracle problem, eight source blocks (different seeds, non-zero on the boundary) and O.vmult of each -- computed once, never changed"""
    cells = cells or _cells(p)
    key = (p, quad, cells, amp)
    if key not in _cache:
        pr = O.Problem(p, cells, quad, deform_amp=amp, kappa=O.kappa_step64)
        src = np.stack([O.deterministic_src(pr.mesh.n_dofs, seed=40 + c) for c in range(N_BLOCKS)])
        ref = R.vmult(pr, src)
        for a in (src, ref):
            a.setflags(write=False)
        _cache[key] = (pr, src, ref)
    return _cache[key]


def _operator(p, quad, cells=None, amp=0.04, **kw):
    key = ("op", p, quad, cells or _cells(p), amp, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = pkg.PoissonOperator(pkg.BrickMesh(p, cells or _cells(p), deform_amp=amp, **kw), quad, pkg.COEF_STEP64)
    return _cache[key]


def block(values, n_local, pad_value=float("nan"), extra=2):
    """(n_components, ld) tensor, ld = n_local rounded up to even + extra (even); rows hold `values`, the padding pad_value"""
    torch = _t()
    values = np.asarray(values)
    nc = values.shape[0]
    ld = n_local + (n_local & 1) + extra
    t = torch.full((nc, ld), pad_value, dtype=torch.float64, device="cuda:0")
    t[:, :n_local] = torch.from_numpy(np.array(values[:, :n_local])).to("cuda:0")
    return t


def check_padding(t, n_local, value):
    pad = t[:, n_local:].cpu().numpy()
    assert pad.size and (np.isnan(pad).all() if np.isnan(value) else (pad == value).all())


# ------------------------------------------------------------------ 1. operator parity
@pytest.mark.parametrize("nc", range(1, N_BLOCKS + 1))
@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("p", range(1, 9))
def test_operator_parity(p, quad, nc):
    torch = _t()
    pr, src, ref = _problem(p, quad)
    op = _operator(p, quad)
    n = op.mf_data.n_local
    s = block(src[:nc], n)
    d = block(np.full((nc, n), np.nan), n, pad_value=SENTINEL)
    op.vmult(d, s)
    got = d[:, :n].cpu().numpy()
    assert not np.isnan(got).any()
    check_padding(d, n, SENTINEL)
    check_padding(s, n, float("nan"))
    for c in range(nc):
        scalar = op.initialize_dof_vector()
        op.vmult(scalar, s[c, :n].clone())
        e_ref, e_scalar = rel(got[c], ref[c]), rel(got[c], scalar.cpu().numpy())
        print(f"p={p} quad={quad} nc={nc} c={c}: vs oracle {e_ref:.2e}, vs scalar vmult {e_scalar:.2e}")
        assert e_ref <= TOL_OP and e_scalar <= TOL_OP and rel(scalar.cpu().numpy(), ref[c]) <= TOL_OP
    x = op.initialize_block_vector(nc)
    ctl = pkg.IterationNumberControl(1, 0.0)
    pkg.SolverCG(ctl).solve(op, x, block(src[:nc], n, extra=0), pkg.DiagonalMatrix())
    assert ctl.last_step() == 1 and ctl.apply_kernel.startswith("apply_pencil_components_kernel<%d,%s," % (p, "true" if quad else "false")), ctl.apply_kernel
    del torch


# ------------------------------------------------------------------ 2. add mode
def _add_mode(p, nc):
    pr, src, ref = _problem(p, 0)
    src = src[:nc]
    op = pkg.PoissonOperator(pkg.BrickMesh(p, _cells(p), deform_amp=0.04), 0, pkg.COEF_STEP64)
    op.do_zero_out = False
    n = op.mf_data.n_local
    pre = np.random.default_rng(5).uniform(-1, 1, (nc, n))
    s, d = block(src, n), block(pre, n, pad_value=SENTINEL)
    op.vmult(d, s)
    got = d[:, :n].cpu().numpy()
    check_padding(d, n, SENTINEL)
    cst = pr.mesh.constrained.astype(np.int64)
    for c in range(nc):
        want = pre[c] + O.apply_cells(pr.mesh, pr.coef, pr.N, pr.D, src[c])
        want[cst] = src[c][cst]
        scalar = _t().from_numpy(pre[c].copy()).to("cuda:0")
        op.vmult(scalar, s[c, :n].clone())                                 # bp5_apply(..., zero_dst = 0) on the same prefill
        assert rel(got[c], want) <= TOL_OP and rel(got[c], scalar.cpu().numpy()) <= TOL_OP
        assert np.array_equal(got[c][cst], src[c][cst])


@pytest.mark.parametrize("p", [2, 4, 5])
def test_add_mode(p):
    _add_mode(p, 3)


@pytest.mark.parametrize("p", [2, 4, 5])
def test_add_mode_eight_components(p):
    _add_mode(p, N_BLOCKS)


# ------------------------------------------------------------------ 3. one cell
def _one_cell(p, nc):
    pr, src, ref = _problem(p, 0, cells=(1, 1, 1))
    op = _operator(p, 0, cells=(1, 1, 1))
    n = op.mf_data.n_local
    s, d = block(src[:nc], n), block(np.full((nc, n), np.nan), n, pad_value=SENTINEL)
    op.vmult(d, s)
    check_padding(d, n, SENTINEL)
    got = d[:, :n].cpu().numpy()
    assert not np.isnan(got).any()
    for c in range(nc):
        assert rel(got[c], ref[c]) <= TOL_OP


@pytest.mark.parametrize("p", [4, 8])
def test_one_cell(p):
    """a single, partially filled team: every other cell slot idle"""
    _one_cell(p, 3)


@pytest.mark.parametrize("p", [4, 8])
def test_one_cell_eight_components(p):
    """... and the longest component loop on it"""
    _one_cell(p, N_BLOCKS)


# ------------------------------------------------------------------ 3b. many workgroups at every degree
def launch_shape(p, n_cells):
    """(cells per team, teams, workgroups) of apply_pencil_components_kernel as bp5_device.hpp launches it: teams of 64 TW lanes, (p+1)^2 lanes
    per cell, TPB teams per workgroup -- one wave per team and four teams per workgroup up to p = 3, four waves and one team beyond"""
    tw, tpb = (1, 4) if p <= 3 else (4, 1)
    cpt = 64 * tw // (p + 1) ** 2
    teams = -(-n_cells // cpt)
    return cpt, teams, -(-teams // tpb)


# (cells, expected workgroups): more than one round of the eight XCDs (teams_per_xcd = 2 or 3), a count that is no multiple of 8 (idle trailing
# workgroups after the remap) and a partly filled last team -- and for p <= 3 a partly filled last workgroup too
MANY_WORKGROUPS = {1: ((12, 9, 6), 11), 2: ((8, 6, 5), 9), 3: ((6, 5, 5), 10), 4: ((9, 6, 4), 22), 5: ((6, 5, 4), 18), 6: ((7, 4, 3), 17),
                   7: ((9, 3, 3), 21), 8: ((5, 5, 2), 17)}


@pytest.mark.parametrize("nc", [1, N_BLOCKS])
@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("p", range(1, 9))
def test_many_workgroups(p, quad, nc):
    """the XCD remap blk = (blockIdx.x & 7) teams_per_xcd + (blockIdx.x >> 3) with teams_per_xcd > 1, idle trailing workgroups and a partly
    filled last team, at a stride far from n_local"""
    cells, expected = MANY_WORKGROUPS[p]
    n_cells = cells[0] * cells[1] * cells[2]
    cpt, teams, workgroups = launch_shape(p, n_cells)
    assert workgroups == expected >= 9 and workgroups % 8 != 0 and n_cells % cpt != 0, (cpt, teams, workgroups)
    pr, src, ref = _problem(p, quad, cells=cells)
    op = _operator(p, quad, cells=cells)
    n = op.mf_data.n_local
    assert n == pr.mesh.n_dofs and op.mf_data.mesh.n_cells == n_cells
    s = block(src[:nc], n, extra=1024)
    d = block(np.full((nc, n), np.nan), n, pad_value=SENTINEL, extra=1024)
    assert d.shape[1] == n + (n & 1) + 1024
    op.vmult(d, s)
    got = d[:, :n].cpu().numpy()
    assert not np.isnan(got).any()
    check_padding(d, n, SENTINEL)
    check_padding(s, n, float("nan"))
    cst = pr.mesh.constrained.astype(np.int64)
    errs = [rel(got[c], ref[c]) for c in range(nc)]
    print(f"p={p} quad={quad} nc={nc} cells={cells} workgroups={workgroups}: max error vs oracle {max(errs):.2e}")
    assert max(errs) <= TOL_OP
    for c in range(nc):
        assert np.array_equal(got[c][cst], src[c][cst])


# ------------------------------------------------------------------ 4. any numbering
@pytest.mark.parametrize("p,cells,kw", [(4, (9, 8, 6), dict(cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1)),
                                        (2, (9, 8, 5), dict(cell_block=(8, 8, 4), dof_numbering=1, cell_block_order=1))])
def test_brick_numbering_equals_lexicographic_through_the_permutation(p, cells, kw):
    pr, src, ref = _problem(p, 0, cells=cells)
    src = src[:3]
    lex = pkg.PoissonOperator(pkg.BrickMesh(p, cells, deform_amp=0.04), 0, pkg.COEF_STEP64)
    brk = pkg.PoissonOperator(pkg.BrickMesh(p, cells, deform_amp=0.04, **kw), 0, pkg.COEF_STEP64)
    n = lex.mf_data.n_local
    perm = brk.mf_data.mesh.global_ids.astype(np.int64)      # local index -> lexicographic id
    assert not np.array_equal(perm, np.arange(n))
    dl, db = block(np.full((3, n), np.nan), n), block(np.full((3, n), np.nan), n)
    lex.vmult(dl, block(src, n))
    brk.vmult(db, block(src[:, perm], n))
    for c in range(3):
        assert rel(db[c, :n].cpu().numpy(), dl[c, :n].cpu().numpy()[perm]) <= TOL_OP
        assert rel(db[c, :n].cpu().numpy(), ref[c][perm]) <= TOL_OP


def test_rank_local_slabs_with_ghosts_and_no_communicator():
    """the z-slab meshes of a two-rank run, one after the other, no communicator: ghost slots are just entries of the block.  Each rank leaves
    partial sums in owned + ghost entries; summed through global_ids they are the global operator, per component"""
    p, cells = 3, (3, 3, 4)
    pr = O.Problem(p, cells, 0, deform_amp=0.03, kappa=O.kappa_step64)
    src = np.stack([O.deterministic_src(pr.mesh.n_dofs, seed=60 + c) for c in range(3)])
    cst = pr.mesh.constrained.astype(np.int64)
    ref = np.stack([O.apply_cells(pr.mesh, pr.coef, pr.N, pr.D, s) for s in src])
    ref[:, cst] = 0.0
    total = np.zeros_like(ref)
    for r in range(2):
        mesh = pkg.BrickMesh(p, cells, deform_amp=0.03, rank=r, n_ranks=2)
        assert (mesh.n_ghost > 0) == (r > 0)
        g = mesh.global_ids.astype(np.int64)
        op = pkg.PoissonOperator(mesh, 0, pkg.COEF_STEP64)
        n = op.mf_data.n_local
        s, d = block(src[:, g], n), block(np.full((3, n), np.nan), n, pad_value=SENTINEL)
        op.vmult(d, s)
        check_padding(d, n, SENTINEL)
        got = d[:, :n].cpu().numpy()
        lc = mesh.constrained.astype(np.int64)
        assert np.array_equal(got[:, lc], src[:, g][:, lc])         # the Dirichlet copy, ghost rows included
        got[:, lc] = 0.0
        for c in range(3):
            np.add.at(total[c], g, got[c])
    for c in range(3):
        assert rel(total[c], ref[c]) <= TOL_OP


# ------------------------------------------------------------------ 5. nothing else moved
def test_scalar_block_kernel_is_untouched_by_a_components_call():
    torch = _t()
    cells = (8, 8, 4)
    op = pkg.PoissonOperator(pkg.BrickMesh(4, cells, deform_amp=0.04, cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1), 0, pkg.COEF_STEP64)
    op.mf_data.set_apply_variant(56)
    n = op.mf_data.n_local
    s = torch.from_numpy(O.deterministic_src(n, seed=9)).to("cuda:0")
    before, after = op.initialize_dof_vector(), op.initialize_dof_vector()
    op.vmult(before, s)
    ctl = pkg.IterationNumberControl(1, 0.0)
    pkg.SolverCG(ctl).solve(op, op.initialize_dof_vector(), s, pkg.DiagonalMatrix())
    assert ctl.apply_kernel.startswith("apply_block_kernel")
    sb = op.initialize_block_vector(3)
    sb[:, :n] = s
    db = op.initialize_block_vector(3)
    op.vmult(db, sb)
    pkg.SolverCG(pkg.IterationNumberControl(2, 0.0)).solve(op, op.initialize_block_vector(3), sb, pkg.DiagonalMatrix())
    op.vmult(after, s)
    assert torch.equal(before, after)
    for c in range(3):
        assert rel(db[c, :n].cpu().numpy(), before.cpu().numpy()) <= TOL_OP


# ------------------------------------------------------------------ 6. refusals
def _raw_apply(op, nc, ld, s, d):
    L = pkg.lib()
    st = L.bp5_apply_components(op.mf_data.handle, C.c_void_p(op.coef.data_ptr()) if op.coef is not None else None, nc, ld, C.c_void_p(s.data_ptr()),
                                C.c_void_p(d.data_ptr()), 1)
    return st, L.bp5_last_error().decode()


def test_unsupported_handles_are_refused_with_their_reason():
    from types import SimpleNamespace
    from deal_and_ceed_on_gpu_amd import _lib
    mesh = pkg.BrickMesh(2, (3, 2, 2))

    def ns(m):
        return SimpleNamespace(degree=m.p, n=m.n, n_cells=m.n_cells, n_interior_cells=m.n_cells, n_owned=m.n_dofs, n_ghost=0, n_local=m.n_dofs,
                               n_global_dofs=m.n_dofs, l2g=m.l2g, coords=m.coords, constrained=m.constrained, n_neighbors=0,
                               neighbor_rank=np.zeros(0, np.int32), send_offsets=np.zeros(1, np.uint32), send_indices=np.zeros(0, np.uint32),
                               recv_offsets=np.zeros(1, np.uint32), cell_block_offsets=None, constraint_mask=m.constraint_mask, rank=0, n_ranks=1)
    comm = pkg.Communicator(0, 1)
    cases = [(pkg.PoissonOperator(mesh, 0, metric_precision="float32"), "FP32"),
             (pkg.HelmholtzOperator(mesh, 0), "Helmholtz"),
             (pkg.PoissonOperator(ns(O.HangingBrickMesh(2, 2, 2, 1, 3)), 0), "hanging"),
             (pkg.PoissonOperator(mesh, 0, geometry=pkg.GEOM_AFFINE), "affine"),
             (pkg.PoissonOperator(pkg.BrickMesh(2, (3, 2, 4), rank=1, n_ranks=2), 0, comm=comm), "communicator")]
    for op, word in cases:
        x, b = op.initialize_block_vector(3), op.initialize_block_vector(3)
        with pytest.raises(pkg.BP5Error) as e:
            op.vmult(x, b)
        assert e.value.status == 5 and word in str(e.value), (word, str(e.value))
        with pytest.raises(pkg.BP5Error) as e:
            pkg.SolverCG(pkg.IterationNumberControl(3, 0.0)).solve(op, x, b, pkg.DiagonalMatrix())
        assert e.value.status == 5 and word in str(e.value), (word, str(e.value))
        assert float(x.abs().max()) == 0.0                                  # refused before any launch
    comm.close()
    # a known CG variant this solver does not offer, and the one INVALID refusal that needs a handle
    op = _operator(2, 0)
    n = op.mf_data.n_local
    x, b = op.initialize_block_vector(3), op.initialize_block_vector(3)
    prm, res = _lib.CGParams(_lib.CG_MERGED, 3, 0.0, 0, 0), _lib.CGResult()
    L = pkg.lib()
    st = L.bp5_cg_solve_components(op.mf_data.handle, C.c_void_p(op.coef.data_ptr()), 3, x.shape[1], None, C.c_void_p(b.data_ptr()), C.c_void_p(x.data_ptr()),
                                   C.byref(prm), C.byref(res))
    assert st == 5 and "BP5_CG_MERGED" in L.bp5_last_error().decode()
    small = (n - 1) - ((n - 1) & 1)                                          # even and < n_local
    st, msg = _raw_apply(op, 3, small, b, x)
    assert st == 1 and "ld <" in msg, msg
    st, msg = _raw_apply(op, 2, x.shape[1], x, x[1:])                        # dst starts inside src
    assert st == 1 and "overlap" in msg, msg


def test_python_mirror_refuses_block_vectors_where_they_are_not_offered():
    op = _operator(2, 0)
    x, b = op.initialize_block_vector(3), op.initialize_block_vector(3)
    assert tuple(x.shape) == (3, op.mf_data.n_local + (op.mf_data.n_local & 1)) and x.is_contiguous() and float(x.abs().max()) == 0.0
    with pytest.raises(pkg.BP5Error) as e:
        pkg.SolverCGFullMerge(pkg.IterationNumberControl(3, 0.0)).solve(op, x, b, pkg.DiagonalMatrix())
    assert e.value.status == 5
    cheb = pkg.PreconditionChebyshev().initialize(op, pkg.PreconditionChebyshev.AdditionalData(degree=2, preconditioner=pkg.DiagonalMatrix(op.compute_diagonal(invert=True))))
    with pytest.raises(pkg.BP5Error) as e:
        cheb.vmult(x, b)
    assert e.value.status == 5
    with pytest.raises(pkg.BP5Error) as e:
        pkg.SolverCG(pkg.IterationNumberControl(3, 0.0)).solve(op, x, b, cheb)
    assert e.value.status == 5
    with pytest.raises(pkg.BP5Error) as e:
        op.vmult(x, op.initialize_block_vector(2))                           # shapes differ
    assert e.value.status == 1
    with pytest.raises(pkg.BP5Error):
        op.initialize_block_vector(9)


# ------------------------------------------------------------------ 7. CG
def _config1():
    if "c1" not in _cache:
        pr = O.Problem(2, (8, 8, 8), O.QUAD_GAUSS)
        _cache["c1"] = (pr, pr.rhs(), pkg.PoissonOperator(pkg.BrickMesh(2, (8, 8, 8)), pkg.QUAD_GAUSS))
    return _cache["c1"]


def _solve(op, B, max_iter, tol=0.0, inv=None, check_every=0):
    n = op.mf_data.n_local
    x = block(np.full((B.shape[0], n), np.nan), n, pad_value=SENTINEL, extra=0 if n & 1 else 2)
    b = block(B, n, extra=0 if n & 1 else 2)
    ctl = pkg.IterationNumberControl(max_iter, tol)
    pkg.SolverCG(ctl, check_every=check_every).solve(op, x, b, pkg.DiagonalMatrix(inv))
    check_padding(x, n, SENTINEL)
    return x[:, :n].cpu().numpy(), ctl


OTHER_COUNTS = [1, 2, 5, 8]     # besides 3: the scalar case, the truncating PARTIAL_STRIDE / n_components (5), the full row (8)


def _scalar_solve(op, b, max_iter, tol=0.0, inv=None):
    """the scalar SolverCG on the same handle: (solution, control)"""
    xs = op.initialize_dof_vector()
    ctl = pkg.IterationNumberControl(max_iter, tol)
    pkg.SolverCG(ctl).solve(op, xs, _t().from_numpy(np.array(b)).to("cuda:0"), pkg.DiagonalMatrix(inv))
    return xs.cpu().numpy(), ctl


def _stacked_recurrence(nc):
    pr, b, op = _config1()
    B = R.rhs_blocks(b, nc)
    xr, k, res = R.cg(pr.vmult, B, 10)
    x, ctl = _solve(op, B, 10)
    errs = [rel(x[c], xr[c]) for c in range(nc)]
    print(f"config 1, {nc} components, per component:", " ".join(f"{e:.2e}" for e in errs))
    assert x.shape[0] == nc and ctl.last_step() == k == 10 and max(errs) <= TOL_CG
    assert abs(ctl.last_value() - res) <= 1e-10 * res
    assert ctl.apply_kernel.startswith("apply_pencil_components_kernel<2,false,")
    if nc == 1:
        xs, _ = _scalar_solve(op, B[0], 10)
        assert rel(xs, xr[0]) <= TOL_CG and rel(x[0], xs) <= TOL_CG


def test_cg_is_the_stacked_recurrence():
    """config 1, 10 iterations, three different right-hand sides: one Krylov space (three separate solves are 1.3e-2 away, tests/test_components_cpu.py)"""
    _stacked_recurrence(3)


@pytest.mark.parametrize("nc", OTHER_COUNTS)
def test_cg_is_the_stacked_recurrence_at_other_component_counts(nc):
    """... and 1, 2, 5 and 8 of them (noise drift of these references: tests/test_components_cpu.py); one component is the scalar SolverCG"""
    _stacked_recurrence(nc)


def test_cg_identical_right_hand_sides_reproduce_the_scalar_solver():
    pr, b, op = _config1()
    x, ctl = _solve(op, np.stack([b, b, b]), 10)
    xs = op.initialize_dof_vector()
    pkg.SolverCG(pkg.IterationNumberControl(10, 0.0)).solve(op, xs, _t().from_numpy(b).to("cuda:0"), pkg.DiagonalMatrix())
    for c in range(3):
        assert rel(x[c], xs.cpu().numpy()) <= TOL_CG


def _with_the_inverse_diagonal(nc):
    prd, Bd, inv = diag_case(nc)
    op = _operator(4, pkg.QUAD_GAUSS, cells=(4, 4, 4))
    dinv = op.compute_diagonal(invert=True)
    assert rel(dinv.cpu().numpy(), inv) <= 1e-13
    xr, k, _ = R.cg(prd.vmult, Bd, 10, inv_diag=inv)
    x, ctl = _solve(op, Bd, 10, inv=dinv)
    errs = [rel(x[c], xr[c]) for c in range(nc)]
    print(f"p = 4 with inverse diagonal, {nc} components, per component:", " ".join(f"{e:.2e}" for e in errs))
    assert x.shape[0] == nc and ctl.last_step() == k == 10 and max(errs) <= TOL_CG
    if nc == 1:
        xs, _ = _scalar_solve(op, Bd[0], 10, inv=dinv)
        assert rel(xs, xr[0]) <= TOL_CG and rel(x[0], xs) <= TOL_CG


def test_cg_with_the_inverse_diagonal():
    """p = 4 (4,4,4), deformed, step-64 kappa, bp5_compute_diagonal(invert = 1), 10 iterations: the reference's noise drift on this case is
    3.8e-16 (tests/test_components_cpu.py asserts < 1e-13), so the fixed-iteration comparison holds to TOL_CG"""
    _with_the_inverse_diagonal(3)


@pytest.mark.parametrize("nc", OTHER_COUNTS)
def test_cg_with_the_inverse_diagonal_at_other_component_counts(nc):
    _with_the_inverse_diagonal(nc)


def _tolerance_stop(check_every, nc):
    pr, b, op = _config1()
    B = R.rhs_blocks(b, nc)
    tol = 1e-8 * np.linalg.norm(B)
    xr, k, _ = R.cg(pr.vmult, B, 1000, tol=tol)
    x, ctl = _solve(op, B, 1000, tol=tol, check_every=check_every)
    assert x.shape[0] == nc and ctl.last_step() == k and ctl.last_value() <= tol
    true_res = np.linalg.norm(B - R.vmult(pr, x))
    print(f"{nc} components: iterations {k}, recomputed FP64 residual {true_res:.3e}, tolerance {tol:.3e}")
    assert true_res <= tol * (1 + 1e-6)
    if nc == 1:      # 53 iterations; the reference moves by 2.3e-16 under operator noise over that many, so TOL_CG holds here too
        xs, cs = _scalar_solve(op, B[0], 1000, tol=tol)
        assert cs.last_step() == k and rel(xs, xr[0]) <= TOL_CG and rel(x[0], xs) <= TOL_CG


@pytest.mark.parametrize("check_every", [0, 3])
def test_cg_tolerance_stop(check_every):
    _tolerance_stop(check_every, 3)


@pytest.mark.parametrize("nc", OTHER_COUNTS)
@pytest.mark.parametrize("check_every", [0, 3])
def test_cg_tolerance_stop_at_other_component_counts(check_every, nc):
    _tolerance_stop(check_every, nc)


# ------------------------------------------------------------------ 7b. the CG at the capped grid
VB, MAXBLK, PARTIAL_STRIDE = 256, 2048, 8192      # bp5_kernels.hpp: threads of a streaming workgroup, their grid cap, the length of a partial-sum row


def cg_grids(n_owned, nc):
    """(uncapped workgroups of the kernels that take two DoFs per thread, of the one that takes one, columns of a partial-sum row per component):
    bp5_cg_solve_components launches min(uncapped, columns) workgroups per component"""
    return min(-(-n_owned // (2 * VB)), MAXBLK), min(-(-n_owned // VB), MAXBLK), PARTIAL_STRIDE // nc


def _capped():
    """the numpy problem of tests/test_components_cpu.py: capped_case() and the operator on it, built once"""
    if "capped" not in _cache:
        pr, b, inv = capped_case()
        op = pkg.PoissonOperator(pkg.BrickMesh(4, CAPPED_CELLS, deform_amp=0.04), pkg.QUAD_GAUSS, pkg.COEF_STEP64)
        dinv = op.compute_diagonal(invert=True)
        assert op.mf_data.n_owned == op.mf_data.n_local == pr.mesh.n_dofs == 85 ** 3 and rel(dinv.cpu().numpy(), inv) <= 1e-13
        _cache["capped"] = (pr, b, inv, op, dinv)
    return _cache["capped"]


@pytest.mark.parametrize("with_diag", [False, True])
@pytest.mark.parametrize("nc,workgroups", [(7, 1170), (8, 1024)])
def test_cg_at_the_capped_grid(nc, workgroups, with_diag):
    """85^3 DoFs: more than 512 PARTIAL_STRIDE / n_components, so every reducing kernel runs on as many workgroups per component as the row has
    columns for it and takes a second grid-stride trip; eight components fill the row to its last word, with the next row right behind it.
    Three iterations: the references move by < 3e-16 under operator noise (tests/test_components_cpu.py)"""
    pr, b, inv, op, dinv = _capped()
    n = 85 ** 3
    two, one, cols = cg_grids(n, nc)
    assert cols == workgroups < two <= one and n > workgroups * 2 * VB, (two, one, cols)      # the cap bites; a second trip at two DoFs per thread
    assert nc * cols == (8190 if nc == 7 else PARTIAL_STRIDE)
    B = R.rhs_blocks(b, nc)
    xr, k, res = R.cg(pr.vmult, B, CAPPED_ITERATIONS, inv_diag=inv if with_diag else None)
    x, ctl = _solve(op, B, CAPPED_ITERATIONS, inv=dinv if with_diag else None)
    errs = [rel(x[c], xr[c]) for c in range(nc)]
    print(f"capped grid, {nc} components on {workgroups} workgroups each, {'inverse diagonal' if with_diag else 'no preconditioner'}: "
          f"max error {max(errs):.2e}, residual {ctl.last_value():.6e} (numpy {res:.6e})")
    assert ctl.last_step() == k == CAPPED_ITERATIONS == 3 and max(errs) <= TOL_CG
    assert abs(ctl.last_value() - res) <= 1e-10 * res
    assert ctl.apply_kernel.startswith("apply_pencil_components_kernel<4,false,")


def test_operator_at_the_capped_grid_size():
    """the same handle and sources, eight components: 927 teams, atomics under contention"""
    pr, b, inv, op, dinv = _capped()
    n = op.mf_data.n_local
    assert launch_shape(4, op.mf_data.mesh.n_cells)[1:] == (927, 927)
    B = R.rhs_blocks(b, N_BLOCKS)
    ref = R.vmult(pr, B)
    s, d = block(B, n), block(np.full((N_BLOCKS, n), np.nan), n, pad_value=SENTINEL)
    op.vmult(d, s)
    check_padding(d, n, SENTINEL)
    got = d[:, :n].cpu().numpy()
    errs = [rel(got[c], ref[c]) for c in range(N_BLOCKS)]
    print(f"85^3 DoFs, eight components: max error vs oracle {max(errs):.2e}")
    assert not np.isnan(got).any() and max(errs) <= TOL_OP


# ------------------------------------------------------------------ 7c. the solver's edges
# EDGES (tests/test_components_cpu.py): (components, the block whose right-hand side is zeroed where one is)
def _edge_case(nc):
    """p = 4 (4,4,4), deformed, step-64 kappa (diag_case): (problem, right-hand sides, operator)"""
    pr, B, _ = diag_case(nc)
    return pr, B, _operator(4, pkg.QUAD_GAUSS, cells=(4, 4, 4))


def _solve_prefilled(op, B, max_iter, inv=None, fill=3.0):
    """x = `fill` on every DoF, sentinel padding"""
    n = op.mf_data.n_local
    x, b = block(np.full(B.shape, fill), n, pad_value=SENTINEL), block(B, n)
    ctl = pkg.IterationNumberControl(max_iter, 0.0)
    pkg.SolverCG(ctl).solve(op, x, b, pkg.DiagonalMatrix(inv))
    check_padding(x, n, SENTINEL)
    return x[:, :n].cpu().numpy(), ctl


@pytest.mark.parametrize("nc,zeroed", EDGES)
def test_cg_zero_right_hand_side(nc, zeroed):
    pr, B, op = _edge_case(nc)
    x, ctl = _solve_prefilled(op, np.zeros_like(B), 5)
    assert ctl.last_step() == 0 and ctl.last_value() == 0.0 and np.array_equal(x, np.zeros_like(B))


@pytest.mark.parametrize("nc,zeroed", EDGES)
def test_cg_zero_right_hand_side_in_one_block(nc, zeroed):
    """g, d and A d of that block are exact zeros (sums of zeros, whatever the order of the atomics), so its x is; the others do not notice.
    With the inverse diagonal: the ten-iteration reference without it moves by 1e-12 under operator noise (tests/test_components_cpu.py)"""
    pr, B, inv = zero_block_case(nc, zeroed)
    op = _edge_case(nc)[2]
    dinv = op.compute_diagonal(invert=True)
    assert rel(dinv.cpu().numpy(), inv) <= 1e-13 and not B[zeroed].any()
    xr, k, res = R.cg(pr.vmult, B, 10, inv_diag=inv)
    x, ctl = _solve_prefilled(op, B, 10, inv=dinv)
    assert ctl.last_step() == k == 10 and abs(ctl.last_value() - res) <= 1e-10 * res
    assert np.array_equal(x[zeroed], np.zeros(B.shape[1])) and not xr[zeroed].any()
    errs = [rel(x[c], xr[c]) for c in range(nc) if c != zeroed]
    print(f"{nc} components, block {zeroed} zero: max error of the others {max(errs):.2e}")
    assert len(errs) == nc - 1 and max(errs) <= TOL_CG


@pytest.mark.parametrize("nc,zeroed", EDGES)
def test_cg_zero_iterations(nc, zeroed):
    pr, B, op = _edge_case(nc)
    x, ctl = _solve_prefilled(op, B, 0)
    assert ctl.last_step() == 0 and np.array_equal(x, np.zeros_like(B))
    assert abs(ctl.last_value() - np.linalg.norm(B)) <= 1e-12 * np.linalg.norm(B)


@pytest.mark.parametrize("nc,zeroed", EDGES)
def test_cg_breakdown_is_reported_and_does_not_stick(nc, zeroed):
    """d.Ad == 0 (an all-zero metric) is BP5_ERR_BREAKDOWN, as from the scalar solver (tests/test_gpu_parity.py); the flag does not outlive the
    solve on that handle (metric restored), and a fresh operator is not affected"""
    pr = O.Problem(2, (2, 2, 2), O.QUAD_GAUSS)
    B = R.rhs_blocks(pr.rhs(), nc)
    xr, k, _ = R.cg(pr.vmult, B, 3)
    op = pkg.PoissonOperator(pkg.BrickMesh(2, (2, 2, 2)), pkg.QUAD_GAUSS)
    metric = op.coef.clone()
    op.coef.zero_()
    n = op.mf_data.n_local
    with pytest.raises(pkg.BP5Error) as e:
        pkg.SolverCG(pkg.IterationNumberControl(5, 0.0)).solve(op, op.initialize_block_vector(nc), block(B, n, extra=0), pkg.DiagonalMatrix())
    assert e.value.status == 6
    op.coef.copy_(metric)
    for healthy in (op, pkg.PoissonOperator(pkg.BrickMesh(2, (2, 2, 2)), pkg.QUAD_GAUSS)):
        x, ctl = _solve(healthy, B, 3)
        assert ctl.last_step() == k == 3 and max(rel(x[c], xr[c]) for c in range(nc)) <= TOL_CG


def test_cg_sequence_on_one_handle():
    """The workspace of bp5_cg_solve_components grows (2 -> 8 components) and is reused at other component counts and strides, and the partial
    sums, scalars and state words are the scalar solvers': every block solve against numpy (noise drift of these references:
    tests/test_components_cpu.py), and the scalar SolverCG and vmult of the handle (block kernel: no atomics) give the same bits before and after"""
    torch = _t()
    p, cells, iters = 4, SEQUENCE_CELLS, SEQUENCE_ITERATIONS
    pr, b_lex, inv = sequence_case()
    op = pkg.PoissonOperator(pkg.BrickMesh(p, cells, deform_amp=0.04, cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1), pkg.QUAD_GAUSS,
                             pkg.COEF_STEP64)
    op.mf_data.set_apply_variant(56)
    n = op.mf_data.n_local
    perm = op.mf_data.mesh.global_ids.astype(np.int64)       # local index -> lexicographic id of the oracle
    dinv = op.compute_diagonal(invert=True)
    assert rel(dinv.cpu().numpy(), inv[perm]) <= 1e-13
    b, s = torch.from_numpy(b_lex[perm]).to("cuda:0"), torch.from_numpy(O.deterministic_src(n, seed=9)).to("cuda:0")

    def scalar():
        x, v = op.initialize_dof_vector(), op.initialize_dof_vector()
        ctl = pkg.IterationNumberControl(iters, 0.0)
        pkg.SolverCG(ctl).solve(op, x, b, pkg.DiagonalMatrix(dinv))
        assert ctl.last_step() == iters and ctl.apply_kernel.startswith("apply_block_kernel")
        op.vmult(v, s)
        return x, v, ctl.last_value()

    before = scalar()
    xs, _, _ = O.cg_plain(pr.vmult, b_lex, iters, diag=inv)
    assert rel(before[0].cpu().numpy(), xs[perm]) <= TOL_CG
    for nc, extra, with_diag in SEQUENCE:
        B = R.rhs_blocks(b_lex, nc)
        xr, k, res = R.cg(pr.vmult, B, iters, inv_diag=inv if with_diag else None)
        x = block(np.full((nc, n), np.nan), n, pad_value=SENTINEL, extra=extra)
        assert x.shape[1] == n + (n & 1) + extra
        ctl = pkg.IterationNumberControl(iters, 0.0)
        pkg.SolverCG(ctl).solve(op, x, block(B[:, perm], n, extra=extra), pkg.DiagonalMatrix(dinv if with_diag else None))
        check_padding(x, n, SENTINEL)
        errs = [rel(x[c, :n].cpu().numpy(), xr[c][perm]) for c in range(nc)]
        print(f"{nc} components, ld = n_local + {x.shape[1] - n}: max error {max(errs):.2e}")
        assert ctl.last_step() == k == iters and max(errs) <= TOL_CG and abs(ctl.last_value() - res) <= 1e-10 * res
        assert ctl.apply_kernel.startswith("apply_pencil_components_kernel<4,false,")
    after = scalar()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]) and before[2] == after[2]


# ------------------------------------------------------------------ 8. facade
def test_facade_example_reproduces_the_python_solve():
    """examples/bp5_bp6: BlockVector, vmult(BlockVector &, const BlockVector &) and SolverCG::solve of the facade give the iteration count and the
    per-component L2 norms of the Python three-component solve"""
    exe = os.path.join(bp5_pkg.ROOT, "examples", "bp5_bp6")
    txt = subprocess.run([exe, "2", "8", "8", "8", "0.05", "1e-8", "1"], capture_output=True, text=True, timeout=300, check=True).stdout
    got = {l.split()[0]: l.split()[1:] for l in txt.splitlines() if l.strip()}
    op = pkg.PoissonOperator(pkg.BrickMesh(2, (8, 8, 8), deform_amp=0.05), pkg.QUAD_GAUSS, pkg.COEF_STEP64)
    n = op.mf_data.n_local
    B = R.rhs_blocks(op.assemble_rhs().cpu().numpy())
    x, b = op.initialize_block_vector(3), op.initialize_block_vector(3)
    b[:, :n] = _t().from_numpy(B).to("cuda:0")
    ctl = pkg.SolverControl(10000, 1e-8 * np.linalg.norm(B))
    pkg.SolverCG(ctl).solve(op, x, b, pkg.DiagonalMatrix(op.compute_diagonal(invert=True)))
    assert int(got["components"][0]) == 3 and int(got["iterations"][0]) == ctl.last_step() > 5
    assert float(got["true_residual"][0]) <= float(got["tolerance"][0]) * (1 + 1e-6)
    assert got["apply_kernel"][0].startswith("apply_pencil_components_kernel<2,false,")
    for c in range(3):
        l2 = op.l2_norm_solution(x[c, :n].clone())
        assert abs(float(got[f"l2_norm_{c}"][0]) - l2) <= 1e-10 * l2, (c, got[f"l2_norm_{c}"], l2)
