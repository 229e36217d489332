"""FP32 metric planes (bp5_mf_set_metric_precision: float planes, double arithmetic and vectors) on the MI355X: sizing, the planes
themselves, the operator on every kernel path against the oracle applied with THE PLANES READ BACK FROM THE LIBRARY (widened floats: the
arithmetic is still double, so the FP64 operator tolerance holds; reading them back avoids the rare entry where the GPU's and numpy's doubles
round to different floats), its pieces, determinism, refusals, the solvers on an FP32 handle, and the mixed-precision multigrid (outer
operator FP64, every level of make_mg_hierarchy(metric_precision="float32") on float planes) against tests/f32_metric_ref.py."""
from types import SimpleNamespace

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import chebyshev_ref as R
import f32_metric_ref as F

pkg = bp5_pkg.load()
pytestmark = pytest.mark.gpu
TOL_OP = 1e-13     # one operator application (tests/test_gpu_parity.py)
TOL_CG = 1e-11     # CG solution vector at a fixed iteration count
F32M, LATT = 536870912, 16777216     # bp5_kernels.hpp: BLK_F32M, BLK_LATT
AMP = 0.05
COARSE = 10
BRICKS = dict(cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1)
# brick shapes of tests/test_gpu_parity.py (partial bricks at the mesh edge)
BRICK_SHAPES = {1: ((17, 9, 10), (8, 8, 8)), 2: ((9, 8, 5), (8, 8, 4)), 3: ((9, 5, 6), (8, 4, 4)), 4: ((9, 8, 6), (4, 4, 4)), 5: ((5, 6, 3), (4, 4, 2)),
                6: ((5, 4, 3), (4, 4, 2)), 7: ((5, 3, 3), (4, 2, 2)), 8: ((3, 3, 3), (2, 2, 2))}


def _t():
    import torch
    return torch


def dev(x):
    return _t().from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _planes(op):
    """the handle's planes as the kernels read them: [6][cell][q] doubles, the mesh's own cell order"""
    m = op.mf_data.mesh
    return op.mf_data.coef_reference_layout(op.coef).cpu().numpy().reshape(6, m.n_cells, -1)


def _local(mesh):
    """the library mesh as the oracle's cell loops take it: its own local_to_global and cell order"""
    return SimpleNamespace(p=mesh.degree, n=mesh.degree + 1, n_cells=mesh.n_cells, n_dofs=mesh.n_local, l2g=np.asarray(mesh.l2g),
                           constrained=np.asarray(mesh.constrained))


def _kernel_bits(name):
    return int(name.split(",")[-1].rstrip(">"))


def _f32(mesh, quad=0, variant=None, wgs=None, lattice=None, coefficient=pkg.COEF_STEP64):
    op = pkg.PoissonOperator(mesh, quad, coefficient, metric_precision="float32")
    if lattice is not None:
        op.mf_data.set_tuning("lattice_indices", lattice)
    if variant is not None:
        op.mf_data.set_apply_variant(variant)
    if wgs is not None:
        op.mf_data.set_block_workgroups(wgs)
    return op


# ------------------------------------------------------------------ sizing, planes
@pytest.mark.parametrize("p,cells", [(1, (3, 3, 3)), (2, (3, 2, 2)), (4, (3, 2, 1)), (4, (2, 2, 2)), (8, (1, 1, 1))])
def test_coef_size(p, cells):
    mesh = pkg.BrickMesh(p, cells)
    n_entries = 6 * mesh.n_cells * (p + 1) ** 3
    mf = pkg.MatrixFree().reinit(mesh, 0, 0)
    assert mf.get_metric_precision() == "float64" and mf.coef_size() == n_entries
    mf32 = pkg.MatrixFree().reinit(mesh, 0, 0)
    mf32.set_metric_precision("float32")
    assert mf32.get_metric_precision() == "float32" and mf32.coef_size() == (n_entries + 1) // 2
    assert mf32.evaluate_coefficients().numel() == max((n_entries + 1) // 2, 1)


@pytest.mark.parametrize("p", [1, 2, 4, 5, 8])
@pytest.mark.parametrize("quad", [0, 1])
def test_planes_are_the_fp64_planes_rounded_once(p, quad):
    cells = (3, 2, 2) if p <= 4 else (2, 2, 1)
    op = _f32(pkg.BrickMesh(p, cells, deform_amp=0.04), quad)
    got = _planes(op)
    assert np.array_equal(got, got.astype(np.float32).astype(np.float64))           # every entry is a float
    ref = O.Problem(p, cells, quad, deform_amp=0.04, kappa=O.kappa_step64).coef
    err, bound = np.abs(got - ref), 2.0 ** -24 * np.abs(ref) + 1e-13 * np.abs(ref).max()
    print(f"p={p} quad={quad}: max |got - ref| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()            # half a float ulp + the slack of the FP64 metric parity test


# ------------------------------------------------------------------ operator
@pytest.mark.parametrize("p", range(1, 9))
@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("path", ["pencil", "packed", "lattice"])
def test_vmult_matches_the_oracle_on_the_read_back_planes(p, quad, path):
    torch = _t()
    if path == "pencil":
        mesh = pkg.BrickMesh(p, (3, 3, 2) if p <= 4 else (3, 2, 1), deform_amp=0.04)
        op = _f32(mesh, quad)
    else:
        cells, block = BRICK_SHAPES[p]
        mesh = pkg.BrickMesh(p, cells, h=0.2, deform_amp=0.03, cell_block=block, dof_numbering=1, cell_block_order=1)
        op = _f32(mesh, quad, variant=56, wgs=8, lattice=1 if path == "lattice" else 0)
        nb, _, packed = op.mf_data.block_plan_info()
        assert packed and op.mf_data.block_plan_lattice() == (nb if path == "lattice" else 0)
    lm = _local(mesh)
    _, _, _, N, D = O.shape_tables(p, quad)
    s = O.deterministic_src(mesh.n_local, seed=61)             # non-zero on the boundary too
    ref = O.vmult(lm, _planes(op), N, D, s)
    outs = []
    for _ in range(2):
        d = op.initialize_dof_vector()
        d.fill_(float("nan"))
        op.vmult(d, dev(s))
        outs.append(d)
    err = rel(outs[0].cpu().numpy(), ref)
    print(f"p={p} quad={quad} {path}: rel err {err:.2e}")
    assert err <= TOL_OP
    # the kernel that ran: the FP32-metric build of the shape the path names
    ctl = pkg.IterationNumberControl(1, 0.0)
    pkg.SolverCG(ctl).solve(op, op.initialize_dof_vector(), op.assemble_rhs(), pkg.DiagonalMatrix())
    bits = _kernel_bits(ctl.apply_kernel)
    assert bits & F32M, ctl.apply_kernel
    if path == "pencil":
        assert ctl.apply_kernel.startswith("apply_pencil_kernel")
    else:
        assert ctl.apply_kernel.startswith("apply_block_kernel") and bool(bits & LATT) == (path == "lattice"), ctl.apply_kernel
        assert torch.equal(outs[0], outs[1])                    # owner stores, no atomics: bitwise reproducible


@pytest.mark.parametrize("p,quad,bricks", [(2, 0, False), (3, 1, False), (4, 0, True), (5, 0, True), (8, 1, False)])
def test_diagonal_on_the_read_back_planes(p, quad, bricks):
    if bricks:
        cells, block = BRICK_SHAPES[p]
        mesh = pkg.BrickMesh(p, cells, h=0.2, deform_amp=0.03, cell_block=block, dof_numbering=1, cell_block_order=1)
    else:
        mesh = pkg.BrickMesh(p, (3, 2, 2), deform_amp=0.04)
    op = _f32(mesh, quad)
    _, _, _, N, D = O.shape_tables(p, quad)
    ref = O.operator_diagonal(_local(mesh), _planes(op), N, D)
    assert rel(op.compute_diagonal().cpu().numpy(), ref) <= 1e-13
    assert rel(op.compute_diagonal(invert=True).cpu().numpy(), 1.0 / ref) <= 1e-13


@pytest.mark.parametrize("p,quad,kw,variant", [(3, 0, dict(rank=1, n_ranks=2), 0),                                   # pencil kernel on a cell range
                                               (4, 0, dict(rank=1, n_ranks=2, cell_block=(4, 4, 2), dof_numbering=1, cell_block_order=1), 56),   # block kernel on whole bricks of the range
                                               (4, 1, dict(rank=0, n_ranks=2, cell_block=(4, 4, 2), dof_numbering=1, cell_block_order=1), 56)])
def test_apply_cells_on_the_interior_range(p, quad, kw, variant):
    """bp5_apply_cells on [0, n_interior_cells) of a slab (single-rank entry point: ghosts are plain entries): accumulates into dst"""
    torch = _t()
    mesh = pkg.BrickMesh(p, (8, 8, 12) if variant else (4, 3, 6), h=0.2, deform_amp=0.03, **kw)
    assert 0 < mesh.n_interior_cells < mesh.n_cells or kw["rank"] == 0
    op = _f32(mesh, quad, variant=variant, wgs=8 if variant else None)
    _, _, _, N, D = O.shape_tables(p, quad)
    s = O.deterministic_src(mesh.n_local, seed=7)
    acc = torch.full((mesh.n_local,), 0.25, dtype=torch.float64, device="cuda:0")
    op.mf_data.cell_loop(op.coef, dev(s), acc, 0, mesh.n_interior_cells)
    ref = O.apply_cells(_local(mesh), _planes(op), N, D, s, cell_range=(0, mesh.n_interior_cells))
    assert rel(acc.cpu().numpy() - 0.25, ref) <= TOL_OP


# ------------------------------------------------------------------ refusals
def _status(call):
    with pytest.raises(pkg.BP5Error) as e:
        call()
    return e.value.status, str(e.value)


def test_refusals_and_a_default_handle_next_to_an_f32_one():
    torch = _t()
    mesh = pkg.BrickMesh(4, (3, 2, 2), deform_amp=0.04)
    INVALID, UNSUPPORTED = 1, 5
    # after the metric array has been sized / filled
    mf = pkg.MatrixFree().reinit(mesh, 0, 1)
    mf.coef_size()
    st, msg = _status(lambda: mf.set_metric_precision("float32"))
    assert st == INVALID and "before" in msg
    mf.set_metric_precision("float64")                                      # (no change: accepted)
    mf2 = pkg.MatrixFree().reinit(mesh, 0, 1)
    mf2.set_metric_precision("float32")
    mf2.evaluate_coefficients()
    assert _status(lambda: mf2.set_metric_precision("float64"))[0] == INVALID
    assert pkg.lib().bp5_mf_set_metric_precision(mf2.handle, 2) == INVALID   # unknown value
    # Helmholtz, affine: both orders
    mf3 = pkg.MatrixFree().reinit(pkg.BrickMesh(2, (2, 2, 2)), 0, 1)
    mf3.set_operator(pkg.OP_HELMHOLTZ)
    st, msg = _status(lambda: mf3.set_metric_precision("float32"))
    assert st == UNSUPPORTED and "Helmholtz" in msg
    mf4 = pkg.MatrixFree().reinit(pkg.BrickMesh(2, (2, 2, 2)), 0, 1)
    mf4.set_metric_precision("float32")
    st, msg = _status(lambda: mf4.set_operator(pkg.OP_HELMHOLTZ))
    assert st == UNSUPPORTED and "Helmholtz" in msg
    st, msg = _status(lambda: mf4.set_geometry_mode(pkg.GEOM_AFFINE))
    assert st == UNSUPPORTED and "affine" in msg
    mf5 = pkg.MatrixFree().reinit(pkg.BrickMesh(2, (2, 2, 2)), 0, 1)
    mf5.set_geometry_mode(pkg.GEOM_AFFINE)
    st, msg = _status(lambda: mf5.set_metric_precision("float32"))
    assert st == UNSUPPORTED and "affine" in msg
    # hanging-node handle
    m = O.HangingBrickMesh(2, 2, 2, 1, 3)
    ns = SimpleNamespace(degree=m.p, n=m.n, n_cells=m.n_cells, n_interior_cells=m.n_cells, n_owned=m.n_dofs, n_ghost=0, n_local=m.n_dofs,
                         n_global_dofs=m.n_dofs, l2g=m.l2g, coords=m.coords, constrained=m.constrained, n_neighbors=0,
                         neighbor_rank=np.zeros(0, np.int32), send_offsets=np.zeros(1, np.uint32), send_indices=np.zeros(0, np.uint32),
                         recv_offsets=np.zeros(1, np.uint32), cell_block_offsets=None, constraint_mask=m.constraint_mask, rank=0, n_ranks=1)
    mfh = pkg.MatrixFree().reinit(ns, 0, 1)
    st, msg = _status(lambda: mfh.set_metric_precision("float32"))
    assert st == UNSUPPORTED and "hanging" in msg
    # apply variants other than 0 and 56: both orders
    op32 = _f32(mesh)
    for v in (3, 10, 50, 70):
        st, msg = _status(lambda: op32.mf_data.set_apply_variant(v))
        assert st == UNSUPPORTED and "variants 0" in msg, (v, st, msg)
    op32.mf_data.set_apply_variant(56)
    op32.mf_data.set_apply_variant(0)
    mf6 = pkg.MatrixFree().reinit(mesh, 0, 1)
    mf6.set_apply_variant(3)
    assert _status(lambda: mf6.set_metric_precision("float32"))[0] == UNSUPPORTED
    with pytest.raises(pkg.BP5Error):
        pkg.PoissonOperator(mesh, 0, 1, metric_precision="float16")
    # a default handle next to the FP32 one on the same mesh object still gives the FP64 operator's bits
    op64 = pkg.PoissonOperator(mesh, 0, pkg.COEF_STEP64)
    s = dev(O.deterministic_src(mesh.n_owned, seed=7))
    before = op64.initialize_dof_vector()
    op64.vmult(before, s)
    d32 = op32.initialize_dof_vector()
    op32.vmult(d32, s)
    pr = O.Problem(4, (3, 2, 2), 0, deform_amp=0.04, kappa=O.kappa_step64)
    assert rel(before.cpu().numpy(), pr.vmult(s.cpu().numpy())) <= TOL_OP
    diff = rel(d32.cpu().numpy(), before.cpu().numpy())
    assert 1e-11 < diff < 1e-6, diff                                      # the rounded operator is another operator, O(1e-8) away
    assert np.array_equal(_planes(op64), op64.mf_data.coef_reference_layout(op64.coef).cpu().numpy().reshape(6, mesh.n_cells, -1))
    assert not np.array_equal(_planes(op64), _planes(op32))


def test_default_handle_keeps_its_bits_on_the_block_kernel():
    """same mesh object, block kernel (bitwise reproducible): the FP64 handle's result before and after an FP32 twin exists and has run"""
    torch = _t()
    mesh = pkg.BrickMesh(4, (9, 8, 6), h=0.2, deform_amp=0.03, **BRICKS)
    op64 = pkg.PoissonOperator(mesh, 0, pkg.COEF_STEP64)
    op64.mf_data.set_apply_variant(56)
    op64.mf_data.set_block_workgroups(8)
    s = dev(O.deterministic_src(mesh.n_owned, seed=8))
    a = op64.initialize_dof_vector()
    op64.vmult(a, s)
    op32 = _f32(mesh, variant=56, wgs=8)
    d = op32.initialize_dof_vector()
    op32.vmult(d, s)
    b = op64.initialize_dof_vector()
    op64.vmult(b, s)
    assert torch.equal(a, b) and not torch.equal(a, d)


# ------------------------------------------------------------------ solvers on an FP32 handle
@pytest.mark.parametrize("kw,variant", [({}, None), (BRICKS, 56)])
def test_cg_solvers_on_an_f32_handle(kw, variant):
    """config 1 (p = 2, 8^3 unit cubes, coefficient 1: the smoke run's problem), 10 iterations: both solvers against the oracle's recurrences
    on the read-back planes; no fused dot products (on the brick mesh the FP64 handle would fuse them).  (Coefficient 1 as in config 1: with
    step-64's kappa on this domain the 10th CG iterate amplifies a 1e-15 perturbation of the planes to 1e-9 in the oracle itself, so a fixed
    iteration count compares nothing there.)"""
    p, cells = 2, (8, 8, 8)
    mesh = pkg.BrickMesh(p, cells, **kw)
    op = _f32(mesh, 0, variant=variant, coefficient=pkg.COEF_ONE)
    assert not np.array_equal(_planes(op), O.Problem(p, cells, 0).coef)         # (the float planes differ from the FP64 ones here too)
    lm = _local(mesh)
    _, _, _, N, D = O.shape_tables(p, 0)
    planes = _planes(op)

    def A(s):
        return O.vmult(lm, planes, N, D, s)

    b = op.assemble_rhs()
    b_ref = b.cpu().numpy()
    pr = O.Problem(p, cells, 0)
    perm = mesh.global_ids.astype(np.int64)
    assert rel(b_ref, pr.rhs()[perm]) <= TOL_OP
    for solver, oracle in ((pkg.SolverCG, O.cg_plain), (pkg.SolverCGFullMerge, O.cg_merged)):
        x = op.initialize_dof_vector()
        ctl = pkg.IterationNumberControl(10, 0.0)
        solver(ctl).solve(op, x, b, pkg.DiagonalMatrix())
        xr, k, _ = oracle(A, b_ref, 10)
        err = rel(x.cpu().numpy(), xr)
        print(f"{solver.__name__} variant={variant}: rel err {err:.2e}, kernel {ctl.apply_kernel}")
        assert ctl.last_step() == k == 10 and err <= TOL_CG
        assert not ctl.dot_products_fused
        assert _kernel_bits(ctl.apply_kernel) & F32M


def test_chebyshev_pcg_on_an_f32_handle_lands_in_the_numpy_count():
    p, cells = 3, (4, 3, 3)
    mesh = pkg.BrickMesh(p, cells, deform_amp=AMP)
    op = _f32(mesh, 0)
    lm = _local(mesh)
    _, _, _, N, D = O.shape_tables(p, 0)
    planes = _planes(op)

    def A(s):
        return O.vmult(lm, planes, N, D, s)

    inv = op.compute_diagonal(invert=True)
    inv_ref = 1.0 / O.operator_diagonal(lm, planes, N, D)
    ch = pkg.PreconditionChebyshev().initialize(op, pkg.PreconditionChebyshev.AdditionalData(degree=4, smoothing_range=20.0, preconditioner=pkg.DiagonalMatrix(inv)))
    lo, hi, k_est = R.lanczos_estimate(A, inv_ref, R.start_vector(mesh.global_ids, mesh.constrained), 8)
    e = ch.estimated_eigenvalues()
    assert e["cg_its"] == k_est and abs(e["max_est"] - hi) <= 1e-10 * hi and abs(e["min_est"] - lo) <= 1e-10 * lo
    mu, Mu = R.bounds(lo, hi, 20.0)
    b = op.assemble_rhs()
    b_ref = b.cpu().numpy()
    tol = 1e-10 * np.linalg.norm(b_ref)
    x = op.initialize_dof_vector()
    ctl = pkg.SolverControl(200, tol)
    pkg.SolverCG(ctl).solve(op, x, b, ch)
    xr, k_ref, _ = R.pcg(A, lambda g: R.vmult(A, inv_ref, g, mu, Mu, 4), b_ref, 200, tol=tol)
    print(f"Chebyshev(4)-PCG on float planes: iterations {ctl.last_step()} (numpy {k_ref})")
    assert ctl.last_step() == k_ref, (ctl.last_step(), k_ref)
    assert rel(x.cpu().numpy(), xr) < 1e-7


# ------------------------------------------------------------------ mixed-precision multigrid
def _perm(op):
    m = op.mf_data.mesh
    return m.global_ids[:m.n_owned].astype(np.int64)


def _dev(v_lex, op):
    x = op.initialize_dof_vector()
    x[:op.mf_data.n_owned] = dev(v_lex[_perm(op)])
    return x


def _lex(x, op, n):
    out = np.zeros(n)
    out[_perm(op)] = x[:op.mf_data.n_owned].cpu().numpy()
    return out


@pytest.mark.parametrize("p", [4, 2])
@pytest.mark.parametrize("bricks", [False, True])
@pytest.mark.parametrize("h_levels", [0, "max"])
def test_mixed_precision_multigrid(p, bricks, h_levels):
    torch = _t()
    cells = (8, 8, 8) if h_levels == "max" or bricks else (6, 6, 6)
    fine = pkg.PoissonOperator(pkg.BrickMesh(p, cells, deform_amp=AMP, **(BRICKS if bricks else {})), pkg.QUAD_GAUSS, pkg.COEF_STEP64)
    assert pkg.make_mg_hierarchy(fine, h_levels=h_levels, metric_precision=None)[0] is fine      # None: nothing changes
    ops = pkg.make_mg_hierarchy(fine, h_levels=h_levels, metric_precision="float32")
    assert ops[0] is not fine and ops[0].mf_data.mesh is fine.mf_data.mesh
    assert all(o.mf_data.get_metric_precision() == "float32" for o in ops) and fine.mf_data.get_metric_precision() == "float64"
    if bricks:
        for o in [fine] + ops:
            o.mf_data.set_apply_variant(56)
    mg = pkg.PreconditionMG(ops, pkg.PreconditionMG.AdditionalData(coarse_degree=COARSE))
    planes = [F.planes_to_lexicographic(o.mf_data.mesh, _planes(o)) for o in ops]
    V = F.VCycle(p, cells, deform_amp=AMP, kappa=O.kappa_step64, h_levels=h_levels, planes=planes, coarse_degree=COARSE)
    info = mg.level_info()
    assert [(d["degree"], d["cells"]) for d in info] == [(q, c) for q, c, _ in V.spec]
    assert (len(V.spec) > len(pkg.mg_coarse_degrees(p))) == (h_levels == "max")
    for d, L in zip(info, V.levels):
        assert d["cg_its"] == L.cg_its and d["chebyshev_degree"] == L.degree
        for k in ("min_est", "max_est", "min_used", "max_used"):
            assert abs(d[k] - getattr(L, k)) <= 1e-10 * abs(getattr(L, k)), (k, d[k], getattr(L, k))
    m0 = V.levels[0].pr.mesh
    n = m0.n_dofs
    # one V-cycle
    s = O.deterministic_src(n, m0.constrained, seed=41)
    dst = ops[0].initialize_dof_vector()
    dst.fill_(float("nan"))
    mg.vmult(dst, _dev(s, ops[0]))
    err = rel(_lex(dst, ops[0], n), V.vmult(s))
    print(f"p={p} bricks={bricks} h_levels={h_levels}: V-cycle rel err {err:.2e}")
    assert err <= 1e-11
    # symmetric on the device's own results
    u, v = O.deterministic_src(n, m0.constrained, seed=42), O.deterministic_src(n, m0.constrained, seed=43)
    Vu, Vv = ops[0].initialize_dof_vector(), ops[0].initialize_dof_vector()
    mg.vmult(Vu, _dev(u, ops[0]))
    mg.vmult(Vv, _dev(v, ops[0]))
    Vu, Vv = _lex(Vu, ops[0], n), _lex(Vv, ops[0], n)
    assert abs(u @ Vv - v @ Vu) <= 1e-12 * abs(u @ Vu)
    # MG-PCG: outer operator FP64
    b = fine.assemble_rhs()
    tol = 1e-10 * float(torch.linalg.norm(b[:fine.mf_data.n_owned]))
    sols = []
    for _ in range(2):
        x = fine.initialize_dof_vector()
        ctl = pkg.SolverControl(200, tol)
        pkg.SolverCG(ctl).solve(fine, x, b, mg)
        sols.append((x, ctl.last_step()))
    if bricks:                                                   # block kernel on every level: bitwise reproducible
        assert sols[0][1] == sols[1][1] and torch.equal(sols[0][0], sols[1][0])
    pr64 = O.Problem(p, cells, O.QUAD_GAUSS, deform_amp=AMP, kappa=O.kappa_step64)
    b_ref = pr64.rhs()
    tol_ref = 1e-10 * np.linalg.norm(b_ref)
    x_ref, k_ref, _ = R.pcg(pr64.vmult, V.vmult, b_ref, 200, tol=tol_ref)
    print(f"p={p} bricks={bricks} h_levels={h_levels}: iterations {sols[0][1]} (numpy {k_ref})")
    assert abs(sols[0][1] - k_ref) <= 1, (sols[0][1], k_ref)
    x_lex = _lex(sols[0][0], fine, n)
    assert rel(x_lex, x_ref) < 1e-7
    assert np.linalg.norm(b_ref - pr64.vmult(x_lex)) <= tol_ref   # the residual, recomputed with the FP64 operator
    mg.clear()


def test_facade_example_with_float32_levels_matches_the_python_solve():
    """examples/bp5_multigrid with its optional trailing argument (old command lines behave as before): level operators on float planes
    through the facade's set_metric_precision, outer CG on an FP64 operator -- the iteration count, level bounds and solution norm of the
    Python solve of the same problem."""
    import os
    import subprocess
    torch = _t()
    exe = os.path.join(bp5_pkg.ROOT, "examples", "bp5_multigrid")
    txt = subprocess.run([exe, "4", "5", "4", "4", "0.05", "1e-8", "1", "0", "float32"], capture_output=True, text=True, timeout=300, check=True).stdout
    got = {l.split()[0]: l.split()[1:] for l in txt.splitlines() if l.strip()}
    assert got["metric_precision"] == ["float32"]
    fine = pkg.PoissonOperator(pkg.BrickMesh(4, (5, 4, 4), deform_amp=0.05), pkg.QUAD_GAUSS, pkg.COEF_STEP64)
    ops = pkg.make_mg_hierarchy(fine, metric_precision="float32")
    mg = pkg.PreconditionMG(ops)
    b = fine.assemble_rhs()
    x = fine.initialize_dof_vector()
    ctl = pkg.SolverControl(200, 1e-8 * float(torch.linalg.norm(b[:fine.mf_data.n_owned])))
    pkg.SolverCG(ctl).solve(fine, x, b, mg)
    assert int(got["iterations"][0]) == ctl.last_step()
    for lev, d in enumerate(mg.level_info()):
        row = got[f"level{lev}"]
        assert int(row[0]) == d["degree"] and int(row[1]) == d["n_owned"]
        assert abs(float(row[3]) - d["max_used"]) <= 1e-12 * d["max_used"]
    xn = float(torch.linalg.norm(x[:fine.mf_data.n_owned]))
    assert abs(float(got["solution_norm"][0]) - xn) <= 1e-10 * xn, (got, xn)
    mg.clear()
