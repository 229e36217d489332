"""The trilinear geometry mode on the GPU (BP5_GEOM_TRILINEAR; deal.II MappingQ1): apply_pencil_trilinear_kernel, the diagonal and the mode's mesh
check against the oracle's ordinary degree-p operator on trilinearised coordinates (tests/trilinear_ref.py; pinned outside itself by
tests/test_trilinear_cpu.py), both CG solvers and the preconditioned one, every refusal, a busy side stream, the bits of neighbouring handles and
the example.  The kernels scatter with atomics: results are compared to the project's tolerances (1e-13 operator, 1e-11 CG at a fixed count).

The sine displacement vanishes at the vertices of (3, 2, 2) and (13, 1, 1) (tests/test_trilinear_cpu.py): those two are the launch-shape cases the
mode was specified with, their trilinearised cells are cubes; SKEWED = (3, 3, 3) and the larger meshes keep skewed cells and run every case too."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import stream_harness as SH
import trilinear_ref as T
from user_mesh import Reference, UserMesh

pytestmark = pytest.mark.gpu
pkg = bp5_pkg.load()
TRI = pkg.GEOM_TRILINEAR
TOL_OP = 1e-13     # one operator application (rounding + atomic summation order)
TOL_CG = 1e-11     # CG solution vector at a fixed iteration count
AMP = T.AMP
SKEWED = (3, 3, 3)
QUADS = {"gauss": (pkg.QUAD_GAUSS, O.QUAD_GAUSS), "gll": (pkg.QUAD_GLL, O.QUAD_GLL)}
_cache = {}


def _t():
    import torch
    return torch


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def dev(a):
    return _t().from_numpy(np.array(a, dtype=np.float64)).to("cuda:0")


def nan_vector(n):
    return _t().full((n,), float("nan"), dtype=_t().float64, device="cuda:0")


def _mesh(p, cells, amp=AMP, **brick):
    key = ("mesh", p, cells, amp, tuple(sorted(brick.items())))
    if key not in _cache:
        _cache[key] = T.user_mesh(pkg, p, cells, amp, **brick)
    return _cache[key]


def _reference(p, cells, quad="gauss", coefficient=pkg.COEF_ONE, amp=AMP, **brick):
    """the oracle on the trilinearised mesh, a source (non-zero on the boundary) and its vmult -- computed once, never changed"""
    key = ("ref", p, cells, quad, coefficient, amp, tuple(sorted(brick.items())))
    if key not in _cache:
        um = _mesh(p, cells, amp, **brick)
        ref = Reference(um, QUADS[quad][1], T.KAPPA[coefficient])
        src = O.deterministic_src(um.n_dofs, seed=60 + p)
        want = ref.vmult(src)
        for a in (src, want):
            a.setflags(write=False)
        _cache[key] = (ref, src, want)
    return _cache[key]


def _operator(p, cells, quad="gauss", coefficient=pkg.COEF_ONE, geometry=TRI, amp=AMP, **brick):
    key = ("op", p, cells, quad, coefficient, geometry, amp, tuple(sorted(brick.items())))
    if key not in _cache:
        _cache[key] = pkg.PoissonOperator(_mesh(p, cells, amp, **brick).namespace(), QUADS[quad][0], coefficient, geometry=geometry)
    return _cache[key]


def launch_shape(p, n_cells):
    """(cells per team, teams, teams per workgroup, workgroups) as csrc/trilinear/bp5_trilinear.hip launches the kernel: DefaultPencil<p> --
    (p+1)^2 lanes per cell; four one-wave teams per workgroup at p <= 3, else one four-wave team"""
    tw, tpb = (1, 4) if p <= 3 else (4, 1)
    cpt = 64 * tw // (p + 1) ** 2
    teams = -(-n_cells // cpt)
    return cpt, teams, tpb, -(-teams // tpb)


def kernel_name(p, quad):
    tw, tpb = (1, 4) if p <= 3 else (4, 1)
    return "apply_pencil_trilinear_kernel<%d,%s,%d,%d,%d>" % (p, "true" if quad == "gll" else "false", tw, (p + 1) ** 2, tpb)


# the kernel names as literals, so that a change of the launch shapes has to be made here too
KERNEL_LITERALS = {
    (1, "gauss"): "apply_pencil_trilinear_kernel<1,false,1,4,4>", (1, "gll"): "apply_pencil_trilinear_kernel<1,true,1,4,4>",
    (2, "gauss"): "apply_pencil_trilinear_kernel<2,false,1,9,4>", (2, "gll"): "apply_pencil_trilinear_kernel<2,true,1,9,4>",
    (3, "gauss"): "apply_pencil_trilinear_kernel<3,false,1,16,4>", (3, "gll"): "apply_pencil_trilinear_kernel<3,true,1,16,4>",
    (4, "gauss"): "apply_pencil_trilinear_kernel<4,false,4,25,1>", (4, "gll"): "apply_pencil_trilinear_kernel<4,true,4,25,1>",
    (5, "gauss"): "apply_pencil_trilinear_kernel<5,false,4,36,1>", (5, "gll"): "apply_pencil_trilinear_kernel<5,true,4,36,1>",
    (6, "gauss"): "apply_pencil_trilinear_kernel<6,false,4,49,1>", (6, "gll"): "apply_pencil_trilinear_kernel<6,true,4,49,1>",
    (7, "gauss"): "apply_pencil_trilinear_kernel<7,false,4,64,1>", (7, "gll"): "apply_pencil_trilinear_kernel<7,true,4,64,1>",
    (8, "gauss"): "apply_pencil_trilinear_kernel<8,false,4,81,1>", (8, "gll"): "apply_pencil_trilinear_kernel<8,true,4,81,1>",
}


def test_kernel_names_follow_the_launch_formula():
    for (p, quad), name in KERNEL_LITERALS.items():
        assert kernel_name(p, quad) == name


def test_every_degree_ends_in_a_partly_filled_team_or_workgroup():
    for p in range(1, 9):
        partial = []
        for n_cells in (12, 13):
            cpt, teams, tpb, _ = launch_shape(p, n_cells)
            partial.append(n_cells % cpt != 0 or teams % tpb != 0)
        assert any(partial), p


# ------------------------------------------------------------------ 1. operator parity
PARITY = [(p, quad, coefficient, cells) for p in range(1, 9) for quad in sorted(QUADS) for coefficient in (pkg.COEF_ONE, pkg.COEF_STEP64)
          for cells in ((3, 2, 2), (13, 1, 1), SKEWED)]
_worst = {}


@pytest.mark.parametrize("p,quad,coefficient,cells", PARITY)
def test_operator_parity(p, quad, coefficient, cells):
    """overwrite mode on a NaN-filled dst, accumulate mode (zero_dst = 0) and bp5_apply_cells on a ragged sub-range and an empty one, both on a
    non-zero dst; coef = NULL and a coef array full of NaN; the kernel that ran; a MERGED6 handle on the same mesh beside it"""
    torch = _t()
    ref, src, want = _reference(p, cells, quad, coefficient)
    op = _operator(p, cells, quad, coefficient)
    mf = op.mf_data
    n_cells = ref.mesh.n_cells
    cpt, teams, tpb, workgroups = launch_shape(p, n_cells)
    assert mf.get_apply_variant() == 0 and op.coef is None
    s = dev(src)
    d = nan_vector(mf.n_local)
    op.vmult(d, s)
    got = d.cpu().numpy()
    assert np.isfinite(got).all()
    e = rel(got, want)
    merged = _operator(p, cells, quad, coefficient, geometry=pkg.GEOM_MERGED6)
    dm = nan_vector(mf.n_local)
    merged.vmult(dm, s)
    em = rel(dm.cpu().numpy(), want)
    _worst[cells] = tuple(max(a, b) for a, b in zip(_worst.get(cells, (0.0, 0.0)), (e, em)))
    print(f"p={p} {quad} coefficient={coefficient} cells={cells}: trilinear {e:.2e}, MERGED6 {em:.2e}; worst so far on {cells}: {_worst[cells][0]:.2e} / {_worst[cells][1]:.2e}")
    assert e <= TOL_OP
    cst = ref.mesh.constrained.astype(np.int64)
    assert np.array_equal(got[cst], src[cst]) and torch.equal(s.cpu(), torch.from_numpy(np.array(src)))
    # a coef array full of NaN is not read
    nan_coef = nan_vector(max(mf.coef_size(), 1))
    op.coef = nan_coef
    try:
        d2 = nan_vector(mf.n_local)
        op.vmult(d2, s)
    finally:
        op.coef = None
    assert rel(d2.cpu().numpy(), want) <= TOL_OP
    # dst += A src, then the Dirichlet copy
    pre = np.random.default_rng(5).uniform(-1, 1, mf.n_local)
    op.do_zero_out = False
    try:
        d = dev(pre)
        op.vmult(d, s)
    finally:
        op.do_zero_out = True
    cells_only = O.apply_cells(ref.mesh, ref.coef, ref.N, ref.D, src)
    wanted = pre + cells_only
    wanted[cst] = src[cst]
    assert rel(d.cpu().numpy(), wanted) <= TOL_OP
    # cells [c0, c1): accumulates, neither end a multiple of the cells per team where there is more than one
    c0, c1 = 1, n_cells - 2
    assert cpt == 1 or c0 % cpt, (c0, cpt)
    for coef in (None, nan_coef):
        d = dev(pre)
        mf.cell_loop(coef, s, d, c0, c1)
        wanted = O.apply_cells(ref.mesh, ref.coef, ref.N, ref.D, src, cell_range=(c0, c1), dst=pre.copy())
        assert rel(d.cpu().numpy(), wanted) <= TOL_OP
    # the empty range changes nothing
    d = dev(pre)
    mf.cell_loop(None, s, d, 3, 3)
    assert np.array_equal(d.cpu().numpy(), pre)
    # the kernel that ran
    for solver in (pkg.SolverCG, pkg.SolverCGFullMerge):
        ctl = pkg.IterationNumberControl(1, 0.0)
        solver(ctl).solve(op, op.initialize_dof_vector(), s, pkg.DiagonalMatrix())          # (b = src: non-zero also where every DoF is a Dirichlet DoF)
        assert ctl.last_step() == 1 and ctl.apply_kernel == KERNEL_LITERALS[p, quad] and not ctl.dot_products_fused, ctl.apply_kernel


@pytest.mark.parametrize("quad", sorted(QUADS))
@pytest.mark.parametrize("p", [1, 4, 6, 8])
def test_one_cell(p, quad):
    """a single, partially filled team: every other cell slot idle.  The cell is made a general hexahedron by moving its vertices."""
    um = UserMesh.from_generator(pkg.BrickMesh(p, (1, 1, 1)))
    shift = np.random.default_rng(3).uniform(-0.1, 0.1, (8, 3))
    V = T.cell_vertices(um) + shift[None]
    um.coords[um.l2g[0, T.vertex_entries(p)]] = V[0]
    T.trilinearise(um)
    ref = Reference(um, QUADS[quad][1], O.kappa_step64)
    src = O.deterministic_src(um.n_dofs, seed=60 + p)
    op = pkg.PoissonOperator(um.namespace(), QUADS[quad][0], pkg.COEF_STEP64, geometry=TRI)
    d = op.initialize_dof_vector()                       # (every DoF of a one-cell mesh may be a Dirichlet DoF: compare the cell loop itself)
    op.mf_data.cell_loop(None, dev(src), d)
    assert rel(d.cpu().numpy(), ref.apply_cells(src)) <= TOL_OP


# one mesh per barrier family: p = 2 wave-local team syncs (four one-wave teams per workgroup), p = 4 the workgroup barrier
MANY_WORKGROUPS = {2: ((5, 5, 11), 10), 4: ((7, 5, 3), 11)}


@pytest.mark.parametrize("p", sorted(MANY_WORKGROUPS))
def test_many_workgroups(p):
    """the XCD remap with teams_per_xcd > 1, idle trailing workgroups and a partly filled last team"""
    cells, expected = MANY_WORKGROUPS[p]
    n_cells = cells[0] * cells[1] * cells[2]
    cpt, teams, tpb, workgroups = launch_shape(p, n_cells)
    assert workgroups == expected >= 9 and workgroups % 8 != 0 and n_cells % cpt != 0, (cpt, teams, workgroups)
    ref, src, want = _reference(p, cells, "gauss", pkg.COEF_STEP64)
    op = _operator(p, cells, "gauss", pkg.COEF_STEP64)
    d = nan_vector(op.mf_data.n_local)
    op.vmult(d, dev(src))
    e = rel(d.cpu().numpy(), want)
    print(f"p={p} cells={cells} workgroups={workgroups}: {e:.2e}")
    assert e <= TOL_OP


def test_brick_ordered_mesh_reports_and_runs_variant_0():
    """cell bricks and block-major numbering, where a MERGED6 handle resolves to the block kernel: the trilinear handle reports and runs variant 0"""
    p, cells = 4, (6, 5, 9)
    brick = dict(cell_block=(4, 4, 4), dof_numbering=1)
    ref, src, want = _reference(p, cells, "gauss", pkg.COEF_STEP64, **brick)
    op = _operator(p, cells, "gauss", pkg.COEF_STEP64, **brick)
    assert op.mf_data.get_apply_variant() == 0
    d = nan_vector(op.mf_data.n_local)
    op.vmult(d, dev(src))
    e = rel(d.cpu().numpy(), want)
    print(f"brick-ordered p={p}: {e:.2e}")
    assert e <= TOL_OP
    for solver in (pkg.SolverCG, pkg.SolverCGFullMerge):
        ctl = pkg.IterationNumberControl(1, 0.0)
        solver(ctl).solve(op, op.initialize_dof_vector(), op.assemble_rhs(), pkg.DiagonalMatrix())
        assert ctl.apply_kernel == KERNEL_LITERALS[p, "gauss"] and not ctl.dot_products_fused, ctl.apply_kernel
    plain = _operator(p, cells, "gauss", pkg.COEF_STEP64, geometry=pkg.GEOM_MERGED6, **brick)
    plain.mf_data.set_apply_variant(56)                                     # (the block kernel exists for this mesh: only the mode keeps the handle above off it)
    assert plain.mf_data.get_apply_variant() == 56
    plain.mf_data.set_apply_variant(0)


# ------------------------------------------------------------------ 2. diagonal
@pytest.mark.parametrize("quad", sorted(QUADS))
@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_diagonal(p, quad):
    ref, _, _ = _reference(p, SKEWED, quad, pkg.COEF_STEP64)
    op = _operator(p, SKEWED, quad, pkg.COEF_STEP64)
    d = op.compute_diagonal().cpu().numpy()
    e = rel(d, ref.diagonal())
    print(f"p={p} {quad}: diagonal {e:.2e}")
    assert e <= TOL_OP
    assert np.all(d[ref.mesh.constrained.astype(np.int64)] == 1.0)
    inv = op.compute_diagonal(invert=True).cpu().numpy()
    assert rel(inv, 1.0 / ref.diagonal()) <= TOL_OP


# ------------------------------------------------------------------ 3. solvers
GPU_SOLVERS = {"plain": (pkg.SolverCG, O.cg_plain), "merged": (pkg.SolverCGFullMerge, O.cg_merged)}
CG_ITERATIONS = 10
CG_CELLS = (4, 4, 4)


def _cg_case(p):
    key = ("cg", p)
    if key not in _cache:
        ref, _, _ = _reference(p, CG_CELLS, "gauss", pkg.COEF_STEP64)
        b, inv = ref.rhs(), 1.0 / ref.diagonal()
        for a in (b, inv):
            a.setflags(write=False)
        _cache[key] = (ref, b, inv)
    return _cache[key]


@pytest.mark.parametrize("solver", sorted(GPU_SOLVERS))
@pytest.mark.parametrize("p", [2, 4])
def test_cg_at_a_fixed_iteration_count(p, solver):
    """ten Jacobi-CG iterations on 4^3 skewed cells with step-64's coefficient against O.cg_plain / O.cg_merged on the reference operator"""
    ref, b, inv = _cg_case(p)
    op = _operator(p, CG_CELLS, "gauss", pkg.COEF_STEP64)
    xr, k, res = GPU_SOLVERS[solver][1](ref.vmult, b, CG_ITERATIONS, diag=inv)
    bg = op.assemble_rhs()
    assert rel(bg.cpu().numpy(), b) <= TOL_OP
    inv_g = op.compute_diagonal(invert=True)
    x = nan_vector(op.mf_data.n_local)
    ctl = pkg.IterationNumberControl(CG_ITERATIONS, 0.0)
    GPU_SOLVERS[solver][0](ctl).solve(op, x, bg, pkg.DiagonalMatrix(inv_g))
    e = rel(x.cpu().numpy(), xr)
    print(f"p={p} {solver}: {e:.2e}, residual {ctl.last_value():.6e} (numpy {res:.6e}), kernel {ctl.apply_kernel}")
    assert ctl.last_step() == k == CG_ITERATIONS and e <= TOL_CG
    assert abs(ctl.last_value() - res) <= 1e-9 * res
    assert ctl.dot_products_fused == 0 and ctl.apply_kernel == KERNEL_LITERALS[p, "gauss"]      # the merged solver runs its separate dot-product kernels


def _stop(A, b, inv, k_min=8, k_max=40):
    """the first iteration k >= k_min whose residual undercuts every earlier one by 8 %, and a tolerance half way (geometrically) between that
    residual and the lowest earlier one (the rule of tests/test_gpu_overint.py)"""
    hist = []
    O.cg_plain(A, b, k_max, diag=inv, history=hist)
    res = [float(np.linalg.norm(b))] + hist
    for k in range(k_min, k_max + 1):
        low = min(res[:k])
        if res[k] < 0.92 * low:
            return k, float(np.sqrt(res[k] * low))
    raise AssertionError("no clear record low in the reference's residual history")


@pytest.mark.parametrize("solver", sorted(GPU_SOLVERS))
def test_cg_tolerance_stop(solver):
    ref, b, inv = _cg_case(4)
    op = _operator(4, CG_CELLS, "gauss", pkg.COEF_STEP64)
    k_stop, tol = _stop(ref.vmult, b, inv)
    _, k_ref, _ = GPU_SOLVERS[solver][1](ref.vmult, b, 100, tol=tol, diag=inv)
    bg, x = op.assemble_rhs(), op.initialize_dof_vector()
    ctl = pkg.IterationNumberControl(100, tol)
    GPU_SOLVERS[solver][0](ctl).solve(op, x, bg, pkg.DiagonalMatrix(op.compute_diagonal(invert=True)))
    true_res = np.linalg.norm(ref.vmult(x.cpu().numpy()) - b)
    print(f"{solver}: stop at {ctl.last_step()} (numpy {k_ref}, record low at {k_stop}), tolerance {tol:.3e}, recomputed residual {true_res:.3e}")
    assert ctl.last_step() == k_ref and (solver != "plain" or k_ref == k_stop)
    assert ctl.last_value() <= tol and true_res <= tol


def _chebyshev_pcg(op, b, tol):
    Cheb = pkg.PreconditionChebyshev
    ch = Cheb().initialize(op, Cheb.AdditionalData(degree=2, smoothing_range=20.0, preconditioner=pkg.DiagonalMatrix(op.compute_diagonal(invert=True))))
    x = op.initialize_dof_vector()
    ctl = pkg.IterationNumberControl(200, tol)
    pkg.SolverCG(ctl).solve(op, x, b, ch)
    return ctl, x, ch.estimated_eigenvalues()


def test_chebyshev_pcg_takes_the_iterations_of_the_merged6_handle():
    """bp5_chebyshev_create and bp5_cg_solve_preconditioned: eigenvalue bounds and iteration count of a MERGED6 handle on the same mesh"""
    tri, merged = (_operator(4, CG_CELLS, "gauss", pkg.COEF_STEP64, geometry=g) for g in (TRI, pkg.GEOM_MERGED6))
    b = merged.assemble_rhs()
    tol = 1e-8 * float(_t().linalg.norm(b))
    (ca, xa, ea), (cb, xb, eb) = _chebyshev_pcg(tri, b, tol), _chebyshev_pcg(merged, b, tol)
    print(f"Chebyshev(2)-PCG: trilinear {ca.last_step()} iterations, MERGED6 {cb.last_step()}; bounds {ea['max_used']:.6e} / {eb['max_used']:.6e}")
    assert ca.last_step() == cb.last_step() < 200 and ca.last_value() <= tol
    assert abs(ea["max_used"] - eb["max_used"]) <= 1e-10 * eb["max_used"] and abs(ea["min_used"] - eb["min_used"]) <= 1e-10 * eb["min_used"]
    assert ca.apply_kernel == KERNEL_LITERALS[4, "gauss"]
    ref, _, _ = _cg_case(4)
    assert np.linalg.norm(ref.vmult(xa.cpu().numpy()) - b.cpu().numpy()) <= 1.01 * tol


def test_cg_through_a_callback_operator():
    """bp5_cg_solve_operator: the solvers need nothing of A but vmult"""
    ref, b, inv = _cg_case(4)
    op = _operator(4, CG_CELLS, "gauss", pkg.COEF_STEP64)

    class Wrapped:                                                           # not a PoissonOperator: solved through the callback entry point
        mf_data = op.mf_data

        def vmult(self, dst, src):
            op.vmult(dst, src)
    xr, k, _ = O.cg_plain(ref.vmult, b, CG_ITERATIONS, diag=inv)
    x = nan_vector(op.mf_data.n_local)
    ctl = pkg.IterationNumberControl(CG_ITERATIONS, 0.0)
    pkg.SolverCG(ctl).solve(Wrapped(), x, op.assemble_rhs(), pkg.DiagonalMatrix(op.compute_diagonal(invert=True)))
    assert ctl.last_step() == k and rel(x.cpu().numpy(), xr) <= TOL_CG


@pytest.mark.parametrize("p", [2, 4])
def test_no_dirichlet_dofs(p):
    """a handle without Dirichlet DoFs: the operator, its null space (constants) and the diagonal"""
    torch = _t()
    um = T.user_mesh(pkg, p, SKEWED)
    um.constrained = np.zeros(0, dtype=np.int64)
    ref = Reference(um, O.QUAD_GAUSS, O.kappa_step64)
    op = pkg.PoissonOperator(um.namespace(), pkg.QUAD_GAUSS, pkg.COEF_STEP64, geometry=TRI)
    n = op.mf_data.n_local
    src = O.deterministic_src(n, seed=60 + p)
    lu = nan_vector(n)
    op.vmult(lu, dev(src))
    assert rel(lu.cpu().numpy(), ref.vmult(src)) <= TOL_OP
    z = nan_vector(n)
    op.vmult(z, torch.ones(n, dtype=torch.float64, device="cuda:0"))
    assert float(z.abs().max()) <= 1e-12 * float(lu.abs().max())
    d = op.compute_diagonal().cpu().numpy()
    assert rel(d, ref.diagonal()) <= TOL_OP and d.min() > 0.0


def test_two_level_multigrid():
    """bp5_mg_create needs the apply and diagonal paths only: a p = 2 -> 1 hierarchy of trilinear handles gives the V-cycle and the PCG iteration
    count of the MERGED6 hierarchy on the same meshes (the p = 1 sine mesh has the fine mesh's vertices and is trilinear as generated)"""
    torch = _t()
    mesh = pkg.BrickMesh(2, SKEWED, deform_amp=AMP)
    view = SimpleNamespace(p=2, l2g=mesh.l2g, coords=np.array(mesh.coords))
    mesh.coords[:] = T.trilinearise(view).coords
    out = {}
    for name, geometry in (("trilinear", TRI), ("merged6", pkg.GEOM_MERGED6)):
        fine = pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_STEP64, geometry=geometry)
        ops = pkg.make_mg_hierarchy(fine)
        assert [o.mf_data.mesh.degree for o in ops] == [2, 1] and all(o.geometry == geometry for o in ops)
        mg = pkg.PreconditionMG(ops)
        b = fine.assemble_rhs()
        v = nan_vector(fine.mf_data.n_local)
        mg.vmult(v, b)
        x = fine.initialize_dof_vector()
        ctl = pkg.IterationNumberControl(100, 1e-10 * float(torch.linalg.norm(b)))
        pkg.SolverCG(ctl).solve(fine, x, b, mg)
        out[name] = (v.cpu().numpy(), ctl.last_step(), x.cpu().numpy())
    e = rel(out["trilinear"][0], out["merged6"][0])
    print(f"two-level V-cycle: {e:.2e}; PCG iterations {out['trilinear'][1]} / {out['merged6'][1]}")
    assert e <= 1e-10                                                        # (the level bounds come from a Lanczos run: rounding amplified)
    assert out["trilinear"][1] == out["merged6"][1] < 100 and rel(out["trilinear"][2], out["merged6"][2]) <= 1e-8


# ------------------------------------------------------------------ 4. the mode's check of the mesh
def _refused(fn):
    with pytest.raises(pkg.BP5Error) as e:
        fn()
    return e.value.status, str(e.value)


def test_the_sine_mesh_is_refused_and_the_handle_stays_merged6():
    p, cells = 2, (3, 2, 2)
    sine = UserMesh.from_generator(pkg.BrickMesh(p, cells, deform_amp=AMP))
    op = pkg.PoissonOperator(sine.namespace(), pkg.QUAD_GAUSS, pkg.COEF_STEP64)
    st, msg = _refused(lambda: op.mf_data.set_geometry_mode(TRI))
    assert st == 5 and "not trilinear" in msg, msg
    ref = Reference(sine, O.QUAD_GAUSS, O.kappa_step64)
    src = O.deterministic_src(sine.n_dofs, seed=3)
    d = nan_vector(op.mf_data.n_local)
    op.vmult(d, dev(src))                                                    # still MERGED6: reads its planes
    assert rel(d.cpu().numpy(), ref.vmult(src)) <= TOL_OP
    st, msg = _refused(lambda: op.mf_data.cell_loop(None, dev(src), d))      # ... and a NULL coef is still an error
    assert st == 1, msg
    st, msg = _refused(lambda: pkg.PoissonOperator(sine.namespace(), pkg.QUAD_GAUSS, geometry=TRI))
    assert st == 5 and "not trilinear" in msg, msg


def test_switching_to_the_mode_and_back():
    ref, src, want = _reference(4, SKEWED, "gauss", pkg.COEF_STEP64)
    op = pkg.PoissonOperator(_mesh(4, SKEWED).namespace(), pkg.QUAD_GAUSS, pkg.COEF_STEP64)
    s = dev(src)
    results = []
    for mode in (pkg.GEOM_MERGED6, TRI, pkg.GEOM_MERGED6, TRI):
        op.mf_data.set_geometry_mode(mode)
        d = nan_vector(op.mf_data.n_local)
        op.vmult(d, s)
        results.append(d.cpu().numpy())
        assert rel(results[-1], want) <= TOL_OP
        ctl = pkg.IterationNumberControl(1, 0.0)
        pkg.SolverCG(ctl).solve(op, op.initialize_dof_vector(), s, pkg.DiagonalMatrix())
        assert ctl.apply_kernel.startswith("apply_pencil_trilinear_kernel<4," if mode == TRI else "apply_pencil_kernel<4,"), ctl.apply_kernel
    st, msg = _refused(lambda: op.mf_data.set_geometry_mode(3))
    assert st == 1 and "unknown geometry mode" in msg, msg


@pytest.mark.parametrize("p", [2, 5])
def test_an_undeformed_mesh_is_accepted_and_equals_the_affine_mode(p):
    mesh = pkg.BrickMesh(p, (3, 2, 2))
    a = pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_STEP64, geometry=TRI)
    b = pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_STEP64, geometry=pkg.GEOM_AFFINE)
    s = dev(O.deterministic_src(mesh.n_local, seed=11))
    da, db = nan_vector(mesh.n_local), nan_vector(mesh.n_local)
    a.vmult(da, s)
    b.vmult(db, s)
    assert rel(da.cpu().numpy(), db.cpu().numpy()) <= TOL_OP
    assert rel(a.compute_diagonal().cpu().numpy(), b.compute_diagonal().cpu().numpy()) <= TOL_OP


# ------------------------------------------------------------------ 5. refusals
def test_refusals():
    """every refusal is BP5_ERR_UNSUPPORTED (5) with the word "trilinear", decided before any launch, in either order of the two setter calls"""
    torch = _t()
    mesh = pkg.BrickMesh(2, (3, 2, 2))
    new = lambda m=mesh, quad=pkg.QUAD_GAUSS: pkg.MatrixFree().reinit(m, quad, pkg.COEF_ONE)

    def tri():
        mf = new()
        mf.set_geometry_mode(TRI)
        return mf

    def both_orders(setter, word):
        mf = tri()
        st, msg = _refused(lambda: setter(mf))                               # the mode first
        assert st == 5 and "trilinear" in msg and word in msg, msg
        mf = new()
        setter(mf)
        st, msg = _refused(lambda: mf.set_geometry_mode(TRI))                # the mode second
        assert st == 5 and "trilinear" in msg and word in msg, msg
    both_orders(lambda mf: mf.set_operator(pkg.OP_HELMHOLTZ), "Helmholtz")
    both_orders(lambda mf: mf.set_operator(pkg.OP_MASS), "mass")
    both_orders(lambda mf: mf.set_metric_precision("float32"), "FP32")
    for v in (10, 50, 56, 70, 110):                                          # (the variants a p = 2 handle takes)
        both_orders(lambda mf: mf.set_apply_variant(v), "variant")
    mf = tri()
    for v in (1, 90):                                                        # (no p = 2 handle takes these: the mode's refusal comes first)
        st, msg = _refused(lambda: mf.set_apply_variant(v))
        assert st == 5 and "trilinear" in msg and mf.get_apply_variant() == 0, msg
    # what is part of the handle from its creation: one call order
    st, msg = _refused(lambda: new(quad=pkg.QUAD_GAUSS_OVER).set_geometry_mode(TRI))
    assert st == 5 and "trilinear" in msg and "quadrature" in msg, msg
    st, msg = _refused(lambda: pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS_OVER, geometry=TRI))
    assert st == 5 and "trilinear" in msg, msg
    hanging = O.HangingBrickMesh(2, 2, 2, 1, 3)
    hns = SimpleNamespace(degree=2, n=3, n_cells=hanging.n_cells, n_interior_cells=hanging.n_cells, n_owned=hanging.n_dofs, n_ghost=0, n_local=hanging.n_dofs,
                          n_global_dofs=hanging.n_dofs, l2g=hanging.l2g, coords=hanging.coords, constrained=hanging.constrained, n_neighbors=0,
                          neighbor_rank=np.zeros(0, np.int32), send_offsets=np.zeros(1, np.uint32), send_indices=np.zeros(0, np.uint32),
                          recv_offsets=np.zeros(1, np.uint32), cell_block_offsets=None, constraint_mask=hanging.constraint_mask, rank=0, n_ranks=1,
                          global_ids=np.arange(hanging.n_dofs, dtype=np.uint64))
    st, msg = _refused(lambda: new(hns).set_geometry_mode(TRI))
    assert st == 5 and "trilinear" in msg and "hanging" in msg, msg
    st, msg = _refused(lambda: tri().get_data())
    assert st == 5 and "trilinear" in msg, msg
    # brick meshes, where a MERGED6 handle takes variant 56: variant 0 is reported, 56 is refused
    bricks = pkg.BrickMesh(4, (8, 8, 8), cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1)
    mf = new(bricks)
    mf.set_apply_variant(56)
    assert mf.get_apply_variant() == 56
    mf.set_apply_variant(0)
    mf.set_geometry_mode(TRI)
    assert mf.get_apply_variant() == 0
    st, msg = _refused(lambda: mf.set_apply_variant(56))
    assert st == 5 and "trilinear" in msg, msg
    # block vectors, x untouched
    op = pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, geometry=TRI)
    x, b = op.initialize_block_vector(3), op.initialize_block_vector(3)
    b.fill_(1.0)
    x.fill_(7.0)
    st, msg = _refused(lambda: op.vmult(x, b))
    assert st == 5 and "trilinear" in msg, msg
    st, msg = _refused(lambda: pkg.SolverCG(pkg.IterationNumberControl(3, 0.0)).solve(op, x, b, pkg.DiagonalMatrix()))
    assert st == 5 and "trilinear" in msg, msg
    assert bool((x == 7.0).all())                                            # refused before any launch
    # elasticity on a handle in the mode (the mode second), and the mode on a handle whose ten planes exist: the entries refuse, x untouched
    el = pkg.ElasticityOperator(mesh, pkg.QUAD_GAUSS)
    el.mf_data.set_geometry_mode(TRI)
    xe, be = el.initialize_block_vector(), el.initialize_block_vector()
    be.fill_(1.0)
    xe.fill_(7.0)
    st, msg = _refused(lambda: el.vmult(xe, be))
    assert st == 5 and "trilinear" in msg and "elasticity" in msg, msg
    st, msg = _refused(lambda: el.cell_loop(be, xe))
    assert st == 5 and "trilinear" in msg, msg
    st, msg = _refused(lambda: el.compute_diagonal())
    assert st == 5 and "trilinear" in msg, msg
    st, msg = _refused(lambda: pkg.SolverCG(pkg.IterationNumberControl(3, 0.0)).solve(el, xe, be, pkg.DiagonalMatrix()))
    assert st == 5 and "trilinear" in msg, msg
    assert bool((xe == 7.0).all())
    el.mf_data.set_geometry_mode(pkg.GEOM_MERGED6)                           # back: the entries work again
    el.vmult(xe, be)
    assert bool(torch.isfinite(xe).all())
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 6. a busy non-blocking side stream
def test_vmult_and_solve_on_a_busy_side_stream():
    torch = _t()
    ref, b_np, inv_np = _cg_case(2)
    src = O.deterministic_src(ref.mesh.n_dofs, seed=62)
    want = ref.vmult(src)
    xr, k, _ = O.cg_plain(ref.vmult, b_np, CG_ITERATIONS, diag=inv_np)
    S = SH.side_stream()
    with torch.cuda.stream(S):
        op = pkg.PoissonOperator(_mesh(2, CG_CELLS).namespace(), pkg.QUAD_GAUSS, pkg.COEF_STEP64, geometry=TRI, stream=S.cuda_stream)
        assert op.mf_data.stream == S.cuda_stream
        good = {name: SH.on_device(a) for name, a in (("src", src), ("b", b_np), ("inv", inv_np))}
        work = {name: torch.empty_like(g) for name, g in good.items()}
        d = torch.empty_like(good["src"])
        x = torch.empty_like(good["src"])
        torch.cuda.synchronize()
    for warmed in (False, True):                                             # bp5_apply is asynchronous: the warmed call returns while the hold lasts
        got, _ = SH.run(S, [(work["src"], good["src"])], [(d, None)], lambda: op.vmult(d, work["src"]), asynchronous=warmed, scale=1.0 if warmed else 2.0)
        assert rel(got[0].cpu().numpy(), want) <= TOL_OP
    for both in (False, True):
        ctl = pkg.IterationNumberControl(CG_ITERATIONS, 0.0)
        got, _ = SH.run(S, [(work["b"], good["b"]), (work["inv"], good["inv"])], [(x, None)],
                        lambda: pkg.SolverCG(ctl).solve(op, x, work["b"], pkg.DiagonalMatrix(work["inv"])), hold_null=both)
        assert ctl.last_step() == k and rel(got[0].cpu().numpy(), xr) <= TOL_CG
        assert ctl.apply_kernel == KERNEL_LITERALS[2, "gauss"]


# ------------------------------------------------------------------ 7. neighbours' bits
def test_other_handles_keep_their_bits():
    """a p = 4 MERGED6 handle's block-kernel vmult and a 5-iteration solve, bit for bit before and after trilinear calls on another handle"""
    torch = _t()
    brick = dict(cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1)
    um = _mesh(4, (6, 5, 9), **brick)
    op = pkg.PoissonOperator(um.namespace(), pkg.QUAD_GAUSS, pkg.COEF_STEP64)
    op.mf_data.set_apply_variant(56)
    s = dev(O.deterministic_src(um.n_dofs, seed=9))
    b = op.assemble_rhs()                                                    # once: its atomic scatter is not reproducible bit by bit

    def run():
        d = op.initialize_dof_vector()
        op.vmult(d, s)
        x = op.initialize_dof_vector()
        ctl = pkg.IterationNumberControl(5, 0.0)
        pkg.SolverCG(ctl).solve(op, x, b, pkg.DiagonalMatrix())
        assert ctl.apply_kernel.startswith("apply_block_kernel<4,false,32,")
        return d.clone(), x.clone()
    before = run()
    tri = pkg.PoissonOperator(um.namespace(), pkg.QUAD_GAUSS, pkg.COEF_STEP64, geometry=TRI)
    y = tri.initialize_dof_vector()
    tri.vmult(y, s)
    tri.compute_diagonal()
    pkg.SolverCGFullMerge(pkg.IterationNumberControl(3, 0.0)).solve(tri, tri.initialize_dof_vector(), tri.assemble_rhs(), pkg.DiagonalMatrix())
    after = run()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


# ------------------------------------------------------------------ 8. the example
def test_example_solves_the_same_problem_in_both_modes():
    exe = os.path.join(bp5_pkg.ROOT, "examples", "bp5_q1_mapping")
    assert os.path.exists(exe), "examples/bp5_q1_mapping missing: run __graft_entry__.build()"
    out = subprocess.run([exe, "3", "4", "1e-10", "0.04"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    vals = dict(line.split("=", 1) for line in out.stdout.split() if "=" in line)
    print(out.stdout.strip())
    a, b = float(vals["l2_norm_trilinear"]), float(vals["l2_norm_merged6"])
    assert a > 0.0 and abs(a - b) <= 1e-10 * b
    assert vals["apply_kernel_trilinear"] == KERNEL_LITERALS[3, "gauss"]
    assert int(vals["iterations_trilinear"]) == int(vals["iterations_merged6"])
