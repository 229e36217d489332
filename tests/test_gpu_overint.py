"""Gauss(p+2) quadrature on the GPU (BP5_QUAD_GAUSS_OVER; CEED BP3 = pkg.PoissonOperator, CEED BP1 = pkg.MassOperator on such a handle): the planes,
the two pencil kernels and the diagonal against the numpy reference of tests/overint_ref.py (pinned outside itself by tests/test_overint_cpu.py),
handles without Dirichlet DoFs, both CG solvers and the Chebyshev-preconditioned one against their numpy statements, every refusal, and the bits of
neighbouring handles.  The kernels scatter with atomics: results are compared to the project's tolerances (1e-13 operator, 1e-11 CG at a fixed
count)."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import chebyshev_ref as CR
import overint_ref as R
from test_overint_cpu import CG_CASES, CG_ITERATIONS, SOLVERS, cg_reference

pytestmark = pytest.mark.gpu
pkg = bp5_pkg.load()
OVER = pkg.QUAD_GAUSS_OVER
TOL_OP = 1e-13     # one operator application (rounding + atomic summation order)
TOL_CG = 1e-11     # CG solution vector at a fixed iteration count
AMP = 0.04
KAPPA = {pkg.COEF_ONE: O.kappa_none, pkg.COEF_STEP64: O.kappa_step64}
CLASSES = {"poisson": pkg.PoissonOperator, "mass": pkg.MassOperator}
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


def namespace(m, constrained=None):
    """an oracle mesh as MatrixFree.reinit takes it (one rank, lexicographic); constrained: another Dirichlet set (empty: BP1)"""
    return SimpleNamespace(degree=m.p, n=m.n, n_cells=m.n_cells, n_interior_cells=m.n_cells, n_owned=m.n_dofs, n_ghost=0, n_local=m.n_dofs,
                           n_global_dofs=m.n_dofs, l2g=m.l2g, coords=m.coords, constrained=m.constrained if constrained is None else constrained,
                           n_neighbors=0, neighbor_rank=np.zeros(0, np.int32), send_offsets=np.zeros(1, np.uint32),
                           send_indices=np.zeros(0, np.uint32), recv_offsets=np.zeros(1, np.uint32), cell_block_offsets=None,
                           constraint_mask=getattr(m, "constraint_mask", None), rank=0, n_ranks=1, global_ids=np.arange(m.n_dofs, dtype=np.uint64))


def _problem(p, cls, cells=(3, 2, 2), amp=AMP, coefficient=pkg.COEF_ONE, dirichlet=True, h=1.0):
    """reference problem, a source (non-zero on the boundary) and its vmult -- computed once, never changed"""
    key = (p, cls, cells, amp, coefficient, dirichlet, h)
    if key not in _cache:
        pr = R.Problem(p, cells, h=h, deform_amp=amp, kappa=KAPPA[coefficient], mass=cls == "mass", dirichlet=dirichlet)
        src = O.deterministic_src(pr.mesh.n_dofs, seed=60 + p)
        ref = pr.vmult(src)
        for a in (src, ref):
            a.setflags(write=False)
        _cache[key] = (pr, src, ref)
    return _cache[key]


def _operator(p, cls, cells=(3, 2, 2), amp=AMP, coefficient=pkg.COEF_ONE, dirichlet=True, h=1.0):
    key = ("op", p, cls, cells, amp, coefficient, dirichlet, h)
    if key not in _cache:
        mesh = pkg.BrickMesh(p, cells, h=h, deform_amp=amp) if dirichlet else namespace(O.BrickMesh(p, cells, h=h, deform_amp=amp), np.zeros(0, np.uint32))
        _cache[key] = CLASSES[cls](mesh, OVER, coefficient)
    return _cache[key]


def launch_shape(p, n_cells):
    """(cells per team, teams, teams per workgroup, workgroups) as csrc/overint/bp5_overint.hip launches both kernels: OverintShape<p> -- (p+2)^2 lanes
    per cell; four one-wave teams per workgroup where a cell fits a wave's share (p <= 3, p = 6), else one four-wave team"""
    one_wave = p <= 3 or p == 6
    tw, tpb = (1, 4) if one_wave else (4, 1)
    cpt = 64 * tw // (p + 2) ** 2
    teams = -(-n_cells // cpt)
    return cpt, teams, tpb, -(-teams // tpb)


def kernel_name(p, cls):
    one_wave = p <= 3 or p == 6
    tw, tpb = (1, 4) if one_wave else (4, 1)
    if cls == "mass":
        return "apply_pencil_mass_q_kernel<%d,%d,%d,%d>" % (p, tw, (p + 2) ** 2, tpb)
    return "apply_pencil_q_kernel<%d,%d,%d,%d,%s>" % (p, tw, (p + 2) ** 2, tpb, "true" if p <= 4 else "false")


# the kernel names as literals, so that a change of the launch shapes has to be made here too
KERNEL_LITERALS = {
    (1, "poisson"): "apply_pencil_q_kernel<1,1,9,4,true>", (2, "poisson"): "apply_pencil_q_kernel<2,1,16,4,true>",
    (3, "poisson"): "apply_pencil_q_kernel<3,1,25,4,true>", (4, "poisson"): "apply_pencil_q_kernel<4,4,36,1,true>",
    (5, "poisson"): "apply_pencil_q_kernel<5,4,49,1,false>", (6, "poisson"): "apply_pencil_q_kernel<6,1,64,4,false>",
    (7, "poisson"): "apply_pencil_q_kernel<7,4,81,1,false>", (8, "poisson"): "apply_pencil_q_kernel<8,4,100,1,false>",
    (1, "mass"): "apply_pencil_mass_q_kernel<1,1,9,4>", (2, "mass"): "apply_pencil_mass_q_kernel<2,1,16,4>",
    (3, "mass"): "apply_pencil_mass_q_kernel<3,1,25,4>", (4, "mass"): "apply_pencil_mass_q_kernel<4,4,36,1>",
    (5, "mass"): "apply_pencil_mass_q_kernel<5,4,49,1>", (6, "mass"): "apply_pencil_mass_q_kernel<6,1,64,4>",
    (7, "mass"): "apply_pencil_mass_q_kernel<7,4,81,1>", (8, "mass"): "apply_pencil_mass_q_kernel<8,4,100,1>",
}


def test_kernel_names_follow_the_launch_formula():
    for (p, cls), name in KERNEL_LITERALS.items():
        assert kernel_name(p, cls) == name


# ------------------------------------------------------------------ 1. sizing and planes
@pytest.mark.parametrize("cls", sorted(CLASSES))
@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_planes_and_coef_size(p, cls):
    """deformed cells + step-64's coefficient: 6 (or 1) planes of n_cells (p+2)^3 entries, through bp5_mf_metric_to_reference_layout"""
    pr, _, _ = _problem(p, cls, coefficient=pkg.COEF_STEP64)
    op = _operator(p, cls, coefficient=pkg.COEF_STEP64)
    planes = 1 if cls == "mass" else 6
    n_entries = planes * pr.mesh.n_cells * (p + 2) ** 3
    assert op.mf_data.coef_size() == n_entries == op.coef.numel()
    got = op.mf_data.coef_reference_layout(op.coef).cpu().numpy().reshape(planes, pr.mesh.n_cells, -1)
    want = pr.coef.reshape(planes, pr.mesh.n_cells, -1)
    e = max(rel(got[c], want[c]) for c in range(3 if planes == 6 else 1))                 # the diagonal planes one by one ...
    eo = np.linalg.norm(got - want) / np.linalg.norm(want)                                  # ... and all of them (the off-diagonal ones are small)
    print(f"p={p} {cls}: planes {e:.2e} / {eo:.2e}")
    assert e <= TOL_OP and eo <= TOL_OP


# ------------------------------------------------------------------ 2. operator parity
def _coefficients(p):
    return {1: (pkg.COEF_STEP64,), 4: (pkg.COEF_ONE, pkg.COEF_STEP64), 8: (pkg.COEF_ONE, pkg.COEF_STEP64)}.get(p, (pkg.COEF_ONE,))


PARITY = [(p, cls, coefficient, cells) for p in range(1, 9) for cls in sorted(CLASSES) for coefficient in _coefficients(p) for cells in ((3, 2, 2), (13, 1, 1))
          if cells == (3, 2, 2) or coefficient == _coefficients(p)[0]]


@pytest.mark.parametrize("p,cls,coefficient,cells", PARITY)
def test_operator_parity(p, cls, coefficient, cells):
    """overwrite mode on a NaN-filled dst, accumulate mode (zero_dst = 0) and bp5_apply_cells on a ragged sub-range, both on a non-zero dst.
    (3, 2, 2): 12 cells end in a partly filled team where 12 is no multiple of the cells per team (p = 1, 4, 5 with the shapes chosen); (13, 1, 1)
    ends in a partly filled team -- at p = 6, one cell per team, a partly filled workgroup -- at EVERY degree"""
    torch = _t()
    pr, src, ref = _problem(p, cls, cells=cells, coefficient=coefficient)
    op = _operator(p, cls, cells=cells, coefficient=coefficient)
    mf = op.mf_data
    n_cells = pr.mesh.n_cells
    cpt, teams, tpb, workgroups = launch_shape(p, n_cells)
    if cells == (13, 1, 1):
        assert n_cells % cpt != 0 or (cpt == 1 and teams % tpb != 0), (p, cpt, teams, tpb)
    else:
        assert (n_cells % cpt != 0) == (p in (1, 4, 5)), (p, cpt)
    assert mf.get_apply_variant() == 0
    s = dev(src)
    d = nan_vector(mf.n_local)
    op.vmult(d, s)
    got = d.cpu().numpy()
    assert np.isfinite(got).all()
    e = rel(got, ref)
    print(f"p={p} {cls} coefficient={coefficient} cells={cells}: vmult {e:.2e}")
    assert e <= TOL_OP
    cst = pr.mesh.constrained.astype(np.int64)
    assert np.array_equal(got[cst], src[cst]) and torch.equal(s.cpu(), torch.from_numpy(np.array(src)))
    # dst += A src, then the Dirichlet copy
    pre = np.random.default_rng(5).uniform(-1, 1, mf.n_local)
    op.do_zero_out = False
    try:
        d = dev(pre)
        op.vmult(d, s)
    finally:
        op.do_zero_out = True
    want = pre + pr.apply_cells(src)
    want[cst] = src[cst]
    assert rel(d.cpu().numpy(), want) <= TOL_OP
    # cells [c0, c1): accumulates, neither end a multiple of the cells per team where there is more than one
    c0, c1 = 1, n_cells - 2
    assert cpt == 1 or c0 % cpt, (c0, cpt)
    d = dev(pre)
    mf.cell_loop(op.coef, s, d, c0, c1)
    want = pr.apply_cells(src, cell_range=(c0, c1), dst=pre.copy())
    assert rel(d.cpu().numpy(), want) <= TOL_OP
    # the empty range changes nothing
    d = dev(pre)
    mf.cell_loop(op.coef, s, d, 3, 3)
    assert np.array_equal(d.cpu().numpy(), pre)
    # the kernel that ran
    ctl = pkg.IterationNumberControl(1, 0.0)
    pkg.SolverCG(ctl).solve(op, op.initialize_dof_vector(), s, pkg.DiagonalMatrix())      # (b = src: non-zero also where every DoF is a Dirichlet DoF, p = 1 on (13, 1, 1))
    assert ctl.last_step() == 1 and ctl.apply_kernel == KERNEL_LITERALS[p, cls] and not ctl.dot_products_fused, ctl.apply_kernel


@pytest.mark.parametrize("cls", sorted(CLASSES))
@pytest.mark.parametrize("p", [1, 4, 6, 8])
def test_one_cell(p, cls):
    """a single, partially filled team: every other cell slot idle"""
    pr, src, ref = _problem(p, cls, cells=(1, 1, 1), coefficient=pkg.COEF_STEP64)
    op = _operator(p, cls, cells=(1, 1, 1), coefficient=pkg.COEF_STEP64)
    d = op.initialize_dof_vector()                       # (every DoF of a one-cell mesh is a Dirichlet DoF: compare the cell loop itself)
    op.mf_data.cell_loop(op.coef, dev(src), d)
    assert rel(d.cpu().numpy(), pr.apply_cells(src)) <= TOL_OP


# one mesh per barrier family: p = 2 wave-local team syncs (four one-wave teams per workgroup), p = 4 the workgroup barrier
MANY_WORKGROUPS = {2: ((7, 7, 3), 10), 4: ((5, 5, 3), 11)}


@pytest.mark.parametrize("cls", sorted(CLASSES))
@pytest.mark.parametrize("p", sorted(MANY_WORKGROUPS))
def test_many_workgroups(p, cls):
    """the XCD remap with teams_per_xcd > 1, idle trailing workgroups and a partly filled last team"""
    cells, expected = MANY_WORKGROUPS[p]
    n_cells = cells[0] * cells[1] * cells[2]
    cpt, teams, tpb, workgroups = launch_shape(p, n_cells)
    assert workgroups == expected >= 9 and workgroups % 8 != 0 and n_cells % cpt != 0, (cpt, teams, workgroups)
    pr, src, ref = _problem(p, cls, cells=cells)
    op = _operator(p, cls, cells=cells)
    d = nan_vector(op.mf_data.n_local)
    op.vmult(d, dev(src))
    e = rel(d.cpu().numpy(), ref)
    print(f"p={p} {cls} cells={cells} workgroups={workgroups}: {e:.2e}")
    assert e <= TOL_OP


def test_brick_ordered_mesh_still_runs_the_pencil_kernel():
    """cell bricks and block-major numbering, where a p + 1 handle resolves to the block kernel: the over-integrated handle reports and runs the
    pencil kernel, and matches the reference through the permutation"""
    p, cells = 4, (6, 5, 9)
    mesh = pkg.BrickMesh(p, cells, deform_amp=AMP, cell_block=(4, 4, 4), dof_numbering=1)
    perm = mesh.global_ids.astype(np.int64)
    for cls in sorted(CLASSES):
        op = CLASSES[cls](mesh, OVER, pkg.COEF_STEP64)
        assert op.mf_data.get_apply_variant() == 0
        pr = R.Problem(p, cells, deform_amp=AMP, kappa=O.kappa_step64, mass=cls == "mass")
        src_lex = O.deterministic_src(pr.mesh.n_dofs, seed=8)
        d = nan_vector(op.mf_data.n_local)
        op.vmult(d, dev(src_lex[perm]))
        e = rel(d.cpu().numpy(), pr.vmult(src_lex)[perm])
        print(f"brick-ordered p={p} {cls}: {e:.2e}")
        assert e <= TOL_OP
        for solver in (pkg.SolverCG, pkg.SolverCGFullMerge):
            ctl = pkg.IterationNumberControl(1, 0.0)
            solver(ctl).solve(op, op.initialize_dof_vector(), op.assemble_rhs(), pkg.DiagonalMatrix())
            assert ctl.apply_kernel == KERNEL_LITERALS[p, cls] and not ctl.dot_products_fused, ctl.apply_kernel
    plain = pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_STEP64)
    plain.mf_data.set_apply_variant(56)                                     # (the block kernel exists for this mesh: only the quadrature keeps the handles above off it)
    assert plain.mf_data.get_apply_variant() == 56


# ------------------------------------------------------------------ 3. diagonal
@pytest.mark.parametrize("cls", sorted(CLASSES))
@pytest.mark.parametrize("p", [2, 4])
def test_diagonal(p, cls):
    pr, _, _ = _problem(p, cls, coefficient=pkg.COEF_STEP64)
    op = _operator(p, cls, coefficient=pkg.COEF_STEP64)
    d = op.compute_diagonal().cpu().numpy()
    assert rel(d, pr.diagonal()) <= TOL_OP
    assert np.all(d[pr.mesh.constrained.astype(np.int64)] == 1.0)
    inv = op.compute_diagonal(invert=True).cpu().numpy()
    assert rel(inv, 1.0 / pr.diagonal()) <= TOL_OP


# ------------------------------------------------------------------ 4. no Dirichlet DoFs (BP1 has no boundary condition)
@pytest.mark.parametrize("p", [2, 4])
def test_no_dirichlet_dofs(p):
    torch = _t()
    cells = (3, 2, 2)
    pr, src, ref = _problem(p, "mass", dirichlet=False)
    op = _operator(p, "mass", dirichlet=False)
    assert pr.mesh.constrained.size == 0
    n = op.mf_data.n_local
    one = torch.ones(n, dtype=torch.float64, device="cuda:0")
    m1 = nan_vector(n)
    op.vmult(m1, one)
    assert rel(m1.cpu().numpy(), pr.vmult(np.ones(n))) <= TOL_OP
    # the volume: sum(M 1) = sum_q JxW, exact on the undeformed mesh (h = 1/2)
    flat = _operator(p, "mass", amp=0.0, dirichlet=False, h=0.5)
    v1 = nan_vector(n)
    flat.vmult(v1, one)
    volume = float(np.prod(cells)) * 0.125
    assert abs(float(v1.sum()) - volume) <= TOL_OP * volume
    u, mu = dev(src), nan_vector(n)
    op.vmult(mu, u)
    assert rel(mu.cpu().numpy(), ref) <= TOL_OP
    d = op.compute_diagonal().cpu().numpy()
    assert rel(d, pr.diagonal()) <= TOL_OP and d.min() > 0.0
    x = op.initialize_dof_vector()
    op.mf_data.copy_constrained_values(one, x)                              # nothing to copy: no launch, no change
    assert float(x.abs().max()) == 0.0
    # the Poisson operator without a boundary condition: constants are its null space
    lap = _operator(p, "poisson", dirichlet=False)
    z = nan_vector(n)
    lap.vmult(z, one)
    lu = nan_vector(n)
    lap.vmult(lu, u)
    assert float(z.abs().max()) <= 1e-12 * float(lu.abs().max())
    # projection returns its input: b = M u_f, Jacobi-CG to 1e-12 |b|
    X = pr.mesh.coords
    uf = (1.0 + X[:, 0] - 0.5 * X[:, 0] ** 2) * (0.3 + X[:, 1] ** 2) * (2.0 - X[:, 2] + 0.25 * X[:, 2] ** 2)
    b = op.initialize_dof_vector()
    op.vmult(b, dev(uf))
    tol = 1e-12 * float(torch.linalg.norm(b))
    for solver in (pkg.SolverCG, pkg.SolverCGFullMerge):
        x = op.initialize_dof_vector()
        ctl = pkg.IterationNumberControl(500, tol)
        solver(ctl).solve(op, x, b, pkg.DiagonalMatrix(op.compute_diagonal(invert=True)))
        e = rel(x.cpu().numpy(), uf)
        print(f"p={p} {solver.__name__}: {ctl.last_step()} iterations, |x - u_f| / |u_f| = {e:.2e}")
        assert ctl.last_step() < 500 and ctl.last_value() <= tol and e <= 1e-10


def test_rhs_and_l2_norm_keep_their_own_quadrature():
    """bp5_assemble_rhs and bp5_l2_norm_solution integrate with Gauss(p+1) by definition: the same numbers on handles of either quadrature"""
    mesh = pkg.BrickMesh(3, (3, 2, 2), deform_amp=AMP)
    a, b = pkg.PoissonOperator(mesh, OVER), pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS)
    ra, rb = a.assemble_rhs(), b.assemble_rhs()
    assert rel(ra.cpu().numpy(), rb.cpu().numpy()) <= 1e-14                # (atomic scatter: the same sums in another order)
    u = dev(O.deterministic_src(mesh.n_local, seed=4))
    la, lb = a.l2_norm_solution(u), b.l2_norm_solution(u)
    assert abs(la - lb) <= 1e-14 * lb and abs(la - O.l2_norm_solution(O.BrickMesh(3, (3, 2, 2), deform_amp=AMP), u.cpu().numpy())) <= 1e-13 * lb
    pr = O.Problem(3, (3, 2, 2), O.QUAD_GAUSS, deform_amp=AMP)
    assert rel(ra.cpu().numpy(), pr.rhs()) <= TOL_OP


# ------------------------------------------------------------------ 5. solvers
GPU_SOLVERS = {"plain": pkg.SolverCG, "merged": pkg.SolverCGFullMerge}
CASE_SETUP = {"config1": (2, (8, 8, 8), pkg.COEF_ONE, "poisson"), "step64": (4, (4, 4, 4), pkg.COEF_STEP64, "poisson"), "mass": (2, (4, 4, 4), pkg.COEF_STEP64, "mass")}


def _case_operator(case):
    p, cells, coefficient, cls = CASE_SETUP[case]
    return _operator(p, cls, cells=cells, coefficient=coefficient)


@pytest.mark.parametrize("solver", sorted(GPU_SOLVERS))
@pytest.mark.parametrize("case", sorted(CG_CASES))
def test_cg_at_a_fixed_iteration_count(case, solver):
    """config 1's geometry, deformed, no preconditioner; p = 4 with step-64's coefficient and the inverse diagonal; the mass operator at p = 2: ten
    iterations against O.cg_plain / O.cg_merged on the reference operator"""
    pr, b, inv = CG_CASES[case]()
    op = _case_operator(case)
    xr, k, res = cg_reference(case, solver)
    bg = op.assemble_rhs()
    assert rel(bg.cpu().numpy(), b) <= TOL_OP
    inv_g = None
    if inv is not None:
        inv_g = op.compute_diagonal(invert=True)
        assert rel(inv_g.cpu().numpy(), inv) <= TOL_OP
    x = nan_vector(op.mf_data.n_local)
    ctl = pkg.IterationNumberControl(CG_ITERATIONS, 0.0)
    GPU_SOLVERS[solver](ctl).solve(op, x, bg, pkg.DiagonalMatrix(inv_g))
    e = rel(x.cpu().numpy(), xr)
    print(f"{case} / {solver}: {e:.2e}, residual {ctl.last_value():.6e} (numpy {res:.6e}), kernel {ctl.apply_kernel}")
    assert ctl.last_step() == k == CG_ITERATIONS and e <= TOL_CG
    assert abs(ctl.last_value() - res) <= 1e-9 * res
    p, _, _, cls = CASE_SETUP[case]
    assert ctl.dot_products_fused == 0 and ctl.apply_kernel == KERNEL_LITERALS[p, cls]      # the merged solver runs its separate dot-product kernels


def _stop(A, b, inv, k_min=8, k_max=40):
    """the rule of _stop_tolerance (tests/test_gpu_multirank_loopback.py) with a preconditioner: the first iteration k >= k_min whose residual
    undercuts every earlier one by 8 %, and a tolerance half way (geometrically) between that residual and the lowest earlier one"""
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
    pr, b, inv = CG_CASES["step64"]()
    op = _case_operator("step64")
    k_stop, tol = _stop(pr.vmult, b, inv)
    _, k_ref, _ = SOLVERS[solver](pr.vmult, b, 100, tol=tol, diag=inv)
    bg, x = op.assemble_rhs(), op.initialize_dof_vector()
    ctl = pkg.IterationNumberControl(100, tol)
    GPU_SOLVERS[solver](ctl).solve(op, x, bg, pkg.DiagonalMatrix(op.compute_diagonal(invert=True)))
    true_res = np.linalg.norm(pr.vmult(x.cpu().numpy()) - b)
    print(f"{solver}: stop at {ctl.last_step()} (numpy {k_ref}, record low at {k_stop}), tolerance {tol:.3e}, recomputed residual {true_res:.3e}")
    assert ctl.last_step() == k_ref and (solver != "plain" or k_ref == k_stop)
    assert ctl.last_value() <= tol and true_res <= tol


def test_chebyshev_pcg_stops_where_numpy_does():
    """Chebyshev(2)-PCG through bp5_cg_solve_preconditioned: the iteration count of tests/chebyshev_ref.py on the reference operator"""
    pr, b, inv = CG_CASES["step64"]()
    op = _case_operator("step64")
    mesh = op.mf_data.mesh
    Cheb = pkg.PreconditionChebyshev
    ch = Cheb().initialize(op, Cheb.AdditionalData(degree=2, smoothing_range=20.0, preconditioner=pkg.DiagonalMatrix(op.compute_diagonal(invert=True))))
    lo, hi, _ = CR.lanczos_estimate(pr.vmult, inv, CR.start_vector(mesh.global_ids, mesh.constrained), 8)
    mu, Mu = CR.bounds(lo, hi, 20.0)
    e = ch.estimated_eigenvalues()
    assert abs(e["min_used"] - mu) <= 1e-10 * mu and abs(e["max_used"] - Mu) <= 1e-10 * Mu, (e, mu, Mu)
    P = lambda g: CR.vmult(pr.vmult, inv, g, mu, Mu, 2)
    res = [float(np.linalg.norm(b))] + [CR.pcg(pr.vmult, P, b, k)[2] for k in range(1, 21)]
    k_stop = next(k for k in range(4, 21) if res[k] < 0.92 * min(res[:k]))
    tol = float(np.sqrt(res[k_stop] * min(res[:k_stop])))
    xr, k_ref, _ = CR.pcg(pr.vmult, P, b, 100, tol=tol)
    x = op.initialize_dof_vector()
    ctl = pkg.IterationNumberControl(100, tol)
    pkg.SolverCG(ctl).solve(op, x, op.assemble_rhs(), ch)
    print(f"Chebyshev(2)-PCG: {ctl.last_step()} iterations (numpy {k_ref}), tolerance {tol:.3e}")
    assert ctl.last_step() == k_ref == k_stop and rel(x.cpu().numpy(), xr) <= TOL_CG


def test_cg_through_a_callback_operator():
    """bp5_cg_solve_operator: the solvers need nothing of A but vmult"""
    pr, b, inv = CG_CASES["step64"]()
    op = _case_operator("step64")

    class Wrapped:                                                           # not a PoissonOperator: solved through the callback entry point
        mf_data = op.mf_data

        def vmult(self, dst, src):
            op.vmult(dst, src)
    xr, k, _ = cg_reference("step64", "plain")
    x = nan_vector(op.mf_data.n_local)
    ctl = pkg.IterationNumberControl(CG_ITERATIONS, 0.0)
    pkg.SolverCG(ctl).solve(Wrapped(), x, op.assemble_rhs(), pkg.DiagonalMatrix(op.compute_diagonal(invert=True)))
    assert ctl.last_step() == k and rel(x.cpu().numpy(), xr) <= TOL_CG


# ------------------------------------------------------------------ 6. refusals
def _refused(fn):
    with pytest.raises(pkg.BP5Error) as e:
        fn()
    return e.value.status, str(e.value)


def test_refusals():
    """every refusal is BP5_ERR_UNSUPPORTED (5) with the word "quadrature", decided before any launch"""
    torch = _t()
    mesh = pkg.BrickMesh(2, (3, 2, 2))
    new = lambda m=mesh: pkg.MatrixFree().reinit(m, OVER, pkg.COEF_ONE)
    # the Helmholtz operator
    st, msg = _refused(lambda: new().set_operator(pkg.OP_HELMHOLTZ))
    assert st == 5 and "quadrature" in msg and "Helmholtz" in msg, msg
    st, msg = _refused(lambda: pkg.HelmholtzOperator(mesh, OVER))
    assert st == 5 and "quadrature" in msg, msg
    # hanging-node masks (part of the mesh: one call order)
    st, msg = _refused(lambda: new(namespace(O.HangingBrickMesh(2, 2, 2, 1, 3))))
    assert st == 5 and "quadrature" in msg and "hanging" in msg, msg
    for cls in (pkg.OP_POISSON, pkg.OP_MASS):                               # the rest in either order with set_operator
        def handle():
            mf = new()
            mf.set_operator(cls)
            return mf
        st, msg = _refused(lambda: handle().set_geometry_mode(pkg.GEOM_AFFINE))
        assert st == 5 and "quadrature" in msg and "affine" in msg, msg
        st, msg = _refused(lambda: handle().set_metric_precision("float32"))
        assert st == 5 and "quadrature" in msg and "FP32" in msg, msg
        for v in (1, 10, 50, 56, 70, 90, 110):
            mf = handle()
            st, msg = _refused(lambda: mf.set_apply_variant(v))
            assert st == 5 and "quadrature" in msg and "variant" in msg and mf.get_apply_variant() == 0, (v, st, msg)
        st, msg = _refused(lambda: handle().get_data())
        assert st == 5 and "quadrature" in msg, msg
    st, msg = _refused(lambda: pkg.PoissonOperator(mesh, OVER, geometry=pkg.GEOM_AFFINE))
    assert st == 5 and "quadrature" in msg, msg
    st, msg = _refused(lambda: pkg.PoissonOperator(mesh, OVER, metric_precision="float32"))
    assert st == 5 and "quadrature" in msg, msg
    # brick meshes where a p + 1 handle resolves to 56: variant 0 is the pencil kernel, 56 is refused
    bricks = pkg.BrickMesh(4, (8, 8, 8), cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1)
    mf = new(bricks)
    assert mf.get_apply_variant() == 0
    st, msg = _refused(lambda: mf.set_apply_variant(56))
    assert st == 5 and "quadrature" in msg, msg
    # block vectors, x untouched
    for cls in sorted(CLASSES):
        op = _operator(2, cls)
        x, b = op.initialize_block_vector(3), op.initialize_block_vector(3)
        b.fill_(1.0)
        x.fill_(7.0)
        st, msg = _refused(lambda: op.vmult(x, b))
        assert st == 5 and "quadrature" in msg, msg
        st, msg = _refused(lambda: pkg.SolverCG(pkg.IterationNumberControl(3, 0.0)).solve(op, x, b, pkg.DiagonalMatrix()))
        assert st == 5 and "quadrature" in msg, msg
        assert bool((x == 7.0).all())                                        # refused before any launch
    # a multigrid level
    st, msg = _refused(lambda: pkg.PreconditionMG([_operator(2, "poisson")]))
    assert st == 5 and "quadrature" in msg, msg
    # an unknown id stays an invalid argument
    st, msg = _refused(lambda: pkg.MatrixFree().reinit(mesh, 7, pkg.COEF_ONE))
    assert st == 1 and "quadrature" in msg, msg
    # the plane count is fixed once the array is sized: Poisson <-> mass
    mf = new()
    mf.coef_size()
    st, msg = _refused(lambda: mf.set_operator(pkg.OP_MASS))
    assert st == 1 and "plane count" in msg, msg
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 7. neighbours' bits
def test_other_handles_keep_their_bits():
    """a p + 1 Poisson handle's block-kernel vmult and a scalar SolverCG solve, bit for bit before and after over-integrated calls on another handle"""
    torch = _t()
    mesh = pkg.BrickMesh(4, (6, 5, 9), deform_amp=AMP, cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1)
    op = pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_STEP64)
    op.mf_data.set_apply_variant(56)
    s = dev(O.deterministic_src(mesh.n_local, seed=9))
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
    for cls in sorted(CLASSES):
        over = CLASSES[cls](mesh, OVER, pkg.COEF_STEP64)
        y = over.initialize_dof_vector()
        over.vmult(y, s)
        over.compute_diagonal()
        pkg.SolverCGFullMerge(pkg.IterationNumberControl(3, 0.0)).solve(over, over.initialize_dof_vector(), over.assemble_rhs(), pkg.DiagonalMatrix())
    after = run()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


# ------------------------------------------------------------------ 8. the example
def test_example_reproduces_the_python_solve():
    exe = os.path.join(bp5_pkg.ROOT, "examples", "bp5_bp3")
    assert os.path.exists(exe), "examples/bp5_bp3 missing: run __graft_entry__.build()"
    p, n, tol_rel, amp = 3, 4, 1e-10, 0.04
    out = subprocess.run([exe, str(p), str(n), repr(tol_rel), repr(amp)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    vals = dict(line.split("=", 1) for line in out.stdout.split() if "=" in line)
    mesh = pkg.BrickMesh(p, (n, n, n), h=1.0 / n, deform_amp=amp)
    op = pkg.PoissonOperator(mesh, OVER, pkg.COEF_ONE)
    b = op.assemble_rhs()
    x = op.initialize_dof_vector()
    ctl = pkg.IterationNumberControl(10000, tol_rel * float(_t().linalg.norm(b)))
    pkg.SolverCG(ctl).solve(op, x, b, pkg.DiagonalMatrix(op.compute_diagonal(invert=True)))
    l2 = op.l2_norm_solution(x)
    print(out.stdout.strip(), f"| python: iterations={ctl.last_step()} l2={l2:.12e}")
    assert int(vals["iterations"]) == ctl.last_step()
    assert abs(float(vals["l2_norm"]) - l2) <= 1e-10 * l2
    assert vals["apply_kernel"] == KERNEL_LITERALS[p, "poisson"]
