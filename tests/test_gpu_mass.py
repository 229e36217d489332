"""The mass operator on the GPU (BP5_OP_MASS, pkg.MassOperator; CEED BP1): the plane, the pencil kernel and the diagonal against the numpy
reference of tests/mass_ref.py (pinned outside itself by tests/test_mass_cpu.py), handles without Dirichlet DoFs through three independent
kernels of the library, both CG solvers and the Chebyshev-preconditioned one against their numpy statements, and every refusal.  The pencil kernel
scatters with atomics: results are compared to the project's tolerances (1e-13 operator, 1e-11 CG at a fixed count); the block kernel
(variant 56 on cell bricks) is deterministic: bitwise equal over repeated launches and solves."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import chebyshev_ref as CR
import mass_ref as M
from test_mass_cpu import BRICK_FREE, CG_CASES, CG_ITERATIONS, SOLVERS, brick_free_case, cg_reference

pytestmark = pytest.mark.gpu
pkg = bp5_pkg.load()
TOL_OP = 1e-13     # one operator application (rounding + atomic summation order)
TOL_CG = 1e-11     # CG solution vector at a fixed iteration count
AMP = 0.04
RHO = {pkg.COEF_ONE: O.kappa_none, pkg.COEF_STEP64: O.kappa_step64}
_cache = {}


def _t():
    import torch
    return torch


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def dev(a):
    return _t().from_numpy(np.array(a, dtype=np.float64)).to("cuda:0")


def _cells(p):
    return (3, 3, 2) if p <= 4 else (11, 1, 1)         # a partial last team at every degree (18 cells: 16 / 7 / 4 / 10 per team at p = 1 ... 4; 11 cells: 7 / 5 / 4 / 3 at p = 5 ... 8)


def namespace(m, constrained=None):
    """an oracle mesh as MatrixFree.reinit takes it (one rank, lexicographic); constrained: another Dirichlet set (empty: BP1)"""
    return SimpleNamespace(degree=m.p, n=m.n, n_cells=m.n_cells, n_interior_cells=m.n_cells, n_owned=m.n_dofs, n_ghost=0, n_local=m.n_dofs,
                           n_global_dofs=m.n_dofs, l2g=m.l2g, coords=m.coords, constrained=m.constrained if constrained is None else constrained,
                           n_neighbors=0, neighbor_rank=np.zeros(0, np.int32), send_offsets=np.zeros(1, np.uint32),
                           send_indices=np.zeros(0, np.uint32), recv_offsets=np.zeros(1, np.uint32), cell_block_offsets=None,
                           constraint_mask=getattr(m, "constraint_mask", None), rank=0, n_ranks=1, global_ids=np.arange(m.n_dofs, dtype=np.uint64))


def _problem(p, quad, cells=None, amp=AMP, coefficient=pkg.COEF_STEP64, dirichlet=True):
    """reference problem, a source (non-zero on the boundary) and M.vmult of it -- computed once, never changed"""
    cells = cells or _cells(p)
    key = (p, quad, cells, amp, coefficient, dirichlet)
    if key not in _cache:
        pr = M.Problem(p, cells, quad, deform_amp=amp, rho=RHO[coefficient], dirichlet=dirichlet)
        src = O.deterministic_src(pr.mesh.n_dofs, seed=60 + p)
        ref = pr.vmult(src)
        for a in (src, ref):
            a.setflags(write=False)
        _cache[key] = (pr, src, ref)
    return _cache[key]


def _operator(p, quad, cells=None, amp=AMP, coefficient=pkg.COEF_STEP64, dirichlet=True):
    cells = cells or _cells(p)
    key = ("op", p, quad, cells, amp, coefficient, dirichlet)
    if key not in _cache:
        mesh = pkg.BrickMesh(p, cells, deform_amp=amp) if dirichlet else namespace(O.BrickMesh(p, cells, deform_amp=amp), np.zeros(0, np.uint32))
        _cache[key] = pkg.MassOperator(mesh, quad, coefficient)
    return _cache[key]


def kernel_name(p, quad):
    tw, tpb = (1, 4) if p <= 3 else (4, 1)
    return "apply_pencil_mass_kernel<%d,%s,%d,%d,%d>" % (p, "true" if quad else "false", tw, (p + 1) ** 2, tpb)


# ------------------------------------------------------------------ 1. sizing and planes
@pytest.mark.parametrize("coefficient", [pkg.COEF_ONE, pkg.COEF_STEP64])
@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("p", [1, 2, 4, 5, 8])
def test_one_plane_rho_jxw(p, quad, coefficient):
    pr, _, _ = _problem(p, quad, coefficient=coefficient)
    op = _operator(p, quad, coefficient=coefficient)
    n_entries = pr.mesh.n_cells * (p + 1) ** 3
    assert op.mf_data.coef_size() == n_entries == op.coef.numel()
    got = op.mf_data.coef_reference_layout(op.coef).cpu().numpy().reshape(pr.mesh.n_cells, -1)
    e = rel(got, pr.S)
    print(f"p={p} quad={quad} coefficient={coefficient}: plane {e:.2e}")
    assert e <= TOL_OP


# ------------------------------------------------------------------ 2. pencil kernel
@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("p", range(1, 9))
def test_pencil_kernel_parity(p, quad):
    """overwrite mode on a NaN-filled dst, accumulate mode (zero_dst = 0) and bp5_apply_cells on a ragged sub-range, both on a non-zero dst"""
    torch = _t()
    pr, src, ref = _problem(p, quad)
    op = _operator(p, quad)
    mf = op.mf_data
    assert mf.get_apply_variant() == 0
    s = dev(src)
    d = torch.full((mf.n_local,), float("nan"), dtype=torch.float64, device="cuda:0")
    op.vmult(d, s)
    got = d.cpu().numpy()
    assert np.isfinite(got).all()
    e = rel(got, ref)
    print(f"p={p} quad={quad}: vmult {e:.2e}")
    assert e <= TOL_OP
    cst = pr.mesh.constrained.astype(np.int64)
    assert np.array_equal(got[cst], src[cst]) and torch.equal(s.cpu(), torch.from_numpy(np.array(src)))
    # dst += M src, then the Dirichlet copy
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
    # cells [c0, c1), neither end a multiple of the cells per team
    cpt = 64 * (1 if p <= 3 else 4) // (p + 1) ** 2
    assert pr.mesh.n_cells % cpt != 0                                       # the whole-range launches above ended in a partly filled team
    c0 = 1
    c1 = next(c for c in (pr.mesh.n_cells - 1, pr.mesh.n_cells - 2) if c % cpt)
    assert c0 % cpt and c1 % cpt and c1 - c0 >= 3
    d = dev(pre)
    mf.cell_loop(op.coef, s, d, c0, c1)
    want = pr.apply_cells(src, cell_range=(c0, c1), dst=pre.copy())
    assert rel(d.cpu().numpy(), want) <= TOL_OP
    # the kernel that ran
    ctl = pkg.IterationNumberControl(1, 0.0)
    pkg.SolverCG(ctl).solve(op, op.initialize_dof_vector(), dev(pr.rhs()), pkg.DiagonalMatrix())
    assert ctl.last_step() == 1 and ctl.apply_kernel == kernel_name(p, quad), ctl.apply_kernel


@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("p", [1, 8])
def test_one_cell(p, quad):
    """a single, partially filled team: every other cell slot idle"""
    pr, src, ref = _problem(p, quad, cells=(1, 1, 1))
    op = _operator(p, quad, cells=(1, 1, 1))
    d = op.initialize_dof_vector()                       # (every DoF of a one-cell mesh is a Dirichlet DoF: compare the cell loop itself)
    op.mf_data.cell_loop(op.coef, dev(src), d)
    assert rel(d.cpu().numpy(), pr.apply_cells(src)) <= TOL_OP


def launch_shape(p, n_cells):
    """(cells per team, teams, workgroups) of apply_pencil_mass_kernel as bp5_device.hpp launches it: the degree's default pencil shape"""
    tw, tpb = (1, 4) if p <= 3 else (4, 1)
    cpt = 64 * tw // (p + 1) ** 2
    teams = -(-n_cells // cpt)
    return cpt, teams, -(-teams // tpb)


# one mesh per barrier family: p = 2 wave-local team syncs (four one-wave teams per workgroup), p = 4 the workgroup barrier
MANY_WORKGROUPS = {2: ((8, 6, 5), 9), 4: ((9, 6, 4), 22)}


@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("p", sorted(MANY_WORKGROUPS))
def test_many_workgroups(p, quad):
    """the XCD remap with teams_per_xcd > 1, idle trailing workgroups and a partly filled last team"""
    cells, expected = MANY_WORKGROUPS[p]
    n_cells = cells[0] * cells[1] * cells[2]
    cpt, teams, workgroups = launch_shape(p, n_cells)
    assert workgroups == expected >= 9 and workgroups % 8 != 0 and n_cells % cpt != 0, (cpt, teams, workgroups)
    pr, src, ref = _problem(p, quad, cells=cells)
    op = _operator(p, quad, cells=cells)
    d = _t().full((op.mf_data.n_local,), float("nan"), dtype=_t().float64, device="cuda:0")
    op.vmult(d, dev(src))
    e = rel(d.cpu().numpy(), ref)
    print(f"p={p} quad={quad} cells={cells} workgroups={workgroups}: {e:.2e}")
    assert e <= TOL_OP


# ------------------------------------------------------------------ 3. block kernel (variant 56)
# degree -> (cells, cell block): the meshes of tests/test_gpu_kernel_selection.py (several bricks, partial bricks, block-major numbering)
BRICKS = {1: ((17, 9, 10), (8, 8, 8)), 2: ((9, 8, 5), (8, 8, 4)), 3: ((9, 5, 6), (8, 4, 4)), 4: ((9, 8, 6), (4, 4, 4)),
          5: ((7, 5, 3), (6, 4, 2)), 6: ((5, 4, 3), (4, 4, 2)), 7: ((5, 3, 3), (4, 2, 2)), 8: ((3, 3, 3), (2, 2, 2))}
# (degree, quadrature) -> (plain, fused): BLK_DEFAULT | BLK_MASS [| BLK_FUSE], overwrite launches (owner stores)
BLOCK_KERNEL = {
    (1, 0): ("apply_block_kernel<1,false,4,1,1074030592>", "apply_block_kernel<1,false,4,1,1075079168>"),
    (1, 1): ("apply_block_kernel<1,true,4,1,1074030592>", "apply_block_kernel<1,true,4,1,1075079168>"),
    (2, 0): ("apply_block_kernel<2,false,9,1,1074030592>", "apply_block_kernel<2,false,9,1,1075079168>"),
    (2, 1): ("apply_block_kernel<2,true,9,1,1074030592>", "apply_block_kernel<2,true,9,1,1075079168>"),
    (3, 0): ("apply_block_kernel<3,false,16,1,1074030592>", "apply_block_kernel<3,false,16,1,1075079168>"),
    (3, 1): ("apply_block_kernel<3,true,16,1,1074030592>", "apply_block_kernel<3,true,16,1,1075079168>"),
    (4, 0): ("apply_block_kernel<4,false,32,1,1074030592>", "apply_block_kernel<4,false,32,1,1075079168>"),
    (4, 1): ("apply_block_kernel<4,true,32,1,1074030592>", "apply_block_kernel<4,true,32,1,1075079168>"),
    (5, 0): ("apply_block_kernel<5,false,36,1,1074030592>", "apply_block_kernel<5,false,36,1,1075079168>"),
    (5, 1): ("apply_block_kernel<5,true,36,1,1074030592>", "apply_block_kernel<5,true,36,1,1075079168>"),
    (6, 0): ("apply_block_kernel<6,false,64,1,1074030592>", "apply_block_kernel<6,false,64,1,1075079168>"),
    (6, 1): ("apply_block_kernel<6,true,64,1,1074030592>", "apply_block_kernel<6,true,64,1,1075079168>"),
    (7, 0): ("apply_block_kernel<7,false,64,1,1074030592>", "apply_block_kernel<7,false,64,1,1075079168>"),
    (7, 1): ("apply_block_kernel<7,true,64,1,1074030592>", "apply_block_kernel<7,true,64,1,1075079168>"),
    (8, 0): ("apply_block_kernel<8,false,81,1,1074030592>", "apply_block_kernel<8,false,81,1,1075079168>"),
    (8, 1): ("apply_block_kernel<8,true,81,1,1074030592>", "apply_block_kernel<8,true,81,1,1075079168>"),
}


def _brick_case(p, quad):
    """(mesh, operator on variant 56 with eight workgroups, reference problem, permutation local -> lexicographic)"""
    key = ("brick", p, quad)
    if key not in _cache:
        cells, blk = BRICKS[p]
        mesh = pkg.BrickMesh(p, cells, h=0.2, deform_amp=0.03, cell_block=blk, dof_numbering=1, cell_block_order=1)
        op = pkg.MassOperator(mesh, quad, pkg.COEF_STEP64)
        op.mf_data.set_apply_variant(56)
        op.mf_data.set_block_workgroups(8)
        pr = M.Problem(p, cells, quad, h=0.2, deform_amp=0.03, rho=O.kappa_step64)
        _cache[key] = (mesh, op, pr, mesh.global_ids.astype(np.int64))
    return _cache[key]


@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("p", range(1, 9))
def test_block_kernel_parity(p, quad):
    """variant 56 against the reference and, entry by entry, against the same handle's pencil kernel; two launches bit for bit; a block-aligned
    cell range in accumulate mode"""
    torch = _t()
    mesh, op, pr, perm = _brick_case(p, quad)
    mf = op.mf_data
    assert mf.get_apply_variant() == 56 and mf.block_plan_info()[2]
    src_lex = O.deterministic_src(pr.mesh.n_dofs, seed=70 + p)
    s = dev(src_lex[perm])
    ref = pr.vmult(src_lex)[perm]
    d = torch.full((mf.n_local,), float("nan"), dtype=torch.float64, device="cuda:0")
    op.vmult(d, s)
    e = rel(d.cpu().numpy(), ref)
    d2 = torch.full((mf.n_local,), float("nan"), dtype=torch.float64, device="cuda:0")
    op.vmult(d2, s)
    assert torch.equal(d, d2)
    mf.set_apply_variant(0)
    try:
        assert mf.get_apply_variant() == 0                                    # (too few bricks for the persistent grid: the library's own choice is the pencil kernel)
        dp = torch.full((mf.n_local,), float("nan"), dtype=torch.float64, device="cuda:0")
        op.vmult(dp, s)
    finally:
        mf.set_apply_variant(56)
    entrywise = float((d - dp).abs().max()) / float(dp.abs().max())
    print(f"p={p} quad={quad}: block kernel vs reference {e:.2e}, vs pencil kernel (max entry) {entrywise:.2e}")
    assert e <= TOL_OP and entrywise <= 1e-13
    # cells of the blocks [1, 3) on a non-zero dst
    off = mesh.cell_block_offsets
    c0, c1 = int(off[1]), int(off[3])
    pre = np.random.default_rng(6).uniform(-1, 1, mf.n_local)
    da = dev(pre)
    mf.cell_loop(op.coef, s, da, c0, c1)
    cell_lex = _lexicographic_cells(mesh, pr.mesh)
    want = np.zeros(pr.mesh.n_dofs)
    for c in cell_lex[c0:c1]:
        pr.apply_cells(src_lex, cell_range=(int(c), int(c) + 1), dst=want)
    assert rel(da.cpu().numpy(), pre + want[perm]) <= TOL_OP


def _lexicographic_cells(mesh, ref_mesh):
    """per cell of the brick-ordered mesh, its index in the reference's lexicographic cell order (matched through the DoF of local index 0)"""
    first = {int(g): c for c, g in enumerate(ref_mesh.l2g[:, 0])}
    gid = mesh.global_ids.astype(np.int64)
    return np.array([first[int(gid[int(l)])] for l in mesh.l2g[:, 0]])


@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("p", range(1, 9))
def test_block_kernel_names_and_fused_dot_products(p, quad):
    """SolverCGFullMerge fused, SolverCG fused, SolverCG with fusion off; lattice-capable bricks and streaming on resolve to the same packed
    builds (the optional bits are dropped, not refused); every solve against the pencil kernel's"""
    mesh, op, pr, perm = _brick_case(p, quad)
    mf = op.mf_data
    plain, fused = BLOCK_KERNEL[p, quad]
    b = op.assemble_rhs()
    inv = None
    nb, _, packed = mf.block_plan_info()
    assert packed and mf.block_plan_lattice() == nb                          # every block a lattice block: the request carries BLK_LATT | BLK_CARRY
    mf.set_apply_variant(0)
    ref = {}
    for solver in (pkg.SolverCGFullMerge, pkg.SolverCG):
        x, ctl = op.initialize_dof_vector(), pkg.IterationNumberControl(2, 0.0)
        solver(ctl).solve(op, x, b, pkg.DiagonalMatrix(inv))
        assert ctl.apply_kernel == kernel_name(p, quad) and not ctl.dot_products_fused
        ref[solver] = x
    mf.set_apply_variant(56)
    try:
        for solver, fusion, want_fused in ((pkg.SolverCGFullMerge, 1, 1), (pkg.SolverCG, 1, 1), (pkg.SolverCG, 0, 0)):
            mf.set_cg_fusion(fusion)
            for streaming in (0, 1):
                mf.set_streaming(streaming)
                x, ctl = op.initialize_dof_vector(), pkg.IterationNumberControl(2, 0.0)
                solver(ctl).solve(op, x, b, pkg.DiagonalMatrix(inv))
                where = (p, quad, solver.__name__, fusion, streaming)
                assert ctl.last_step() == 2 and ctl.apply_kernel == (fused if want_fused else plain), (where, ctl.apply_kernel)
                assert ctl.dot_products_fused == bool(want_fused), where
                assert float((x - ref[solver]).abs().max()) < 1e-12 * float(ref[solver].abs().max()), where
    finally:
        mf.set_cg_fusion(1)
        mf.set_streaming(-1)


# ------------------------------------------------------------------ 4. no Dirichlet DoFs (BP1 has no boundary condition)
@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("p", [2, 4])
def test_no_dirichlet_dofs(p, quad):
    """three independent kernels of the library agree: the operator, assemble_rhs (row sums) and l2_norm_solution (the energy)"""
    torch = _t()
    pr, src, ref = _problem(p, quad, coefficient=pkg.COEF_ONE, dirichlet=False)
    op = _operator(p, quad, coefficient=pkg.COEF_ONE, dirichlet=False)
    assert pr.mesh.constrained.size == 0
    n = op.mf_data.n_local
    one = torch.ones(n, dtype=torch.float64, device="cuda:0")
    m1 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
    op.vmult(m1, one)
    # the volume: sum(M 1) = sum_q JxW, exact on the undeformed mesh (h = 1/2)
    flat = pkg.MassOperator(namespace(O.BrickMesh(p, _cells(p), h=0.5), np.zeros(0, np.uint32)), quad, pkg.COEF_ONE)
    v1 = flat.initialize_dof_vector()
    flat.vmult(v1, one)
    volume = float(np.prod(_cells(p))) * 0.125
    assert abs(float(v1.sum()) - volume) <= TOL_OP * volume
    assert rel(m1.cpu().numpy(), pr.vmult(np.ones(n))) <= TOL_OP
    if quad == 0:                                                           # (assemble_rhs and the L2 norm integrate with Gauss(p+1), whatever the handle's quadrature)
        assert rel(m1.cpu().numpy(), op.assemble_rhs().cpu().numpy()) <= TOL_OP
        u, mu = dev(src), op.initialize_dof_vector()
        op.vmult(mu, u)
        energy, l2 = float(u @ mu), op.l2_norm_solution(u) ** 2
        assert abs(energy - l2) <= TOL_OP * l2
    d = op.compute_diagonal().cpu().numpy()
    assert rel(d, pr.diagonal()) <= TOL_OP and d.min() > 0.0
    x = op.initialize_dof_vector()
    op.mf_data.copy_constrained_values(one, x)                              # nothing to copy: no launch, no change
    assert float(x.abs().max()) == 0.0


def test_projection_returns_the_polynomial():
    """b = M u_f for nodal values u_f of a polynomial of degree <= p per variable; Jacobi-CG to 1e-12 |b| returns u_f to 1e-10"""
    p = 2
    pr, _, _ = _problem(p, 0, coefficient=pkg.COEF_ONE, dirichlet=False)
    op = _operator(p, 0, coefficient=pkg.COEF_ONE, dirichlet=False)
    X = pr.mesh.coords
    uf = (1.0 + X[:, 0] - 0.5 * X[:, 0] ** 2) * (0.3 + X[:, 1] ** 2) * (2.0 - X[:, 2] + 0.25 * X[:, 2] ** 2)
    b = op.initialize_dof_vector()
    op.vmult(b, dev(uf))
    assert rel(b.cpu().numpy(), pr.vmult(uf)) <= TOL_OP
    tol = 1e-12 * float(_t().linalg.norm(b))
    for solver in (pkg.SolverCG, pkg.SolverCGFullMerge):
        x = op.initialize_dof_vector()
        ctl = pkg.IterationNumberControl(500, tol)
        solver(ctl).solve(op, x, b, pkg.DiagonalMatrix(op.compute_diagonal(invert=True)))
        e = rel(x.cpu().numpy(), uf)
        print(f"{solver.__name__}: {ctl.last_step()} iterations, |x - u_f| / |u_f| = {e:.2e}")
        assert ctl.last_step() < 500 and ctl.last_value() <= tol and e <= 1e-10


def _without_dirichlet(mesh):
    """a library mesh (cell bricks, block-major numbering, global_ids) with an empty constrained set: views of its arrays"""
    free = SimpleNamespace(**{k: v for k, v in vars(mesh).items() if k != "_h"})
    free.constrained = np.zeros(0, np.uint32)
    free.keep = mesh
    return free


def _brick_free(p, quad, h=0.2, amp=0.03):
    """(mesh, mass operator with rho = 1 on variant 56 and eight workgroups, reference, permutation) on the bricks of BRICKS, no Dirichlet DoFs"""
    key = ("brick_free", p, quad, h, amp)
    if key not in _cache:
        cells, blk = BRICKS[p]
        mesh = pkg.BrickMesh(p, cells, h=h, deform_amp=amp, cell_block=blk, dof_numbering=1, cell_block_order=1)
        op = pkg.MassOperator(_without_dirichlet(mesh), quad, pkg.COEF_ONE)
        op.mf_data.set_apply_variant(56)
        op.mf_data.set_block_workgroups(8)
        pr = M.Problem(p, cells, quad, h=h, deform_amp=amp, dirichlet=False)
        _cache[key] = (mesh, op, pr, mesh.global_ids.astype(np.int64))
    return _cache[key]


@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("p", [2, 4])
def test_no_dirichlet_dofs_on_the_block_kernel(p, quad):
    """the same three agreements with the BLK_MASS build: run tables without a Dirichlet flag, owner stores and combine pass with nothing to copy"""
    torch = _t()
    mesh, op, pr, perm = _brick_free(p, quad)
    mf = op.mf_data
    assert pr.mesh.constrained.size == 0 and mf.get_apply_variant() == 56
    n = mf.n_local
    one = torch.ones(n, dtype=torch.float64, device="cuda:0")
    m1 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
    op.vmult(m1, one)
    assert rel(m1.cpu().numpy(), pr.vmult(np.ones(n))[perm]) <= TOL_OP
    _, flat, _, _ = _brick_free(p, quad, h=0.5, amp=0.0)                     # the volume: sum(M 1) = sum_q JxW, exact on the undeformed mesh
    v1 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
    flat.vmult(v1, one)
    volume = float(np.prod(BRICKS[p][0])) * 0.125
    assert abs(float(v1.sum()) - volume) <= TOL_OP * volume
    src_lex = O.deterministic_src(pr.mesh.n_dofs, seed=90 + p)
    u, mu = dev(src_lex[perm]), torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
    op.vmult(mu, u)
    assert rel(mu.cpu().numpy(), pr.vmult(src_lex)[perm]) <= TOL_OP
    if quad == 0:
        assert rel(m1.cpu().numpy(), op.assemble_rhs().cpu().numpy()) <= TOL_OP
        energy, l2 = float(u @ mu), op.l2_norm_solution(u) ** 2
        assert abs(energy - l2) <= TOL_OP * l2
    # the kernel that ran, plain and fused
    for solver, name in ((pkg.SolverCGFullMerge, BLOCK_KERNEL[p, quad][1]), (pkg.SolverCG, BLOCK_KERNEL[p, quad][1])):
        ctl = pkg.IterationNumberControl(1, 0.0)
        solver(ctl).solve(op, op.initialize_dof_vector(), mu, pkg.DiagonalMatrix())
        assert ctl.apply_kernel == name and ctl.dot_products_fused
    mf.set_cg_fusion(0)
    try:
        ctl = pkg.IterationNumberControl(1, 0.0)
        pkg.SolverCG(ctl).solve(op, op.initialize_dof_vector(), mu, pkg.DiagonalMatrix())
        assert ctl.apply_kernel == BLOCK_KERNEL[p, quad][0] and not ctl.dot_products_fused
    finally:
        mf.set_cg_fusion(1)


@pytest.mark.parametrize("solver", sorted(SOLVERS))
def test_fused_cg_without_dirichlet_dofs(solver):
    """ten unpreconditioned iterations on the block kernel with the dot products fused into its write-out, against numpy; the same bits run to run;
    and the projection: Jacobi-CG (plain solver: d.h from the kernel) to 1e-12 |b| returns the vector b was made from"""
    torch = _t()
    p, cells, h, amp = BRICK_FREE
    pr, b, _ = brick_free_case()
    mesh, op, _, perm = _brick_free(p, 0, h=h, amp=amp)
    gpu_solver = {"plain": pkg.SolverCG, "merged": pkg.SolverCGFullMerge}[solver]
    xr, k, res = SOLVERS[solver](pr.vmult, b, CG_ITERATIONS)
    bg = dev(b[perm])
    xs = []
    for _ in range(2):
        x = torch.full((op.mf_data.n_local,), float("nan"), dtype=torch.float64, device="cuda:0")
        ctl = pkg.IterationNumberControl(CG_ITERATIONS, 0.0)
        gpu_solver(ctl).solve(op, x, bg, pkg.DiagonalMatrix())
        assert ctl.last_step() == k == CG_ITERATIONS and ctl.dot_products_fused == 1 and ctl.apply_kernel == BLOCK_KERNEL[p, 0][1], ctl.apply_kernel
        assert abs(ctl.last_value() - res) <= 1e-9 * res
        xs.append(x.clone())
    e = rel(xs[0].cpu().numpy(), xr[perm])
    print(f"no Dirichlet DoFs, block kernel, fused / {solver}: {e:.2e}")
    assert e <= TOL_CG and torch.equal(xs[0], xs[1])
    if solver == "plain":
        u_f = O.deterministic_src(pr.mesh.n_dofs, seed=81)
        x = op.initialize_dof_vector()
        ctl = pkg.IterationNumberControl(500, 1e-12 * float(torch.linalg.norm(bg)))
        pkg.SolverCG(ctl).solve(op, x, bg, pkg.DiagonalMatrix(op.compute_diagonal(invert=True)))
        assert ctl.last_step() < 500 and ctl.dot_products_fused == 1 and rel(x.cpu().numpy(), u_f[perm]) <= 1e-10


# ------------------------------------------------------------------ 5. diagonal
@pytest.mark.parametrize("p", range(1, 9))
def test_diagonal(p):
    pr, _, _ = _problem(p, 0)
    op = _operator(p, 0)
    d = op.compute_diagonal().cpu().numpy()
    assert rel(d, pr.diagonal()) <= TOL_OP
    assert np.all(d[pr.mesh.constrained.astype(np.int64)] == 1.0)
    inv = op.compute_diagonal(invert=True).cpu().numpy()
    assert rel(inv, 1.0 / pr.diagonal()) <= TOL_OP


@pytest.mark.parametrize("p", [1, 2, 4, 5, 8])
def test_collocated_operator_is_its_diagonal(p):
    pr, src, ref = _problem(p, 1)
    op = _operator(p, 1)
    d = op.compute_diagonal()
    assert rel(d.cpu().numpy(), pr.diagonal()) <= TOL_OP
    y = op.initialize_dof_vector()
    s = dev(src)
    op.vmult(y, s)
    free = np.ones(pr.mesh.n_dofs, bool)
    free[pr.mesh.constrained.astype(np.int64)] = False
    assert rel(y.cpu().numpy()[free], (d * s).cpu().numpy()[free]) <= 1e-14


# ------------------------------------------------------------------ 6. solvers
GPU_SOLVERS = {"plain": pkg.SolverCG, "merged": pkg.SolverCGFullMerge}


def _case_operator(case):
    key = ("case", case)
    if key not in _cache:
        pr, b, inv = CG_CASES[case]()
        p, cells, amp, coefficient = {"config1": (2, (8, 8, 8), 0.0, pkg.COEF_ONE), "step64": (4, (4, 4, 4), 0.05, pkg.COEF_STEP64)}[case]
        _cache[key] = pkg.MassOperator(pkg.BrickMesh(p, cells, deform_amp=amp), 0, coefficient)
    return _cache[key]


@pytest.mark.parametrize("solver", sorted(GPU_SOLVERS))
@pytest.mark.parametrize("case", sorted(CG_CASES))
def test_cg_at_a_fixed_iteration_count(case, solver):
    """config 1 with rho = 1 and no preconditioner, p = 4 deformed with step-64's rho and the inverse diagonal: ten iterations against numpy"""
    pr, b, inv = CG_CASES[case]()
    op = _case_operator(case)
    xr, k, res = cg_reference(case, solver)
    bg = op.assemble_rhs()
    assert rel(bg.cpu().numpy(), b) <= TOL_OP
    inv_g = None
    if inv is not None:
        inv_g = op.compute_diagonal(invert=True)
        assert rel(inv_g.cpu().numpy(), inv) <= TOL_OP
    x = _t().full((op.mf_data.n_local,), float("nan"), dtype=_t().float64, device="cuda:0")
    ctl = pkg.IterationNumberControl(CG_ITERATIONS, 0.0)
    GPU_SOLVERS[solver](ctl).solve(op, x, bg, pkg.DiagonalMatrix(inv_g))
    e = rel(x.cpu().numpy(), xr)
    print(f"{case} / {solver}: {e:.2e}, residual {ctl.last_value():.6e} (numpy {res:.6e}), kernel {ctl.apply_kernel}")
    assert ctl.last_step() == k == CG_ITERATIONS and e <= TOL_CG
    assert abs(ctl.last_value() - res) <= 1e-9 * res
    assert ctl.dot_products_fused == 0 and ctl.apply_kernel.startswith("apply_pencil_mass_kernel<")   # lexicographic cells: the pencil kernel, separate dot products


@pytest.mark.parametrize("solver", sorted(GPU_SOLVERS))
def test_cg_on_the_block_kernel_fuses_its_dot_products_and_is_reproducible(solver):
    """config 1 on 4x4x4 bricks, variant 56: ten iterations against numpy, the dot products inside the kernel's write-out, the same bits run to run"""
    torch = _t()
    pr, b, _ = CG_CASES["config1"]()
    xr, k, res = cg_reference("config1", solver)
    mesh = pkg.BrickMesh(2, (8, 8, 8), cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1)
    op = pkg.MassOperator(mesh, 0, pkg.COEF_ONE)
    op.mf_data.set_apply_variant(56)
    perm = mesh.global_ids.astype(np.int64)
    bg = op.assemble_rhs()
    assert rel(bg.cpu().numpy(), b[perm]) <= TOL_OP
    xs = []
    for _ in range(2):
        x = torch.full((op.mf_data.n_local,), float("nan"), dtype=torch.float64, device="cuda:0")
        ctl = pkg.IterationNumberControl(CG_ITERATIONS, 0.0)
        GPU_SOLVERS[solver](ctl).solve(op, x, bg, pkg.DiagonalMatrix())
        assert ctl.last_step() == k and ctl.dot_products_fused == 1 and ctl.apply_kernel == BLOCK_KERNEL[2, 0][1], ctl.apply_kernel
        assert abs(ctl.last_value() - res) <= 1e-9 * res
        xs.append(x.clone())
    e = rel(xs[0].cpu().numpy(), xr[perm])
    print(f"config1 on bricks / {solver}: {e:.2e}")
    assert e <= TOL_CG and torch.equal(xs[0], xs[1])


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


def test_collocated_jacobi_cg_is_exact_after_one_iteration():
    """GLL collocation: the operator is diagonal, so Jacobi-CG has converged after one iteration (further ones would divide 0 by 0)"""
    pr, _, _ = _problem(4, 1)
    op = _operator(4, 1)
    b = op.assemble_rhs()
    inv = op.compute_diagonal(invert=True)
    want = (b * inv).cpu().numpy()
    for solver in GPU_SOLVERS.values():
        x = op.initialize_dof_vector()
        ctl = pkg.IterationNumberControl(1, 0.0)
        solver(ctl).solve(op, x, b, pkg.DiagonalMatrix(inv))
        assert ctl.last_step() == 1 and rel(x.cpu().numpy(), want) <= 1e-14
        x = op.initialize_dof_vector()
        ctl = pkg.IterationNumberControl(50, 1e-8 * float(_t().linalg.norm(b)))
        solver(ctl).solve(op, x, b, pkg.DiagonalMatrix(inv))
        assert ctl.last_step() == 1 and rel(x.cpu().numpy(), want) <= 1e-14


def test_check_every_does_not_change_the_bits():
    """on two cells no DoF has more than two contributions, so the atomic scatter is order-independent and the solve reproducible bit by bit"""
    torch = _t()
    op = pkg.MassOperator(namespace(O.BrickMesh(2, (2, 1, 1), deform_amp=0.0), np.zeros(0, np.uint32)), 0, pkg.COEF_STEP64)
    b = op.assemble_rhs()
    inv = op.compute_diagonal(invert=True)
    xs = []
    for check_every in (0, 1, 0):
        x = op.initialize_dof_vector()
        ctl = pkg.IterationNumberControl(6, 0.0)
        pkg.SolverCG(ctl, check_every=check_every).solve(op, x, b, pkg.DiagonalMatrix(inv))
        assert ctl.last_step() == 6
        xs.append(x.clone())
    assert torch.equal(xs[0], xs[1]) and torch.equal(xs[0], xs[2])


@pytest.mark.parametrize("solver", sorted(GPU_SOLVERS))
def test_cg_edges(solver):
    """max_iter = 0 leaves x = 0 and reports |b|; b = 0 stops at once with x = 0"""
    torch = _t()
    op = _case_operator("config1")
    b = op.assemble_rhs()
    x = torch.full((op.mf_data.n_local,), 3.0, dtype=torch.float64, device="cuda:0")
    ctl = pkg.IterationNumberControl(0, 0.0)
    GPU_SOLVERS[solver](ctl).solve(op, x, b, pkg.DiagonalMatrix())
    assert ctl.last_step() == 0 and float(x.abs().max()) == 0.0 and abs(ctl.last_value() - float(torch.linalg.norm(b))) <= 1e-14 * ctl.last_value()
    x = torch.full((op.mf_data.n_local,), 3.0, dtype=torch.float64, device="cuda:0")
    ctl = pkg.IterationNumberControl(5, 0.0)
    GPU_SOLVERS[solver](ctl).solve(op, x, torch.zeros_like(b), pkg.DiagonalMatrix())
    assert ctl.last_step() == 0 and float(x.abs().max()) == 0.0 and ctl.last_value() == 0.0


def test_chebyshev_pcg_stops_where_numpy_does():
    """Chebyshev(2)-PCG through bp5_cg_solve_preconditioned on a mass handle: the iteration count of tests/chebyshev_ref.py on the reference operator"""
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


# ------------------------------------------------------------------ 7. refusals
def _refused(fn):
    with pytest.raises(pkg.BP5Error) as e:
        fn()
    return e.value.status, str(e.value)


def test_refusals():
    mesh = pkg.BrickMesh(2, (3, 2, 2))
    new = lambda m=mesh: pkg.MatrixFree().reinit(m, 0, pkg.COEF_ONE)
    # hanging-node masks (part of the mesh: one call order)
    st, msg = _refused(lambda: new(namespace(O.HangingBrickMesh(2, 2, 2, 1, 3))).set_operator(pkg.OP_MASS))
    assert st == 5 and "hanging" in msg, msg
    # affine geometry, either order
    mf = new()
    mf.set_geometry_mode(pkg.GEOM_AFFINE)
    st, msg = _refused(lambda: mf.set_operator(pkg.OP_MASS))
    assert st == 5 and "affine" in msg, msg
    mf = new()
    mf.set_operator(pkg.OP_MASS)
    st, msg = _refused(lambda: mf.set_geometry_mode(pkg.GEOM_AFFINE))
    assert st == 5 and "affine" in msg and "mass" in msg, msg
    # FP32 planes, either order
    mf = new()
    mf.set_metric_precision("float32")
    st, msg = _refused(lambda: mf.set_operator(pkg.OP_MASS))
    assert st == 5 and "FP32" in msg, msg
    mf = new()
    mf.set_operator(pkg.OP_MASS)
    st, msg = _refused(lambda: mf.set_metric_precision("float32"))
    assert st == 5 and "FP32" in msg and "mass" in msg, msg
    # apply variants, either order
    for v in (1, 10, 50, 70, 110):
        mf = new()
        mf.set_operator(pkg.OP_MASS)
        st, msg = _refused(lambda: mf.set_apply_variant(v))
        assert st == 5 and "mass" in msg and mf.get_apply_variant() == 0, (v, st, msg)
    mf = new()
    mf.set_apply_variant(56)
    mf.set_operator(pkg.OP_MASS)                                            # 56 and the mass operator go together, in either order
    mf = new()
    mf.set_operator(pkg.OP_MASS)
    mf.set_apply_variant(56)
    mf = new()
    mf.set_apply_variant(10)
    st, msg = _refused(lambda: mf.set_operator(pkg.OP_MASS))
    assert st == 5 and "variant" in msg, msg
    # the plane count is fixed once the array is sized or filled: every direction between 1, 6 and 7 planes
    for first, others in ((pkg.OP_MASS, (pkg.OP_POISSON, pkg.OP_HELMHOLTZ)), (pkg.OP_POISSON, (pkg.OP_MASS,)), (pkg.OP_HELMHOLTZ, (pkg.OP_MASS,))):
        for sized_by in ("coef_size", "evaluate_coefficients"):
            mf = new()
            mf.set_operator(first)
            getattr(mf, sized_by)()
            for other in others:
                st, msg = _refused(lambda: mf.set_operator(other))
                assert st == 1 and "plane count" in msg, (first, other, msg)
            mf.set_operator(first)                                          # the same operator again is no change
    # an unknown operator
    st, msg = _refused(lambda: new().set_operator(3))
    assert st == 1 and "unknown operator" in msg, msg


def test_block_vectors_are_refused_by_name():
    op = _operator(2, 0)
    x, b = op.initialize_block_vector(3), op.initialize_block_vector(3)
    b.fill_(1.0)
    st, msg = _refused(lambda: op.vmult(x, b))
    assert st == 5 and "mass operator" in msg, msg
    st, msg = _refused(lambda: pkg.SolverCG(pkg.IterationNumberControl(3, 0.0)).solve(op, x, b, pkg.DiagonalMatrix()))
    assert st == 5 and "mass operator" in msg, msg
    assert float(x.abs().max()) == 0.0                                      # refused before any launch


# ------------------------------------------------------------------ 8. neighbours' bits
def test_other_handles_keep_their_bits():
    """a Poisson and a Helmholtz handle created before mass calls on the same device and used after them: the block kernel's vmult bit for bit"""
    torch = _t()
    mesh = pkg.BrickMesh(4, (6, 5, 9), deform_amp=AMP, cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1)
    ops = [pkg.PoissonOperator(mesh, 0, pkg.COEF_STEP64), pkg.HelmholtzOperator(mesh, 0, pkg.COEF_STEP64)]
    s = dev(O.deterministic_src(mesh.n_local, seed=9))
    before = []
    for op in ops:
        op.mf_data.set_apply_variant(56)
        d = op.initialize_dof_vector()
        op.vmult(d, s)
        before.append(d.clone())
    mop = pkg.MassOperator(mesh, 0, pkg.COEF_STEP64)
    y = mop.initialize_dof_vector()
    mop.vmult(y, s)
    mop.compute_diagonal()
    mop.mf_data.set_apply_variant(56)                                       # ... and the mass build of the block kernel
    y56 = mop.initialize_dof_vector()
    mop.vmult(y56, s)
    assert float((y56 - y).abs().max()) <= 1e-13 * float(y.abs().max())
    pkg.SolverCGFullMerge(pkg.IterationNumberControl(3, 0.0)).solve(mop, mop.initialize_dof_vector(), mop.assemble_rhs(), pkg.DiagonalMatrix())
    for op, want in zip(ops, before):
        d = op.initialize_dof_vector()
        op.vmult(d, s)
        assert torch.equal(d, want)
    # ... and the mass handle on this brick-numbered mesh against the reference through the permutation
    pr = M.Problem(4, (6, 5, 9), deform_amp=AMP, rho=O.kappa_step64)
    perm = mesh.global_ids.astype(np.int64)
    full = np.zeros(mesh.n_local)
    full[perm] = s.cpu().numpy()                                            # local i == lexicographic perm[i]
    assert rel(y.cpu().numpy(), pr.vmult(full)[perm]) <= TOL_OP


# ------------------------------------------------------------------ 9. the example
def test_example_reproduces_the_python_solve():
    exe = os.path.join(bp5_pkg.ROOT, "examples", "bp5_bp1")
    assert os.path.exists(exe), "examples/bp5_bp1 missing: run __graft_entry__.build()"
    p, n, tol_rel = 3, 4, 1e-10
    out = subprocess.run([exe, str(p), str(n), repr(tol_rel)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    vals = dict(line.split("=", 1) for line in out.stdout.split() if "=" in line)
    mesh = pkg.BrickMesh(p, (n, n, n), h=1.0 / n)
    op = pkg.MassOperator(mesh, 0, pkg.COEF_ONE)
    X = _t().from_numpy(np.array(mesh.coords)).to("cuda:0")
    f = _t().sin(np.pi * X[:, 0]) * _t().sin(np.pi * X[:, 1]) * _t().sin(np.pi * X[:, 2]) * _t().exp(X[:, 0] * X[:, 1] - X[:, 2])
    b = op.initialize_dof_vector()
    op.vmult(b, f)
    op.mf_data.set_constrained_values(0.0, b)
    x = op.initialize_dof_vector()
    ctl = pkg.IterationNumberControl(1000, tol_rel * float(_t().linalg.norm(b)))
    pkg.SolverCG(ctl).solve(op, x, b, pkg.DiagonalMatrix(op.compute_diagonal(invert=True)))
    l2 = op.l2_norm_solution(x)
    print(out.stdout.strip(), f"| python: iterations={ctl.last_step()} l2={l2:.12e}")
    assert int(vals["iterations"]) == ctl.last_step()
    assert abs(float(vals["l2_norm"]) - l2) <= 1e-10 * l2
