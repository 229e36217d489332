"""Accumulate mode (dst += A src) of every operator kernel build against the oracle.

Every operator entry point has two contracts for dst: overwrite (dst = A src, prior content ignored) and accumulate (dst += A src:
bp5_apply(..., zero_dst = 0), bp5_apply_cells, MatrixFree.cell_loop, vmult with do_zero_out = False).  The accumulate contract runs device
code of its own -- the SC_OWNER_ADD / SC_OWNER_ADD_ATOMIC instantiations of the team and block kernels, a read-modify-write owner write-out,
an adding combine pass -- for every degree, quadrature and operator class.  Each test here does the same thing: a small mesh, a seeded source,
the plain reference A_cells src from the oracle function of the operator class, a prefill `pre` of dst, ONE accumulate call through the public
interface, and a comparison with pre + A_cells src (the Dirichlet copy on top for vmult / bp5_apply).

Prefill: sign * U(0.5, 1) * max|A_cells src| with a seed of its own, ghost entries included -- every entry is detectably non-zero, so one entry
that was stored instead of added (or added twice) moves the result by at least 0.5 max|A src|.  Metric: max|got - want| <= TOL_OP max|want|
per case (the operator tolerance of tests/test_gpu_parity.py; the one extra addition costs a few ulp), no NaN, and for block kernels without
atomics two runs from the same prefill are the same bits.  Every case prints its error; DESIGN.md 4a records the largest one measured."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
from test_gpu_f32_metric import _local, _planes
from test_gpu_parity import TOL_CG, TOL_OP, _refined, _with_cell_blocks

pytestmark = pytest.mark.gpu
pkg = bp5_pkg.load()
PREFILL_SEED = 20240607
WORST = {"err": 0.0, "case": ""}      # largest error of the cases run so far (printed with every case)

# ------------------------------------------------------------------ the tables
# A. default pencil kernel (variant 0, default numbering): the meshes of test_cell_loop_all_degrees
PENCIL = [(p, quad) for p in range(1, 9) for quad in (0, 1)]
# B. cell-interior DoFs numbered first (dof_numbering = 2): (p, cells, cell block, slab) -- the meshes of
# test_cell_interior_dofs_numbered_first_are_stored_plainly; p = 3 is the control (the team kernel runs there); the last one has ghost entries
INTERIOR_FIRST = [(5, (4, 3, 5), (2, 2, 2), {}), (6, (3, 4, 3), (0, 0, 0), {}), (7, (3, 2, 3), (2, 2, 2), {}), (8, (3, 3, 2), (0, 0, 0), {}),
                  (8, (4, 4, 4), (2, 2, 2), {}), (3, (4, 3, 3), (0, 0, 0), {}), (5, (4, 3, 5), (2, 2, 2), dict(rank=1, n_ranks=2))]
# C. team kernel: (p, variant, quad) on the meshes of test_kernel_variants
TEAM = ([(p, 10, 0) for p in range(1, 9)] + [(p, 10, 1) for p in (2, 4, 7)] + [(4, v, 0) for v in (11, 12, 13, 110)])
TEAM_WAVES = {10: 4, 11: 8, 12: 4, 13: 2, 110: 4}          # waves per team (bp5_device.hpp: TEAM_CASE)
# D. block kernel: degree -> [(cells, cell block)], the brick meshes of test_native_helmholtz_operator_block_kernel (full and partial bricks)
BRICKS = {1: [((17, 9, 10), (8, 8, 8))], 2: [((9, 8, 5), (8, 8, 4))], 3: [((9, 5, 6), (8, 4, 4))], 4: [((9, 8, 6), (4, 4, 4)), ((6, 5, 5), (4, 4, 2))],
          5: [((7, 5, 3), (6, 4, 2))], 6: [((5, 4, 3), (4, 4, 2))], 7: [((5, 3, 3), (4, 2, 2))], 8: [((3, 3, 3), (2, 2, 2))]}
BLOCK = [(p, k, quad) for p in range(1, 9) for k in range(len(BRICKS[p])) for quad in (0, 1)]
P4_SIBLINGS = [50, 55, 52, 57]
# E. the other operator classes
HELMHOLTZ_PENCIL = [(2, 0, (4, 3, 3), 0.03), (4, 0, (3, 2, 2), 0.04), (6, 1, (2, 2, 2), 0.03)]      # of test_native_helmholtz_operator_pencil_kernel
HELMHOLTZ_BLOCK = [(p, quad) for p in (1, 3, 4, 5, 8) for quad in (0, 1)]
HANGING = [(kind, p) for kind in ("stairs", "L", "core") for p in (1, 2, 3, 4)]
HANGING_GROUP = {"stairs": 3, "L": 2, "core": 3}             # cells per group, as test_hanging_nodes_in_the_deterministic_block_kernel
AFFINE_PENCIL = [2, 5, 8]
AFFINE_P4 = [(10, (0, 0, 0), 0), (50, (4, 4, 4), 1), (51, (4, 4, 2), 0), (54, (4, 4, 4), 1), (55, (4, 4, 4), 0), (56, (4, 4, 4), 1)]   # of test_affine_mode_team_and_block_kernels
F32_PENCIL = [3, 8]
F32_BLOCK = {4: ((9, 8, 6), (4, 4, 4)), 5: ((5, 6, 3), (4, 4, 2))}                                 # of tests/test_gpu_f32_metric.py
MARCH = [(1, (3, 2, 40), 70), (2, (5, 3, 6), 70), (3, (4, 3, 5), 70), (4, (7, 3, 5), 70), (4, (3, 3, 4), 71)]   # of test_march_kernel


# ------------------------------------------------------------------ plumbing
def _t():
    import torch
    return torch


def dev(x):
    return _t().from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _reference(cls, p, cells, quad, h, amp, seed):
    """(oracle problem, source, A_cells source) in the oracle's numbering, computed once per mesh and shared (read-only)"""
    pr = O.Problem(p, cells, quad, h=h, deform_amp=amp, kappa=O.kappa_none if cls == "helmholtz" else O.kappa_step64)
    s = O.deterministic_src(pr.mesh.n_dofs, seed=seed)
    if cls == "helmholtz":
        ref = O.apply_helmholtz_cells(pr.mesh, pr.N, pr.D, pr.w, s)
    else:
        ref = O.apply_cells(pr.mesh, pr.coef, pr.N, pr.D, s)
    return (pr,) + _frozen(s, ref)


def _on_mesh(mesh, cls, quad, seed):
    """source, reference and Dirichlet rows in the numbering of a single-rank library mesh"""
    pr, s, ref = _reference(cls, mesh.degree, mesh.cells, quad, mesh.h, mesh.deform_amp, seed)
    perm = mesh.global_ids.astype(np.int64)
    assert perm.size == pr.mesh.n_dofs
    c = np.asarray(mesh.constrained).astype(np.int64)
    assert np.array_equal(np.sort(perm[c]), np.sort(pr.mesh.constrained.astype(np.int64)))
    return s[perm], ref[perm], c


def _on_slab(mesh, quad, seed):
    """... of a slab with ghost entries: the oracle's metric and cell loop on the slab's own cells, coordinates and local_to_global"""
    lm = SimpleNamespace(p=mesh.degree, n=mesh.n, n_cells=mesh.n_cells, n_dofs=mesh.n_local, l2g=np.asarray(mesh.l2g), coords=np.asarray(mesh.coords))
    _, _, w, N, D = O.shape_tables(mesh.degree, quad)
    s = O.deterministic_src(mesh.n_local, seed=seed)
    ref = O.apply_cells(lm, O.merged_metric(lm, N, D, w, O.kappa_step64), N, D, s)
    return s, ref, np.asarray(mesh.constrained).astype(np.int64)


def _prefill(ref):
    rng = np.random.default_rng(PREFILL_SEED)
    return rng.choice([-1.0, 1.0], ref.size) * rng.uniform(0.5, 1.0, ref.size) * np.abs(ref).max()


def _accumulate_and_check(op_or_mf, call, src, ref, constrained=None, interior=0, bitwise=False, label=""):
    """dst = pre; call(dst, src on the device) -- ONE accumulate-mode application, possibly in several cell ranges --; dst against pre + ref
    (constrained: the rows of the Dirichlet copy that vmult / bp5_apply make on top).  interior: the first `interior` entries are checked on their
    own first (cell-interior DoFs numbered first).  bitwise: a second run from the same prefill must give the same bits.  Returns dst."""
    torch = _t()
    mf = getattr(op_or_mf, "mf_data", op_or_mf)
    assert src.size == ref.size == mf.n_local
    pre = _prefill(ref)
    want = pre + ref
    if constrained is not None:
        want[constrained] = src[constrained]
    scale = np.abs(want).max()
    s_dev = dev(src)
    dst = dev(pre)
    call(dst, s_dev)
    got = dst.cpu().numpy()
    err = np.abs(got - want).max() / scale
    if err > WORST["err"]:
        WORST["err"], WORST["case"] = float(err), label
    print(f"add mode {label}: max |got - want| / max |want| = {err:.2e}   (largest so far {WORST['err']:.2e}: {WORST['case']})")
    assert not np.isnan(got).any(), label
    if interior:
        err_interior = np.abs(got[:interior] - want[:interior]).max() / scale
        assert err_interior <= TOL_OP, f"{label}: cell-interior entries hold something else than pre + A src ({err_interior:.2e}: stored, not added?)"
    assert err <= TOL_OP, (label, err)
    if bitwise:
        again = dev(pre)
        call(again, s_dev)
        assert torch.equal(dst, again), f"{label}: two runs from the same prefill differ"
    return dst


def _vmult_add(op):
    def call(dst, src):
        op.do_zero_out = False
        try:
            op.vmult(dst, src)
        finally:
            op.do_zero_out = True
    return call


def _cell_ranges(op, edges):
    """cell_loop over [edges[0], edges[1]), [edges[1], edges[2]), ... one after the other onto the same dst"""
    def call(dst, src):
        for a, b in zip(edges[:-1], edges[1:]):
            op.mf_data.cell_loop(op.coef, src, dst, int(a), int(b))
    return call


def _brick_mesh(p, cells, block, **kw):
    return pkg.BrickMesh(p, cells, h=0.2, deform_amp=0.03, cell_block=block, dof_numbering=1, cell_block_order=1, **kw)


def _block_operator(cls, mesh, quad, lattice=None):
    if cls == "helmholtz":
        op = pkg.HelmholtzOperator(mesh, quad, pkg.COEF_STEP64)
    else:
        op = pkg.PoissonOperator(mesh, quad, pkg.COEF_STEP64, **({"metric_precision": "float32"} if cls == "f32" else {}))
    mf = op.mf_data
    if lattice is not None:
        mf.set_tuning("lattice_indices", lattice)
    mf.set_apply_variant(56)
    mf.set_block_workgroups(8)
    n_blocks, _, packed = mf.block_plan_info()
    assert packed and n_blocks >= 4                       # (eight workgroups: several bricks each on the meshes with more than eight)
    assert mf.block_plan_carry()[1] > 0                   # DoFs shared between bricks: the partial slab and the (adding) combine pass are live
    return op


def _block_whole_and_ranges(op, mesh, src, ref, c, label):
    """the two launches of the block kernel: the whole range (owner add + combine add; no atomics: bitwise reproducible) and brick-aligned
    sub-ranges one after the other (owner add, the DoFs shared across a range boundary by atomics)"""
    _accumulate_and_check(op, _vmult_add(op), src, ref, c, bitwise=True, label=label + " whole")
    _block_ranges(op, mesh, src, ref, label)


def _block_ranges(op, mesh, src, ref, label):
    off = [int(x) for x in mesh.cell_block_offsets]
    edges = [0, off[1], off[len(off) // 2], off[-2], mesh.n_cells]
    assert edges == sorted(set(edges)) and len(edges) == 5
    _accumulate_and_check(op, _cell_ranges(op, edges), src, ref, label=label + " brick ranges")


# ------------------------------------------------------------------ A. default pencil kernel
@pytest.mark.parametrize("p,quad", PENCIL)
def test_pencil_kernel(p, quad):
    mesh = pkg.BrickMesh(p, (3, 3, 2) if p <= 4 else (3, 2, 1), deform_amp=0.04)
    op = pkg.PoissonOperator(mesh, quad, pkg.COEF_STEP64)
    s, ref, c = _on_mesh(mesh, "poisson", quad, seed=3)
    assert op.mf_data.get_apply_variant() == (10 if p in (1, 3) else 0)
    _accumulate_and_check(op, _vmult_add(op), s, ref, c, label=f"variant 0 p={p} quad={quad}")
    if p in (1, 3):                                    # (0 resolves to the team kernel there: the pencil kernel of the degree by its own number)
        op.mf_data.set_apply_variant(1)
        _accumulate_and_check(op, _vmult_add(op), s, ref, c, label=f"pencil p={p} quad={quad}")


# ------------------------------------------------------------------ B. cell-interior DoFs numbered first
@pytest.mark.parametrize("p,cells,block,kw", INTERIOR_FIRST)
def test_interior_stores_build_is_not_taken_on_a_prefilled_dst(p, cells, block, kw):
    """The PEN_INTERIOR_STORES build of the default pencil kernel (p >= 5, dof_numbering = 2) writes the (p-1)^3 entries a cell owns alone with
    plain stores: right on a zeroed dst (what the solvers hand it), wrong on the caller's own content.  An accumulate call must therefore take the
    atomics; the entries 0 ... n_cells (p-1)^3 - 1 are checked on their own so that a failure names the defect.  Knob on and off."""
    blocked = all(b > 0 for b in block)
    mesh = pkg.BrickMesh(p, cells, h=0.25, deform_amp=0.03, cell_block=block, dof_numbering=2, cell_block_order=1 if blocked else 0, **kw)
    per = (p - 1) ** 3
    inner = np.asarray(mesh.l2g).reshape(mesh.n_cells, p + 1, p + 1, p + 1)[:, 1:p, 1:p, 1:p].reshape(mesh.n_cells, per)
    assert np.array_equal(inner, np.arange(mesh.n_cells * per, dtype=np.int64).reshape(mesh.n_cells, per))
    op = pkg.PoissonOperator(mesh, 0, pkg.COEF_STEP64)
    assert op.mf_data.get_apply_variant() == (10 if p == 3 else 0)
    if kw:
        assert mesh.n_ghost > 0
        s, ref, c = _on_slab(mesh, 0, seed=3)
    else:
        s, ref, c = _on_mesh(mesh, "poisson", 0, seed=3)
    k = mesh.n_cells // 2 + 1
    assert 0 < k < mesh.n_cells
    for knob in (0, 1):                                   # (off first: the plain pencil kernel is the control of the build under test)
        op.mf_data.set_tuning("interior_stores", knob)
        where = f"interior first p={p} {cells} {'slab ' if kw else ''}knob={knob}"
        _accumulate_and_check(op, _vmult_add(op), s, ref, c, interior=mesh.n_cells * per, label=where + " vmult")
        _accumulate_and_check(op, _cell_ranges(op, [0, mesh.n_cells]), s, ref, interior=mesh.n_cells * per, label=where + " cell_loop")
        _accumulate_and_check(op, _cell_ranges(op, [0, k, mesh.n_cells]), s, ref, interior=mesh.n_cells * per, label=where + f" cell_loop split at {k}")


# ------------------------------------------------------------------ C. team kernel
@pytest.mark.parametrize("p,variant,quad", TEAM)
def test_team_kernel(p, variant, quad):
    """whole range: the SC_OWNER_ADD build and an adding combine pass (variant 110: atomics); two ranges split inside a team: the atomic build
    with masked cells"""
    mesh = pkg.BrickMesh(p, (7, 3, 1) if p <= 5 else (5, 1, 1), deform_amp=0.03)
    op = pkg.PoissonOperator(mesh, quad, pkg.COEF_STEP64)
    op.mf_data.set_apply_variant(variant)
    s, ref, c = _on_mesh(mesh, "poisson", quad, seed=5)
    where = f"team variant={variant} p={p} quad={quad}"
    _accumulate_and_check(op, _vmult_add(op), s, ref, c, label=where + " whole")
    cells_per_team = 64 * TEAM_WAVES[variant] // (p + 1) ** 2
    k = next(k for k in range(mesh.n_cells // 2, mesh.n_cells) if k % cells_per_team)
    assert 0 < k < mesh.n_cells and k % cells_per_team != 0
    _accumulate_and_check(op, _cell_ranges(op, [0, k, mesh.n_cells]), s, ref, label=where + f" split at {k}")


# ------------------------------------------------------------------ D. block kernel
@pytest.mark.parametrize("p,k,quad", BLOCK)
def test_block_kernel(p, k, quad):
    cells, block = BRICKS[p][k]
    mesh = _brick_mesh(p, cells, block)
    op = _block_operator("poisson", mesh, quad)
    s, ref, c = _on_mesh(mesh, "poisson", quad, seed=61)
    _block_whole_and_ranges(op, mesh, s, ref, c, f"block p={p} {cells} quad={quad}")


@pytest.mark.parametrize("carry", [0, 1])
def test_block_kernel_p4_face_carry(carry):
    """the face carry of the p = 4 lattice build in accumulate mode: the carried faces skip the partial slab, the combine pass of that launch walks
    shorter tables (mesh of test_face_carry_keeps_shared_faces_in_lds_and_changes_no_bit_of_v: two bricks per workgroup)"""
    mesh = _brick_mesh(4, (13, 8, 6), (4, 4, 4))
    op = _block_operator("poisson", mesh, 0)
    mf = op.mf_data
    mf.set_tuning("face_carry", carry)
    faces, n_shared, _ = mf.block_plan_carry()
    assert faces > 0 and n_shared > 0 and mf.block_plan_lattice() == mf.block_plan_info()[0]
    s, ref, c = _on_mesh(mesh, "poisson", 0, seed=61)
    _accumulate_and_check(op, _vmult_add(op), s, ref, c, bitwise=True, label=f"block p=4 carry={carry} whole")
    in_tables = mf.block_plan_carry()[2]                 # of the last block launch: the accumulate one
    assert in_tables < n_shared if carry else in_tables == n_shared
    _block_ranges(op, mesh, s, ref, f"block p=4 carry={carry}")


@pytest.mark.parametrize("lattice", [1, 0])
def test_block_kernel_p4_lattice_and_packed_indices(lattice):
    cells, block = BRICKS[4][0]
    mesh = _brick_mesh(4, cells, block)
    op = _block_operator("poisson", mesh, 0, lattice=lattice)
    n_blocks = op.mf_data.block_plan_info()[0]
    assert op.mf_data.block_plan_lattice() == (n_blocks if lattice else 0)
    s, ref, c = _on_mesh(mesh, "poisson", 0, seed=61)
    _block_whole_and_ranges(op, mesh, s, ref, c, f"block p=4 lattice={lattice}")


@pytest.mark.parametrize("variant", P4_SIBLINGS)
def test_block_kernel_p4_other_shapes(variant):
    """25 / 32 lanes per cell, list write-out, brick-surface DoFs by atomics (55): whole range only (their cell ranges take the team kernel)"""
    cells, block = BRICKS[4][0]
    mesh = _brick_mesh(4, cells, block)
    op = _block_operator("poisson", mesh, 0)
    op.mf_data.set_apply_variant(variant)
    s, ref, c = _on_mesh(mesh, "poisson", 0, seed=61)
    _accumulate_and_check(op, _vmult_add(op), s, ref, c, bitwise=variant != 55, label=f"block variant={variant} p=4")


# ------------------------------------------------------------------ E. the other operator classes
@pytest.mark.parametrize("p,quad,cells,amp", HELMHOLTZ_PENCIL)
def test_helmholtz_pencil_kernel(p, quad, cells, amp):
    mesh = pkg.BrickMesh(p, cells, h=0.25, deform_amp=amp)
    op = pkg.HelmholtzOperator(mesh, quad, pkg.COEF_STEP64)
    assert op.mf_data.get_apply_variant() == 0
    s, ref, c = _on_mesh(mesh, "helmholtz", quad, seed=81)
    _accumulate_and_check(op, _vmult_add(op), s, ref, c, label=f"helmholtz pencil p={p} quad={quad}")
    _accumulate_and_check(op, _cell_ranges(op, [0, 1, mesh.n_cells]), s, ref, label=f"helmholtz pencil p={p} quad={quad} ranges")


@pytest.mark.parametrize("p,quad", HELMHOLTZ_BLOCK)
def test_helmholtz_block_kernel(p, quad):
    cells, block = BRICKS[p][0]
    mesh = _brick_mesh(p, cells, block)
    op = _block_operator("helmholtz", mesh, quad)
    s, ref, c = _on_mesh(mesh, "helmholtz", quad, seed=82)
    _block_whole_and_ranges(op, mesh, s, ref, c, f"helmholtz block p={p} quad={quad}")


@pytest.mark.parametrize("kind,p", HANGING)
def test_hanging_nodes(kind, p):
    """2:1 meshes handed over in cell groups with block-major numbering: the atomic pencil kernel (variant 90) and the block kernel (56) on one
    handle; reference: the oracle's cell loop, which resolves the hanging nodes (O.resolve_hanging) after the gather and before the scatter"""
    m = _refined(kind, p, 0.03)
    assert (m.constraint_mask != 0).any()
    _, _, w, N, D = O.shape_tables(p, 0)
    s_old = O.deterministic_src(m.n_dofs, seed=73)
    ref_old = O.apply_cells(m, O.merged_metric(m, N, D, w, O.kappa_step64), N, D, s_old)
    ns, new_of_old = _with_cell_blocks(m, HANGING_GROUP[kind])
    s, ref = np.empty_like(s_old), np.empty_like(ref_old)
    s[new_of_old], ref[new_of_old] = s_old, ref_old
    c = np.asarray(ns.constrained).astype(np.int64)
    op = pkg.PoissonOperator(ns, 0, pkg.COEF_STEP64)
    mf = op.mf_data
    mf.set_block_workgroups(8)
    mf.set_apply_variant(90)
    _accumulate_and_check(op, _vmult_add(op), s, ref, c, label=f"hanging {kind} p={p} pencil")
    _accumulate_and_check(op, _cell_ranges(op, [0, 3, m.n_cells]), s, ref, label=f"hanging {kind} p={p} pencil ranges")
    mf.set_apply_variant(56)
    assert mf.block_plan_info()[2] and mf.block_plan_carry()[1] > 0
    _accumulate_and_check(op, _vmult_add(op), s, ref, c, bitwise=True, label=f"hanging {kind} p={p} block whole")
    off = [int(x) for x in ns.cell_block_offsets]
    edges = sorted({0, off[1], off[len(off) // 2], m.n_cells})
    assert len(edges) >= 3
    _accumulate_and_check(op, _cell_ranges(op, edges), s, ref, label=f"hanging {kind} p={p} block group ranges")


@pytest.mark.parametrize("p", AFFINE_PENCIL)
def test_affine_pencil_kernel(p):
    mesh = pkg.BrickMesh(p, (3, 3, 2) if p <= 4 else (3, 2, 1), h=0.5)
    op = pkg.PoissonOperator(mesh, 0, pkg.COEF_STEP64, geometry=pkg.GEOM_AFFINE)
    s, ref, c = _on_mesh(mesh, "poisson", 0, seed=17)
    _accumulate_and_check(op, _vmult_add(op), s, ref, c, label=f"affine pencil p={p}")


@pytest.mark.parametrize("variant,block,numbering", AFFINE_P4)
def test_affine_team_and_block_kernels(variant, block, numbering):
    mesh = pkg.BrickMesh(4, (8, 5, 4), h=0.25, cell_block=block, dof_numbering=numbering)
    op = pkg.PoissonOperator(mesh, 0, pkg.COEF_STEP64, geometry=pkg.GEOM_AFFINE)
    op.mf_data.set_apply_variant(variant)
    if variant == 56:
        assert op.mf_data.block_plan_info()[2] and op.mf_data.block_plan_carry()[1] > 0
    s, ref, c = _on_mesh(mesh, "poisson", 0, seed=19)
    _accumulate_and_check(op, _vmult_add(op), s, ref, c, bitwise=variant in (50, 51, 56), label=f"affine variant={variant} p=4")


def _f32_reference(op, mesh, quad, seed):
    _, _, _, N, D = O.shape_tables(mesh.degree, quad)
    s = O.deterministic_src(mesh.n_local, seed=seed)
    return s, O.apply_cells(_local(mesh), _planes(op), N, D, s), np.asarray(mesh.constrained).astype(np.int64)     # the planes read back: widened floats


@pytest.mark.parametrize("p", F32_PENCIL)
def test_f32_metric_pencil_kernel(p):
    mesh = pkg.BrickMesh(p, (3, 3, 2) if p <= 4 else (3, 2, 1), deform_amp=0.04)
    op = pkg.PoissonOperator(mesh, 0, pkg.COEF_STEP64, metric_precision="float32")
    s, ref, c = _f32_reference(op, mesh, 0, seed=61)
    _accumulate_and_check(op, _vmult_add(op), s, ref, c, label=f"f32 metric pencil p={p}")
    _accumulate_and_check(op, _cell_ranges(op, [0, 2, mesh.n_cells]), s, ref, label=f"f32 metric pencil p={p} ranges")


@pytest.mark.parametrize("p", sorted(F32_BLOCK))
def test_f32_metric_block_kernel(p):
    cells, block = F32_BLOCK[p]
    mesh = _brick_mesh(p, cells, block)
    op = _block_operator("f32", mesh, 0)
    s, ref, c = _f32_reference(op, mesh, 0, seed=61)
    _block_whole_and_ranges(op, mesh, s, ref, c, f"f32 metric block p={p}")


@pytest.mark.parametrize("p,cells,variant", MARCH)
@pytest.mark.parametrize("quad", [0, 1])
def test_march_kernel(p, cells, variant, quad):
    numbering, block = (1, (2, 2, 2)) if p == 3 else (0, (0, 0, 0))
    mesh = pkg.BrickMesh(p, cells, deform_amp=0.03, cell_block=block, dof_numbering=numbering)
    op = pkg.PoissonOperator(mesh, quad, pkg.COEF_STEP64)
    op.mf_data.set_apply_variant(variant)
    s, ref, c = _on_mesh(mesh, "poisson", quad, seed=23)
    _accumulate_and_check(op, _vmult_add(op), s, ref, c, label=f"march variant={variant} p={p} quad={quad}")


# ------------------------------------------------------------------ F. what the plumbing gives for free
def _handles():
    """(label, operator, mesh, a cell index a range may end at, block kernel?): one handle per scatter family"""
    out = []
    mesh = pkg.BrickMesh(6, (3, 2, 1), deform_amp=0.04)
    out.append(("pencil p=6", pkg.PoissonOperator(mesh, 0, pkg.COEF_STEP64), mesh, 2, False))
    mesh = pkg.BrickMesh(5, (4, 3, 5), h=0.25, deform_amp=0.03, cell_block=(2, 2, 2), dof_numbering=2, cell_block_order=1)
    out.append(("interior first p=5", pkg.PoissonOperator(mesh, 0, pkg.COEF_STEP64), mesh, 7, False))
    mesh = pkg.BrickMesh(4, (7, 3, 1), deform_amp=0.03)
    op = pkg.PoissonOperator(mesh, 0, pkg.COEF_STEP64)
    op.mf_data.set_apply_variant(10)
    out.append(("team p=4", op, mesh, 7, False))
    mesh = _brick_mesh(4, *BRICKS[4][0])
    out.append(("block p=4", _block_operator("poisson", mesh, 0), mesh, int(mesh.cell_block_offsets[3]), True))
    return out


def test_the_empty_range_changes_no_bit():
    torch = _t()
    for label, op, mesh, k, _ in _handles():
        s, ref, _c = _on_mesh(mesh, "poisson", 0, seed=11)
        pre = dev(_prefill(ref))
        dst = pre.clone()
        for c in (0, k, mesh.n_cells):
            op.mf_data.cell_loop(op.coef, dev(s), dst, c, c)
        assert torch.equal(dst, pre), label


def test_no_add_or_set_state_leaks_between_accumulate_calls_and_solves():
    """accumulate, a three-iteration merged solve (overwrite mode, dst zeroed by the solver: the interior-stores build where the mesh has it),
    accumulate again on the same handle: the same accumulate result (bitwise without atomics), and the solve of a fresh handle"""
    torch = _t()
    for (label, op, mesh, _, deterministic), (_, fresh, _, _, _) in zip(_handles(), _handles()):
        s, ref, c = _on_mesh(mesh, "poisson", 0, seed=11)
        first = _accumulate_and_check(op, _vmult_add(op), s, ref, c, bitwise=deterministic, label=f"{label} before the solve")
        xs, b = [], op.assemble_rhs()                      # (one right-hand side for both: its assembly scatters with atomics)
        for o in (op, fresh):
            x, ctl = o.initialize_dof_vector(), pkg.IterationNumberControl(3, 0.0)
            pkg.SolverCGFullMerge(ctl).solve(o, x, b, pkg.DiagonalMatrix())
            xs.append(x)
            assert ctl.apply_kernel.endswith(",32>") == label.startswith("interior first"), (label, ctl.apply_kernel)
        second = _accumulate_and_check(op, _vmult_add(op), s, ref, c, label=f"{label} after the solve")
        if deterministic:                                  # the block kernel: no atomics in the operator, the dot products fused into it
            assert torch.equal(first, second) and torch.equal(xs[0], xs[1]), label
        else:
            assert float((xs[0] - xs[1]).abs().max()) <= TOL_CG * float(xs[1].abs().max()), label


@pytest.mark.parametrize("p,cells,kw", [(5, (4, 3, 5), dict(cell_block=(2, 2, 2), dof_numbering=2, cell_block_order=1, rank=1, n_ranks=2)),
                                        (4, (8, 8, 12), dict(cell_block=(4, 4, 2), dof_numbering=1, cell_block_order=1, rank=1, n_ranks=2)),
                                        (4, (5, 4, 7), dict(rank=2, n_ranks=3))])
def test_slab_meshes_leave_no_entry_untouched(p, cells, kw):
    """Why no test here runs the zero-fill + ADD branch that an overwrite call takes on a plan that does not cover every entry: the ghost entries
    of a slab ARE the entries its own cells touch beyond the owned ones, so every plan of a generated mesh covers all"""
    mesh = pkg.BrickMesh(p, cells, deform_amp=0.03, **kw)
    assert mesh.n_ghost > 0
    assert np.bincount(np.asarray(mesh.l2g).ravel().astype(np.int64), minlength=mesh.n_local).min() > 0
