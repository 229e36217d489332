"""The block kernel's plan recognisers (get_plan_raw: detect_lattice_blocks, find / mark_carry_faces, interior_runs_cover; bp5_mf_create:
cell interiors first) on hand-altered user meshes, one case per decision.

Every other GPU test feeds either the library's generator (every block a lattice block) or a mesh that fails every recogniser at once.  The
meshes here (tests/user_mesh.py, pinned on the CPU by tests/test_user_mesh_cpu.py) sit in between.  Rules of every case:
  * the reference is the oracle run on the altered arrays themselves;
  * the operator at TOL_OP = 1e-13 (relative l2) with dst pre-filled with NaN, at variant 56 with 2 and 8 workgroups (the same bits run to
    run) and at variant 0, and entry by entry against the atomic pencil kernel of the same handle;
  * a second handle with lattice_indices = 0 gives the bits of the first;
  * CG (SolverCGFullMerge and SolverCG, 8 iterations) against O.cg_plain on the altered mesh at TOL_CG = 1e-11 where the case says so;
  * EACH CASE ASSERTS ITS PLAN FACTS (lattice blocks, BLK_LATT in the kernel id, carried faces, the fused-update build): without them a case
    could pass through the generic path and test nothing.
Base mesh: p = 4, 8 x 8 x 8 cells in eight 4 x 4 x 4 bricks (35 937 DoFs); cases A, B, D, E, F also at p = 1, 2, 7, 8 (MESHES)."""
import functools

import numpy as np
import pytest
import torch

import bp5_oracle as O
import bp5_pkg
import components_ref as CoR
import mass_ref as M
import user_mesh as U
from test_gpu_stream_ordering import bits

pytestmark = pytest.mark.gpu
pkg = bp5_pkg.load()
TOL_OP, TOL_CG = 1e-13, 1e-11
LATT, UPD = 16777216, 131072                 # bp5_kernels.hpp: BLK_LATT, BLK_UPD
NAN = float("nan")
MESHES = {4: ((8, 8, 8), (4, 4, 4)), 1: ((8, 8, 8), (4, 4, 4)), 2: ((8, 8, 4), (4, 4, 2)), 7: ((4, 2, 2), (2, 2, 2)), 8: ((4, 2, 2), (2, 2, 2))}
DEGREES = [4, 1, 2, 7, 8]


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


@functools.lru_cache(maxsize=None)
def generator_mesh(p):
    cells, block = MESHES[p]
    return pkg.BrickMesh(p, cells, h=0.2, deform_amp=0.03, cell_block=block, dof_numbering=1, cell_block_order=1)


def start(p):
    return U.UserMesh.from_generator(generator_mesh(p))


def atomic_variant(p):
    return 1 if p in (1, 3) else 3 if p == 4 else 0          # the pencil / team kernel that scatters with atomics (test_lattice_blocks_need_no_index_stream)


def operator(ns, lattice=1):
    op = pkg.PoissonOperator(ns, 0, pkg.COEF_STEP64)
    op.mf_data.set_tuning("lattice_indices", lattice)
    op.mf_data.set_apply_variant(56)
    return op


def apply(op, src, variant=56, wgs=8):
    op.mf_data.set_apply_variant(variant)
    op.mf_data.set_block_workgroups(wgs)
    d = op.initialize_dof_vector()
    d.fill_(NAN)
    op.vmult(d, src)
    return d


def kernel_name(op, solver=pkg.SolverCGFullMerge, its=2):
    """the operator kernel of a short solve at variant 56 (the id of the build is its last template argument)"""
    op.mf_data.set_apply_variant(56)
    ctl = pkg.IterationNumberControl(its, 0.0)
    solver(ctl).solve(op, op.initialize_dof_vector(), op.assemble_rhs(), pkg.DiagonalMatrix())
    return ctl.apply_kernel


def check_operator(um, extra_variants=(), cg=0, rhs_and_diagonal=False, seed=3):
    """the rules of the module docstring on one altered mesh; returns (operator at variant 56, reference, source on the device, result at 8 workgroups)"""
    p = um.p
    ns, ref = um.namespace(), U.Reference(um)
    s = O.deterministic_src(um.n_dofs, seed=seed)              # non-zero on the Dirichlet DoFs too
    want = ref.vmult(s)
    src = dev(s)
    op = operator(ns)
    out = {}
    for wgs in (2, 8):
        out[wgs] = apply(op, src, 56, wgs)
        assert rel(out[wgs].cpu().numpy(), want) < TOL_OP, wgs
        assert torch.equal(apply(op, src, 56, wgs), out[wgs]), wgs           # the same bits run to run
    assert rel(apply(op, src, 0).cpu().numpy(), want) < TOL_OP
    for v in extra_variants:
        assert rel(apply(op, src, v).cpu().numpy(), want) < TOL_OP, v
    atomic = apply(op, src, atomic_variant(p))
    assert float((atomic - out[8]).abs().max()) < 1e-12 * float(atomic.abs().max())
    c = ns.constrained.astype(np.int64)
    assert np.array_equal(out[8].cpu().numpy()[c], s[c])                       # dst[c] = src[c], exactly
    packed = operator(ns, lattice=0)                                           # the packed-index build on the same mesh: the same bits
    assert packed.mf_data.block_plan_lattice() == 0
    assert torch.equal(apply(packed, src, 56, 8), out[8]) and torch.equal(apply(packed, src, 56, 2), out[2])
    if rhs_and_diagonal:
        op.mf_data.set_apply_variant(0)
        assert rel(op.assemble_rhs().cpu().numpy(), ref.rhs()) < 1e-13
        assert rel(op.compute_diagonal().cpu().numpy(), ref.diagonal()) < 1e-13
    if cg:
        check_cg(op, ref, 8 if cg is True else cg)
    op.mf_data.set_apply_variant(56)
    op.mf_data.set_block_workgroups(8)
    return op, ref, src, out[8]


def check_cg(op, ref, its=8):
    xr, _, _ = O.cg_plain(ref.vmult, ref.rhs(), its)
    for v in (56, 0):
        op.mf_data.set_apply_variant(v)
        b = op.assemble_rhs()
        for solver in (pkg.SolverCGFullMerge, pkg.SolverCG):
            x = op.initialize_dof_vector()
            ctl = pkg.IterationNumberControl(its, 0.0)
            solver(ctl).solve(op, x, b, pkg.DiagonalMatrix())
            assert ctl.last_step() == its and rel(x.cpu().numpy(), xr) < TOL_CG, (v, solver.__name__)


def check_other_operators(um):
    """block vectors (n = 3), the mass operator and the Helmholtz operator on the same arrays -- they share the plan -- at the tolerances of
    tests/test_gpu_components.py, tests/test_gpu_mass.py and test_native_helmholtz_operator_pencil_kernel"""
    ns, ref = um.namespace(), U.Reference(um)
    lm = ref.mesh
    n = um.n_dofs
    c = lm.constrained.astype(np.int64)
    src = np.stack([O.deterministic_src(n, seed=40 + k) for k in range(3)])
    op = operator(ns)
    want = np.stack([ref.vmult(v) for v in src])
    ld = n + (n & 1) + 2
    for variant in (56, 0):
        op.mf_data.set_apply_variant(variant)
        sb = torch.full((3, ld), NAN, dtype=torch.float64, device="cuda:0")
        sb[:, :n] = dev(src)
        db = torch.full((3, ld), NAN, dtype=torch.float64, device="cuda:0")
        op.vmult(db, sb)
        for k in range(3):
            assert rel(db[k, :n].cpu().numpy(), want[k]) <= TOL_OP, (variant, k)
    b3 = CoR.rhs_blocks(ref.rhs())
    xr, _, _ = CoR.cg(ref.vmult, b3, 6)
    op.mf_data.set_apply_variant(56)
    x = op.initialize_block_vector(3)
    bb = op.initialize_block_vector(3)
    bb[:, :n] = dev(b3)
    pkg.SolverCG(pkg.IterationNumberControl(6, 0.0)).solve(op, x, bb, pkg.DiagonalMatrix())
    assert rel(x[:, :n].cpu().numpy(), xr) <= TOL_CG
    s = src[0]
    plane = M.plane(lm, ref.N, ref.D, ref.w, O.kappa_step64)
    mass = pkg.MassOperator(ns, 0, pkg.COEF_STEP64)
    helm = pkg.HelmholtzOperator(ns, 0, pkg.COEF_STEP64)
    hw = O.apply_helmholtz_cells(lm, ref.N, ref.D, ref.w, s)
    hw[c] = s[c]
    for o, w in ((mass, M.vmult(lm, ref.N, ref.w, s, S=plane)), (helm, hw)):
        got = {}
        for variant in (56, 0):
            got[variant] = apply(o, dev(s), variant, 8)
            assert rel(got[variant].cpu().numpy(), w) < TOL_OP, (type(o).__name__, variant)
        assert torch.equal(apply(o, dev(s), 56, 8), got[56])


def plan(op):
    mf = op.mf_data
    mf.set_apply_variant(56)
    return mf.block_plan_info()[0], mf.block_plan_lattice(), mf.block_plan_carry()[0]


# ------------------------------------------------------------------ A - F: at every degree of MESHES
@pytest.mark.parametrize("p", DEGREES)
def test_a_control_generator_arrays_through_the_namespace(p):
    """nothing altered: every block a lattice block, the BLK_LATT build, and the bits of the handle built from the BrickMesh object"""
    um = start(p)
    op, ref, src, got = check_operator(um, cg=True, rhs_and_diagonal=True)
    nb, lattice, faces = plan(op)
    assert nb == len(generator_mesh(p).cell_block_offsets) - 1 and lattice == nb
    assert bits(kernel_name(op)) & LATT
    if p == 4:
        assert faces == 4                                    # the generator hands the bricks over x fastest: four pairs of +x neighbours
    twin = operator(generator_mesh(p))
    assert plan(twin) == (nb, lattice, faces) and torch.equal(apply(twin, src), got)
    check_other_operators(um)


@pytest.mark.parametrize("p", DEGREES)
def test_b_two_dofs_swapped_inside_one_brick_interior(p):
    """only the entry-by-entry stage can reject brick 1; a mixed plan runs the packed build as a whole, and carries nothing"""
    um = start(p)
    inner = um.block_interior_dofs(1)
    um.swap_dofs(int(inner[inner.size // 3]), int(inner[2 * inner.size // 3]))
    op, *_ = check_operator(um, cg=True, rhs_and_diagonal=True)
    nb, lattice, faces = plan(op)
    assert lattice == nb - 1 and faces == 0
    assert not bits(kernel_name(op)) & LATT


def test_c_two_dofs_swapped_inside_a_shared_face():
    """the face interior bricks 0 and 1 meet in: both lose their lattice status, the run tables of both change"""
    um = start(4)
    face = um.shared_face_dofs(0, 1)
    assert face.size == 15 * 15
    um.swap_dofs(int(face[7]), int(face[100]))
    op, *_ = check_operator(um, cg=True)
    nb, lattice, faces = plan(op)
    assert lattice == nb - 2 and faces == 0 and not bits(kernel_name(op)) & LATT


@pytest.mark.parametrize("p", DEGREES)
def test_d_single_cells_in_rotated_local_frames(p):
    """one cell of brick 0 turned by 90 degrees about its z, one cell of brick 1 by 180 degrees about its x: the 'parallel local axes' condition,
    and gathers through rotated frames in every kernel family"""
    um = start(p)
    off = um.block_offsets
    um.rotate_cells([off[0] + 1], U.ROT90_Z).rotate_cells([off[2] - 2], U.ROT180_X)
    extra = (10, 50) + ((3, 49, 59, 52) if p == 4 else ())
    op, *_ = check_operator(um, extra_variants=extra, cg=True, rhs_and_diagonal=True)
    nb, lattice, faces = plan(op)
    assert lattice == nb - 2 and not bits(kernel_name(op)) & LATT
    check_other_operators(um)


@pytest.mark.parametrize("p", DEGREES)
def test_e_a_whole_brick_rotated(p):
    """every cell of brick 1 turned by the same 90 degrees about z: the topology passes (a box in the rotated frame), only the numbering check rejects"""
    um = start(p)
    um.rotate_cells(np.arange(um.block_offsets[1], um.block_offsets[2]), U.ROT90_Z)
    op, *_ = check_operator(um)
    nb, lattice, faces = plan(op)
    assert lattice == nb - 1 and not bits(kernel_name(op)) & LATT


@pytest.mark.parametrize("p", DEGREES)
def test_f_cells_shuffled_inside_their_bricks(p):
    """still all lattice: the closed-form indices take a cell's position from the search, not from the cell order"""
    um = start(p).shuffle_within_blocks(np.random.default_rng(p))
    op, *_ = check_operator(um, cg=True)
    nb, lattice, faces = plan(op)
    assert lattice == nb and bits(kernel_name(op)) & LATT


# ------------------------------------------------------------------ G - J: p = 4 (face carry and the fused update are p = 4 builds)
ORDERS = {"reversed": [7, 6, 5, 4, 3, 2, 1, 0], "random": [5, 2, 7, 0, 3, 6, 1, 4], "x_neighbours": [4, 5, 0, 1, 6, 7, 2, 3], "y_neighbours": [0, 2, 1, 3, 4, 6, 5, 7]}


def fused_update_solves(op, its=3):
    """the merged solve with the fused_update knob at 0 and 1: (x, kernel name) each; the same bits are asserted"""
    mf = op.mf_data
    mf.set_apply_variant(56)
    b = op.assemble_rhs()
    out = []
    for knob in (0, 1):
        mf.set_tuning("fused_update", knob)
        x = op.initialize_dof_vector()
        ctl = pkg.IterationNumberControl(its, 0.0)
        pkg.SolverCGFullMerge(ctl).solve(op, x, b, pkg.DiagonalMatrix())
        assert ctl.last_step() == its and ctl.dot_products_fused
        out.append((x, ctl.apply_kernel))
    assert torch.equal(out[0][0], out[1][0])
    assert not bits(out[0][1]) & UPD
    return out


@pytest.mark.parametrize("order", list(ORDERS))
def test_g_bricks_handed_over_in_another_order(order):
    """lattice blocks in an order the generator does not produce: carry pairs it never forms (+x neighbours in another sequence, +y neighbours),
    none at all (reversed); v is the same bits with and without face carry and for every workgroup count; the fused update still qualifies"""
    um = start(4).permute_blocks(ORDERS[order])
    op, ref, src, got = check_operator(um, cg=True, rhs_and_diagonal=order == "random")
    nb, lattice, faces = plan(op)
    assert lattice == nb == 8 and bits(kernel_name(op)) & LATT
    if order.endswith("neighbours"):
        assert faces == 4
    if order in ("reversed", "random"):
        assert faces == 0                                    # a brick's HIGH face is handed to the next one, never its low face; no neighbours in the random order
    mf = op.mf_data
    for carry in (0, 1):
        mf.set_tuning("face_carry", carry)
        for wgs in (2, 8, 0):
            assert torch.equal(apply(op, src, 56, wgs), got), (carry, wgs)
        for wgs in (2, 8):
            mf.set_block_workgroups(wgs)
            (x0, _), (x1, name1) = fused_update_solves(op)
            assert bits(name1) & UPD and bits(name1) & LATT, (carry, wgs, name1)
            xr, _, _ = O.cg_plain(ref.vmult, ref.rhs(), 3)
            assert rel(x1.cpu().numpy(), xr) < TOL_CG
    if order == "random":
        check_other_operators(um)


def _h_start(slowest):
    """the base mesh with the cells of brick 2 in lexicographic order, direction `slowest` slowest (the generator hands them over by parity
    class), so that its first 32 cells are the lower half of the brick in that direction"""
    um = start(4)
    assert np.array_equal(um.block_offsets, np.arange(9) * 64)
    um.sort_block_cells(2, slowest)
    top = lambda c0, c1: um.coords[um.l2g[c0:c1].ravel()][:, slowest].max()
    assert top(128, 160) < top(160, 192) - 0.3               # two layers of cells below the upper half's top
    return um


def test_h_bricks_merged_halved_and_one_cell_moved():
    """bricks 0 + 1 as one block of 8 x 4 x 4 cells (a box with foreign numbering: its interior holds two interior runs and a face), brick 2 in
    two halves, the last cell of brick 4 moved into brick 5 (no boxes: 63 and 65 cells); the untouched bricks 3, 6, 7 stay lattice blocks.
    Halved across z (4 x 4 x 2), the slowest direction of every entity's numbering, the halves ARE lattice blocks, legitimately: each of their
    27 entities is a consecutive piece, x fastest, of an entity of the brick (the half's interior: layers 1..7 of the brick's interior; the
    face between the halves: layer 8; its edges and corners: rows and ends of the brick's faces and edges).  Halved across x (2 x 4 x 4) a
    row of the brick's interior run leaves the half after 7 entries: 225 runs for the interior alone, more than the 128 the packed indices
    allow -- the plan then has no packed stream and, by the library's rule, no lattice blocks at all; the unpacked build must still be right."""
    for slowest, want in ((2, 5), (0, 0)):
        um = _h_start(slowest).regroup([0, 128, 160, 192, 256, 319, 384, 448, 512])
        op, *_ = check_operator(um, cg=True)
        nb, lattice, faces = plan(op)
        assert nb == 8 and lattice == want and faces == 0 and not bits(kernel_name(op)) & LATT, (slowest, lattice)
        assert op.mf_data.block_plan_info()[2] == (slowest == 2) and (op.mf_data.block_plan_info()[1] > 128) == (slowest == 0)
    # each alteration alone, so that the box test and the numbering test are told apart
    halved = [0, 64, 128, 160, 192, 256, 320, 384, 448, 512]
    for slowest, offsets, want in ((2, [0, 128, 192, 256, 320, 384, 448, 512], 6), (0, halved, 0), (2, [0, 64, 128, 192, 256, 319, 384, 448, 512], 6)):
        one = operator(_h_start(slowest).regroup(offsets).namespace())
        assert plan(one)[:2] == (len(offsets) - 1, want) and one.mf_data.block_plan_info()[2] == (want > 0), offsets
    # brick 2 halved across z alone: nine lattice blocks, a plan of a kind the generator never makes -- the halves hand their common face on
    # (the pairs (0, 1), (2a, 2b), (4, 5), (6, 7) carry; 2b and 3 no longer match in size), and the interior runs no longer cover [0, n_int):
    # layer 8 of brick 2's interior is a shared face now, so the fused update must stay off
    um = _h_start(2).regroup(halved)
    op, ref, *_ = check_operator(um, cg=True)
    nb, lattice, faces = plan(op)
    assert nb == lattice == 9 and faces == 4 and bits(kernel_name(op)) & LATT
    for wgs in (2, 8):
        op.mf_data.set_block_workgroups(wgs)
        (x0, name0), (x1, name1) = fused_update_solves(op)
        assert not bits(name1) & UPD and name1 == name0


def test_i_interior_runs_that_do_not_start_at_zero():
    """the numbering shifted cyclically so that the brick interiors, still consecutive and brick after brick, end at the last DoF and do not
    begin at DoF 0: every block stays a lattice block, the fused update must not qualify.  (The shift is by -n_int, n_int the size of the
    interior class: by +n_int the wrap-around would fall INSIDE a brick's interior run and cost that brick its lattice status, which is
    case B again.)"""
    um = start(4)
    n_int = sum(um.block_interior_dofs(b).size for b in range(um.n_blocks))
    assert n_int == 8 * 15 ** 3
    runs = lambda m: [1 + int((np.diff(np.unique(m.l2g[m.block_offsets[b]:m.block_offsets[b + 1]])) != 1).sum()) for b in range(m.n_blocks)]
    before = runs(um)
    um.shift_dofs(um.n_dofs - n_int)
    assert runs(um) == before and um.block_interior_dofs(0)[0] == um.n_dofs - n_int         # no entity is cut
    op, ref, *_ = check_operator(um, cg=True)
    nb, lattice, faces = plan(op)
    assert lattice == nb and faces == 4 and bits(kernel_name(op)) & LATT
    for wgs in (2, 8):
        op.mf_data.set_block_workgroups(wgs)
        (x0, name0), (x1, name1) = fused_update_solves(op)
        assert not bits(name1) & UPD and name1 == name0
    # the control: unshifted, the fused build runs
    (_, _), (_, name) = fused_update_solves(operator(start(4).namespace()))
    assert bits(name) & UPD


@pytest.mark.parametrize("where", ["brick_interior", "carried_face"])
def test_j_a_dirichlet_dof_in_an_awkward_place(where):
    """the 'unconstrained' conditions: (i) a Dirichlet DoF inside a brick interior switches the fused update off, (ii) one inside the face bricks
    0 and 1 carry in case A takes that face out of the carried set -- the library exposes the NUMBER of carried faces (block_plan_carry()[0]),
    which is the fact asserted: one fewer than in A"""
    um = start(4)
    pool = um.block_interior_dofs(1) if where == "brick_interior" else um.shared_face_dofs(0, 1)
    new = int(pool[pool.size // 2])
    um.constrain([new])
    op, ref, src, got = check_operator(um, cg=True)
    assert got[new].item() == src[new].item() != 0.0
    nb, lattice, faces = plan(op)
    assert lattice == nb and bits(kernel_name(op)) & LATT
    assert faces == (4 if where == "brick_interior" else 3)
    for wgs in (2, 8):
        op.mf_data.set_block_workgroups(wgs)
        (x0, name0), (x1, name1) = fused_update_solves(op)
        assert bool(bits(name1) & UPD) == (where == "carried_face"), name1
        xr, _, _ = O.cg_plain(ref.vmult, ref.rhs(), 3)
        assert rel(x1.cpu().numpy(), xr) < TOL_CG and x1[new].item() == 0.0


# ------------------------------------------------------------------ K: the ring
@pytest.mark.parametrize("p,nx", [(4, 4), (2, 2)])
@pytest.mark.parametrize("blocks", ["one", "per_layer"])
def test_k_ring(p, nx, blocks):
    """cells that are cyclic neighbours (nx = 2: two cells that share BOTH x faces): the breadth-first search meets a position conflict, a block
    that holds a full ring is no lattice block"""
    um = U.UserMesh.ring(p, nx, 1, 2)
    um.regroup([0, 2 * nx] if blocks == "one" else [0, nx, 2 * nx])
    # (p = 2: twelve unknowns, and CG is exact after six iterations; compared after three)
    op, *_ = check_operator(um, extra_variants=(10, 50), cg=8 if p == 4 else 3, rhs_and_diagonal=True)
    nb, lattice, faces = plan(op)
    assert nb == (1 if blocks == "one" else 2) and lattice == 0 and faces == 0
    assert not bits(kernel_name(op)) & LATT


# ------------------------------------------------------------------ L: cell interiors first
@pytest.mark.parametrize("swapped", [False, True])
def test_l_cell_interiors_first_near_miss(swapped):
    """dof_numbering = 2 at p = 5: untouched, the pencil kernel stores the cell interiors plainly (kernel id 32); with ONE interior DoF swapped
    against a face DoF the plain stores must be off -- overwrite and accumulate mode against the oracle"""
    p, cells = 5, (3, 2, 2)
    g = pkg.BrickMesh(p, cells, h=0.25, deform_amp=0.03, dof_numbering=2)
    um = U.UserMesh.from_generator(g)
    if swapped:
        count = np.bincount(um.l2g.ravel(), minlength=um.n_dofs)
        count[um.constrained] = 0
        face = int(np.nonzero(count == 2)[0][3])
        assert face >= um.n_cells * (p - 1) ** 3
        um.swap_dofs((p - 1) ** 3 + 5, face)                 # an interior DoF of cell 1
    ns, ref = um.namespace(), U.Reference(um)
    s = O.deterministic_src(um.n_dofs, seed=3)
    op = pkg.PoissonOperator(ns, 0, pkg.COEF_STEP64)
    assert op.mf_data.get_apply_variant() == 0
    d = op.initialize_dof_vector()
    d.fill_(NAN)
    op.vmult(d, dev(s))
    assert rel(d.cpu().numpy(), ref.vmult(s)) < TOL_OP
    acc = torch.full_like(d, 0.25)
    op.mf_data.cell_loop(op.coef, dev(s), acc)
    assert rel(acc.cpu().numpy() - 0.25, ref.apply_cells(s)) < TOL_OP
    ctl = pkg.IterationNumberControl(3, 0.0)
    x = op.initialize_dof_vector()
    pkg.SolverCGFullMerge(ctl).solve(op, x, op.assemble_rhs(), pkg.DiagonalMatrix())
    xr, _, _ = O.cg_plain(ref.vmult, ref.rhs(), 3)
    assert rel(x.cpu().numpy(), xr) < TOL_CG
    assert ctl.apply_kernel.startswith("apply_pencil_kernel") and ctl.apply_kernel.endswith(",32>") == (not swapped), ctl.apply_kernel


# ------------------------------------------------------------------ the p-transfer between handles whose cells sit in rotated local frames
def _column(p, cells, R=None):
    b = O.BrickMesh(p, cells, deform_amp=0.03)
    um = U.UserMesh(p, b.l2g, b.coords, b.constrained, None, cells)
    return um if R is None else um.rotate_cells(np.arange(um.n_cells), R)


@pytest.mark.parametrize("R", [U.ROT90_Z, U.ROT180_X, U.ROT120_DIAG], ids=["z90", "x180", "diag120"])
def test_transfer_between_handles_rotated_alike(R):
    """(1, 1, 3) cells, degrees 4 -> 2, every cell of BOTH handles turned by the same R: the transfer assembled in numpy from the altered arrays
    (user_mesh.dense_transfer; equal to tests/multigrid_ref.py's on the unrotated mesh: test_user_mesh_cpu.py), and the adjoint identity, at
    the tolerances of test_transfer_matches_numpy_and_is_adjoint"""
    cells = (1, 1, 3)
    uf, uc = _column(4, cells, R), _column(2, cells, R)
    fine, coarse = pkg.PoissonOperator(uf.namespace(), 0, pkg.COEF_STEP64), pkg.PoissonOperator(uc.namespace(), 0, pkg.COEF_STEP64)
    P = U.dense_transfer(uf, uc)
    nf, nc = uf.n_dofs, uc.n_dofs
    tr = pkg.MGTwoLevelTransfer(fine, coarse)
    rng = np.random.default_rng(4)
    ec, x0 = rng.uniform(-1, 1, nc), rng.uniform(-1, 1, nf)          # non-zero on the boundary too: Dirichlet DoFs count as 0
    rf, b0 = rng.uniform(-1, 1, nf), rng.uniform(-1, 1, nc)
    x = dev(x0)
    tr.prolongate_and_add(x, dev(ec))
    pe = x.cpu().numpy() - x0
    assert rel(pe, P @ ec) < 1e-13
    b = dev(b0)
    tr.restrict_and_add(b, dev(rf))
    got = b.cpu().numpy()
    bc = np.zeros(nc, dtype=bool)
    bc[uc.constrained] = True
    assert np.array_equal(got[bc], b0[bc])                           # Dirichlet rows unchanged
    assert rel(got[~bc] - b0[~bc], (P.T @ rf)[~bc]) < 1e-13
    lhs, rhs = (got - b0) @ np.where(bc, 0.0, ec), rf @ pe           # <R r, e> = <r, P e> with the device's own results
    assert abs(lhs - rhs) <= 1e-13 * np.abs(rf).sum() * np.abs(ec).max() * 8
    tr.clear()


@pytest.mark.parametrize("cells,reason", [((1, 1, 3), "cell 0"), ((2, 2, 2), "corner DoFs differ")], ids=["column_1x1x3", "cube_2x2x2"])
def test_transfer_refuses_handles_in_different_local_frames(cells, reason):
    """only the fine handle's cells turned by 90 degrees about z.  On (2, 2, 2) the corner DoFs no longer pair up one to one; on the column
    (1, 1, 3) they still do -- the geometry check refuses it, and names the cell"""
    fine = pkg.PoissonOperator(_column(4, cells, U.ROT90_Z).namespace(), 0, pkg.COEF_STEP64)
    coarse = pkg.PoissonOperator(_column(2, cells).namespace(), 0, pkg.COEF_STEP64)
    with pytest.raises(pkg.BP5Error) as e:
        pkg.MGTwoLevelTransfer(fine, coarse)
    assert "multigrid transfer" in str(e.value) and reason in str(e.value), str(e.value)
    assert e.value.status == 1                                       # BP5_ERR_INVALID
    # unrotated, the same pair is accepted
    same = pkg.PoissonOperator(_column(4, cells).namespace(), 0, pkg.COEF_STEP64)
    pkg.MGTwoLevelTransfer(same, coarse).clear()
