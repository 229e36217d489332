"""Block vectors behind the halo exchange, one process, REAL RCCL through a self neighbour (the recipe of
test_halo_exchange_through_rccl_with_a_self_neighbour in tests/test_gpu_parity.py: the slab mesh of a rank > 0 supplies cells that read
ghost DoFs, the 'owner' of the ghost plane is this rank's own DoFs).  bp5_halo_*_components against the same steps by torch indexing,
bitwise; bp5_apply_components_distributed against bp5_apply_distributed block by block and against the sequence done by hand;
bp5_cg_solve_components_distributed on the glued mesh; refusals and the fallback of a handle without a communicator.

The start / finish halves of the two exchanges are internal, so 'work between start and finish' cannot be enqueued from here: with overlap
on, the exchange is called with the compute stream still busy (fills enqueued just before and just after), which is what makes a missing
event between the two streams visible."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
from test_gpu_parity import TOL_OP, _consistent_self_glue

pytestmark = pytest.mark.gpu
pkg = bp5_pkg.load()
SENTINEL = -7.25
UNSUPPORTED = 5


def _t():
    import torch
    return torch


def ptr(t):
    return C.c_void_p(t.data_ptr())


def _self_neighbour_mesh(m1, tables):
    return SimpleNamespace(degree=m1.degree, n=m1.degree + 1, cells=m1.cells, n_cells=m1.n_cells, n_interior_cells=m1.n_interior_cells, n_owned=m1.n_owned,
                           n_ghost=m1.n_ghost, n_local=m1.n_owned + m1.n_ghost, n_global_dofs=m1.n_owned, l2g=m1.l2g, coords=m1.coords,
                           global_ids=m1.global_ids, constrained=m1.constrained, cell_block_offsets=None, rank=0, n_ranks=1, h=1.0, deform_amp=0.03, **tables)


def _one_neighbour(m1, send_idx):
    ng = m1.n_ghost
    return dict(n_neighbors=1, neighbor_rank=np.zeros(1, np.int32), send_offsets=np.asarray([0, ng], np.uint32), send_indices=send_idx,
                recv_offsets=np.asarray([0, ng], np.uint32))


def _block(nc, n_local, ld, gen, zero_ghosts_from=None):
    """(n_components, ld) block vector of random entries, SENTINEL in the padding [n_local, ld)"""
    torch = _t()
    v = torch.full((nc, ld), SENTINEL, dtype=torch.float64, device="cuda:0")
    v[:, :n_local] = torch.rand((nc, n_local), dtype=torch.float64, device="cuda:0", generator=gen)
    if zero_ghosts_from is not None:
        v[:, zero_ghosts_from:n_local] = 0.0
    return v


def _lds(n_local):
    return (n_local + (n_local & 1), n_local + 66 + (n_local & 1))       # n_local rounded up to even; 66 more (a padding the exchange must not touch)


def _exchange_checks(op, m1, send_idx, nc, ld):
    """gather, scatter-add, zero-ghosts against torch indexing, bitwise, padding included; overlap off and on"""
    torch = _t()
    L, h = pkg.lib(), op.mf_data.handle
    no, ng = m1.n_owned, m1.n_ghost
    nl = no + ng
    idx = torch.from_numpy(send_idx.astype(np.int64)).cuda()
    g = torch.Generator(device="cuda:0").manual_seed(40 + nc)
    busy = torch.zeros(1 << 21, dtype=torch.float64, device="cuda:0")
    for overlap in (0, 1):
        assert L.bp5_mf_set_overlap(h, overlap) == 0
        v = _block(nc, nl, ld, g)
        ref = v.clone()
        ref[:, no:nl] = ref[:, idx]
        v[:, no:nl] = float("nan")                                          # whatever the ghosts held is replaced
        assert L.bp5_vec_fill(h, ptr(busy), 1.0, busy.numel()) == 0
        assert L.bp5_halo_gather_components(h, nc, ld, ptr(v)) == 0, L.bp5_last_error()
        assert L.bp5_vec_fill(h, ptr(busy), 2.0, busy.numel()) == 0
        assert torch.equal(v, ref), (overlap, "gather")
        w = _block(nc, nl, ld, g)
        refw = w.clone()
        refw[:, idx] += refw[:, no:nl]
        refw[:, no:nl] = 0.0
        assert L.bp5_vec_fill(h, ptr(busy), 3.0, busy.numel()) == 0
        assert L.bp5_halo_scatter_add_components(h, nc, ld, ptr(w)) == 0, L.bp5_last_error()
        assert L.bp5_vec_fill(h, ptr(busy), 4.0, busy.numel()) == 0
        assert torch.equal(w, refw), (overlap, "scatter-add")
        z = _block(nc, nl, ld, g)
        refz = z.clone()
        refz[:, no:nl] = 0.0
        assert L.bp5_halo_zero_ghosts_components(h, nc, ld, ptr(z)) == 0
        assert torch.equal(z, refz), (overlap, "zero ghosts")
    op.mf_data.synchronize()


# ------------------------------------------------------------------ 1. the exchange, one neighbour
@pytest.mark.parametrize("nc", [1, 3, 8])
def test_exchange_is_bitwise_the_indexing_and_leaves_the_padding_alone(nc):
    p, cells = 3, (4, 3, 5)
    m1 = pkg.BrickMesh(p, cells, deform_amp=0.03, rank=1, n_ranks=2)
    no, ng = m1.n_owned, m1.n_ghost
    assert ng > 0
    send_idx = np.arange(no - ng, no, dtype=np.uint32)                      # this rank's last owned DoFs play the neighbour's plane
    comm = pkg.Communicator(0, 1)
    op = pkg.PoissonOperator(_self_neighbour_mesh(m1, _one_neighbour(m1, send_idx)), 0, pkg.COEF_ONE, comm=comm)
    for ld in _lds(no + ng):
        _exchange_checks(op, m1, send_idx, nc, ld)
    # growing and shrinking n_components on ONE handle: the staging buffers follow (grown on demand, messages re-laid out)
    for other in (8, 1):
        _exchange_checks(op, m1, send_idx, other, _lds(no + ng)[0])
    op.mf_data.close()
    comm.close()


# ------------------------------------------------------------------ 2. two neighbours, one receive-only and one send-only
@pytest.mark.parametrize("nc", [1, 3, 8])
def test_exchange_with_the_tables_of_a_middle_rank_skips_zero_length_messages(nc):
    p, cells = 3, (4, 3, 7)
    m1 = pkg.BrickMesh(p, cells, deform_amp=0.03, rank=1, n_ranks=3)
    no, ng = m1.n_owned, m1.n_ghost
    assert m1.n_neighbors == 2 and list(m1.send_offsets) == [0, 0, ng] and list(m1.recv_offsets) == [0, ng, ng]
    tables = dict(n_neighbors=2, neighbor_rank=np.zeros(2, np.int32), send_offsets=m1.send_offsets, send_indices=m1.send_indices, recv_offsets=m1.recv_offsets)
    comm = pkg.Communicator(0, 1)
    op = pkg.PoissonOperator(_self_neighbour_mesh(m1, tables), 0, pkg.COEF_ONE, comm=comm)
    for ld in _lds(no + ng):
        _exchange_checks(op, m1, np.asarray(m1.send_indices), nc, ld)
    op.mf_data.close()
    comm.close()


# ------------------------------------------------------------------ 3. the application
CELLS_PER_TEAM = {2: 7, 4: 10}       # 64 TW / LPC of the degree's default pencil (p <= 3: one wave, (p+1)^2 lanes per cell; p >= 4: four waves)
APPLY_CELLS = {2: (5, 3, 7), 4: (11, 3, 5)}


def _apply_setup(p, quadrature):
    m1 = pkg.BrickMesh(p, APPLY_CELLS[p], deform_amp=0.03, rank=1, n_ranks=2)
    send_idx = _consistent_self_glue(m1)
    mesh = _self_neighbour_mesh(m1, _one_neighbour(m1, send_idx))
    comm = pkg.Communicator(0, 1)
    op = pkg.PoissonOperator(mesh, quadrature, pkg.COEF_STEP64, comm=comm)
    twin = pkg.PoissonOperator(mesh, quadrature, pkg.COEF_STEP64)          # the same rank-local mesh without a communicator: no exchange
    return m1, send_idx, comm, op, twin


@pytest.mark.parametrize("p,quadrature", [(2, 0), (4, 0), (2, 1)])
def test_partly_filled_teams_sit_at_every_range_boundary(p, quadrature):
    """the ranges of the three-phase schedule, [0, split), [n_interior, n_cells), [split, n_interior): none starts or ends on a team boundary"""
    m1 = pkg.BrickMesh(p, APPLY_CELLS[p], deform_amp=0.03, rank=1, n_ranks=2)
    lanes = (p + 1) ** 2
    cpt = 64 * (1 if p <= 3 else 4) // lanes
    assert cpt == CELLS_PER_TEAM[p]
    n_int, n_cells = m1.n_interior_cells, m1.n_cells
    split = n_int // 2
    lengths = (split, n_int - split, n_cells - n_int, n_int, n_cells)
    assert 0 < split < n_int < n_cells and all(v % cpt for v in lengths), (lengths, cpt)
    assert min(split, n_int - split, n_cells - n_int) > cpt                 # more than one team in every range


@pytest.mark.parametrize("p,quadrature", [(2, 0), (4, 0), (2, 1)])
def test_application_equals_the_scalar_path_and_the_sequence_by_hand(p, quadrature):
    torch = _t()
    m1, send_idx, comm, op, twin = _apply_setup(p, quadrature)
    L, h = pkg.lib(), op.mf_data.handle
    no, ng = m1.n_owned, m1.n_ghost
    nl = no + ng
    idx = torch.from_numpy(send_idx.astype(np.int64)).cuda()
    con = torch.from_numpy(m1.constrained.astype(np.int64)).cuda()
    rel = lambda a, b: float(torch.linalg.norm(a - b) / torch.linalg.norm(b))
    g = torch.Generator(device="cuda:0").manual_seed(9)
    for nc in (1, 3, 8):
        ld = _lds(nl)[1 if nc == 3 else 0]
        src = _block(nc, nl, ld, g, zero_ghosts_from=no)
        # the scalar path, block by block, on the same handle (meshes this small: the atomic pencil kernel, whose twin the block-vector kernel is)
        scalar = torch.zeros_like(src)
        for c in range(nc):
            s_in, d = src[c, :nl].clone(), op.initialize_dof_vector()
            assert L.bp5_mf_set_overlap(h, 0) == 0
            assert L.bp5_apply_distributed(h, ptr(op.coef), ptr(s_in), ptr(d), 1) == 0
            scalar[c, :nl] = d
        # the sequence by hand: gather by indexing, all cells on the communicator-free twin, add, zero, Dirichlet copy
        s2 = src.clone()
        s2[:, no:nl] = s2[:, idx]
        hand = torch.zeros_like(src)
        assert L.bp5_apply_components(twin.mf_data.handle, ptr(twin.coef), nc, ld, ptr(s2), ptr(hand), 1) == 0, L.bp5_last_error()
        hand[:, idx] += hand[:, no:nl]
        hand[:, no:nl] = 0.0
        hand[:, con] = src[:, con]
        for overlap in (0, 1):
            assert L.bp5_mf_set_overlap(h, overlap) == 0
            s_in = src.clone()
            dst = torch.full_like(src, float("nan"))                         # overwrite mode: whatever dst held is gone
            dst[:, nl:] = SENTINEL
            assert L.bp5_apply_components_distributed(h, ptr(op.coef), nc, ld, ptr(s_in), ptr(dst), 1) == 0, L.bp5_last_error()
            assert bool(torch.isfinite(dst).all())
            assert torch.equal(s_in, src)                                    # ghosts of src zeroed again, owned entries and padding untouched
            assert float(dst[:, no:nl].abs().max()) == 0.0 and bool((dst[:, nl:] == SENTINEL).all())
            assert torch.equal(dst[:, con], src[:, con])                     # Dirichlet rows copied
            for c in range(nc):
                e1, e2 = rel(dst[c, :nl], scalar[c, :nl]), rel(dst[c, :nl], hand[c, :nl])
                print(f"p = {p} quadrature {quadrature} nc = {nc} overlap {overlap} block {c}: vs scalar {e1:.2e}, vs by hand {e2:.2e}")
                assert e1 < TOL_OP and e2 < TOL_OP, (nc, overlap, c, e1, e2)
            # accumulate mode: dst += A src on a non-zero dst (ghost entries of dst hold contributions only: zero on entry)
            acc = torch.full_like(src, 0.25)
            acc[:, no:nl] = 0.0
            acc[:, nl:] = SENTINEL
            s_in = src.clone()
            assert L.bp5_apply_components_distributed(h, ptr(op.coef), nc, ld, ptr(s_in), ptr(acc), 0) == 0
            want = dst + 0.25
            want[:, no:nl] = 0.0
            want[:, con] = src[:, con]
            want[:, nl:] = SENTINEL
            assert rel(acc[:, :nl], want[:, :nl]) < TOL_OP and bool((acc[:, nl:] == SENTINEL).all()), (nc, overlap)
    for o in (op, twin):
        o.mf_data.synchronize()
        o.mf_data.close()
    comm.close()


# ------------------------------------------------------------------ 4. CG on the glued mesh
@pytest.mark.parametrize("with_diag", [False, True])
def test_cg_recurrence_residual_is_the_true_residual_through_the_exchange(with_diag):
    """12 iterations on three components: the glued mesh is still SPD on the free DoFs, so the recurrence residual equals the true residual
    through bp5_apply_components_distributed to 1e-9 of the initial one, and has dropped below half of it (the bounds of the scalar test)"""
    torch = _t()
    from deal_and_ceed_on_gpu_amd import _lib
    p, cells, nc = 3, (4, 3, 5), 3
    m1 = pkg.BrickMesh(p, cells, deform_amp=0.03, rank=1, n_ranks=2)
    no, ng = m1.n_owned, m1.n_ghost
    nl = no + ng
    send_idx = np.arange(no - ng, no, dtype=np.uint32)                      # the gluing of the scalar test
    comm = pkg.Communicator(0, 1)
    op = pkg.PoissonOperator(_self_neighbour_mesh(m1, _one_neighbour(m1, send_idx)), 0, pkg.COEF_STEP64, comm=comm)
    L, h = pkg.lib(), op.mf_data.handle
    b0 = op.assemble_rhs()                                                   # ghost contributions travel to their (faked) owners
    ld = _lds(nl)[1]
    i = torch.arange(no, dtype=torch.float64, device="cuda:0")
    B = torch.full((nc, ld), SENTINEL, dtype=torch.float64, device="cuda:0")
    B[:, :nl] = 0.0
    for c in range(nc):
        B[c, :no] = b0[:no] * (1.0 + 0.5 * torch.sin(0.37 * (c + 1) * i))
    inv = op.compute_diagonal(invert=True) if with_diag else None
    for overlap in (0, 1):
        assert L.bp5_mf_set_overlap(h, overlap) == 0
        x = torch.full_like(B, float("nan"))
        x[:, nl:] = SENTINEL
        prm, res = _lib.CGParams(_lib.CG_PLAIN, 12, 0.0, 0, 0), _lib.CGResult()
        st = L.bp5_cg_solve_components_distributed(h, ptr(op.coef), nc, ld, ptr(inv) if inv is not None else None, ptr(B), ptr(x), C.byref(prm), C.byref(res))
        assert st == 0, L.bp5_last_error()
        assert res.iterations == 12 and res.exchange_schedule == (3 if overlap else 1)
        assert bool((x[:, nl:] == SENTINEL).all()) and bool(torch.isfinite(x[:, :no]).all())
        xin = x.clone()
        xin[:, no:nl] = 0.0
        Ax = torch.zeros_like(B)
        assert L.bp5_apply_components_distributed(h, ptr(op.coef), nc, ld, ptr(xin), ptr(Ax), 1) == 0
        true_res = float(torch.linalg.norm((Ax - B)[:, :no]))
        print(f"overlap {overlap} diag {with_diag}: recurrence {res.residual:.6e} true {true_res:.6e} initial {res.initial_residual:.6e}")
        assert abs(true_res - res.residual) < 1e-9 * res.initial_residual
        assert res.residual < 0.5 * res.initial_residual
    op.mf_data.synchronize()
    op.mf_data.close()
    comm.close()


# ------------------------------------------------------------------ 5. refusals and the fallback
def test_unsupported_handles_are_refused_and_a_handle_without_a_communicator_runs():
    torch = _t()
    from deal_and_ceed_on_gpu_amd import _lib
    L = pkg.lib()
    mesh = pkg.BrickMesh(2, (3, 2, 2))

    def ns(m):
        return SimpleNamespace(degree=m.p, n=m.n, n_cells=m.n_cells, n_interior_cells=m.n_cells, n_owned=m.n_dofs, n_ghost=0, n_local=m.n_dofs,
                               n_global_dofs=m.n_dofs, l2g=m.l2g, coords=m.coords, constrained=m.constrained, n_neighbors=0,
                               neighbor_rank=np.zeros(0, np.int32), send_offsets=np.zeros(1, np.uint32), send_indices=np.zeros(0, np.uint32),
                               recv_offsets=np.zeros(1, np.uint32), cell_block_offsets=None, constraint_mask=m.constraint_mask, rank=0, n_ranks=1)
    cases = [(pkg.PoissonOperator(mesh, 0, metric_precision="float32"), "FP32"),
             (pkg.HelmholtzOperator(mesh, 0), "Helmholtz"),
             (pkg.PoissonOperator(ns(O.HangingBrickMesh(2, 2, 2, 1, 3)), 0), "hanging"),
             (pkg.PoissonOperator(mesh, 0, geometry=pkg.GEOM_AFFINE), "affine")]
    for op, word in cases:
        x, b = op.initialize_block_vector(3), op.initialize_block_vector(3)
        b.fill_(1.0)
        coef = ptr(op.coef) if op.coef is not None else None
        st = L.bp5_apply_components_distributed(op.mf_data.handle, coef, 3, x.shape[1], ptr(b), ptr(x), 1)
        assert st == UNSUPPORTED and word in L.bp5_last_error().decode(), (word, st, L.bp5_last_error())
        prm, res = _lib.CGParams(_lib.CG_PLAIN, 3, 0.0, 0, 0), _lib.CGResult()
        st = L.bp5_cg_solve_components_distributed(op.mf_data.handle, coef, 3, x.shape[1], None, ptr(b), ptr(x), C.byref(prm), C.byref(res))
        assert st == UNSUPPORTED and word in L.bp5_last_error().decode(), (word, st, L.bp5_last_error())
        op.mf_data.synchronize()
        assert float(x.abs().max()) == 0.0 and bool((b == 1.0).all())          # refused before any launch
    # no communicator: not an error, the one-rank path
    op = pkg.PoissonOperator(pkg.BrickMesh(2, (3, 2, 4), deform_amp=0.03), 0, pkg.COEF_STEP64)
    g = torch.Generator(device="cuda:0").manual_seed(3)
    nl = op.mf_data.n_local
    ld = _lds(nl)[1]
    src = _block(3, nl, ld, g)
    a, d = torch.full_like(src, float("nan")), torch.full_like(src, float("nan"))
    assert L.bp5_apply_components(op.mf_data.handle, ptr(op.coef), 3, ld, ptr(src), ptr(a), 1) == 0
    assert L.bp5_apply_components_distributed(op.mf_data.handle, ptr(op.coef), 3, ld, ptr(src), ptr(d), 1) == 0
    e = float(torch.linalg.norm(d[:, :nl] - a[:, :nl]) / torch.linalg.norm(a[:, :nl]))
    assert e < TOL_OP, e
    for fn in (L.bp5_halo_gather_components, L.bp5_halo_scatter_add_components, L.bp5_halo_zero_ghosts_components):
        v = src.clone()
        assert fn(op.mf_data.handle, 3, ld, ptr(v)) == 0 and torch.equal(v, src)   # no neighbours, no ghosts: nothing to do
    # BP5_CG_MERGED is known and not offered, as on one rank
    x = torch.zeros_like(src)
    prm, res = _lib.CGParams(_lib.CG_MERGED, 3, 0.0, 0, 0), _lib.CGResult()
    st = L.bp5_cg_solve_components_distributed(op.mf_data.handle, ptr(op.coef), 3, ld, None, ptr(src), ptr(x), C.byref(prm), C.byref(res))
    assert st == UNSUPPORTED and "BP5_CG_MERGED" in L.bp5_last_error().decode() and float(x.abs().max()) == 0.0
    # ... and PLAIN on this handle is the one-rank solve: same iteration count and residual, schedule 0
    B = src.clone()
    B[:, nl:] = 0.0
    outs = []
    for fn in (L.bp5_cg_solve_components, L.bp5_cg_solve_components_distributed):
        x = torch.zeros_like(src)
        prm, res = _lib.CGParams(_lib.CG_PLAIN, 6, 0.0, 0, 0), _lib.CGResult()
        assert fn(op.mf_data.handle, ptr(op.coef), 3, ld, None, ptr(B), ptr(x), C.byref(prm), C.byref(res)) == 0
        outs.append((x, res.iterations, res.residual, res.exchange_schedule))
    assert outs[0][1] == outs[1][1] == 6 and outs[1][3] == 0
    assert abs(outs[0][2] - outs[1][2]) <= 1e-11 * outs[0][2]
    assert float(torch.linalg.norm(outs[1][0] - outs[0][0]) / torch.linalg.norm(outs[0][0])) < 1e-11
