"""BP5_TUNE_FUSED_UPDATE: the merged CG's vector update of the brick interiors inside the p = 4 lattice block kernel (BLK_UPD builds).

Every comparison is the solve with the knob at 1 against the SAME solve with the knob at 0 -- the separate update launch over all DoFs --
and asks for the same bits: x, the residuals, the iteration count.  The kernel names are literals: ..., 286550016> is the fused lattice
build without the update, + 131072 (BLK_UPD) = 286681088 with it, + 32768 (non-temporal metric loads) = 286713856.

Meshes: the smallest on which the brick prologue can go wrong -- eight whole 4x4x4 bricks, and the (9, 8, 6) mesh of
test_gpu_kernel_selection.py with partial bricks of several interior sizes (one of them a single pass long).  Eight workgroups give about
one brick per workgroup (the first-brick prologue), two workgroups several consecutive bricks each (the prologue rolled ahead into the
previous brick's last pass, the 128-byte line two consecutive interior runs share, the face carry)."""
import functools

import pytest
import torch

import bp5_pkg

pytestmark = pytest.mark.gpu
pkg = bp5_pkg.load()

PLAIN = "apply_block_kernel<4,{c},32,1,286550016>"
PLAIN_NT = "apply_block_kernel<4,false,32,1,286582784>"      # Gauss only: GLL has no non-temporal build of the plain kernel
FUSED = "apply_block_kernel<4,{c},32,1,286681088>"
FUSED_NT = "apply_block_kernel<4,{c},32,1,286713856>"
MESHES = [(8, 8, 8), (9, 8, 6)]


@functools.lru_cache(maxsize=None)
def _mesh(cells, numbering=1):
    return pkg.BrickMesh(4, cells, h=0.2, deform_amp=0.03, cell_block=(4, 4, 4), dof_numbering=numbering, cell_block_order=1)


def _operator(cells, quad, numbering=1, lattice=1):
    op = pkg.PoissonOperator(_mesh(cells, numbering), quad, pkg.COEF_STEP64)
    op.mf_data.set_tuning("lattice_indices", lattice)
    op.mf_data.set_apply_variant(56)
    return op


def _solve(op, b, control, precond=None, solver=pkg.SolverCGFullMerge, check_every=0):
    x = op.initialize_dof_vector()
    solver(control, check_every=check_every).solve(op, x, b, precond if precond is not None else pkg.DiagonalMatrix())
    return x


def _same(op, b, make_control, where, **kw):
    """the solve with the knob at 0, 1 and -1: same bits; returns the three controls"""
    out = []
    for knob in (0, 1, -1):
        op.mf_data.set_tuning("fused_update", knob)
        ctl = make_control()
        x = _solve(op, b, ctl, **kw)
        out.append((x, ctl))
    (x0, c0) = out[0]
    for knob, (x, c) in zip((1, -1), out[1:]):
        assert torch.equal(x, x0), (where, knob)
        assert c.initial_value() == c0.initial_value() and c.last_value() == c0.last_value() and c.last_step() == c0.last_step(), (where, knob)
        assert c.dot_products_fused == c0.dot_products_fused, (where, knob)
    return [c for _, c in out]


def _names(quad, streaming):
    c = "true" if quad else "false"
    plain = PLAIN_NT if (streaming and not quad) else PLAIN.format(c=c)
    return plain, (FUSED_NT if streaming else FUSED).format(c=c)


@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("cells", MESHES)
def test_fused_update_gives_the_bits_of_the_separate_update(cells, quad):
    """k = 1 (only the first iteration, whose p comes from the init kernel: no fused-update launch at all), 2, 3, 4, 7 iterations: both x
    parities and both x epilogues; metric loads plain / non-temporal, face carry off / on, about one brick / several bricks per workgroup."""
    op = _operator(cells, quad)
    mf = op.mf_data
    b = op.assemble_rhs()
    assert mf.block_plan_lattice() == mf.block_plan_info()[0]
    for wgs in (8, 2):
        mf.set_block_workgroups(wgs)
        for streaming in (0, 1):
            mf.set_streaming(streaming)
            plain, fused = _names(quad, streaming)
            for carry in (0, 1):
                mf.set_tuning("face_carry", carry)
                for k in (1, 2, 3, 4, 7):
                    where = (cells, quad, wgs, streaming, carry, k)
                    c0, c1, cm = _same(op, b, lambda: pkg.IterationNumberControl(k, 0.0), where)
                    assert c0.last_step() == k and c0.dot_products_fused, where
                    assert c0.apply_kernel == plain and cm.apply_kernel == plain, (where, c0.apply_kernel, cm.apply_kernel)   # -1: by size, far below the threshold here
                    assert c1.apply_kernel == (fused if k > 1 else plain), (where, c1.apply_kernel)
    # the metric loads of a fused-update launch are non-temporal unless the handle says otherwise
    mf.set_streaming(-1)
    mf.set_tuning("fused_update", 1)
    ctl = pkg.IterationNumberControl(3, 0.0)
    _solve(op, b, ctl)
    assert ctl.apply_kernel == FUSED_NT.format(c="true" if quad else "false")


@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("cells", MESHES)
def test_a_solve_that_stops_on_its_tolerance_applies_the_x_epilogue_once(cells, quad):
    """check_every = 3: the host looks at the stop flag every third iteration, so a tolerance met at an iteration that is no multiple of 3 has stopped
    iterations launched behind it -- the block kernel and the rest update are no-ops in them, and the pending x update is applied once, by the
    launch behind the loop"""
    op = _operator(cells, quad)
    mf = op.mf_data
    b = op.assemble_rhs()
    mf.set_tuning("fused_update", 0)
    probe = pkg.IterationNumberControl(1, 0.0)
    _solve(op, b, probe)
    seen = set()
    for wgs in (8, 2):
        mf.set_block_workgroups(wgs)
        for factor in (0.5, 0.2, 0.1, 0.05, 0.02, 0.01, 5e-3, 2e-3, 1e-3, 1e-4):   # several stops: both x epilogues, one or two stopped iterations behind them
            tol = factor * probe.initial_value()
            c0, c1, _ = _same(op, b, lambda: pkg.SolverControl(2000, tol), (cells, quad, wgs, factor), check_every=3)
            assert 1 < c0.last_step() < 2000 and c0.last_value() <= tol, (cells, quad, wgs, factor, c0.last_step(), c0.last_value())
            assert c1.apply_kernel == _names(quad, 1)[1]
            seen.add(c0.last_step() % 3)
    assert seen & {1, 2}, seen   # at least one solve stopped at an iteration after which stopped iterations were launched


@pytest.mark.parametrize("cells", MESHES)
def test_jacobi_preconditioned_solves_keep_the_separate_update(cells):
    """the fused dot products need D = 1: with the Jacobi diagonal the merged solver forms them itself and the knob changes nothing"""
    op = _operator(cells, 0)
    op.mf_data.set_block_workgroups(2)
    b = op.assemble_rhs()
    jacobi = pkg.DiagonalMatrix(op.compute_diagonal(invert=True))
    for k in (2, 3):
        c0, c1, _ = _same(op, b, lambda: pkg.IterationNumberControl(k, 0.0), (cells, k), precond=jacobi)
        assert not c1.dot_products_fused and c1.apply_kernel == c0.apply_kernel == "apply_block_kernel<4,false,32,1,285534208>", (cells, k, c1.apply_kernel)


@pytest.mark.parametrize("what", ["packed plan", "lexicographic numbering", "fusion off", "SolverCG"])
def test_what_does_not_qualify_takes_the_separate_update(what):
    """knob 1 on a solve outside the build's scope: the same bits, the kernel launched today, no error"""
    cells = (9, 8, 6)
    op = _operator(cells, 0, numbering=0 if what == "lexicographic numbering" else 1, lattice=0 if what == "packed plan" else 1)
    mf = op.mf_data
    mf.set_block_workgroups(2)
    mf.set_streaming(0)
    if what == "fusion off":
        mf.set_cg_fusion(0)
    b = op.assemble_rhs()
    solver = pkg.SolverCG if what == "SolverCG" else pkg.SolverCGFullMerge
    for k in (2, 3):
        c0, c1, _ = _same(op, b, lambda: pkg.IterationNumberControl(k, 0.0), (what, k), solver=solver)
        assert c1.apply_kernel == c0.apply_kernel and str(131072 + 286550016) not in c1.apply_kernel, (what, c1.apply_kernel)
    want = {"packed plan": "apply_block_kernel<4,false,32,1,1337344>", "lexicographic numbering": "apply_block_kernel<4,false,32,1,10240>",
            "fusion off": "apply_block_kernel<4,false,32,1,285501440>", "SolverCG": PLAIN.format(c="false")}[what]
    assert c1.apply_kernel == want and c1.dot_products_fused == (what in ("packed plan", "SolverCG")), (what, c1.apply_kernel)


def test_the_knob_takes_three_values():
    op = _operator((8, 8, 8), 0)
    assert op.mf_data.get_tuning("fused_update") == -1   # by size: on above 2.4e7 local DoFs
    for v in (-1, 1, 0):
        op.mf_data.set_tuning("fused_update", v)
        assert op.mf_data.get_tuning("fused_update") == v
    for v in (-2, 2):
        with pytest.raises(pkg.BP5Error):
            op.mf_data.set_tuning("fused_update", v)
