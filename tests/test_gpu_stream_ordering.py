"""Every entry point on a busy non-blocking side stream (tests/stream_harness.py has the protocol and why the null stream hides what it finds).

Each case builds its handle under `with torch.cuda.stream(S)`, fills the working inputs with NaN, holds S, enqueues the producers of the good inputs
behind the hold, asserts that the hold still lasts and makes the library call -- so everything the call enqueues is enqueued while its inputs are
NaN -- and takes the result with a clone on S.  References and tolerances are those of each family's own GPU test: 1e-13 for an operator
application, 1e-11 for CG at a fixed iteration count, 1e-10 for a Lanczos estimate and a tolerance stop, 1e-12 / 1e-11 for Chebyshev and the
V-cycle.  Calls that include/bp5.h documents as asynchronous are made twice; the second, warmed call must return while the hold still lasts.
Deterministic paths (block kernel, merged CG on it) must give the bits of the same call on a null-stream twin handle."""
import ctypes as C
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bp5_oracle as O
import bp5_pkg
import chebyshev_ref as CR
import components_ref as CoR
import elasticity_ref as ER
import f32_metric_ref as F
import hmg_ref as H
import mass_ref as M
import overint_ref as OR
import stream_harness as SH
from stream_harness import SENTINEL, held, hold, on_device, side_stream
from test_gpu_chebyshev import _PyOperator
from test_gpu_f32_metric import _planes
from test_gpu_multirank_loopback import _stop_tolerance
from test_gpu_parity import _hanging_namespace

pytestmark = pytest.mark.gpu
pkg = bp5_pkg.load()
TOL_OP, TOL_CG, TOL_STOP, TOL_EST, TOL_CHEB, TOL_MG = 1e-13, 1e-11, 1e-10, 1e-10, 1e-12, 1e-11
AMP = 0.04
LATT, NT, FUSED_UPDATE = 16777216, 32768, 131072        # bp5_kernels.hpp: BLK_LATT, non-temporal metric loads, the fused vector update
EXTRA = 66                                              # padding entries behind every block of a block vector (tests/test_gpu_elasticity.py)
NAN = float("nan")
_cache = {}


def S1():
    if "S" not in _cache:
        _cache["S"], _cache["S2"] = side_stream(), side_stream()
        SH.calibrate()
    return _cache["S"]


def S2():
    S1()
    return _cache["S2"]


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def rel_max(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def lm_of(mesh):
    """a library mesh as the numpy references take it: its own local_to_global, cell order and coordinates"""
    return SimpleNamespace(p=mesh.degree, n=mesh.degree + 1, n_cells=mesh.n_cells, n_dofs=mesh.n_local, l2g=np.asarray(mesh.l2g),
                           coords=np.asarray(mesh.coords), constrained=np.asarray(mesh.constrained))


def cells_slice(lm, c0, c1):
    return SimpleNamespace(**{**vars(lm), "n_cells": c1 - c0, "l2g": lm.l2g[c0:c1]})


def bits(name):
    return int(name.split(",")[-1].rstrip(">"))


# ------------------------------------------------------------------ the operator families
BRICK = dict(cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1)
SMALL = (3, 2, 2)


def _block(op, lattice, wgs, streaming=None):
    mf = op.mf_data
    mf.set_tuning("lattice_indices", lattice)
    mf.set_apply_variant(56)
    mf.set_block_workgroups(wgs)
    if streaming is not None:
        mf.set_streaming(streaming)


def _poisson_like(kind, p, cells=SMALL, quad=0, brick=False, mesh_kw=None, **op_kw):
    """(operator, cell-loop reference, kernel predicate) of the scalar families on a generated mesh"""
    kw = {"deform_amp": AMP, **(BRICK if brick else {}), **(mesh_kw or {})}
    if kind == "affine":
        kw = dict(h=0.5)
    mesh = pkg.BrickMesh(p, cells, **kw)
    lm = lm_of(mesh)
    _, _, w, N, D = O.shape_tables(p, 1 if quad == 1 else 0)
    if kind == "helmholtz":
        op = pkg.HelmholtzOperator(mesh, quad, pkg.COEF_STEP64)

        def cells_ref(s, c0, c1, dst):
            sub = cells_slice(lm, c0, c1)
            return dst + O.apply_helmholtz_cells(sub, N, D, w, s)
    elif kind == "mass":
        op = pkg.MassOperator(mesh, quad, pkg.COEF_STEP64)
        plane = M.plane(lm, N, D, w, O.kappa_step64)

        def cells_ref(s, c0, c1, dst):
            return M.apply_cells(lm, N, w, s, S=plane, cell_range=(c0, c1), dst=dst)
    elif kind in ("overint", "overint_mass"):
        op = (pkg.MassOperator if kind == "overint_mass" else pkg.PoissonOperator)(mesh, pkg.QUAD_GAUSS_OVER, pkg.COEF_STEP64)
        pr = OR.Problem(p, cells, kappa=O.kappa_step64, mass=kind == "overint_mass", mesh=lm)

        def cells_ref(s, c0, c1, dst):
            return pr.apply_cells(s, (c0, c1), dst)
    else:
        extra = dict(geometry=pkg.GEOM_AFFINE) if kind == "affine" else dict(metric_precision="float32") if kind == "f32" else {}
        op = pkg.PoissonOperator(mesh, quad, pkg.COEF_STEP64, **extra, **op_kw)
        coef = [None if kind == "f32" else O.merged_metric(lm, N, D, w, O.kappa_step64)]

        def cells_ref(s, c0, c1, dst):
            if coef[0] is None:                     # float planes: the reference applies the planes read back (tests/test_gpu_f32_metric.py)
                torch.cuda.synchronize()
                coef[0] = _planes(op)
            return O.apply_cells(lm, coef[0], N, D, s, cell_range=(c0, c1), dst=dst)
    return op, lm, cells_ref


def _scalar(op, lm, cells_ref, kernel, solver=pkg.SolverCG, deterministic=False, seed=7):
    n = lm.n_dofs
    s = O.deterministic_src(n, seed=seed)
    c = np.asarray(lm.constrained).astype(np.int64)
    return SimpleNamespace(op=op, mf=op.mf_data, lm=lm, n=n, n_cells=lm.n_cells, shape=(n,), valid=slice(0, n), s=s, c=c, cells_ref=cells_ref,
                           kernel=kernel, solver=solver, deterministic=deterministic, block=False,
                           cell_loop=lambda dst, src, c0, c1: op.mf_data.cell_loop(op.coef, src, dst, c0, c1))


def _pencil(p, **kw):
    op, lm, ref = _poisson_like("poisson", p, **kw)
    return _scalar(op, lm, ref, lambda name: name.startswith(f"apply_pencil_kernel<{p},"))


def _interior_first():
    op, lm, ref = _poisson_like("poisson", 5, mesh_kw=dict(dof_numbering=2))
    return _scalar(op, lm, ref, lambda name: name.startswith("apply_pencil_kernel<5,") and name.endswith(",32>"))


def _team():
    op, lm, ref = _poisson_like("poisson", 3)
    assert op.mf_data.get_apply_variant() == 10
    return _scalar(op, lm, ref, lambda name: name.startswith("apply_team_kernel"))


def _march():
    op, lm, ref = _poisson_like("poisson", 2, cells=(5, 3, 6), mesh_kw=dict(deform_amp=0.03))
    op.mf_data.set_apply_variant(70)
    return _scalar(op, lm, ref, lambda name: name.startswith("apply_march_kernel"))


def _brick_family(kind, lattice, wgs, streaming=None, cells=(8, 4, 4)):
    op, lm, ref = _poisson_like(kind, 4, cells=cells, brick=True)
    _block(op, lattice, wgs, streaming)

    def kernel(name):
        if kind not in ("poisson", "f32"):
            return name.startswith("apply_block_kernel<4,")
        if not name.startswith("apply_block_kernel<4,false,32,1,"):
            return False
        b = bits(name)
        return bool(b & LATT) == bool(lattice) and (streaming is None or kind != "poisson" or bool(b & NT) == bool(streaming))
    f = _scalar(op, lm, ref, kernel, solver=pkg.SolverCGFullMerge, deterministic=True, seed=61)
    f.range = (int(op.mf_data.mesh.cell_block_offsets[1]), lm.n_cells)       # forced variant 56: ranges are unions of whole bricks
    assert 0 < f.range[0] < f.range[1]
    return f


def _kind(kind, p, kernel_prefix, **kw):
    op, lm, ref = _poisson_like(kind, p, **kw)
    return _scalar(op, lm, ref, lambda name: name.startswith(kernel_prefix))


def _hanging():
    m = O.HangingBrickMesh(2, 2, 2, 1, 3, H=0.5, deform_amp=0.03)
    _, _, w, N, D = O.shape_tables(2, 0)
    coef = O.merged_metric(m, N, D, w, O.kappa_step64)
    op = pkg.PoissonOperator(_hanging_namespace(m), 0, pkg.COEF_STEP64)
    assert op.mf_data.get_apply_variant() == 90 and (m.constraint_mask != 0).any()
    return _scalar(op, m, lambda s, c0, c1, dst: O.apply_cells(m, coef, N, D, s, cell_range=(c0, c1), dst=dst),
                   lambda name: name.startswith("apply_pencil_kernel<2,"))


def _padded(values, n, pad=SENTINEL):
    """(rows, ld) array: the rows' first n entries hold `values`, the padding behind them the sentinel"""
    values = np.asarray(values)
    out = np.full((values.shape[0], n + (n & 1) + EXTRA), pad)
    out[:, :n] = values[:, :n]
    return out


def _components(nc):
    op, lm, ref = _poisson_like("poisson", 2)
    n = lm.n_dofs
    s = _padded(np.stack([O.deterministic_src(n, seed=21 + c) for c in range(nc)]), n)

    def cells_ref(src, c0, c1, dst):
        return np.stack([ref(src[c, :n].copy(), c0, c1, dst[c, :n].copy()) for c in range(nc)])
    f = _scalar(op, lm, cells_ref, lambda name: name.startswith("apply_pencil_components_kernel<2,false,"))
    f.shape, f.valid, f.s, f.block, f.cell_loop = s.shape, (slice(None), slice(0, n)), s, True, None
    return f


def _elasticity(p):
    pr = ER.Problem(p, SMALL, 0, deform_amp=AMP, kappa=O.kappa_step64)
    op = pkg.ElasticityOperator(pkg.BrickMesh(p, SMALL, deform_amp=AMP), 0, pkg.COEF_STEP64, lam=ER.LAME[0][0], mu=ER.LAME[0][1])
    n = pr.mesh.n_dofs
    assert n == op.mf_data.n_local
    s = _padded(np.stack([O.deterministic_src(n, seed=60 + c) for c in range(3)]), n)
    f = _scalar(op, pr.mesh, lambda src, c0, c1, dst: pr.apply_cells(src[:, :n], (c0, c1), dst[:, :n].copy()),
                lambda name: name.startswith(f"apply_pencil_elasticity_kernel<{p},false,"))
    f.shape, f.valid, f.s, f.block, f.pr = s.shape, (slice(None), slice(0, n)), s, True, pr
    f.cell_loop = lambda dst, src, c0, c1: op.cell_loop(src, dst, c0, c1)
    return f


FAMILIES = {
    "pencil p=2": lambda: _pencil(2),
    "pencil p=8": lambda: _pencil(8),
    "pencil p=5 interior stores": _interior_first,
    "team p=3": _team,
    "march p=2": _march,
    "block packed": lambda: _brick_family("poisson", 0, 2),
    "block lattice": lambda: _brick_family("poisson", 1, 8),
    "block lattice non-temporal": lambda: _brick_family("poisson", 1, 2, streaming=1),
    "helmholtz pencil": lambda: _kind("helmholtz", 2, "apply_pencil_kernel<2,"),
    "helmholtz block": lambda: _brick_family("helmholtz", 1, 8),
    "mass pencil": lambda: _kind("mass", 2, "apply_pencil_mass_kernel<2,false,"),
    "mass block": lambda: _brick_family("mass", 0, 8),
    "mass collocation": lambda: _kind("mass", 2, "apply_pencil_mass_kernel<2,true,", quad=1),
    "overint poisson": lambda: _kind("overint", 2, "apply_pencil_q_kernel<2,"),
    "overint mass": lambda: _kind("overint_mass", 2, "apply_pencil_mass_q_kernel<2,"),
    "f32 pencil": lambda: _kind("f32", 2, "apply_pencil_kernel<2,"),
    "f32 block": lambda: _brick_family("f32", 1, 8),
    "affine": lambda: _kind("affine", 2, "apply_pencil_kernel<2,"),
    "hanging": _hanging,
    "components n=1": lambda: _components(1),
    "components n=3": lambda: _components(3),
    "elasticity p=2": lambda: _elasticity(2),
    "elasticity p=4": lambda: _elasticity(4),
}


def family(name, stream=None, fresh=False):
    """the family's handle on `stream` (None: S1; 0: the null stream), built once per process unless fresh"""
    key = (name, "S" if stream is None else stream)
    if fresh or key not in _cache:
        if stream == 0:
            f = FAMILIES[name]()
        else:
            with torch.cuda.stream(S1() if stream is None else stream):
                f = FAMILIES[name]()
                torch.cuda.synchronize()
        assert f.mf.stream == (0 if stream == 0 else (S1() if stream is None else stream).cuda_stream)
        if fresh:
            return f
        _cache[key] = f
    return _cache[key]


def tensors(f, good, stream=None):
    """(working tensor, staging tensor) of one vector of the family"""
    with torch.cuda.stream(stream or S1()):
        g = on_device(np.asarray(good).reshape(f.shape))
        return torch.empty_like(g), g


def pre_content(f, values=None):
    """staging of an output: NaN (overwrite) or `values` (accumulate) in the valid entries, the sentinel in the padding"""
    out = np.full(f.shape, SENTINEL)
    out[f.valid] = NAN if values is None else np.asarray(values)[f.valid]
    return out


def protocol(S, inputs, outputs, call, check, asynchronous):
    """the case once; an asynchronous entry point twice: the second, warmed call has to return while the hold lasts"""
    for warmed in ((False, True) if asynchronous else (False,)):
        got, value = SH.run(S, inputs, outputs, call, asynchronous=warmed, scale=1.0 if warmed else 2.0)   # (a first call may build a plan on the host)
        check([g.cpu().numpy() for g in got], value)


def check_kernel(f):
    """the kernel a one-iteration solve on the handle reports"""
    with torch.cuda.stream(S1()):
        ctl = pkg.IterationNumberControl(1, 0.0)
        b = torch.ones(f.shape, dtype=torch.float64, device="cuda:0")
        x = torch.zeros_like(b)
        (pkg.SolverCG if f.block else f.solver)(ctl).solve(f.op, x, b, pkg.DiagonalMatrix())
    assert ctl.last_step() == 1 and f.kernel(ctl.apply_kernel), ctl.apply_kernel


def want_of(f, mode, pre):
    """the reference of one application in `mode`: (c0, c1), expected valid entries"""
    c0, c1 = getattr(f, "range", (1, f.n_cells - 1)) if mode == "cell_loop" else (0, f.n_cells)
    base = np.zeros(f.shape) if mode == "overwrite" else np.array(pre)
    want = np.array(f.cells_ref(f.s, c0, c1, base), dtype=np.float64)
    want = want.reshape(-1, f.n) if f.block else want
    if mode != "cell_loop":
        src = f.s[f.valid]
        if f.block:
            want[:, f.c] = src[:, f.c]
        else:
            want[f.c] = src[f.c]
    return (c0, c1), want


def apply_case(f, mode, S=None, asynchronous=True, pre=None):
    """one operator application through the protocol; returns the output of the last pass (valid entries and padding)"""
    S = S or S1()
    rng = np.random.default_rng(20240607)
    if pre is None:
        pre = rng.choice([-1.0, 1.0], f.shape) * rng.uniform(0.5, 1.0, f.shape)
    (c0, c1), want = want_of(f, mode, pre)
    src_w, src_g = tensors(f, f.s, S)
    dst, dst_pre = tensors(f, pre_content(f, None if mode == "overwrite" else pre), S)
    last = []

    def call():
        if mode == "cell_loop":
            f.cell_loop(dst, src_w, c0, c1)
        else:
            f.op.do_zero_out = mode == "overwrite"
            try:
                f.op.vmult(dst, src_w)
            finally:
                f.op.do_zero_out = True

    def check(got, _):
        out = got[0]
        last[:] = [out]
        valid = out[f.valid]
        assert np.isfinite(valid).all(), f"{mode}: non-finite entries -- something ran ahead of the producers"
        e = rel(valid, want) if mode == "overwrite" else rel_max(valid, want)
        print(f"{mode}: error {e:.2e}")
        assert e <= TOL_OP, (mode, e)
        if f.block:
            assert (out[:, f.n:] == SENTINEL).all(), "padding written"
    protocol(S, [(src_w, src_g)], [(dst, dst_pre)], call, check, asynchronous)
    return last[0], pre


# (block vectors have no ranged entry point: bp5_apply_components is the whole range)
APPLICATIONS = [(name, mode) for name in sorted(FAMILIES) for mode in ("overwrite", "accumulate", "cell_loop")
                if not (mode == "cell_loop" and name.startswith("components"))]


@pytest.mark.parametrize("name,mode", APPLICATIONS)
def test_operator_application(name, mode):
    """vmult overwrite, vmult accumulate (do_zero_out = False: the zero-fill is a launch of its own) and cell_loop on a ragged range.  Block kernel:
    a fresh handle per mode -- the plan is built and uploaded during the hold of the first call, the second call runs on it -- and the bits of
    the null-stream twin for the whole-range calls."""
    block_kernel = name.split()[1] == "block" if " " in name else False
    f = family(name, fresh=block_kernel)
    assert mode != "cell_loop" or f.cell_loop is not None
    out, pre = apply_case(f, mode)
    if f.deterministic and mode != "cell_loop":         # (ragged ranges add the DoFs shared across the range's ends atomically)
        twin = family(name, stream=0, fresh=True)
        src, dst = on_device(twin.s), on_device(pre_content(twin, None if mode == "overwrite" else pre))
        twin.op.do_zero_out = mode == "overwrite"
        twin.op.vmult(dst, src)
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy(), out), "not the bits of the null-stream twin"
    check_kernel(f)


# ------------------------------------------------------------------ the harness has teeth
def test_control_a_null_stream_op_during_the_hold_sees_the_poison():
    S = S1()
    with torch.cuda.stream(S):
        good = on_device(np.arange(1.0, 4097.0))
        work = torch.full_like(good, NAN)
    work * 1.0                                          # (the kernel and the null stream's memory pool exist before the hold)
    with torch.cuda.stream(S):
        torch.cuda.synchronize()
        ev = hold(S)
        work.copy_(good)
    assert held(ev)
    seen = work * 1.0                                   # the null stream: does not wait for S
    torch.cuda.default_stream().synchronize()
    assert held(ev), "the null stream waited for the side stream: the side stream is a blocking one"
    assert torch.isnan(seen).all()
    S.synchronize()
    assert torch.equal(work, good)


def test_control_a_null_stream_handle_reads_the_poison():
    """a handle deliberately created with stream = 0, inputs produced on S behind the hold: the application runs ahead of them"""
    S = S1()
    f = family("pencil p=2", stream=0)
    assert f.mf.stream == 0
    src_w, src_g = tensors(f, f.s)
    with torch.cuda.stream(S):
        dst = torch.zeros_like(src_w)
        src_w.fill_(NAN)
        torch.cuda.synchronize()
        ev = hold(S)
        src_w.copy_(src_g)
        assert held(ev)
        f.op.vmult(dst, src_w)
        torch.cuda.default_stream().synchronize()
        assert held(ev)
        out = dst.clone()
        S.synchronize()
    assert not torch.isfinite(out).any()
    f.op.vmult(dst, src_w)                              # the same call with its inputs in place
    torch.cuda.synchronize()
    _, want = want_of(f, "overwrite", None)
    assert rel(dst.cpu().numpy(), want) <= TOL_OP


# ------------------------------------------------------------------ setup and reductions
def _with_coef_as_input(f):
    """the handle's planes as a working input: (op.coef, staging copy)"""
    if "coef_good" not in vars(f):
        with torch.cuda.stream(S1()):
            f.coef_good = f.op.coef.clone()
            torch.cuda.synchronize()
    return f.op.coef, f.coef_good


def test_evaluate_coefficients_and_reference_layout():
    f = family("pencil p=2")
    lm = f.lm
    _, _, w, N, D = O.shape_tables(2, 0)
    want = O.merged_metric(lm, N, D, w, O.kappa_step64)
    with torch.cuda.stream(S1()):
        coef = torch.empty_like(f.op.coef)
        planes = torch.empty_like(coef)
    pre = torch.full_like(coef, NAN)

    def check(got, _):
        with torch.cuda.stream(S1()):
            e = rel(f.mf.coef_reference_layout(on_device(got[0])).cpu().numpy().reshape(want.shape), want)
        print(f"planes: {e:.2e}")
        assert e <= TOL_OP
    protocol(S1(), [], [(coef, pre)], lambda: f.mf.evaluate_coefficients(coef), check, True)
    # the permutation to the reference layout, its input produced behind the hold
    good = coef.clone()

    def layout():
        _lib_check(pkg.lib().bp5_mf_metric_to_reference_layout(f.mf.handle, C.c_void_p(coef.data_ptr()), C.c_void_p(planes.data_ptr())))

    def check_layout(got, _):
        assert rel(got[0].reshape(want.shape), want) <= TOL_OP
    protocol(S1(), [(coef, good)], [(planes, pre)], layout, check_layout, True)


def _lib_check(status):
    assert status == 0, pkg.lib().bp5_last_error().decode()


def test_elasticity_compute_metric():
    f = family("elasticity p=2")
    want = ER.planes_device_layout(f.pr).reshape(10, -1)
    with torch.cuda.stream(S1()):
        coef = torch.empty_like(f.op.coef)
    pre = torch.full_like(coef, NAN)

    def check(got, _):
        g = got[0].reshape(10, -1)
        e_k, e_s = rel_max(g[:9], want[:9]), rel_max(g[9], want[9])
        print(f"K {e_k:.2e}, kappa JxW {e_s:.2e}")
        assert e_k <= 1e-13 and e_s <= 1e-13
    protocol(S1(), [], [(coef, pre)], lambda: _lib_check(pkg.lib().bp5_elasticity_compute_metric(f.mf.handle, C.c_void_p(coef.data_ptr()))), check, True)


def _diagonal_reference(name, f):
    if name == "pencil p=2":
        _, _, w, N, D = O.shape_tables(2, 0)
        return O.operator_diagonal(f.lm, O.merged_metric(f.lm, N, D, w, O.kappa_step64), N, D)
    if name == "mass pencil":
        _, _, w, N, D = O.shape_tables(2, 0)
        return M.diagonal(f.lm, N, w, S=M.plane(f.lm, N, D, w, O.kappa_step64))
    if name == "overint poisson":
        return OR.Problem(2, SMALL, kappa=O.kappa_step64, mesh=f.lm).diagonal()
    if name == "hanging":
        _, _, w, N, D = O.shape_tables(2, 0)
        return O.operator_diagonal(f.lm, O.merged_metric(f.lm, N, D, w, O.kappa_step64), N, D)
    return f.pr.diagonal()


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("name", ["pencil p=2", "mass pencil", "overint poisson", "hanging", "elasticity p=2"])
def test_compute_diagonal(name, invert):
    """the planes are produced behind the hold; the zero-fill, the diagonal kernels, the Dirichlet ones and the reciprocal all follow them"""
    f = family(name)
    want = _diagonal_reference(name, f)
    want = 1.0 / want if invert else want
    coef, good = _with_coef_as_input(f)

    def check(_, d):
        d = d.cpu().numpy()
        got = d[f.valid] if f.block else d
        e = rel(got, want)
        print(f"{name} invert={invert}: {e:.2e}")
        assert e <= TOL_OP
    for warmed in (False, True):                         # asynchronous entry points (include/bp5.h): the warmed call returns during the hold
        got, d = SH.run(S1(), [(coef, good)], [], lambda: f.op.compute_diagonal(invert=invert), asynchronous=warmed)
        check(got, d)


@pytest.mark.parametrize("name", ["pencil p=2", "hanging", "block lattice"])
def test_assemble_rhs(name):
    f = family(name)
    want = O.assemble_rhs(f.lm)
    for warmed in (False, True):                         # asynchronous, as above
        _, b = SH.run(S1(), [], [], f.op.assemble_rhs, asynchronous=warmed)
        assert rel(b.cpu().numpy(), want) <= TOL_OP


def test_constrained_values():
    f = family("pencil p=2")
    pre = np.random.default_rng(3).uniform(-1, 1, f.n)
    src_w, src_g = tensors(f, f.s)
    dst, dst_pre = tensors(f, pre)
    want = pre.copy()
    want[f.c] = f.s[f.c]
    protocol(S1(), [(src_w, src_g)], [(dst, dst_pre)], lambda: f.mf.copy_constrained_values(src_w, dst),
             lambda got, _: np.testing.assert_array_equal(got[0], want), True)
    want = pre.copy()
    want[f.c] = -2.5
    protocol(S1(), [], [(dst, dst_pre)], lambda: f.mf.set_constrained_values(-2.5, dst),
             lambda got, _: np.testing.assert_array_equal(got[0], want), True)


@pytest.mark.parametrize("name", ["pencil p=2", "hanging"])
def test_l2_norm_solution(name):
    f = family(name)
    u = O.deterministic_src(f.n, seed=5)
    want = O.l2_norm_solution(f.lm, u)
    u_w, u_g = tensors(f, u)
    for both in (False, True):
        _, got = SH.run(S1(), [(u_w, u_g)], [], lambda: f.op.l2_norm_solution(u_w), hold_null=both)
        assert abs(got - want) <= 1e-12 * want, (got, want)


def test_vector_blas():
    """bp5_vec_*: the stream kernels (asynchronous) and the reductions (host-synchronous: the value comes from inputs produced behind the hold).
    Bounds from the format: a fused multiply-add rounds once where numpy rounds twice (2^-52 of the terms' magnitudes); a sum of n products
    carries at most n 2^-53 of the sum of their magnitudes, in any order."""
    f = family("pencil p=2")
    n = f.mf.mesh.n_owned
    u = 2.0 ** -52
    xs, ys = O.deterministic_src(f.n, seed=11), O.deterministic_src(f.n, seed=12)
    x, y = pkg.Vector(f.mf), pkg.Vector(f.mf)
    x_g, y_g = on_device(xs), on_device(ys)
    S = S1()

    def exact_or_fma(want, scale):
        """|got - want| <= 2^-52 scale on the owned entries (scale 0: the same bits), the entries behind them untouched"""
        def check(got, _):
            assert (np.abs(got[0][:n] - want[:n]) <= u * scale).all() and np.array_equal(got[0][n:], ys[n:])
        return check
    protocol(S, [(x.values, x_g)], [(y.values, y_g)], lambda: y.add(0.75, x), exact_or_fma(ys + 0.75 * xs, 2.0), True)
    protocol(S, [(x.values, x_g)], [(y.values, y_g)], lambda: y.equ(-1.5, x), exact_or_fma(-1.5 * xs, 0.0), True)
    protocol(S, [(x.values, x_g)], [(y.values, y_g)], lambda: y.sadd(0.5, 0.75, x), exact_or_fma(0.5 * ys + 0.75 * xs, 2.0), True)
    protocol(S, [], [(y.values, y_g)], lambda: y.assign(3.25), lambda got, _: np.testing.assert_array_equal(got[0], np.full(f.n, 3.25)), True)
    # reductions
    L = pkg.lib()

    def dot():
        r = C.c_double()
        _lib_check(L.bp5_vec_dot(f.mf.handle, C.c_void_p(x.values.data_ptr()), C.c_void_p(y.values.data_ptr()), n, C.byref(r)))
        return r.value
    for both in (False, True):
        _, got = SH.run(S, [(x.values, x_g), (y.values, y_g)], [], dot, hold_null=both)
        assert abs(got - xs[:n] @ ys[:n]) <= n * u * np.abs(xs[:n] * ys[:n]).sum()
        _, got = SH.run(S, [(x.values, x_g)], [], x.l2_norm, hold_null=both)
        assert abs(got - np.linalg.norm(xs[:n])) <= n * u * np.linalg.norm(xs[:n])
        _, got = SH.run(S, [(x.values, x_g)], [], x.all_zero, hold_null=both)
        assert got is False
        _, got = SH.run(S, [(x.values, torch.zeros_like(x_g))], [], x.all_zero)
        assert got is True


# ------------------------------------------------------------------ solvers
def _operator_of(f):
    def A(v):
        d = f.cells_ref(v, 0, f.n_cells, np.zeros(f.shape))
        d[f.c] = v[f.c]
        return d
    return A


def _solve_case(f, solver, b_np, inv_np, control, reference, tol, check_every=0, twin=None, S=None):
    """A x = b with b (and the inverse diagonal) produced behind the hold; x is NaN until the solver writes it.  The solve returns host
    values: it has to wait for the hold.  Returns the control."""
    S = S or S1()
    b_w, b_g = tensors(f, b_np, S)
    x, x_pre = tensors(f, pre_content(f), S)
    inputs = [(b_w, b_g)]
    d_w = None
    if inv_np is not None:
        d_w, d_g = tensors(f, inv_np, S)
        inputs.append((d_w, d_g))
    ctl = []

    def call():
        ctl[:] = [control()]
        solver(ctl[0], check_every=check_every).solve(f.op, x, b_w, pkg.DiagonalMatrix(d_w))
    outs = []
    for both in (False, True):                           # (also: the first solve on a handle allocates its workspace, the second is the warmed one)
        got, _v = SH.run(S, inputs, [(x, x_pre)], call, hold_null=both)
        out = got[0].cpu().numpy()
        outs.append(out)
        xr, k = reference
        assert ctl[0].last_step() == k, (ctl[0].last_step(), k)
        e = rel(out[f.valid], xr)
        print(f"{solver.__name__} check_every={check_every}: {k} iterations, error {e:.2e}, kernel {ctl[0].apply_kernel}")
        assert e <= tol, e
        if f.block:
            assert (out[:, f.n:] == SENTINEL).all()
    if twin is not None:
        assert np.array_equal(outs[0], outs[1])
        bt, xt = on_device(np.asarray(b_np).reshape(twin.shape)), on_device(pre_content(twin))
        c = control()
        solver(c, check_every=check_every).solve(twin.op, xt, bt, pkg.DiagonalMatrix(on_device(inv_np) if inv_np is not None else None))
        torch.cuda.synchronize()
        assert np.array_equal(xt.cpu().numpy(), outs[1]), "not the bits of the null-stream twin"
    return ctl[0]


def _scalar_problem(name):
    key = ("problem", name)
    if key not in _cache:
        f = family(name)
        A = _operator_of(f)
        b = O.assemble_rhs(f.lm)
        d = None
        if name in ("pencil p=2", "block lattice"):
            _, _, w, N, D = O.shape_tables(f.lm.p, 0)
            d = 1.0 / O.operator_diagonal(f.lm, O.merged_metric(f.lm, N, D, w, O.kappa_step64), N, D)
        _cache[key] = (f, A, b, d)
    return _cache[key]


@pytest.mark.parametrize("check_every", [0, 3])
@pytest.mark.parametrize("jacobi", [False, True])
@pytest.mark.parametrize("solver", ["SolverCG", "SolverCGFullMerge"])
@pytest.mark.parametrize("name", ["pencil p=2", "block lattice"])
def test_cg_at_a_fixed_iteration_count(name, solver, jacobi, check_every):
    f, A, b, d = _scalar_problem(name)
    iters = 8
    merged = solver == "SolverCGFullMerge"
    xr, k, _ = (O.cg_merged if merged else O.cg_plain)(A, b, iters, diag=d if jacobi else None)
    twin = family(name, stream=0) if f.deterministic and merged and not jacobi else None    # fused dot products: fixed summation orders
    ctl = _solve_case(f, getattr(pkg, solver), b, d if jacobi else None, lambda: pkg.IterationNumberControl(iters, 0.0), (xr, k), TOL_CG,
                      check_every=check_every, twin=twin)
    if name == "block lattice":
        assert ctl.apply_kernel.startswith("apply_block_kernel<4,"), ctl.apply_kernel
        if merged and not jacobi:
            assert ctl.dot_products_fused
    else:
        assert ctl.apply_kernel.startswith("apply_pencil_kernel<2,")


@pytest.mark.parametrize("check_every", [0, 3])
@pytest.mark.parametrize("solver", ["SolverCG", "SolverCGFullMerge"])
def test_cg_that_stops_on_a_tolerance(solver, check_every):
    """constant coefficient, (4, 4, 4) cells: a tolerance half way between two record lows of the oracle's own residual history (_stop_tolerance)"""
    key = "stop problem"
    if key not in _cache:
        with torch.cuda.stream(S1()):
            mesh = pkg.BrickMesh(2, (4, 4, 4), deform_amp=0.03)
            op = pkg.PoissonOperator(mesh, 0, pkg.COEF_ONE)
        lm = lm_of(mesh)
        _, _, w, N, D = O.shape_tables(2, 0)
        coef = O.merged_metric(lm, N, D, w)
        f = _scalar(op, lm, lambda s, c0, c1, dst: O.apply_cells(lm, coef, N, D, s, cell_range=(c0, c1), dst=dst), None)
        A, b = _operator_of(f), O.assemble_rhs(lm)
        k_stop, tol = _stop_tolerance(SimpleNamespace(vmult=A, rhs=lambda: b), k_min=5)
        xr, k, _ = O.cg_plain(A, b, 400, tol=tol)
        assert k == k_stop
        _cache[key] = (f, b, tol, xr, k)
    f, b, tol, xr, k = _cache[key]
    ctl = _solve_case(f, getattr(pkg, solver), b, None, lambda: pkg.SolverControl(400, tol), (xr, k), TOL_STOP, check_every=check_every)
    assert ctl.last_value() <= tol


def test_merged_cg_with_the_fused_vector_update():
    """BP5_TUNE_FUSED_UPDATE = 1 on (8, 8, 8) lattice bricks: p, r and x are updated by the operator launch"""
    def build():
        f = _brick_family("poisson", 1, 8, cells=(8, 8, 8))
        f.mf.set_tuning("fused_update", 1)
        return f
    with torch.cuda.stream(S1()):
        f = build()
        torch.cuda.synchronize()
    twin = build()
    A, b = _operator_of(f), O.assemble_rhs(f.lm)
    iters = 4
    xr, k, _ = O.cg_merged(A, b, iters)
    ctl = _solve_case(f, pkg.SolverCGFullMerge, b, None, lambda: pkg.IterationNumberControl(iters, 0.0), (xr, k), TOL_CG, twin=twin)
    assert ctl.dot_products_fused and bits(ctl.apply_kernel) & FUSED_UPDATE, ctl.apply_kernel


@pytest.mark.parametrize("jacobi", [False, True])
def test_components_cg(jacobi):
    f = family("components n=3")
    _, A1, b1, d = _scalar_problem("pencil p=2")
    B = CoR.rhs_blocks(b1, 3)
    iters = 8
    xr, k, _ = CoR.cg(A1, B, iters, inv_diag=d if jacobi else None)
    S = S1()
    b_w, b_g = tensors(f, _padded(B, f.n), S)
    x, x_pre = tensors(f, pre_content(f), S)
    inputs = [(b_w, b_g)]
    d_w = None
    if jacobi:
        with torch.cuda.stream(S):
            d_g = on_device(d)
            d_w = torch.empty_like(d_g)
        inputs.append((d_w, d_g))
    for both in (False, True):
        ctl = pkg.IterationNumberControl(iters, 0.0)
        got, _v = SH.run(S, inputs, [(x, x_pre)], lambda: pkg.SolverCG(ctl).solve(f.op, x, b_w, pkg.DiagonalMatrix(d_w)), hold_null=both)
        out = got[0].cpu().numpy()
        e = max(rel(out[c, :f.n], xr[c]) for c in range(3))
        print(f"components CG jacobi={jacobi}: {e:.2e}")
        assert ctl.last_step() == k == iters and e <= TOL_CG
        assert (out[:, f.n:] == SENTINEL).all() and ctl.apply_kernel.startswith("apply_pencil_components_kernel<2,false,")


@pytest.mark.parametrize("jacobi", [False, True])
def test_elasticity_cg(jacobi):
    f = family("elasticity p=2")
    pr = f.pr
    B = pr.body_force_rhs((0.3, -0.2, -1.0))
    inv = 1.0 / pr.diagonal() if jacobi else None
    iters = 8
    xr, k, _ = ER.cg(pr.vmult, B, iters, inv_diag=inv)
    _solve_case(f, pkg.SolverCG, _padded(B, f.n), _padded(inv, f.n) if jacobi else None, lambda: pkg.IterationNumberControl(iters, 0.0),
                (xr, k), TOL_CG)


def _chebyshev_problem():
    f, A, b, d = _scalar_problem("pencil p=2")
    v = CR.start_vector(f.mf.mesh.global_ids, f.mf.mesh.constrained)
    return f, A, d, v


@pytest.mark.parametrize("path", ["native", "callback"])
def test_chebyshev(path):
    """initialize: the Lanczos estimate (its history comes back through a legacy copy) with the inverse diagonal produced behind the hold; then
    vmult and step (asynchronous).  callback: the operator is a Python object, its vmult enqueues on torch's current stream"""
    f, A, d, v = _chebyshev_problem()
    S = S1()
    op = f.op if path == "native" else _PyOperator(f.op)
    with torch.cuda.stream(S):
        d_g = on_device(d)
        d_w = torch.empty_like(d_g)
    its, srange, degree = 8, 20.0, 4
    lo, hi, k = CR.lanczos_estimate(A, d, v, its)
    for both in (False, True):
        _, ch = SH.run(S, [(d_w, d_g)], [], lambda: pkg.PreconditionChebyshev().initialize(
            op, pkg.PreconditionChebyshev.AdditionalData(degree=degree, smoothing_range=srange, eig_cg_n_iterations=its, preconditioner=pkg.DiagonalMatrix(d_w))),
            hold_null=both)
        e = ch.estimated_eigenvalues()
        print(f"{path}: estimate [{e['min_est']:.6f}, {e['max_est']:.6f}], numpy [{lo:.6f}, {hi:.6f}]")
        assert e["cg_its"] == k and abs(e["min_est"] - lo) <= TOL_EST * lo and abs(e["max_est"] - hi) <= TOL_EST * hi, (e, lo, hi)
        mu, Mu = CR.bounds(lo, hi, srange)
        assert abs(e["min_used"] - mu) <= TOL_EST * mu and abs(e["max_used"] - Mu) <= TOL_EST * Mu
    src = O.deterministic_src(f.n, seed=31)
    x0 = O.deterministic_src(f.n, seed=131)
    s_w, s_g = tensors(f, src)
    dst, nan_pre = tensors(f, pre_content(f))
    _, x0_g = tensors(f, x0)
    want = CR.vmult(A, d, src, e["min_used"], e["max_used"], degree)
    protocol(S, [(s_w, s_g), (d_w, d_g)], [(dst, nan_pre)], lambda: ch.vmult(dst, s_w), lambda got, _: _assert_rel(got[0], want, TOL_CHEB), path == "native")
    want = CR.step(A, d, x0, src, e["min_used"], e["max_used"], degree)
    protocol(S, [(s_w, s_g), (d_w, d_g)], [(dst, x0_g)], lambda: ch.step(dst, s_w), lambda got, _: _assert_rel(got[0], want, TOL_CHEB), path == "native")
    if path == "callback":                               # ... and CG over the callback operator (bp5_cg_solve_operator)
        b = O.assemble_rhs(f.lm)
        xr, kk, _ = O.cg_plain(A, b, 8)
        g = SimpleNamespace(**{**vars(f), "op": op})
        _solve_case(g, pkg.SolverCG, b, None, lambda: pkg.IterationNumberControl(8, 0.0), (xr, kk), TOL_CG)


def _assert_rel(got, want, tol):
    assert np.isfinite(got).all()
    e = rel(got, want)
    print(f"error {e:.2e}")
    assert e <= tol, e


MG_CELLS, MG_AMP, MG_COARSE = (4, 4, 4), 0.05, 10


def _mg(precision, stream):
    """fine operator (p = 4, (4, 4, 4) cells) on `stream`, the hierarchy below it with one geometric level, the preconditioner and its numpy twin"""
    with torch.cuda.stream(stream):
        fine = pkg.PoissonOperator(pkg.BrickMesh(4, MG_CELLS, deform_amp=MG_AMP), pkg.QUAD_GAUSS, pkg.COEF_STEP64)
        ops = pkg.make_mg_hierarchy(fine, h_levels=1, min_cells=2, metric_precision=precision)
        assert [(o.mf_data.mesh.degree, o.mf_data.mesh.cells) for o in ops] == [(4, MG_CELLS), (2, MG_CELLS), (1, MG_CELLS), (1, (2, 2, 2))]
        assert all(o.mf_data.stream == stream.cuda_stream for o in ops)
        mg = pkg.PreconditionMG(ops, pkg.PreconditionMG.AdditionalData(coarse_degree=MG_COARSE))
        torch.cuda.synchronize()
        if precision == "float32":
            planes = [F.planes_to_lexicographic(o.mf_data.mesh, _planes(o)) for o in ops]
            V = F.VCycle(4, MG_CELLS, deform_amp=MG_AMP, kappa=O.kappa_step64, h_levels=1, min_cells=2, planes=planes, coarse_degree=MG_COARSE)
        else:
            V = H.HybridVCycle(4, MG_CELLS, deform_amp=MG_AMP, kappa=O.kappa_step64, h_levels=1, min_cells=2, coarse_degree=MG_COARSE)
    return fine, ops, mg, V


def _mg_cases(fine, ops, mg, V, S):
    """one V-cycle and MG-PCG through the protocol (lexicographic mesh: the library's numbering is the oracle's)"""
    pr = O.Problem(4, MG_CELLS, O.QUAD_GAUSS, deform_amp=MG_AMP, kappa=O.kappa_step64)
    n = pr.mesh.n_dofs
    assert n == fine.mf_data.n_local and np.array_equal(fine.mf_data.mesh.global_ids[:n].astype(np.int64), np.arange(n))
    f = SimpleNamespace(shape=(n,), valid=slice(0, n), n=n, op=fine, block=False, deterministic=False)
    s = O.deterministic_src(n, pr.mesh.constrained, seed=41)
    s_w, s_g = tensors(f, s, S)
    dst, nan_pre = tensors(f, pre_content(f), S)
    want = V.vmult(s)
    protocol(S, [(s_w, s_g)], [(dst, nan_pre)], lambda: mg.vmult(dst, s_w), lambda got, _: _assert_rel(got[0], want, TOL_MG), True)
    b = pr.rhs()
    tol = 1e-8 * np.linalg.norm(b)
    xr, k_ref, _ = CR.pcg(pr.vmult, V.vmult, b, 300, tol=tol)
    b_w, b_g = tensors(f, b, S)
    for both in (False, True):
        ctl = pkg.SolverControl(300, tol)
        got, _v = SH.run(S, [(b_w, b_g)], [(dst, nan_pre)], lambda: pkg.SolverCG(ctl).solve(fine, dst, b_w, mg), hold_null=both)
        print(f"MG-PCG: {ctl.last_step()} iterations (numpy {k_ref})")
        assert abs(ctl.last_step() - k_ref) <= 1 and ctl.last_value() <= tol
        assert rel(got[0].cpu().numpy(), xr) < 1e-7


@pytest.mark.parametrize("precision", [None, "float32"])
def test_multigrid(precision):
    S = S1()
    fine, ops, mg, V = _mg(precision, S)
    _mg_cases(fine, ops, mg, V, S)
    mg.clear()


def test_make_mg_hierarchy_takes_the_fine_operators_stream():
    """fine_op on S while torch's current stream is the null stream: the levels follow fine_op, and the hierarchy works"""
    S = S1()
    fine = pkg.PoissonOperator(pkg.BrickMesh(4, MG_CELLS, deform_amp=MG_AMP), pkg.QUAD_GAUSS, pkg.COEF_STEP64, stream=S)
    assert torch.cuda.current_stream() == torch.cuda.default_stream() and fine.mf_data.stream == S.cuda_stream
    for precision in (None, "float32"):
        ops = pkg.make_mg_hierarchy(fine, h_levels=1, min_cells=2, metric_precision=precision)
        assert len(ops) == 4 and all(o.mf_data.stream == S.cuda_stream for o in ops)
        torch.cuda.synchronize()
        mg = pkg.PreconditionMG(ops, pkg.PreconditionMG.AdditionalData(coarse_degree=MG_COARSE))
        if precision is None:
            V = H.HybridVCycle(4, MG_CELLS, deform_amp=MG_AMP, kappa=O.kappa_step64, h_levels=1, min_cells=2, coarse_degree=MG_COARSE)
            s = O.deterministic_src(fine.mf_data.n_local, fine.mf_data.mesh.constrained, seed=41)
            with torch.cuda.stream(S):
                dst = torch.full((s.size,), NAN, dtype=torch.float64, device="cuda:0")
                mg.vmult(dst, on_device(s))
                S.synchronize()
            _assert_rel(dst.cpu().numpy(), V.vmult(s), TOL_MG)
        mg.clear()


def test_levels_on_different_streams_are_refused():
    S = S1()
    with torch.cuda.stream(S):
        fine = pkg.PoissonOperator(pkg.BrickMesh(2, MG_CELLS), pkg.QUAD_GAUSS, pkg.COEF_ONE)
        ops = pkg.make_mg_hierarchy(fine)
        torch.cuda.synchronize()
    mg = pkg.PreconditionMG(ops)
    ops[1].mf_data.set_stream(S2())
    with pytest.raises(pkg.BP5Error) as e:
        pkg.PreconditionMG(ops)
    assert e.value.status == 1 and "one stream" in str(e.value)
    # the library's own check (bp5_mg_create), with the transfers built while the streams agreed
    n = len(ops)
    mfs = (C.c_void_p * n)(*[o.mf_data.handle.value for o in ops])
    coefs = (C.c_void_p * n)(*[o.coef.data_ptr() for o in ops])
    trs = (C.c_void_p * (n - 1))(*[t.handle.value for t in mg.transfers])
    prm = pkg._lib.MGParams(4, 20.0, 10, 60, 1000.0, 30, None)
    h = C.c_void_p()
    assert pkg.lib().bp5_mg_create(n, mfs, coefs, trs, C.byref(prm), C.byref(h)) == 1 and not h
    assert "one stream" in pkg.lib().bp5_last_error().decode()
    ops[1].mf_data.set_stream(S)
    pkg.PreconditionMG(ops).clear()
    mg.clear()


# ------------------------------------------------------------------ bp5_mf_set_stream
def test_set_stream_moves_everything_built_on_the_handle():
    """a handle used on the null stream -- plans, CG workspaces, the communication stream, a Chebyshev object exist -- then moved to S, to a second
    side stream and back to 0: an application, a merged solve and the Chebyshev vmult each time"""
    f = family("block lattice", stream=0, fresh=True)
    _, A, b, d = _scalar_problem("block lattice")
    xr, k, _ = O.cg_merged(A, b, 6)
    mf = f.mf
    mf.wait_value_available()                          # creates the communication stream
    x = on_device(np.zeros(f.n))
    pkg.SolverCGFullMerge(pkg.IterationNumberControl(6, 0.0)).solve(f.op, x, on_device(b), pkg.DiagonalMatrix())
    inv = on_device(d)
    ch = pkg.PreconditionChebyshev().initialize(f.op, pkg.PreconditionChebyshev.AdditionalData(degree=3, max_eigenvalue=2.1, min_eigenvalue=0.15, preconditioner=pkg.DiagonalMatrix(inv)))
    torch.cuda.synchronize()
    x0 = x.cpu().numpy()
    assert rel(x0, xr) <= TOL_CG
    src = O.deterministic_src(f.n, seed=31)
    want_ch = CR.vmult(A, d, src, 0.15, 2.1, 3)
    for S in (S1(), S2()):
        torch.cuda.synchronize()
        mf.set_stream(S)
        assert mf.stream == S.cuda_stream
        out, _ = apply_case(f, "overwrite", S=S)
        _solve_case(f, pkg.SolverCGFullMerge, b, None, lambda: pkg.IterationNumberControl(6, 0.0), (x0, k), 0.0, S=S)     # the bits of the null-stream solve
        s_w, s_g = tensors(f, src, S)
        dst, nan_pre = tensors(f, pre_content(f), S)
        protocol(S, [(s_w, s_g)], [(dst, nan_pre)], lambda: ch.vmult(dst, s_w), lambda got, _: _assert_rel(got[0], want_ch, TOL_CHEB), True)
    torch.cuda.synchronize()
    with pytest.raises(pkg.BP5Error):
        mf.set_stream(None)                            # (None is torch's current stream in reinit: never a silent move)
    mf.set_stream(0)
    assert mf.stream == 0
    dst = on_device(np.full(f.n, NAN))
    f.op.vmult(dst, on_device(f.s))
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), out)
    ch.clear()


def test_set_stream_moves_a_hierarchy():
    fine, ops, mg, V = _mg(None, S1())
    torch.cuda.synchronize()
    for o in ops:
        o.mf_data.set_stream(S2())
    _mg_cases(fine, ops, mg, V, S2())
    mg.clear()


# ------------------------------------------------------------------ two handles, two streams
def test_two_handles_on_two_streams_do_not_wait_for_each_other():
    """A on S1, held; B (another mesh and degree) on S2, free and warmed.  A's vmult is enqueued behind the hold; B's ten-iteration solve runs to
    completion on the host meanwhile: a warmed solve synchronises its own stream only and neither allocates nor frees (include/bp5.h)."""
    A = family("pencil p=2")
    with torch.cuda.stream(S2()):
        mesh = pkg.BrickMesh(3, (4, 3, 3), deform_amp=0.03)
        opB = pkg.PoissonOperator(mesh, 0, pkg.COEF_STEP64)
        lmB = lm_of(mesh)
        bB = opB.assemble_rhs()
        xB = opB.initialize_dof_vector()
        solve = lambda: pkg.SolverCG(pkg.IterationNumberControl(10, 0.0)).solve(opB, xB, bB, pkg.DiagonalMatrix())   # noqa: E731
        solve()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solve()
        solve_ms = 1e3 * (time.perf_counter() - t0)
    scale = max(1.0, 20.0 * solve_ms / SH.HOLD_MS)
    print(f"B's warmed ten-iteration solve: {solve_ms:.2f} ms; A's hold: {scale * SH.HOLD_MS:.0f} ms")
    assert scale * SH.HOLD_MS <= 2000.0, "B's solve is far slower than it should be: the hold would not be a short one"
    _, _, w, N, D = O.shape_tables(3, 0)
    coefB = O.merged_metric(lmB, N, D, w, O.kappa_step64)
    cB = lmB.constrained.astype(np.int64)

    def AB(v):
        d = O.apply_cells(lmB, coefB, N, D, v)
        d[cB] = v[cB]
        return d
    xr, _, _ = O.cg_plain(AB, O.assemble_rhs(lmB), 10)
    _, want = want_of(A, "overwrite", None)
    src_w, src_g = tensors(A, A.s)
    with torch.cuda.stream(S1()):
        dst = torch.empty_like(src_w)
        src_w.fill_(NAN)
        torch.cuda.synchronize()
        evA = hold(S1(), scale)
        src_w.copy_(src_g)
        dst.fill_(NAN)
        assert held(evA)
        A.op.vmult(dst, src_w)
        assert held(evA)
    with torch.cuda.stream(S2()):
        solve()
    assert held(evA), "B's solve waited for A's stream"
    S1().synchronize()
    S2().synchronize()
    assert rel(dst.cpu().numpy(), want) <= TOL_OP and rel(xB.cpu().numpy(), xr) <= TOL_CG
