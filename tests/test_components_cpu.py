"""CPU checks of block vectors (bp5_apply_components, bp5_cg_solve_components; CEED BP6): the entry points exist and validate their arguments
before anything touches a device, and the numpy statement of the stacked CG (tests/components_ref.py) that the GPU tests compare against means
what they rely on -- one Krylov space is NOT three separate solves, but it is the scalar solve when the right-hand sides coincide."""
import ctypes as C

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import components_ref as R

pkg = bp5_pkg.load()
INVALID, NO_DEVICE = 1, 3
_cache = {}


def _config1():
    if "c1" not in _cache:
        pr = O.Problem(2, (8, 8, 8), O.QUAD_GAUSS)       # BASELINE config 1: p = 2, 8^3 cells, kappa = 1, no deformation
        _cache["c1"] = (pr, pr.rhs())
    return _cache["c1"]


def diag_case(n_components=3):
    """the preconditioned fixed-iteration case of the GPU test: p = 4, (4,4,4), deformed, step-64 kappa, inverse diagonal, 10 iterations"""
    if "d" not in _cache:
        pr = O.Problem(4, (4, 4, 4), O.QUAD_GAUSS, deform_amp=0.04, kappa=O.kappa_step64)
        inv = 1.0 / O.operator_diagonal(pr.mesh, pr.coef, pr.N, pr.D)
        _cache["d"] = (pr, pr.rhs(), inv)
    pr, b, inv = _cache["d"]
    return pr, R.rhs_blocks(b, n_components), inv


EDGES = [(3, 1), (8, 6)]       # (components, the block whose right-hand side is zeroed) of the GPU tests of the solver's edges


def zero_block_case(n_components, zeroed):
    """diag_case with one right-hand side zeroed"""
    pr, B, inv = diag_case(n_components)
    B[zeroed] = 0.0
    return pr, B, inv


# the solves the GPU test runs one after the other on one handle: (components, ld - n_local rounded up to even, with the inverse diagonal)
SEQUENCE, SEQUENCE_CELLS, SEQUENCE_ITERATIONS = ((2, 2, False), (8, 2, True), (3, 64, True), (2, 2, False)), (8, 8, 4), 5


def sequence_case():
    """p = 4, (8,8,4), deformed, step-64 kappa: (problem, scalar right-hand side, inverse diagonal)"""
    if "seq" not in _cache:
        pr = O.Problem(4, SEQUENCE_CELLS, O.QUAD_GAUSS, deform_amp=0.04, kappa=O.kappa_step64)
        _cache["seq"] = (pr, pr.rhs(), 1.0 / O.operator_diagonal(pr.mesh, pr.coef, pr.N, pr.D))
    return _cache["seq"]


CAPPED_CELLS, CAPPED_ITERATIONS = (21, 21, 21), 3


def capped_case():
    """the case of the GPU test at the capped grid: p = 4, Gauss, (21,21,21) cells = 85^3 DoFs, deformed, step-64 kappa; (problem, scalar
    right-hand side, inverse diagonal), built once per process"""
    if "capped" not in _cache:
        pr = O.Problem(4, CAPPED_CELLS, O.QUAD_GAUSS, deform_amp=0.04, kappa=O.kappa_step64)
        b, inv = pr.rhs(), 1.0 / O.operator_diagonal(pr.mesh, pr.coef, pr.N, pr.D)
        for a in (b, inv):
            a.setflags(write=False)
        _cache["capped"] = (pr, b, inv)
    return _cache["capped"]


def test_symbols_are_exported_and_listed():
    L = pkg.lib()
    for s in ("bp5_apply_components", "bp5_cg_solve_components"):
        assert s in pkg.HEADER_SYMBOLS and hasattr(L, s) and s in L._protos
    from deal_and_ceed_on_gpu_amd import _lib
    text = open(bp5_pkg.ROOT + "/include/bp5.h").read()
    assert "#define BP5_MAX_COMPONENTS 8" in text and _lib.MAX_COMPONENTS == 8


def _buffers():
    """two 16-byte aligned host buffers: the refusals under test are decided before any pointer is dereferenced"""
    a = np.zeros(64 + 2)
    off = (-a.ctypes.data // 8) % 2
    return a.ctypes.data + 8 * off, a.ctypes.data + 8 * off + 8 * 32, a


def test_invalid_arguments_are_refused_without_a_device():
    """Every BP5_ERR_INVALID refusal that can be stated without a handle (ld < n_local needs one: tests/test_gpu_components.py), each with its
    reason in bp5_last_error.  The layout checks come before the handle is looked at, so a NULL handle does not mask them."""
    L = pkg.lib()
    from deal_and_ceed_on_gpu_amd import _lib
    src, dst, keep = _buffers()
    null = C.c_void_p()
    prm, res = _lib.CGParams(_lib.CG_PLAIN, 10, 0.0, 0, 0), _lib.CGResult()

    def apply(nc=3, ld=8, s=src, d=dst, mf=null):
        st = L.bp5_apply_components(mf, C.c_void_p(src), nc, ld, C.c_void_p(s) if s else None, C.c_void_p(d) if d else None, 1)
        return st, L.bp5_last_error().decode()

    def solve(nc=3, ld=8, b=src, x=dst, p=prm, r=res):
        st = L.bp5_cg_solve_components(null, C.c_void_p(src), nc, ld, None, C.c_void_p(b) if b else None, C.c_void_p(x) if x else None,
                                       C.byref(p) if p is not None else None, C.byref(r) if r is not None else None)
        return st, L.bp5_last_error().decode()

    for fn in (apply, solve):
        for kw, word in ((dict(nc=0), "n_components"), (dict(nc=9), "n_components"), (dict(nc=-1), "n_components"), (dict(ld=7), "even"),
                         (dict(**{"s" if fn is apply else "b": src + 8}), "aligned"), (dict(**{"d" if fn is apply else "x": dst + 8}), "aligned"),
                         (dict(**{"d" if fn is apply else "x": src}), "overlap"), (dict(**{"s" if fn is apply else "b": None}), "null"),
                         (dict(**{"d" if fn is apply else "x": None}), "null"), (dict(), "null handle")):
            st, msg = fn(**kw)
            assert st == INVALID and word in msg, (fn.__name__, kw, st, msg)
    assert solve(p=None)[0] == INVALID and solve(r=None)[0] == INVALID
    st, msg = solve(p=_lib.CGParams(7, 10, 0.0, 0, 0))
    assert st == INVALID and "variant" in msg, msg
    st, msg = solve(p=_lib.CGParams(_lib.CG_PLAIN, -1, 0.0, 0, 0))
    assert st == INVALID and "max_iter" in msg, msg
    del keep


def test_no_device_no_fallback():
    """A valid call needs a handle, and a machine without a GPU cannot make one: BP5_ERR_NO_DEVICE from the operator the block vector would come
    from -- there is no host path behind initialize_block_vector / vmult / SolverCG.solve."""
    import torch
    if torch.cuda.is_available():
        op = pkg.PoissonOperator(pkg.BrickMesh(2, (2, 2, 2)), pkg.QUAD_GAUSS)
        assert tuple(op.initialize_block_vector(3).shape) == (3, op.mf_data.n_local + (op.mf_data.n_local & 1))
        return
    with pytest.raises(pkg.BP5Error) as e:
        pkg.PoissonOperator(pkg.BrickMesh(2, (2, 2, 2)), pkg.QUAD_GAUSS, stream=0)     # (stream given: torch is not asked for one)
    assert e.value.status == NO_DEVICE


def test_stacked_cg_is_one_krylov_space():
    """config 1, 10 iterations, three different right-hand sides: the stacked solution is about 1e-2 away from three separate solves (a solver
    that ran independent CGs fails the GPU test's 1e-11), and with identical right-hand sides it IS the scalar solve"""
    pr, b = _config1()
    B = R.rhs_blocks(b)
    xs, k, _ = R.cg(pr.vmult, B, 10)
    xi = R.separate(pr.vmult, B, 10)
    d = np.linalg.norm(xs - xi) / np.linalg.norm(xi)
    print(f"stacked vs separate: {d:.3e}")
    assert k == 10 and 3e-3 < d < 5e-2, d
    B1 = np.stack([b, b, b])
    x1, k1, _ = R.cg(pr.vmult, B1, 10)
    x0, _, _ = O.cg_plain(pr.vmult, b, 10)
    same = max(np.linalg.norm(x1[c] - x0) / np.linalg.norm(x0) for c in range(3))
    print(f"identical right-hand sides vs scalar: {same:.3e}")
    assert k1 == 10 and same <= 1e-14, same


def test_fixed_iteration_references_are_stable_under_operator_noise():
    """The GPU test compares 10 fixed iterations to 1e-11 (TOL_CG).  That needs references that 1e-16 relative noise in the operator moves by
    far less: config 1 (measured 3e-16) and the preconditioned case p = 4 (4,4,4) with the inverse diagonal, which has to stay below 1e-13."""
    pr, b = _config1()
    d1 = R.noise_drift(pr.vmult, R.rhs_blocks(b), 10)
    prd, Bd, inv = diag_case()
    d2 = R.noise_drift(prd.vmult, Bd, 10, inv_diag=inv)
    print(f"noise drift: config 1 {d1:.3e}, p = 4 (4,4,4) with inverse diagonal {d2:.3e}")
    assert d1 < 1e-14 and d2 < 1e-13, (d1, d2)


@pytest.mark.parametrize("nc", [1, 2, 5, 8])
def test_fixed_iteration_references_are_stable_at_every_component_count(nc):
    """the same two cases with the component counts the GPU tests add: two decades under TOL_CG"""
    pr, b = _config1()
    d1 = R.noise_drift(pr.vmult, R.rhs_blocks(b, nc), 10)
    prd, Bd, inv = diag_case(nc)
    d2 = R.noise_drift(prd.vmult, Bd, 10, inv_diag=inv)
    print(f"noise drift, {nc} components: config 1 {d1:.3e}, p = 4 (4,4,4) with inverse diagonal {d2:.3e}")
    assert Bd.shape[0] == nc and d1 < 1e-13 and d2 < 1e-13, (d1, d2)


@pytest.mark.parametrize("nc,zeroed", EDGES)
def test_zero_block_reference_is_stable_under_operator_noise(nc, zeroed):
    """One right-hand side zeroed, inverse diagonal, 10 iterations: two decades under TOL_CG.  Without the preconditioner this operator
    (step-64 kappa) does not give that: the residual stagnates and the ten-iteration reference moves by 5e-13 ... 3e-12, printed here."""
    pr, B, inv = zero_block_case(nc, zeroed)
    d, plain = R.noise_drift(pr.vmult, B, 10, inv_diag=inv), R.noise_drift(pr.vmult, B, 10)
    x, _, _ = R.cg(pr.vmult, B, 10, inv_diag=inv)
    print(f"noise drift, {nc} components, block {zeroed} zero: {d:.3e} with the inverse diagonal, {plain:.3e} without")
    assert d < 1e-13 and not x[zeroed].any() and x[(zeroed + 1) % nc].any(), d


def test_sequence_references_are_stable_under_operator_noise():
    pr, b, inv = sequence_case()
    drifts = [R.noise_drift(pr.vmult, R.rhs_blocks(b, nc), SEQUENCE_ITERATIONS, inv_diag=inv if with_diag else None) for nc, _, with_diag in SEQUENCE[:3]]
    print("noise drift, the solves of the sequence on one handle:", " ".join(f"{d:.3e}" for d in drifts))
    assert max(drifts) < 1e-13, drifts


def test_one_component_tolerance_stop_reference_is_stable_under_operator_noise():
    """the GPU test compares the one-component solve that stops at 1e-8 ||b|| with the scalar solver at TOL_CG: over that many iterations (53)
    the reference has to stay two decades below it as well"""
    pr, b = _config1()
    B = R.rhs_blocks(b, 1)
    _, k, _ = R.cg(pr.vmult, B, 1000, tol=1e-8 * np.linalg.norm(B))
    d = R.noise_drift(pr.vmult, B, k)
    print(f"noise drift, config 1, one component, {k} iterations: {d:.3e}")
    assert 40 < k < 70 and d < 1e-13, (k, d)


@pytest.mark.parametrize("with_diag", [False, True])
@pytest.mark.parametrize("nc", [7, 8])
def test_capped_grid_references_are_stable_under_operator_noise(nc, with_diag):
    """The GPU test at the capped grid (85^3 DoFs, 7 and 8 components, 3 iterations, with and without the inverse diagonal) compares to
    TOL_CG = 1e-11: its references have to stay two decades below that under 1e-16 operator noise."""
    pr, b, inv = capped_case()
    d = R.noise_drift(pr.vmult, R.rhs_blocks(b, nc), CAPPED_ITERATIONS, inv_diag=inv if with_diag else None)
    print(f"noise drift, {pr.mesh.n_dofs} DoFs, {nc} components, {'inverse diagonal' if with_diag else 'no preconditioner'}: {d:.3e}")
    assert pr.mesh.n_dofs == 85 ** 3 and d < 1e-13, d
