"""CPU checks of linear elasticity (bp5_elasticity_*, bp5_cg_solve_elasticity): the numpy reference the GPU tests compare against
(tests/elasticity_ref.py) is pinned OUTSIDE itself -- rigid-body modes, exact energies of linear fields, symmetry, the dense cell matrices built
from the definition, the coupling that separates the operator from three Laplacians -- and the library side that needs no device: symbols,
prototypes, every refusal that can be stated without a handle, no CPU fallback.  The drift of every fixed-iteration CG reference of the GPU
tests under 1e-16 operator noise is asserted below 1e-13."""
import ctypes as C

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import elasticity_ref as R

pkg = bp5_pkg.load()
INVALID, NO_DEVICE, UNSUPPORTED = 1, 3, 5
MESHES = [(2, (3, 2, 2), 0.0), (2, (3, 2, 2), 0.04), (3, (2, 2, 2), 0.04)]


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.mark.parametrize("p,cells,amp", MESHES)
@pytest.mark.parametrize("quad", [O.QUAD_GAUSS, O.QUAD_GLL])
def test_rigid_body_modes_are_annihilated(p, cells, amp, quad):
    """Without Dirichlet rows the three translations and the three rotations u = omega x X lie in the null space, on the affine AND on the
    deformed mesh: the coordinate field is in the isoparametric space, so eps(u) vanishes at every quadrature point, whatever the quadrature."""
    pr = R.Problem(p, cells, quad, deform_amp=amp, kappa=O.kappa_step64, lam=10.0, mu=1.0, free=True)
    w = pr.source()
    ref = np.linalg.norm(pr.vmult(w)) / np.linalg.norm(w)
    for m, u in enumerate(pr.rigid_body_modes()):
        r = np.linalg.norm(pr.vmult(u)) / np.linalg.norm(u) / ref
        print(f"p={p} amp={amp} quad={quad} mode {m}: |A u| / |u| relative to a random source {r:.2e}")
        assert r < 1e-12, (m, r)


@pytest.mark.parametrize("p,cells,amp", MESHES)
def test_energies_of_linear_fields_are_exact(p, cells, amp):
    """u = (a x, 0, 0): (lam + 2 mu) a^2 sum kappa JxW; u = (y, 0, 0): mu sum kappa JxW -- exact on deformed cells too (u is a linear function of
    the coordinate field), through the integrate step (u.A u) and from the quadrature points"""
    lam, mu, a = 10.0, 1.0, 0.7
    pr = R.Problem(p, cells, O.QUAD_GAUSS, deform_amp=amp, kappa=O.kappa_step64, lam=lam, mu=mu, free=True)
    X = pr.mesh.coords.T
    vol = float(pr.s.sum())
    zero = np.zeros(X.shape[1])
    for u, want in ((np.stack([a * X[0], zero, zero]), (lam + 2 * mu) * a * a * vol), (np.stack([X[1], zero, zero]), mu * vol),
                    (np.stack([zero, zero, a * X[2]]), (lam + 2 * mu) * a * a * vol), (np.stack([zero, X[2], zero]), mu * vol)):
        e1, e2 = float(np.sum(u * pr.vmult(u))), pr.energy(u)
        assert abs(e1 - want) < 1e-12 * want and abs(e2 - want) < 1e-12 * want, (e1, e2, want)


@pytest.mark.parametrize("lam,mu", R.LAME)
def test_symmetry_and_positive_energy(lam, mu):
    pr = R.Problem(2, (3, 2, 2), O.QUAD_GAUSS, deform_amp=0.04, kappa=O.kappa_step64, lam=lam, mu=mu)
    u, v = pr.source(1), pr.source(2)
    Au, Av = pr.vmult(u), pr.vmult(v)
    assert abs(np.sum(v * Au) - np.sum(u * Av)) < 1e-13 * abs(np.sum(u * Au)) and np.sum(u * Au) > 0


@pytest.mark.parametrize("p,quad", [(1, 0), (2, 0), (2, 1), (3, 0), (4, 1)])
@pytest.mark.parametrize("lam,mu", R.LAME)
def test_matrix_free_apply_and_diagonal_equal_the_dense_cell_matrices(p, quad, lam, mu):
    pr = R.Problem(p, (2, 2, 1), quad, deform_amp=0.04, kappa=O.kappa_step64, lam=lam, mu=mu, free=True)    # (the cell loop: no Dirichlet rows)
    u = pr.source()
    a, b = pr.apply_cells(u), pr.apply_dense(u)
    for c in range(3):
        assert rel(a[c], b[c]) < 1e-13, (c, rel(a[c], b[c]))
    d, dd = pr.diagonal(), pr.diagonal_dense()
    assert np.abs(d - dd).max() < 1e-13 * np.abs(dd).max()
    A = pr.cell_matrix(0)
    assert np.abs(A - A.T).max() < 1e-13 * np.abs(A).max()


def test_the_operator_couples_the_components():
    """A source with only component 0 non-zero produces non-zero components 1 and 2 (lam = 10, mu = 1, deformed): three uncoupled Laplacians
    (CEED BP6) give exact zeros there"""
    pr = R.Problem(2, (3, 2, 2), O.QUAD_GAUSS, deform_amp=0.04, kappa=O.kappa_step64, lam=10.0, mu=1.0)
    u = pr.source()
    u[1:] = 0.0
    y = pr.vmult(u)
    n0 = np.linalg.norm(y[0])
    assert np.linalg.norm(y[1]) > 0.05 * n0 and np.linalg.norm(y[2]) > 0.05 * n0, [np.linalg.norm(c) for c in y]


def test_device_layout_restatement_is_a_permutation():
    for n in range(2, 10):
        q = np.arange(n ** 3)
        assert sorted(R.coef_off(n, q % n, q // n).tolist()) == q.tolist()


# ---- library side, without a device
SYMBOLS = ("bp5_elasticity_coef_size", "bp5_elasticity_compute_metric", "bp5_elasticity_apply", "bp5_elasticity_apply_cells",
           "bp5_elasticity_compute_diagonal", "bp5_cg_solve_elasticity")


def test_symbols_are_exported_and_listed():
    L = pkg.lib()
    for s in SYMBOLS:
        assert s in pkg.HEADER_SYMBOLS and hasattr(L, s) and s in L._protos, s
    assert len(L._protos["bp5_elasticity_apply"][1]) == 8 and len(L._protos["bp5_cg_solve_elasticity"][1]) == 10
    assert hasattr(pkg, "ElasticityOperator")


def _buffers():
    """two 16-byte aligned host buffers: the refusals under test are decided before any pointer is dereferenced"""
    a = np.zeros(64 + 2)
    off = (-a.ctypes.data // 8) % 2
    return a.ctypes.data + 8 * off, a.ctypes.data + 8 * off + 8 * 32, a


def test_handle_free_refusals_name_elasticity():
    """Every BP5_ERR_INVALID refusal that can be stated without a handle (ld < n_local and the BP5_ERR_UNSUPPORTED ones need one:
    tests/test_gpu_elasticity.py), each with its reason and the word "elasticity" in bp5_last_error.  Layout and parameters come before the
    handle is looked at, so a NULL handle does not mask them."""
    L = pkg.lib()
    from deal_and_ceed_on_gpu_amd import _lib
    src, dst, keep = _buffers()
    null = C.c_void_p()
    prm, res = _lib.CGParams(_lib.CG_PLAIN, 10, 0.0, 0, 0), _lib.CGResult()
    vp = lambda p: C.c_void_p(p) if p else None

    def apply(lam=1.0, mu=1.0, ld=8, s=src, d=dst):
        return L.bp5_elasticity_apply(null, vp(src), lam, mu, ld, vp(s), vp(d), 1), L.bp5_last_error().decode()

    def cells(lam=1.0, mu=1.0, ld=8, s=src, d=dst):
        return L.bp5_elasticity_apply_cells(null, vp(src), lam, mu, ld, vp(s), vp(d), 0, 1), L.bp5_last_error().decode()

    def solve(lam=1.0, mu=1.0, ld=8, s=src, d=dst, p=prm, r=res):
        st = L.bp5_cg_solve_elasticity(null, vp(src), lam, mu, ld, None, vp(s), vp(d), C.byref(p) if p is not None else None, C.byref(r) if r is not None else None)
        return st, L.bp5_last_error().decode()

    def diagonal(lam=1.0, mu=1.0, ld=8, s=None, d=dst):
        return L.bp5_elasticity_compute_diagonal(null, vp(src), lam, mu, ld, vp(d), 0), L.bp5_last_error().decode()

    common = ((dict(ld=7), "even"), (dict(d=dst + 8), "aligned"), (dict(d=None), "null"), (dict(mu=0.0), "mu"), (dict(mu=-1.0), "mu"),
              (dict(lam=-0.7, mu=1.0), "bulk"), (dict(lam=float("nan")), "finite"), (dict(mu=float("inf")), "finite"), (dict(), "null handle"))
    two = ((dict(s=src + 8), "aligned"), (dict(s=None), "null"), (dict(d=src), "overlap"))
    for fn in (apply, cells, solve, diagonal):
        for kw, word in common + (two if fn is not diagonal else ()):
            st, msg = fn(**kw)
            assert st == INVALID and word in msg and "elasticity" in msg, (fn.__name__, kw, st, msg)
    assert solve(p=None)[0] == INVALID and solve(r=None)[0] == INVALID
    for p, word in ((_lib.CGParams(7, 10, 0.0, 0, 0), "variant"), (_lib.CGParams(_lib.CG_PLAIN, -1, 0.0, 0, 0), "max_iter")):
        st, msg = solve(p=p)
        assert st == INVALID and word in msg and "elasticity" in msg, msg
    n = C.c_size_t()
    for st in (L.bp5_elasticity_coef_size(null, C.byref(n)), L.bp5_elasticity_coef_size(null, None), L.bp5_elasticity_compute_metric(null, vp(src)),
               L.bp5_elasticity_compute_metric(null, None)):
        assert st == INVALID and "elasticity" in L.bp5_last_error().decode()
    del keep


def test_no_device_no_fallback():
    """A valid call needs a handle, and a machine without a GPU cannot make one: BP5_ERR_NO_DEVICE from the operator's constructor -- there is
    no host path behind ElasticityOperator.vmult / SolverCG.solve."""
    import torch
    if torch.cuda.is_available():
        op = pkg.ElasticityOperator(pkg.BrickMesh(2, (2, 2, 2)), pkg.QUAD_GAUSS, lam=1.0, mu=1.0)
        assert tuple(op.initialize_block_vector().shape) == (3, op.mf_data.n_local + (op.mf_data.n_local & 1))
        return
    with pytest.raises(pkg.BP5Error) as e:
        pkg.ElasticityOperator(pkg.BrickMesh(2, (2, 2, 2)), pkg.QUAD_GAUSS, lam=1.0, mu=1.0, stream=0)     # (stream given: torch is not asked for one)
    assert e.value.status == NO_DEVICE


def test_python_refusals_need_no_device():
    """SolverCGFullMerge, PreconditionChebyshev and PreconditionMG refuse the operator class by name (BP5Error 5) before anything is launched"""
    op = object.__new__(pkg.ElasticityOperator)
    op.mf_data = None
    with pytest.raises(pkg.BP5Error) as e:
        pkg.PreconditionChebyshev().initialize(op)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(pkg.BP5Error) as e:
        pkg.PreconditionMG([op])
    assert e.value.status == UNSUPPORTED

    class AnyPreconditioner:
        def vmult(self, dst, src):
            raise AssertionError("never applied")
    for solver, pre in ((pkg.SolverCGFullMerge, None), (pkg.SolverCGFullMerge, pkg.DiagonalMatrix()), (pkg.SolverCGFullMerge, AnyPreconditioner()),
                        (pkg.SolverCG, AnyPreconditioner()), (pkg.SolverCG, object())):
        with pytest.raises(pkg.BP5Error) as e:
            solver(pkg.IterationNumberControl(3, 0.0)).solve(op, None, None, pre)
        assert e.value.status == UNSUPPORTED and "elasticity" in str(e.value), (solver.__name__, pre, str(e.value))


# ---- the fixed-iteration references of the GPU tests
@pytest.mark.parametrize("name", ["p2", "p4"])
def test_fixed_iteration_references_are_stable_under_operator_noise(name):
    """tests/test_gpu_elasticity.py compares fixed-iteration solves with the block inverse diagonal to 1e-11 per block: the references have to
    stay two decades below that under 1e-16 relative noise in every operator application.  Without the preconditioner the step-64 kappa does
    not give that at p = 4, printed here."""
    pr, b, inv, its = R.cg_case(name)
    d = R.noise_drift(pr.vmult, b, its, inv_diag=inv)
    plain = R.noise_drift(pr.vmult, b, its)
    x, k, res = R.cg(pr.vmult, b, its, inv_diag=inv)
    print(f"noise drift {name}: {d:.3e} with the block inverse diagonal, {plain:.3e} without; residual after {k} iterations {res:.6e}")
    assert k == its and d < 1e-13, d
    assert all(np.linalg.norm(x[c]) > 0 for c in range(3))


def test_identity_preconditioned_reference_is_stable_under_operator_noise():
    """tests/test_gpu_elasticity.py::test_cg_edges also compares the solve WITHOUT a preconditioner (inv_diag NULL), R.IDENTITY_ITERATIONS
    iterations on the p = 2 case, to 1e-11 per block: that reference too has to stay two decades below it"""
    pr, b, _, _ = R.cg_case(R.IDENTITY_CASE)
    d = R.noise_drift(pr.vmult, b, R.IDENTITY_ITERATIONS)
    x, k, res = R.cg(pr.vmult, b, R.IDENTITY_ITERATIONS)
    print(f"noise drift {R.IDENTITY_CASE}, no preconditioner, {k} iterations: {d:.3e}; residual {res:.6e}")
    assert k == R.IDENTITY_ITERATIONS == 3 and d < 1e-13, d
    assert all(np.linalg.norm(x[c]) > 0 for c in range(3))
