"""PreconditionChebyshev without a GPU: the numpy reference (tests/chebyshev_ref.py) against closed forms, and the library's host-side
tridiagonal eigenvalue solver (bp5_tridiagonal_eigenvalues) against numpy."""
import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import chebyshev_ref as R

pkg = bp5_pkg.load()


@pytest.mark.parametrize("degree", range(1, 9))
def test_reference_vmult_is_the_chebyshev_residual_polynomial(degree):
    """A = diag(lambda), D = I: one vmult gives p(lambda_i) src_i with 1 - lambda p(lambda) = T_k((theta - lambda)/delta) / T_k(theta/delta)."""
    lo, hi = 0.3, 2.4
    lam = np.concatenate([np.linspace(lo, hi, 40), np.linspace(0.05, 3.0, 17)])   # inside and outside the bounds
    src = np.random.default_rng(degree).uniform(-1, 1, lam.size)
    got = R.vmult(lambda v: lam * v, None, src, lo, hi, degree)
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    T = np.polynomial.chebyshev.Chebyshev.basis(degree)
    p = (1.0 - T((theta - lam) / delta) / T(theta / delta)) / lam
    assert np.abs(got - p * src).max() <= 1e-13 * np.abs(p * src).max()


@pytest.mark.parametrize("degree", [1, 2, 3, 6])
def test_reference_step_is_the_error_propagation_polynomial(degree):
    """step from x_0: the error x* - x_k is multiplied by T_k((theta - lambda)/delta) / T_k(theta/delta)."""
    lo, hi = 0.2, 2.0
    lam = np.linspace(0.1, 2.5, 31)
    rng = np.random.default_rng(7 + degree)
    xs, x0 = rng.uniform(-1, 1, lam.size), rng.uniform(-1, 1, lam.size)
    got = R.step(lambda v: lam * v, None, x0, lam * xs, lo, hi, degree)
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    T = np.polynomial.chebyshev.Chebyshev.basis(degree)
    want = xs - T((theta - lam) / delta) / T(theta / delta) * (xs - x0)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


def test_reference_lanczos_estimate_lies_inside_the_spectrum_and_converges():
    """The Ritz values of the CG-Lanczos tridiagonal are inside [lambda_min, lambda_max] and reach both ends on a small diagonal matrix."""
    lam = np.linspace(0.5, 4.0, 30)
    v = R.start_vector(np.arange(lam.size), np.zeros(0, dtype=np.uint32))
    lo, hi, k = R.lanczos_estimate(lambda u: lam * u, None, v, 6, rel_tol=0.0)
    assert k == 6 and lam[0] <= lo and hi <= lam[-1] * (1 + 1e-14) and hi > 0.9 * lam[-1]
    lo, hi, k = R.lanczos_estimate(lambda u: lam * u, None, v, 60, rel_tol=1e-12)
    assert abs(lo - lam[0]) < 1e-8 and abs(hi - lam[-1]) < 1e-8 and k <= 31


def test_reference_pcg_with_a_diagonal_is_the_oracle_jacobi_cg():
    """pcg with P = D^-1 is the oracle's Jacobi-PCG (the plain recurrence with diag) iterate for iterate."""
    pr = O.Problem(2, (3, 3, 2), O.QUAD_GAUSS, deform_amp=0.05, kappa=O.kappa_step64)
    inv = 1.0 / O.operator_diagonal(pr.mesh, pr.coef, pr.N, pr.D)
    b = pr.rhs()
    x1, k1, r1 = R.pcg(pr.vmult, lambda g: inv * g, b, 12)
    x2, k2, r2 = O.cg_plain(pr.vmult, b, 12, diag=inv)
    assert k1 == k2 == 12 and np.linalg.norm(x1 - x2) <= 1e-13 * np.linalg.norm(x2)


@pytest.mark.parametrize("n", list(range(1, 41)))
def test_tridiagonal_eigenvalues_match_numpy(n):
    """bp5_tridiagonal_eigenvalues (host, Sturm bisection) == numpy.linalg.eigvalsh on random symmetric tridiagonals, 1e-12 relative."""
    rng = np.random.default_rng(1000 + n)
    for scale in (1.0, 1e-3, 1e4):
        d, e = scale * rng.uniform(-2, 3, n), scale * rng.uniform(-1, 1, n - 1)
        if n > 3:
            e[n // 2] = 0.0                                   # a split matrix
        ref = np.linalg.eigvalsh(np.diag(d) + np.diag(e, 1) + np.diag(e, -1))
        got = pkg.tridiagonal_eigenvalues(d, e)
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (scale, got, ref)


def test_tridiagonal_eigenvalues_of_clusters_and_a_lanczos_matrix():
    """Repeated eigenvalues (diagonal matrix with equal entries) and the positive-definite Lanczos tridiagonal of a CG run."""
    got = pkg.tridiagonal_eigenvalues(np.array([2.0, 2.0, 1.0, 2.0]), np.zeros(3))
    assert np.abs(got - [1.0, 2.0, 2.0, 2.0]).max() <= 1e-15 * 2
    d = np.array([2.0, 2.0, 2.0, 2.0, 2.0])
    e = -np.ones(4)
    ref = 2.0 - 2.0 * np.cos(np.arange(1, 6) * np.pi / 6)    # closed form of the 1-D Laplacian
    assert np.abs(pkg.tridiagonal_eigenvalues(d, e) - ref).max() <= 1e-14 * 4


def test_chebyshev_entry_points_validate_their_arguments_without_a_gpu():
    """Argument checks that return before any HIP call."""
    import ctypes as C
    L = pkg.lib()
    out = np.zeros(2)
    assert L.bp5_tridiagonal_eigenvalues(0, out.ctypes.data, out.ctypes.data, out.ctypes.data) == 1
    assert L.bp5_chebyshev_create(None, None, None, None, None, None, C.byref(C.c_void_p())) == 1
    assert L.bp5_chebyshev_vmult(None, None, None) == 1
    assert L.bp5_cg_solve_preconditioned(None, None, None, None, None, None, None, None, None, None) == 1
