"""numpy reference of PreconditionChebyshev (include/bp5.h: bp5_chebyshev_*) and of CG with a general preconditioner
(bp5_cg_solve_preconditioned), on top of the oracle's operator (bp5_oracle.vmult, bp5_oracle.operator_diagonal).  Shared by the CPU
and GPU tests of the Chebyshev preconditioner and by the loopback worker."""
import numpy as np


def coefficients(min_used, max_used, degree):
    """theta, delta and the step factors f1_k, f2_k (k = 1 .. degree-1) of the three-term recurrence"""
    theta, delta = 0.5 * (max_used + min_used), 0.5 * (max_used - min_used)
    rho, f1, f2 = delta / theta, [], []
    for _ in range(1, degree):
        rho_new = 1.0 / (2.0 * theta / delta - rho)
        f1.append(rho_new * rho)
        f2.append(2.0 * rho_new / delta)
        rho = rho_new
    return theta, delta, f1, f2


def vmult(A, inv_diag, src, min_used, max_used, degree):
    """dst = P src: x_1 = D^-1 src / theta, x_{k+1} = x_k + f1 (x_k - x_{k-1}) + f2 D^-1 (src - A x_k)"""
    theta, _, f1, f2 = coefficients(min_used, max_used, degree)
    Di = np.ones_like(src) if inv_diag is None else inv_diag
    x_old, x = np.zeros_like(src), (1.0 / theta) * (Di * src)
    for k in range(1, degree):
        t = A(x)
        x, x_old = x + f1[k - 1] * (x - x_old) + f2[k - 1] * (Di * (src - t)), x
    return x


def step(A, inv_diag, dst, src, min_used, max_used, degree):
    """smoother: x_0 = dst, x_1 = x_0 + D^-1 (src - A x_0) / theta, then the same recurrence (degree operator applications)"""
    theta, _, f1, f2 = coefficients(min_used, max_used, degree)
    Di = np.ones_like(src) if inv_diag is None else inv_diag
    x_old = dst.copy()
    x = x_old + (1.0 / theta) * (Di * (src - A(x_old)))
    for k in range(1, degree):
        t = A(x)
        x, x_old = x + f1[k - 1] * (x - x_old) + f2[k - 1] * (Di * (src - t)), x
    return x


def start_vector(global_ids, constrained):
    """v_i = (global id mod 11) - 5, 0 on Dirichlet DoFs: the same vector for every numbering and rank count"""
    v = (np.asarray(global_ids, dtype=np.int64) % 11).astype(np.float64) - 5.0
    v[np.asarray(constrained, dtype=np.int64)] = 0.0
    return v


def lanczos_estimate(A, inv_diag, v, n_its, rel_tol=1e-5):
    """Jacobi-PCG on A x = v (x_0 = 0, the plain recurrence of bp5_oracle.cg_plain), n_its steps or fewer at ||r|| <= rel_tol ||v||;
    (min_est, max_est, iterations) from the Lanczos tridiagonal of its alpha / beta history"""
    Di = np.ones_like(v) if inv_diag is None else inv_diag
    tol = rel_tol * np.linalg.norm(v)
    g = -v.copy()
    h = Di * g
    d = -h
    gh = g @ h
    alphas, betas = [], []
    for k in range(1, n_its + 1):
        h = A(d)
        alpha = gh / (d @ h)
        alphas.append(alpha)
        g = g + alpha * h
        if np.sqrt(g @ g) <= tol or k == n_its:
            break
        h = Di * g
        gh_old, gh = gh, g @ h
        beta = gh / gh_old
        betas.append(beta)
        d = beta * d - h
    m = len(alphas)
    T = np.zeros((m, m))
    for j in range(m):
        T[j, j] = 1.0 / alphas[j] + (betas[j - 1] / alphas[j - 1] if j > 0 else 0.0)
        if j + 1 < m:
            T[j, j + 1] = T[j + 1, j] = np.sqrt(betas[j]) / alphas[j]
    ev = np.linalg.eigvalsh(T)
    return float(ev[0]), float(ev[-1]), m


def bounds(min_est, max_est, smoothing_range):
    """(min_used, max_used) as bp5_chebyshev_create forms them"""
    max_used = 1.2 * max_est
    min_used = max_used / smoothing_range if smoothing_range > 1.0 else min(0.9 * max_used, min_est)
    return min_used, max_used


def pcg(A, P, b, max_iter, tol=0.0):
    """deal.II SolverCG with z = P g (x_0 = 0), the stopping rule of bp5_oracle.cg_plain: (x, iterations, last residual)"""
    x = np.zeros_like(b)
    g = -b.copy()
    res = np.sqrt(g @ g)
    if res <= tol:
        return x, 0, res
    z = P(g)
    d = -z
    gh = g @ z
    k = 0
    while True:
        k += 1
        h = A(d)
        alpha = gh / (d @ h)
        x = x + alpha * d
        g = g + alpha * h
        res = np.sqrt(g @ g)
        if res <= tol or k == max_iter:
            return x, k, res
        z = P(g)
        gh_old, gh = gh, g @ z
        d = (gh / gh_old) * d - z
