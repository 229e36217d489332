"""numpy statement of what bp5_cg_solve_components computes (CEED BP6): deal.II's SolverCG recurrence (O.cg_plain) on the STACKED system
diag(A, ..., A) x = b of a block vector -- ONE Krylov space, alpha, beta and the stop test shared by all components -- and the block-vector
operator next to it.  Blocks are rows of an (n_components, n_dofs) array; the operator, the Dirichlet set and the diagonal are the scalar
problem's."""
import numpy as np

import bp5_oracle as O


def vmult(pr, src):
    """A on every block: (n_components, n_dofs) -> (n_components, n_dofs)"""
    return np.stack([pr.vmult(s) for s in src])


def stacked(A, n_components):
    """v -> concat(A v_c): the stacked operator on the concatenated vector"""
    return lambda v: np.concatenate([A(vc) for vc in v.reshape(n_components, -1)])


def cg(A, b, max_iter, tol=0.0, inv_diag=None):
    """(x, iterations, residual) of O.cg_plain on the stacked system; b, x: (n_components, n_dofs); inv_diag: per scalar DoF, applied to every
    block"""
    nc = b.shape[0]
    diag = None if inv_diag is None else np.tile(inv_diag, nc)
    x, k, res = O.cg_plain(stacked(A, nc), b.reshape(-1), max_iter, tol=tol, diag=diag)
    return x.reshape(nc, -1), k, res


def separate(A, b, max_iter, tol=0.0, inv_diag=None):
    """n_components independent solves (what the stacked solve is NOT, unless the right-hand sides coincide)"""
    return np.stack([O.cg_plain(A, bc, max_iter, tol=tol, diag=inv_diag)[0] for bc in b])


def rhs_blocks(b, n_components=3):
    """the right-hand sides of the BP6 tests: b (1 + 0.5 sin(0.37 (c + 1) i)), c = 0 .. n_components - 1"""
    i = np.arange(b.size)
    return np.stack([b * (1.0 + 0.5 * np.sin(0.37 * (c + 1) * i)) for c in range(n_components)])


def noise_drift(A, b, max_iter, inv_diag=None, eps=1e-16, seed=11):
    """How far the fixed-iteration stacked solution moves under a relative perturbation eps of every operator application: what a bound on a
    fixed-iteration comparison has to leave room for (relative l2 over all blocks)."""
    rng = np.random.default_rng(seed)
    x0, _, _ = cg(A, b, max_iter, inv_diag=inv_diag)

    def noisy(v):
        y = A(v)
        return y * (1.0 + eps * rng.uniform(-1.0, 1.0, y.size))
    x1, _, _ = cg(noisy, b, max_iter, inv_diag=inv_diag)
    return np.linalg.norm(x1 - x0) / np.linalg.norm(x0)
