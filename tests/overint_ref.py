"""numpy statement of the over-integrated operators (BP5_QUAD_GAUSS_OVER: Gauss(p+2) points, CEED BP1 / BP3) on the oracle's own pieces
(O.gauss_01, O.lagrange_tables, O._grad_ref, O._interp, O.element_matrix, O.cg_plain, O.cg_merged): rectangular Q x n tables, Q = p + 2, and Q^3
entries per cell and plane.  tests/test_overint_cpu.py pins it against quantities that do not come from this file (O.Problem and tests/mass_ref on
affine cells, O.element_matrix per cell on deformed ones, symmetry, null space, volume)."""
from types import SimpleNamespace

import numpy as np

import bp5_oracle as O

QUAD_GAUSS_OVER = 2
EINSUM_T = "ck,bj,ai,...cba->...kji"     # (Z x Y x X)^T, as the oracle writes it


def tables(p, extra=1):
    """(nodes[n], pts[Q], w[Q], N[Q, n], D[Q, n]) of FE_Q(p) on GLL nodes with Gauss(p + 1 + extra) points on [0, 1]; extra = 0: the square tables"""
    nodes = O.gll_01(p + 1)[0]
    pts, w = O.gauss_01(p + 1 + extra)
    N, D = O.lagrange_tables(nodes, pts)
    return nodes, pts, w, N, D


def jacobians(mesh, N, D, w):
    """K = J^{-1} (K[d][e] = d xi_d / d x_e), JxW and the q-point coordinates at the Q^3 points: [cell][q], q = qi + Q (qj + Q qk)"""
    n, Q = mesh.n, N.shape[0]
    Xc = mesh.coords[mesh.l2g.astype(np.int64)].reshape(mesh.n_cells, n, n, n, 3)
    J = np.empty((mesh.n_cells, Q, Q, Q, 3, 3))
    for e in range(3):
        g = O._grad_ref(Xc[..., e], N, D)
        for d in range(3):
            J[..., e, d] = g[d]                        # J[e][d] = d x_e / d xi_d
    K = np.linalg.inv(J)
    W = w[:, None, None] * w[None, :, None] * w[None, None, :]
    JxW = np.abs(np.linalg.det(J)) * W[None]
    xq = np.stack([O._interp(Xc[..., e], N) for e in range(3)], axis=-1)
    return K.reshape(mesh.n_cells, Q ** 3, 3, 3), JxW.reshape(mesh.n_cells, Q ** 3), xq.reshape(mesh.n_cells, Q ** 3, 3)


def merged_metric(mesh, N, D, w, kappa=O.kappa_none):
    """coef[c][cell][q] = kappa(x_q) JxW (K K^T)_c, six planes in the order 00, 11, 22, 01, 02, 12"""
    K, JxW, xq = jacobians(mesh, N, D, w)
    G = np.einsum("cqdf,cqef->cqde", K, K)
    s = JxW * kappa(xq)
    return np.ascontiguousarray(np.stack([s * G[:, :, d, e] for (d, e) in O.PLANE_PAIRS], axis=0))


def mass_plane(mesh, N, D, w, rho=O.kappa_none):
    _, JxW, xq = jacobians(mesh, N, D, w)
    return JxW * rho(xq)


def apply_poisson_cells(mesh, coef, N, D, src, cell_range=None, dst=None):
    """dst [+]= sum_cells P^T B^T S B P src (no Dirichlet step), sum-factorised"""
    n, Q = mesh.n, N.shape[0]
    if dst is None:
        dst = np.zeros(mesh.n_dofs)
    lo, hi = (0, mesh.n_cells) if cell_range is None else cell_range
    idx = mesh.l2g[lo:hi].astype(np.int64)
    g0, g1, g2 = O._grad_ref(src[idx].reshape(hi - lo, n, n, n), N, D)
    S = coef[:, lo:hi].reshape(6, hi - lo, Q, Q, Q)
    t0 = S[0] * g0 + S[3] * g1 + S[4] * g2
    t1 = S[3] * g0 + S[1] * g1 + S[5] * g2
    t2 = S[4] * g0 + S[5] * g1 + S[2] * g2
    y = (np.einsum(EINSUM_T, N, N, D, t0, optimize=True) + np.einsum(EINSUM_T, N, D, N, t1, optimize=True)
         + np.einsum(EINSUM_T, D, N, N, t2, optimize=True))
    np.add.at(dst, idx.ravel(), y.reshape(-1))
    return dst


def apply_mass_cells(mesh, S, N, src, cell_range=None, dst=None):
    n, Q = mesh.n, N.shape[0]
    if dst is None:
        dst = np.zeros(mesh.n_dofs)
    lo, hi = (0, mesh.n_cells) if cell_range is None else cell_range
    idx = mesh.l2g[lo:hi].astype(np.int64)
    uq = O._interp(src[idx].reshape(hi - lo, n, n, n), N)
    y = np.einsum(EINSUM_T, N, N, N, uq * S[lo:hi].reshape(hi - lo, Q, Q, Q), optimize=True)
    np.add.at(dst, idx.ravel(), y.reshape(-1))
    return dst


def poisson_diagonal(mesh, coef, N, D):
    """diag(A_eff): six transposed contractions with the entrywise products N.N, D.D, N.D (Q x n); 1 on Dirichlet DoFs"""
    n, Q = mesh.n, N.shape[0]
    NN, DD, ND = N * N, D * D, N * D
    fac = [(DD, NN, NN, 1.0), (NN, DD, NN, 1.0), (NN, NN, DD, 1.0), (ND, ND, NN, 2.0), (ND, NN, ND, 2.0), (NN, ND, ND, 2.0)]
    S = coef.reshape(6, mesh.n_cells, Q, Q, Q)
    y = np.zeros((mesh.n_cells, n, n, n))
    for c, (X, Y, Z, f) in enumerate(fac):
        y += f * np.einsum(EINSUM_T, Z, Y, X, S[c], optimize=True)
    d = np.zeros(mesh.n_dofs)
    np.add.at(d, mesh.l2g.astype(np.int64).ravel(), y.reshape(-1))
    d[mesh.constrained.astype(np.int64)] = 1.0
    return d


def mass_diagonal(mesh, S, N):
    n, Q = mesh.n, N.shape[0]
    NN = N * N
    y = np.einsum(EINSUM_T, NN, NN, NN, S.reshape(mesh.n_cells, Q, Q, Q), optimize=True)
    d = np.zeros(mesh.n_dofs)
    np.add.at(d, mesh.l2g.astype(np.int64).ravel(), y.reshape(-1))
    d[mesh.constrained.astype(np.int64)] = 1.0
    return d


def mass_element_matrix(S_cell, N):
    """dense B^T diag(S) B of one cell, B = N x N x N ([Q^3][n^3])"""
    B = np.kron(N, np.kron(N, N))
    return B.T @ (S_cell[:, None] * B)


def without_dirichlet(mesh):
    """the same mesh with an empty constrained set (BP1 has no boundary condition): a view, the arrays are shared"""
    m = SimpleNamespace(**vars(mesh))
    m.constrained = np.zeros(0, np.uint32)
    return m


class Problem:
    """O.Problem's interface on Gauss(p + 1 + extra) points: mesh + tables + planes; vmult, apply_cells, diagonal, rhs.  mass=True: the mass operator
    with rho = kappa"""

    def __init__(self, p, cells, h=1.0, deform_amp=0.0, kappa=O.kappa_none, mass=False, dirichlet=True, extra=1, mesh=None):
        mesh = mesh if mesh is not None else O.BrickMesh(p, cells, h=h, deform_amp=deform_amp)
        self.mesh = mesh if dirichlet else without_dirichlet(mesh)
        self.nodes, self.pts, self.w, self.N, self.D = tables(p, extra)
        self.mass = mass
        self.coef = mass_plane(mesh, self.N, self.D, self.w, kappa) if mass else merged_metric(mesh, self.N, self.D, self.w, kappa)

    def apply_cells(self, src, cell_range=None, dst=None):
        if self.mass:
            return apply_mass_cells(self.mesh, self.coef, self.N, src, cell_range, dst)
        return apply_poisson_cells(self.mesh, self.coef, self.N, self.D, src, cell_range, dst)

    def vmult(self, src):
        dst = self.apply_cells(src)
        c = self.mesh.constrained.astype(np.int64)
        dst[c] = src[c]
        return dst

    def diagonal(self):
        return mass_diagonal(self.mesh, self.coef, self.N) if self.mass else poisson_diagonal(self.mesh, self.coef, self.N, self.D)

    def rhs(self):
        return O.assemble_rhs(self.mesh)       # Gauss(p+1) by definition, whatever the operator's quadrature


def noise_drift(A, b, max_iter, inv_diag=None, eps=1e-16, seed=11, solver=None):
    """the probe of tests/components_ref.py on a scalar solve: how far the fixed-iteration solution moves under a relative perturbation eps of
    every operator application (relative l2)"""
    solver = solver or O.cg_plain
    rng = np.random.default_rng(seed)
    x0 = solver(A, b, max_iter, diag=inv_diag)[0]

    def noisy(v):
        y = A(v)
        return y * (1.0 + eps * rng.uniform(-1.0, 1.0, y.size))
    x1 = solver(noisy, b, max_iter, diag=inv_diag)[0]
    return np.linalg.norm(x1 - x0) / np.linalg.norm(x0)
