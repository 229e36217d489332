"""numpy statement of the mass operator (BP5_OP_MASS; CEED BP1, deal.II MatrixFreeOperators::MassOperator) on the oracle's own pieces
(O.shape_tables, O.jacobians, O._interp): M = sum_cells P^T B^T diag(rho JxW) B P with B = N x N x N.  tests/test_mass_cpu.py pins it against
quantities that do not come from this file (O.assemble_rhs, O.l2_norm_solution, O.apply_helmholtz_cells - O.apply_cells, textbook 1-D mass
matrices)."""
from types import SimpleNamespace

import numpy as np

import bp5_oracle as O

EINSUM_T = "ck,bj,ai,...cba->...kji"     # (N x N x N)^T, as the oracle writes it


def _D(mesh, N):
    """the derivative table that goes with N (the Jacobians need it; the operator does not): collocation has N == I exactly"""
    return O.shape_tables(mesh.p, O.QUAD_GLL if np.array_equal(N, np.eye(mesh.n)) else O.QUAD_GAUSS)[4]


def plane(mesh, N, D, w, rho=O.kappa_none):
    """rho(x_q) JxW, [cell][q] with q = qi + n (qj + n qk): the one plane of a mass handle in the reference layout"""
    _, JxW, xq = O.jacobians(mesh, N, D, w)
    return JxW * rho(xq)


def apply_cells(mesh, N, w, src, rho=O.kappa_none, D=None, cell_range=None, dst=None, S=None):
    """dst [+]= sum_cells P^T B^T S B P src (no Dirichlet step).  S: a precomputed plane (else from rho; D is needed for the Jacobians only)"""
    n = mesh.n
    if S is None:
        S = plane(mesh, N, _D(mesh, N) if D is None else D, w, rho)
    if dst is None:
        dst = np.zeros(mesh.n_dofs)
    lo, hi = (0, mesh.n_cells) if cell_range is None else cell_range
    idx = mesh.l2g[lo:hi].astype(np.int64)
    uq = O._interp(src[idx].reshape(hi - lo, n, n, n), N)
    y = np.einsum(EINSUM_T, N, N, N, uq * S[lo:hi].reshape(hi - lo, n, n, n), optimize=True)
    np.add.at(dst, idx.ravel(), y.reshape(-1))
    return dst


def vmult(mesh, N, w, src, rho=O.kappa_none, S=None):
    """MassOperator::vmult with the library's Dirichlet contract: cell loop on unmodified src, then dst[c] = src[c] on Dirichlet DoFs"""
    dst = apply_cells(mesh, N, w, src, rho, S=S)
    c = mesh.constrained.astype(np.int64)
    dst[c] = src[c]
    return dst


def diagonal(mesh, N, w, rho=O.kappa_none, S=None):
    """diag(M_eff): sum over cells of (N.N x N.N x N.N)^T S through l2g, 1 on Dirichlet DoFs"""
    n = mesh.n
    if S is None:
        S = plane(mesh, N, _D(mesh, N), w, rho)
    NN = N * N
    y = np.einsum(EINSUM_T, NN, NN, NN, S.reshape(mesh.n_cells, n, n, n), optimize=True)
    d = np.zeros(mesh.n_dofs)
    np.add.at(d, mesh.l2g.astype(np.int64).ravel(), y.reshape(-1))
    d[mesh.constrained.astype(np.int64)] = 1.0
    return d


def without_dirichlet(mesh):
    """the same mesh with an empty constrained set (BP1 has no boundary condition): a view, the arrays are shared"""
    m = SimpleNamespace(**vars(mesh))
    m.constrained = np.zeros(0, np.uint32)
    return m


class Problem:
    """O.Problem's interface for the mass operator: mesh + tables + plane; vmult, diagonal, rhs"""

    def __init__(self, p, cells, quadrature=O.QUAD_GAUSS, h=1.0, deform_amp=0.0, rho=O.kappa_none, dirichlet=True):
        mesh = O.BrickMesh(p, cells, h=h, deform_amp=deform_amp)
        self.mesh = mesh if dirichlet else without_dirichlet(mesh)
        self.nodes, self.pts, self.w, self.N, self.D = O.shape_tables(p, quadrature)
        self.S = plane(self.mesh, self.N, self.D, self.w, rho)
        self.quadrature, self.rho = quadrature, rho

    def apply_cells(self, src, cell_range=None, dst=None):
        return apply_cells(self.mesh, self.N, self.w, src, S=self.S, cell_range=cell_range, dst=dst)

    def vmult(self, src):
        return vmult(self.mesh, self.N, self.w, src, S=self.S)

    def diagonal(self):
        return diagonal(self.mesh, self.N, self.w, S=self.S)

    def rhs(self):
        return O.assemble_rhs(self.mesh)


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
