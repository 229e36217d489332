"""numpy reference of the p-multigrid transfer and V-cycle (include/bp5.h: bp5_mg_transfer_*, bp5_mg_*), on the oracle's lexicographic
BrickMesh.  There the global prolongation P is the Kronecker product of three banded 1-D matrices (M repeated cell by cell along each
direction), applied by three sweeps (one matrix product per direction) and never assembled.  The V-cycle reuses chebyshev_ref.py.  Shared by the CPU and GPU tests of
the multigrid preconditioner and by the loopback worker."""
import numpy as np

import bp5_oracle as O
import chebyshev_ref as R


def coarse_degree(pf):
    return max(1, pf // 2)


def degrees(p):
    out = [p]
    while out[-1] > 1:
        out.append(coarse_degree(out[-1]))
    return out


def lagrange_matrix(pf, pc):
    """M[a][b] = phi_b^pc(xi_a^pf) on the FE_Q (GLL) nodes, product formula; the two end rows exact unit vectors"""
    xf, _ = O.gll_01(pf + 1)
    xc, _ = O.gll_01(pc + 1)
    M = np.ones((pf + 1, pc + 1))
    for b in range(pc + 1):
        for m in range(pc + 1):
            if m != b:
                M[:, b] *= (xf - xc[m]) / (xc[b] - xc[m])
    M[0, :] = 0.0
    M[0, 0] = 1.0
    M[-1, :] = 0.0
    M[-1, -1] = 1.0
    return M


def prolongation_1d(M, n_cells):
    """the 1-D factor of P along a direction of n_cells cells: rows p_f c + a, columns p_c c + b hold M[a][b]"""
    pf, pc = M.shape[0] - 1, M.shape[1] - 1
    P = np.zeros((pf * n_cells + 1, pc * n_cells + 1))
    for c in range(n_cells):
        P[pf * c:pf * c + pf + 1, pc * c:pc * c + pc + 1] = M
    return P


class Transfer:
    """P Z_c and Z_c P^T (Z_c: zero the coarse Dirichlet entries) between the lexicographic meshes of degrees pf and pc"""

    def __init__(self, cells, pf, pc=None):
        pc = coarse_degree(pf) if pc is None else pc
        self.cells, self.pf, self.pc = tuple(cells), pf, pc
        self.M = lagrange_matrix(pf, pc)
        self.P1 = [prolongation_1d(self.M, n) for n in self.cells]       # x, y, z
        self.shape_f = tuple(pf * n + 1 for n in self.cells[::-1])      # (NZ, NY, NX)
        self.shape_c = tuple(pc * n + 1 for n in self.cells[::-1])
        bc = np.zeros(self.shape_c, dtype=bool)
        bc[0], bc[-1], bc[:, 0], bc[:, -1], bc[:, :, 0], bc[:, :, -1] = True, True, True, True, True, True
        self.boundary_c = bc.ravel()

    @staticmethod
    def _sweeps(u, Px, Py, Pz):
        """(Pz x Py x Px) u on u[z][y][x], one direction at a time (x, y, z): three matrix products, no intermediate larger than the
        result, so the 1.4e8-DoF meshes of the full-size tests fit too"""
        u = u @ Px.T
        u = np.matmul(Py, u)
        return np.tensordot(Pz, u, axes=(1, 0))

    def prolongate(self, ec):
        u = np.where(self.boundary_c, 0.0, ec).reshape(self.shape_c)
        Px, Py, Pz = self.P1
        return self._sweeps(u, Px, Py, Pz).ravel()

    def restrict(self, rf):
        u = rf.reshape(self.shape_f)
        Px, Py, Pz = self.P1
        r = self._sweeps(u, Px.T, Py.T, Pz.T).ravel()
        r[self.boundary_c] = 0.0
        return r


class HelmholtzProblem:
    """O.Problem's interface for step-64's Helmholtz operator (HelmholtzOperator, BP5_OP_HELMHOLTZ): (grad v, grad u) + (v, a u), the
    gradient term with coefficient 1 and a = coefficient(x) in the mass term.  vmult is O.apply_helmholtz_cells with the geometry
    evaluated once: the merged metric for the gradient term, a JxW at the quadrature points for the mass term."""

    def __init__(self, p, cells, quadrature=O.QUAD_GAUSS, h=1.0, deform_amp=0.0, coefficient=O.kappa_step64):
        self.pr = O.Problem(p, cells, quadrature, h=h, deform_amp=deform_amp, kappa=O.kappa_none)
        self.mesh, self.N, self.D, self.w, self.coef = self.pr.mesh, self.pr.N, self.pr.D, self.pr.w, self.pr.coef
        _, JxW, xq = O.jacobians(self.mesh, self.N, self.D, self.w)
        n = self.mesh.n
        self.mass = (coefficient(xq) * JxW).reshape(self.mesh.n_cells, n, n, n)

    def apply_cells(self, src):
        m, N, n = self.mesh, self.N, self.mesh.n
        dst = O.apply_cells(m, self.coef, N, self.D, src)
        idx = m.l2g.astype(np.int64)
        uq = np.einsum("ck,bj,ai,...kji->...cba", N, N, N, src[idx].reshape(m.n_cells, n, n, n), optimize=True)
        y = np.einsum("ck,bj,ai,...cba->...kji", N, N, N, self.mass * uq, optimize=True)
        np.add.at(dst, idx.ravel(), y.reshape(-1))
        return dst

    def vmult(self, src):
        dst = self.apply_cells(src)
        c = self.mesh.constrained.astype(np.int64)
        dst[c] = src[c]
        return dst

    def diagonal(self):
        """O.operator_diagonal plus the mass term's diagonal (N * N in every direction on the a JxW plane), 1 on Dirichlet DoFs"""
        m, NN = self.mesh, self.N * self.N
        y = np.einsum("ck,bj,ai,...cba->...kji", NN, NN, NN, self.mass, optimize=True)
        d = O.operator_diagonal(m, self.coef, self.N, self.D)
        np.add.at(d, m.l2g.astype(np.int64).ravel(), y.reshape(-1))
        d[m.constrained.astype(np.int64)] = 1.0
        return d

    def rhs(self):
        return self.pr.rhs()


def problem(operator, p, cells, quadrature=O.QUAD_GAUSS, h=1.0, deform_amp=0.0, kappa=O.kappa_none):
    """(problem, diagonal): "poisson": O.Problem with kappa in the gradient term (PoissonOperator); "helmholtz": HelmholtzProblem with
    kappa as the mass coefficient a (HelmholtzOperator: COEF_STEP64 -> O.kappa_step64, COEF_ONE -> O.kappa_none)"""
    if operator == "poisson":
        pr = O.Problem(p, cells, quadrature, h=h, deform_amp=deform_amp, kappa=kappa)
        return pr, O.operator_diagonal(pr.mesh, pr.coef, pr.N, pr.D)
    if operator == "helmholtz":
        pr = HelmholtzProblem(p, cells, quadrature, h=h, deform_amp=deform_amp, coefficient=kappa)
        return pr, pr.diagonal()
    raise ValueError(f"unknown operator {operator!r}")


class Level:
    """one level: the oracle problem (Poisson or Helmholtz operator), its inverse diagonal and the Chebyshev bounds of bp5_mg_create"""

    def __init__(self, p, cells, quadrature, deform_amp, kappa, degree, smoothing_range, eig_its, h=1.0, operator="poisson"):
        self.pr, diag = problem(operator, p, cells, quadrature, h=h, deform_amp=deform_amp, kappa=kappa)
        m = self.pr.mesh
        self.inv = 1.0 / diag
        v = R.start_vector(np.arange(m.n_dofs), m.constrained)
        self.min_est, self.max_est, self.cg_its = R.lanczos_estimate(self.pr.vmult, self.inv, v, eig_its)
        self.min_used, self.max_used = R.bounds(self.min_est, self.max_est, smoothing_range)
        self.degree = degree

    def A(self, x):
        return self.pr.vmult(x)

    def vmult(self, b):
        return R.vmult(self.A, self.inv, b, self.min_used, self.max_used, self.degree)

    def step(self, x, b):
        return R.step(self.A, self.inv, x, b, self.min_used, self.max_used, self.degree)


class VCycle:
    """PreconditionMG of bp5_mg_create with its default parameters (or the given ones)"""

    def __init__(self, p, cells, quadrature=O.QUAD_GAUSS, deform_amp=0.0, kappa=O.kappa_none, smoother_degree=4, smoothing_range=20.0,
                 eig_cg_n_iterations=10, coarse_degree=60, coarse_range=1000.0, coarse_eig_cg_n_iterations=30, operator="poisson"):
        ds = degrees(p)
        self.levels = []
        for lev, q in enumerate(ds):
            last = lev + 1 == len(ds)
            self.levels.append(Level(q, cells, quadrature, deform_amp, kappa, coarse_degree if last else smoother_degree,
                                     coarse_range if last else smoothing_range, coarse_eig_cg_n_iterations if last else eig_cg_n_iterations,
                                     operator=operator))
        self.transfers = [Transfer(cells, f, c) for f, c in zip(ds[:-1], ds[1:])]

    def level(self, lev, b):
        L = self.levels[lev]
        if lev + 1 == len(self.levels):
            return L.vmult(b)
        x = L.vmult(b)
        T = self.transfers[lev]
        bc = T.restrict(b - L.A(x))
        x = x + T.prolongate(self.level(lev + 1, bc))
        return L.step(x, b)

    def vmult(self, b):
        return self.level(0, b)
