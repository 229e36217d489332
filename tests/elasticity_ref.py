"""numpy statement of the linear elasticity operator (bp5_elasticity_*, include/bp5.h) and of the solve on it:
a(v, u) = sum_q kappa JxW [ lam (div v)(div u) + 2 mu eps(v) : eps(u) ] on three-component fields over ONE scalar DoF layout, built on the
oracle's geometry (O.jacobians: K[d][e] = d xi_d / d x_e), reference gradients (O._grad_ref), tables (O.shape_tables) and coefficients
(O.kappa_*).  Blocks are rows of a (3, n_dofs) array.  tests/test_elasticity_cpu.py pins this file outside itself (rigid-body modes, exact
energies, the dense cell matrices)."""
import numpy as np

import bp5_oracle as O

LAME = ((0.5769, 0.3846), (10.0, 1.0))          # (lambda, mu): E = 1, nu = 0.3; nearly incompressible


class Problem:
    """mesh + tables + K, s = kappa JxW; constrained: the mesh's Dirichlet set, or none (free = True: the rigid-body modes are the null space)"""

    def __init__(self, p, cells, quadrature=O.QUAD_GAUSS, deform_amp=0.0, kappa=O.kappa_none, lam=LAME[0][0], mu=LAME[0][1], free=False, h=1.0):
        self.mesh = O.BrickMesh(p, cells, h=h, deform_amp=deform_amp)
        self.nodes, self.pts, self.w, self.N, self.D = O.shape_tables(p, quadrature)
        self.K, JxW, xq = O.jacobians(self.mesh, self.N, self.D, self.w)     # [cell][q][d][e], [cell][q]
        self.s = JxW * kappa(xq)
        self.lam, self.mu, self.quadrature = float(lam), float(mu), quadrature
        self.constrained = np.zeros(0, np.int64) if free else self.mesh.constrained.astype(np.int64)

    # ---- operator
    def _phys_grad(self, src, c0, c1):
        m, n = self.mesh, self.mesh.n
        idx = m.l2g[c0:c1].astype(np.int64)
        G = np.empty((c1 - c0, n ** 3, 3, 3))                             # G[cell][q][c][e] = d u_c / d x_e
        for c in range(3):
            g = np.stack([x.reshape(c1 - c0, -1) for x in O._grad_ref(src[c][idx].reshape(c1 - c0, n, n, n), self.N, self.D)], axis=-1)   # [cell][q][d]
            G[:, :, c, :] = np.einsum("cqde,cqd->cqe", self.K[c0:c1], g)
        return G, idx

    def stress(self, G, c0, c1):
        tr = G[..., 0, 0] + G[..., 1, 1] + G[..., 2, 2]
        sig = self.mu * (G + np.swapaxes(G, -1, -2))
        for c in range(3):
            sig[..., c, c] += self.lam * tr
        return sig * self.s[c0:c1, :, None, None]

    def apply_cells(self, src, cell_range=None, dst=None):
        """dst (+)= sum over the cells of the range, no Dirichlet step; src, dst: (3, n_dofs)"""
        m, n = self.mesh, self.mesh.n
        dst = np.zeros((3, m.n_dofs)) if dst is None else dst
        c0, c1 = (0, m.n_cells) if cell_range is None else cell_range
        if c1 <= c0:
            return dst
        G, idx = self._phys_grad(src, c0, c1)
        sig = self.stress(G, c0, c1)
        t = np.einsum("cqde,cqae->cqad", self.K[c0:c1], sig)              # t[cell][q][component][d]
        N, D = self.N, self.D
        for c in range(3):
            tc = t[:, :, c, :].reshape(c1 - c0, n, n, n, 3)
            y = (np.einsum("ck,bj,ai,...cba->...kji", N, N, D, tc[..., 0], optimize=True)
                 + np.einsum("ck,bj,ai,...cba->...kji", N, D, N, tc[..., 1], optimize=True)
                 + np.einsum("ck,bj,ai,...cba->...kji", D, N, N, tc[..., 2], optimize=True))
            np.add.at(dst[c], idx.ravel(), y.reshape(-1))
        return dst

    def vmult(self, src):
        """A src with dst_c = src_c on the Dirichlet set"""
        dst = self.apply_cells(src)
        dst[:, self.constrained] = src[:, self.constrained]
        return dst

    def energy(self, u):
        """a(u, u) from the quadrature points directly (not through the integrate step)"""
        G, _ = self._phys_grad(u, 0, self.mesh.n_cells)
        eps = 0.5 * (G + np.swapaxes(G, -1, -2))
        tr = G[..., 0, 0] + G[..., 1, 1] + G[..., 2, 2]
        return float(np.sum(self.s * (self.lam * tr * tr + 2.0 * self.mu * np.sum(eps * eps, axis=(-1, -2)))))

    # ---- dense cell matrix and diagonal
    def cell_matrix(self, cell):
        """dense (3 n^3) x (3 n^3) matrix of one cell, rows / columns ordered component-major: from the definition, basis function by basis
        function, through physical gradients -- no sum factorisation, no shared code with apply_cells but the geometry"""
        n3 = self.mesh.n ** 3
        N, D = self.N, self.D
        B = np.stack([np.kron(N, np.kron(N, D)), np.kron(N, np.kron(D, N)), np.kron(D, np.kron(N, N))])    # [d][q][i]
        P = np.einsum("qde,dqi->eqi", self.K[cell], B)                      # P[e][q][i] = d phi_i / d x_e at q
        s = self.s[cell]
        A = np.zeros((3, n3, 3, n3))
        gg = np.einsum("q,eqi,fqj->efij", s, P, P)                         # int s d_e phi_i d_f phi_j
        lap = gg[0, 0] + gg[1, 1] + gg[2, 2]
        for a in range(3):
            for b in range(3):
                A[a, :, b, :] = self.lam * gg[a, b] + self.mu * gg[b, a] + (self.mu * lap if a == b else 0.0)
        return A.reshape(3 * n3, 3 * n3)

    def apply_dense(self, src):
        m, n3 = self.mesh, self.mesh.n ** 3
        dst = np.zeros((3, m.n_dofs))
        for cell in range(m.n_cells):
            idx = m.l2g[cell].astype(np.int64)
            y = (self.cell_matrix(cell) @ src[:, idx].reshape(-1)).reshape(3, n3)
            for c in range(3):
                np.add.at(dst[c], idx, y[c])
        return dst

    def diagonal(self):
        """(3, n_dofs): diag_a[i] = sum s [ (lam + mu) (d_a phi_i)^2 + mu |grad phi_i|^2 ], 1 on the Dirichlet set -- sum-factorised as the
        library does it (the entrywise products N*N, D*D, N*D as 1-D factors)"""
        m, n = self.mesh, self.mesh.n
        N, D = self.N, self.D
        NN, DD, ND = N * N, D * D, N * D
        fac = [(0, 0, DD, NN, NN, 1.0), (1, 1, NN, DD, NN, 1.0), (2, 2, NN, NN, DD, 1.0), (0, 1, ND, ND, NN, 2.0), (0, 2, ND, NN, ND, 2.0), (1, 2, NN, ND, ND, 2.0)]
        KKt = np.einsum("cqde,cqfe->cqdf", self.K, self.K)
        diag = np.zeros((3, m.n_dofs))
        idx = m.l2g.astype(np.int64).ravel()
        for a in range(3):
            y = np.zeros((m.n_cells, n, n, n))
            for d, e, X, Y, Z, f in fac:
                S = self.s * ((self.lam + self.mu) * self.K[:, :, d, a] * self.K[:, :, e, a] + self.mu * KKt[:, :, d, e])
                y += f * np.einsum("ck,bj,ai,...cba->...kji", Z, Y, X, S.reshape(m.n_cells, n, n, n), optimize=True)
            np.add.at(diag[a], idx, y.reshape(-1))
        diag[:, self.constrained] = 1.0
        return diag

    def diagonal_dense(self):
        m, n3 = self.mesh, self.mesh.n ** 3
        diag = np.zeros((3, m.n_dofs))
        for cell in range(m.n_cells):
            d = np.diag(self.cell_matrix(cell)).reshape(3, n3)
            for c in range(3):
                np.add.at(diag[c], m.l2g[cell].astype(np.int64), d[c])
        diag[:, self.constrained] = 1.0
        return diag

    # ---- right-hand sides and sources
    def body_force_rhs(self, f=(0.0, 0.0, -1.0)):
        b = O.assemble_rhs(self.mesh)
        b[self.constrained] = 0.0
        return np.stack([fc * b for fc in f])

    def source(self, seed=20190930):
        """deterministic (3, n_dofs) in [-1, 1], zero on the Dirichlet set"""
        s = np.random.default_rng(seed).uniform(-1.0, 1.0, size=(3, self.mesh.n_dofs))
        s[:, self.constrained] = 0.0
        return s

    def rigid_body_modes(self):
        """the three translations and the three rotations u = omega x X as nodal fields (the coordinate field is in the FE space)"""
        X = self.mesh.coords.T                                            # (3, n_dofs)
        one, zero = np.ones(X.shape[1]), np.zeros(X.shape[1])
        modes = [np.stack([one, zero, zero]), np.stack([zero, one, zero]), np.stack([zero, zero, one])]
        for w in np.eye(3):
            modes.append(np.cross(w[:, None], X, axis=0))
        return modes


def cg(A, b, max_iter, tol=0.0, inv_diag=None):
    """(x, iterations, residual) of O.cg_plain on the stacked system; A: (3, n) -> (3, n); b, x: (3, n); inv_diag: a BLOCK inverse diagonal
    (3, n) or None -- tests/components_ref.py::cg with a diagonal per block"""
    shape = b.shape
    x, k, res = O.cg_plain(lambda v: A(v.reshape(shape)).reshape(-1), b.reshape(-1), max_iter, tol=tol, diag=None if inv_diag is None else inv_diag.reshape(-1))
    return x.reshape(shape), k, res


def noise_drift(A, b, max_iter, inv_diag=None, eps=1e-16, seed=11):
    """How far the fixed-iteration solution moves under a relative perturbation eps of every operator application (relative l2 over all blocks):
    what a bound on a fixed-iteration comparison has to leave room for"""
    rng = np.random.default_rng(seed)
    x0, _, _ = cg(A, b, max_iter, inv_diag=inv_diag)

    def noisy(v):
        y = A(v)
        return y * (1.0 + eps * rng.uniform(-1.0, 1.0, y.shape))
    x1, _, _ = cg(noisy, b, max_iter, inv_diag=inv_diag)
    return np.linalg.norm(x1 - x0) / np.linalg.norm(x0)


def planes(pr):
    """the ten planes in reference order [plane][cell][q], q = qi + n (qj + n qk): K[d][e] at 3 d + e, kappa JxW at 9"""
    out = np.empty((10,) + pr.s.shape)
    for d in range(3):
        for e in range(3):
            out[3 * d + e] = pr.K[:, :, d, e]
    out[9] = pr.s
    return out


def coef_off(n, qi, ab):
    """numpy restatement of coef_off<n> (csrc/bp5_kernels.hpp): offset of quadrature point (qi, ab = qj + n qk) in a cell's plane, pair layout"""
    qi, ab = np.asarray(qi), np.asarray(ab)
    return np.where(qi < 2 * (n // 2), (qi // 2) * (2 * n * n) + 2 * ab + (qi & 1), (n // 2) * (2 * n * n) + ab)


def planes_device_layout(pr):
    """planes(pr) permuted into the device layout: flat [plane][cell][coef_off]"""
    n = pr.mesh.n
    q = np.arange(n ** 3)
    off = coef_off(n, q % n, q // n)
    ref = planes(pr)
    out = np.empty_like(ref)
    out[:, :, off] = ref
    return out.reshape(-1)


# ---- the fixed cases the GPU tests solve (their drift is asserted in tests/test_elasticity_cpu.py); built once per process
_cache = {}
IDENTITY_CASE, IDENTITY_ITERATIONS = "p2", 3     # the solve WITHOUT a preconditioner (inv_diag NULL == identity) the GPU tests also compare


def cg_case(name):
    """(problem, b, block inverse diagonal, iterations): 'p2' = p 2, 8^3 cells; 'p4' = p 4, (4,4,4); both deformed 0.04, step-64 kappa,
    E = 1 / nu = 0.3, body force (0, 0, -1) modulated per DoF so that the three blocks differ"""
    if name not in _cache:
        p, cells, its = {"p2": (2, (8, 8, 8), 10), "p4": (4, (4, 4, 4), 10)}[name]
        pr = Problem(p, cells, O.QUAD_GAUSS, deform_amp=0.04, kappa=O.kappa_step64)
        base = O.assemble_rhs(pr.mesh)
        i = np.arange(base.size)
        b = np.stack([base * (0.3 * np.sin(0.37 * i)), base * (0.2 * np.cos(0.11 * i)), -base])
        inv = 1.0 / pr.diagonal()
        for a in (b, inv):
            a.setflags(write=False)
        _cache[name] = (pr, b, inv, its)
    return _cache[name]
