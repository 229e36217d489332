"""numpy statement of the finite-strain neo-Hookean operators (bp5_hyperelasticity_*, include/bp5.h) and of Newton's method on them, built on
tests/elasticity_ref.Problem (its K, s = kappa JxW, _phys_grad and the integrate einsums of apply_cells):
  Phi(F) = lam / 2 (ln J)^2 - mu ln J + mu / 2 (tr F^T F - 3),  F = I + grad_x u,  J = det F,  B = F^-T,
  P = mu (F - B) + lam ln J B,   dP = mu G + (mu - lam ln J) B G^T B + lam (B : G) B.
Blocks are rows of a (3, n_dofs) array.  tests/test_hyperelasticity_cpu.py pins this file outside itself (finite differences of the energy and of
the residual, the linear limit, symmetry, objectivity, a homogeneous stretch)."""
import numpy as np

import bp5_oracle as O
import elasticity_ref as E

LAME = E.LAME
I3 = np.eye(3)


def phi(F, lam, mu):
    """the energy density at one deformation gradient (or an array of them, [..., 3, 3])"""
    lnJ = np.log(np.linalg.det(F))
    return 0.5 * lam * lnJ ** 2 - mu * lnJ + 0.5 * mu * (np.einsum("...ce,...ce->...", F, F) - 3.0)


def piola(F, lam, mu):
    """P(F) = mu (F - B) + lam ln J B, B = F^-T"""
    B = np.swapaxes(np.linalg.inv(F), -1, -2)
    lnJ = np.log(np.linalg.det(F))
    return mu * (F - B) + lam * lnJ[..., None, None] * B


class Problem(E.Problem):
    """elasticity_ref.Problem plus the neo-Hookean energy, residual, tangent, state and Newton's method"""

    def _F(self, u, c0=0, c1=None):
        c1 = self.mesh.n_cells if c1 is None else c1
        G, idx = self._phys_grad(u, c0, c1)
        return G + I3, idx

    @staticmethod
    def _B_lnJ(F):
        with np.errstate(invalid="ignore", divide="ignore"):
            J = np.linalg.det(F)
            lnJ = np.where(J > 0.0, np.log(np.where(J > 0.0, J, 1.0)), np.nan)      # J <= 0: NaN, as the kernel
        return np.swapaxes(np.linalg.inv(F), -1, -2), lnJ

    def _integrate(self, T, idx, c0, c1, dst):
        """dst_c += sum_q s K[d][e] T[c][e] against the reference gradients of the test functions: the tail of elasticity_ref.apply_cells"""
        n = self.mesh.n
        t = np.einsum("cqde,cqae->cqad", self.K[c0:c1], T * self.s[c0:c1, :, None, None])
        N, D = self.N, self.D
        for c in range(3):
            tc = t[:, :, c, :].reshape(c1 - c0, n, n, n, 3)
            y = (np.einsum("ck,bj,ai,...cba->...kji", N, N, D, tc[..., 0], optimize=True)
                 + np.einsum("ck,bj,ai,...cba->...kji", N, D, N, tc[..., 1], optimize=True)
                 + np.einsum("ck,bj,ai,...cba->...kji", D, N, N, tc[..., 2], optimize=True))
            np.add.at(dst[c], idx.ravel(), y.reshape(-1))
        return dst

    def energy(self, u):
        """sum_q s Phi(F_q), from the quadrature points directly"""
        F, _ = self._F(u)
        return float(np.sum(self.s * phi(F, self.lam, self.mu)))

    def residual_cells(self, u, cell_range=None, dst=None):
        """dst (+)= F_int(u) over the cells of the range, no Dirichlet step"""
        m = self.mesh
        dst = np.zeros((3, m.n_dofs)) if dst is None else dst
        c0, c1 = (0, m.n_cells) if cell_range is None else cell_range
        if c1 <= c0:
            return dst
        F, idx = self._F(u, c0, c1)
        B, lnJ = self._B_lnJ(F)
        P = self.mu * (F - B) + self.lam * lnJ[..., None, None] * B
        return self._integrate(P, idx, c0, c1, dst)

    def residual(self, u):
        """F_int(u) with zeros on the Dirichlet set (u may carry prescribed values there)"""
        r = self.residual_cells(u)
        r[:, self.constrained] = 0.0
        return r

    def tangent_cells(self, u, v, cell_range=None, dst=None):
        """dst (+)= T(u) v over the cells of the range, no Dirichlet step"""
        m = self.mesh
        dst = np.zeros((3, m.n_dofs)) if dst is None else dst
        c0, c1 = (0, m.n_cells) if cell_range is None else cell_range
        if c1 <= c0:
            return dst
        F, idx = self._F(u, c0, c1)
        B, lnJ = self._B_lnJ(F)
        G, _ = self._phys_grad(v, c0, c1)
        BGtB = np.einsum("...ca,...ba,...be->...ce", B, G, B)                        # B G^T B
        BG = np.einsum("...ce,...ce->...", B, G)
        dP = self.mu * G + (self.mu - self.lam * lnJ)[..., None, None] * BGtB + self.lam * BG[..., None, None] * B
        return self._integrate(dP, idx, c0, c1, dst)

    def tangent(self, u, v):
        """T(u) v with dst_c = v_c on the Dirichlet set"""
        dst = self.tangent_cells(u, v)
        dst[:, self.constrained] = v[:, self.constrained]
        return dst

    def state(self, u):
        """the ten state planes in reference order [plane][cell][q], q = qi + n (qj + n qk): B[c][e] at 3 c + e, ln J at 9"""
        F, _ = self._F(u)
        B, lnJ = self._B_lnJ(F)
        out = np.empty((10,) + self.s.shape)
        for c in range(3):
            for e in range(3):
                out[3 * c + e] = B[:, :, c, e]
        out[9] = lnJ
        return out

    def to_device_layout(self, planes):
        """[plane][cell][q] permuted into the device layout: flat [plane][cell][coef_off] (elasticity_ref.coef_off)"""
        n = self.mesh.n
        q = np.arange(n ** 3)
        off = E.coef_off(n, q % n, q // n)
        out = np.empty_like(planes)
        out[:, :, off] = planes
        return out.reshape(-1)

    def newton(self, f_ext, u0=None, precond=None, max_newton=20, abs_tol=0.0, rel_tol=1e-10, cg_max_iter=2000, cg_rel_tol=1e-12, max_backtracks=8):
        """bp5_hyperelasticity_newton's algorithm with elasticity_ref.cg as the inner solver (precond: a block inverse diagonal or None).
        Returns (u, dict(newton_iterations, total_cg_iterations, history, backtracks, status)); status: 'ok', 'no_convergence', 'breakdown'"""
        u = np.zeros_like(f_ext) if u0 is None else u0.copy()

        def res(v):
            r = f_ext - self.residual(v)
            r[:, self.constrained] = 0.0
            return r, float(np.linalg.norm(r))
        r, rn = res(u)
        info = dict(newton_iterations=0, total_cg_iterations=0, history=[rn], backtracks=0, status="no_convergence")
        tol = max(abs_tol, rel_tol * rn)
        for _ in range(max_newton):
            if rn <= tol:
                break
            base = u
            delta, its, _ = E.cg(lambda v: self.tangent(base, v), r, cg_max_iter, tol=cg_rel_tol * rn, inv_diag=precond)
            info["total_cg_iterations"] += its
            alpha, bt = 1.0, 0
            while True:
                trial = u + alpha * delta
                with np.errstate(invalid="ignore"):
                    rt, rtn = res(trial)
                if np.isfinite(rtn) and rtn < rn:
                    break
                if bt == max_backtracks:
                    info["status"] = "breakdown"
                    return u, info
                alpha *= 0.5
                bt += 1
                info["backtracks"] += 1
            u, r, rn = trial, rt, rtn
            info["newton_iterations"] += 1
            info["history"].append(rn)
        if rn <= tol:
            info["status"] = "ok"
        return u, info


def smooth_displacement(pr, amp=0.2, clamped=False):
    """a smooth (3, n_dofs) field scaled to max |d u_c / d x_e| = amp over the quadrature points.  clamped = False: it is non-zero on the Dirichlet
    set too (a prescribed displacement); True: it carries a bubble factor that vanishes on the faces of the brick, and zeros on the Dirichlet set"""
    X = pr.mesh.coords.T
    lo, L = X.min(axis=1)[:, None], (X.max(axis=1) - X.min(axis=1))[:, None]
    x, y, z = (X - lo) / L
    u = np.stack([np.sin(2.0 * x + 0.3) * np.cos(2.0 * y) + 0.3 * z * z,
                  0.7 * np.cos(2.0 * y + 0.1) * np.sin(2.0 * z + 0.2) - 0.2 * x * y,
                  0.5 * np.sin(2.0 * z) * np.cos(2.0 * x + 0.4) + 0.25 * x * z])
    if clamped:
        u *= 64.0 * x * (1.0 - x) * y * (1.0 - y) * z * (1.0 - z)
        u[:, pr.constrained] = 0.0
    return u * (amp / max_grad(pr, u))


def max_grad(pr, u):
    G, _ = pr._phys_grad(u, 0, pr.mesh.n_cells)
    return float(np.abs(G).max())


def input_noise_drift(pr, u, eps=1e-16, seed=11):
    """How far the reference's own residual and state move under a relative perturbation eps of u (elasticity_ref.noise_drift's idea, on the
    input): (residual: relative l2; planes 0..8 and plane 9: max |difference| / max |plane values|) -- what a parity bound has to leave room for"""
    un = u * (1.0 + eps * np.random.default_rng(seed).uniform(-1.0, 1.0, u.shape))
    r0, r1, s0, s1 = pr.residual(u), pr.residual(un), pr.state(u), pr.state(un)
    return (float(np.linalg.norm(r1 - r0) / np.linalg.norm(r0)), float(np.abs(s1[:9] - s0[:9]).max() / np.abs(s0[:9]).max()),
            float(np.abs(s1[9] - s0[9]).max() / np.abs(s0[9]).max()))


# ---- the fixed cases the GPU tests run (their properties are asserted in tests/test_hyperelasticity_cpu.py); built once per process
_cache = {}
NEWTON_CELLS, NEWTON_P = (4, 4, 4), 2
NEWTON_LOAD = 0.1            # body force (0, 0, -NEWTON_LOAD) on E = 1, nu = 0.3: tests/test_hyperelasticity_cpu.py asserts what this choice has to deliver
NEWTON_PARAMS = dict(max_newton=20, abs_tol=0.0, rel_tol=1e-10, cg_max_iter=2000, cg_rel_tol=1e-12, max_backtracks=8)
BACKTRACK_FACTOR = 20.0      # the second case: 20 x that load, cut off after three Newton steps (each of them backtracks)
BACKTRACK_PARAMS = dict(NEWTON_PARAMS, max_newton=3)


def newton_case(backtracking=False):
    """(problem, f_ext, u, info) of the clamped block under body force: p 2, 4^3 cells, deformed 0.04, step-64 kappa, E = 1 / nu = 0.3"""
    key = ("newton", backtracking)
    if key not in _cache:
        pr = Problem(NEWTON_P, NEWTON_CELLS, O.QUAD_GAUSS, deform_amp=0.04, kappa=O.kappa_step64)
        f = pr.body_force_rhs((0.0, 0.0, -NEWTON_LOAD * (BACKTRACK_FACTOR if backtracking else 1.0)))
        u, info = pr.newton(f, **(BACKTRACK_PARAMS if backtracking else NEWTON_PARAMS))
        for a in (f, u):
            a.setflags(write=False)
        _cache[key] = (pr, f, u, info)
    return _cache[key]


def cg_case(name):
    """(problem, u, b, iterations) of the fixed-iteration CG on the tangent: 'p2' = p 2, 4^3 cells; 'p4' = p 4, (3,3,2); deformed 0.04, step-64 kappa,
    E = 1 / nu = 0.3, the tangent at smooth_displacement with zero Dirichlet values, elasticity_ref.cg_case's modulated body force"""
    key = ("cg", name)
    if key not in _cache:
        p, cells, its = {"p2": (2, (4, 4, 4), 10), "p4": (4, (3, 3, 2), 10)}[name]
        pr = Problem(p, cells, O.QUAD_GAUSS, deform_amp=0.04, kappa=O.kappa_step64)
        u = smooth_displacement(pr, 0.2, clamped=True)
        base = O.assemble_rhs(pr.mesh)
        i = np.arange(base.size)
        b = np.stack([base * (0.3 * np.sin(0.37 * i)), base * (0.2 * np.cos(0.11 * i)), -base])
        b[:, pr.constrained] = 0.0
        for a in (u, b):
            a.setflags(write=False)
        _cache[key] = (pr, u, b, its)
    return _cache[key]
