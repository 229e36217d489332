"""numpy statement of the elasticity preconditioners (include/bp5.h: bp5_elasticity_chebyshev_create, bp5_elasticity_mg_create,
bp5_mg_transfer_*_components, bp5_cg_solve_elasticity_preconditioned), composed from the project's own references and nothing else:
elasticity_ref.Problem (operator, three diagonals), multigrid_ref.Transfer / hmg_ref.GeometricTransfer applied block by block, hmg_ref.hierarchy,
and chebyshev_ref (polynomial, Lanczos estimate, PCG) on flattened (3, n) arrays.  tests/test_elasticity_mg_cpu.py pins this file outside itself
(symmetry of the cycle, the iteration counts of the three preconditioners, the stability of every comparison the GPU tests make)."""
import numpy as np

import bp5_oracle as O
import chebyshev_ref as C
import elasticity_ref as E
import hmg_ref as H
import multigrid_ref as G

AMP = 0.04
MG_DEFAULTS = dict(smoother_degree=4, smoothing_range=20.0, eig_cg_n_iterations=10, coarse_degree=60, coarse_range=1000.0, coarse_eig_cg_n_iterations=30)


def start_vector(global_ids, constrained):
    """(3, n): v_c[i] = ((3 id_i + c) mod 11) - 5, 0 on Dirichlet DoFs -- chebyshev_ref.start_vector of the stacked numbering 3 id + c"""
    ids = np.asarray(global_ids, dtype=np.int64)
    v = np.stack([((3 * ids + c) % 11).astype(np.float64) - 5.0 for c in range(3)])
    v[:, np.asarray(constrained, dtype=np.int64)] = 0.0
    return v


def rhs(pr):
    """the right-hand side of elasticity_ref.cg_case on any problem: the load vector modulated per DoF so that the three blocks differ"""
    base = O.assemble_rhs(pr.mesh)
    i = np.arange(base.size)
    return np.stack([base * (0.3 * np.sin(0.37 * i)), base * (0.2 * np.cos(0.11 * i)), -base])


def flat(f, shape):
    """an operator on (3, n) arrays as one on flattened arrays (what chebyshev_ref works on)"""
    return lambda v: f(v.reshape(shape)).reshape(-1)


def lanczos_residuals(A, inv_diag, v, n_its):
    """||g_k|| / ||v||, k = 1 .. (the step chebyshev_ref.lanczos_estimate stops at), of the same Jacobi-PCG recurrence: how far the stop decision
    of the estimate (||g|| <= 1e-5 ||v||) is from flipping"""
    Di = np.ones_like(v) if inv_diag is None else inv_diag
    nv = np.linalg.norm(v)
    g = -v.copy()
    h = Di * g
    d = -h
    gh = g @ h
    out = []
    for k in range(1, n_its + 1):
        h = A(d)
        g = g + (gh / (d @ h)) * h
        out.append(np.sqrt(g @ g) / nv)
        if out[-1] <= 1e-5 or k == n_its:
            break
        h = Di * g
        gh_old, gh = gh, g @ h
        d = (gh / gh_old) * d - h
    return out


class Noise:
    """a relative perturbation eps of every operator application (elasticity_ref.noise_drift's method)"""

    def __init__(self, eps=1e-16, seed=11):
        self.eps, self.rng = eps, np.random.default_rng(seed)

    def __call__(self, y):
        return y * (1.0 + self.eps * self.rng.uniform(-1.0, 1.0, y.shape))


class Level:
    """one level: the elasticity problem, its block inverse diagonal and the Chebyshev bounds of bp5_elasticity_chebyshev_create; all on (3, n)"""

    def __init__(self, p, cells, h, quadrature, deform_amp, kappa, lam, mu, degree, smoothing_range, eig_its, block_diagonal=True):
        self.pr = E.Problem(p, cells, quadrature, deform_amp=deform_amp, kappa=kappa, lam=lam, mu=mu, h=h)
        m = self.pr.mesh
        self.shape = (3, m.n_dofs)
        self.inv = 1.0 / self.pr.diagonal() if block_diagonal else None
        self.noise = None
        v = start_vector(np.arange(m.n_dofs), m.constrained).reshape(-1)
        fi = None if self.inv is None else self.inv.reshape(-1)
        self.min_est, self.max_est, self.cg_its = C.lanczos_estimate(flat(self.pr.vmult, self.shape), fi, v, eig_its)
        self.residuals = lanczos_residuals(flat(self.pr.vmult, self.shape), fi, v, eig_its)
        self.min_used, self.max_used = C.bounds(self.min_est, self.max_est, smoothing_range)
        self.degree = degree

    def A(self, x):
        y = self.pr.vmult(x)
        return y if self.noise is None else self.noise(y)

    def vmult(self, b):
        return C.vmult(self.A, self.inv, b, self.min_used, self.max_used, self.degree)

    def step(self, x, b):
        return C.step(self.A, self.inv, x, b, self.min_used, self.max_used, self.degree)


class BlockTransfer:
    """a scalar transfer (multigrid_ref.Transfer or hmg_ref.GeometricTransfer) applied to every block"""

    def __init__(self, T):
        self.T = T

    def prolongate(self, ec):
        return np.stack([self.T.prolongate(e) for e in ec])

    def restrict(self, rf):
        return np.stack([self.T.restrict(r) for r in rf])


class VCycle:
    """PreconditionMG of bp5_elasticity_mg_create on hmg_ref.hierarchy(p, cells, h_levels, min_cells) with bp5_mg_params' defaults (or the
    given ones): multigrid_ref.VCycle's recursion on (3, n) arrays"""

    def __init__(self, p, cells, quadrature=O.QUAD_GAUSS, deform_amp=AMP, kappa=O.kappa_step64, lam=E.LAME[0][0], mu=E.LAME[0][1], h_levels=0, min_cells=4,
                 **params):
        prm = dict(MG_DEFAULTS, **params)
        self.spec = H.hierarchy(p, cells, h_levels, min_cells)
        self.levels = []
        for lev, (q, c, h) in enumerate(self.spec):
            last = lev + 1 == len(self.spec)
            self.levels.append(Level(q, c, h, quadrature, deform_amp, kappa, lam, mu, prm["coarse_degree"] if last else prm["smoother_degree"],
                                     prm["coarse_range"] if last else prm["smoothing_range"],
                                     prm["coarse_eig_cg_n_iterations"] if last else prm["eig_cg_n_iterations"]))
        self.transfers = [BlockTransfer(G.Transfer(fc, pf, pc) if pf != pc else H.GeometricTransfer(cc, pc))
                          for (pf, fc, _), (pc, cc, _) in zip(self.spec[:-1], self.spec[1:])]

    def set_noise(self, noise):
        for L in self.levels:
            L.noise = noise

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


def pcg(A, P, b, max_iter, tol=0.0):
    """chebyshev_ref.pcg on the stacked system; A, P: (3, n) -> (3, n); (x, iterations, last residual)"""
    x, k, res = C.pcg(flat(A, b.shape), flat(P, b.shape), b.reshape(-1), max_iter, tol=tol)
    return x.reshape(b.shape), k, res


def drift(run, set_noise, eps=1e-16, seed=11):
    """relative l2 distance between run() without and with a relative perturbation eps of every operator application"""
    set_noise(None)
    x0 = run()
    set_noise(Noise(eps, seed))
    x1 = run()
    set_noise(None)
    return np.linalg.norm(x1 - x0) / np.linalg.norm(x0)


# ---- the cases the GPU tests compare (tests/test_gpu_elasticity_mg.py); tests/test_elasticity_mg_cpu.py asserts their stability.  Built once per process
# The degree-1 level of (3, 3, 2) stops its Lanczos estimate within a factor 10 of the 1e-5 threshold for both quadratures and both Lame pairs
# (residuals 6.6e-5 / 1.9e-6, 3.9e-5 / 6.3e-6, 1.2e-5 / 3.9e-6, 1.6e-5 / 2.8e-6 at the last two steps), and so do (3, 3, 3) and (4, 3, 2): p = 2 and
# p = 3 are therefore compared on (3, 2, 2) with GLL and on (2, 2, 2), whose levels all stop a factor >= 50 away (test_elasticity_mg_cpu.py asserts 10).
# On (3, 2, 2) and on the hybrid (4, 4, 4) the Gauss / first-pair level is marginal too (3.5e-5; 9.2e-5 / 2.8e-5): those cases take GLL / the second pair.
VCYCLE_CASES = {     # name: (p, cells, quadrature, Lame pair, h_levels, min_cells)
    "p2_gll": (2, (3, 2, 2), O.QUAD_GLL, 0, 0, 4), "p2_gll_lame1": (2, (3, 2, 2), O.QUAD_GLL, 1, 0, 4), "p3": (3, (2, 2, 2), O.QUAD_GAUSS, 0, 0, 4),
    "p4_gll_lame1": (4, (3, 2, 2), O.QUAD_GLL, 1, 0, 4), "p6_lame1": (6, (2, 2, 2), O.QUAD_GAUSS, 1, 0, 4), "p8": (8, (2, 2, 2), O.QUAD_GAUSS, 0, 0, 4),
    "p2_hybrid_lame1": (2, (4, 4, 4), O.QUAD_GAUSS, 1, 1, 2),
}
SOLVE_CASES = {"p4": (4, (4, 4, 4)), "p2": (2, (4, 4, 4))}          # V-cycle-PCG and Chebyshev(4)-PCG to 1e-8 ||b||, Gauss, Lame pair 0
CHEBYSHEV_CASES = [(p, degree, block_diagonal) for p in (2, 4) for degree in (4, 5) for block_diagonal in (True, False)]   # on (3, 2, 2), Gauss, Lame pair 0
CHEBYSHEV_CELLS = (3, 2, 2)
_cache = {}


def vcycle_case(name):
    """(VCycle, source): the source is non-zero on the boundary too"""
    if ("v", name) not in _cache:
        p, cells, quad, lame, h_levels, min_cells = VCYCLE_CASES[name]
        V = VCycle(p, cells, quad, lam=E.LAME[lame][0], mu=E.LAME[lame][1], h_levels=h_levels, min_cells=min_cells)
        n = V.levels[0].pr.mesh.n_dofs
        s = np.stack([O.deterministic_src(n, seed=70 + c) for c in range(3)])
        s.setflags(write=False)
        _cache["v", name] = (V, s)
    return _cache["v", name]


def solve_case(name):
    """(VCycle, b): the mesh of elasticity_ref.cg_case("p4") and p = 2 on the same cells"""
    if ("s", name) not in _cache:
        p, cells = SOLVE_CASES[name]
        V = VCycle(p, cells)
        b = rhs(V.levels[0].pr)
        b.setflags(write=False)
        _cache["s", name] = (V, b)
    return _cache["s", name]


def chebyshev_case(p, degree, block_diagonal, smoothing_range=20.0, eig_its=8):
    """(Level, src, x0): one Chebyshev polynomial on (3, 2, 2) as bp5_elasticity_chebyshev_create builds it"""
    key = ("c", p, degree, block_diagonal)
    if key not in _cache:
        L = Level(p, CHEBYSHEV_CELLS, 1.0, O.QUAD_GAUSS, AMP, O.kappa_step64, E.LAME[0][0], E.LAME[0][1], degree, smoothing_range, eig_its, block_diagonal)
        n = L.pr.mesh.n_dofs
        src = np.stack([O.deterministic_src(n, seed=80 + c) for c in range(3)])
        x0 = np.stack([O.deterministic_src(n, seed=90 + c) for c in range(3)])
        for a in (src, x0):
            a.setflags(write=False)
        _cache[key] = (L, src, x0)
    return _cache[key]
