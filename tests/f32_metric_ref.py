"""numpy reference of the operators and the V-cycle on FP32 metric planes (include/bp5.h: bp5_mf_set_metric_precision): the arithmetic of
multigrid_ref / hmg_ref in double, on planes that hold float values.  A level takes its planes as given (the planes read back from the
library, widened: bp5_mf_metric_to_reference_layout, in the oracle's lexicographic cell order) or rounds the oracle's own planes through
np.float32; its diagonal (O.operator_diagonal) and its Chebyshev bounds (CG-Lanczos) are computed from THOSE planes.  Not a test."""
import numpy as np

import bp5_oracle as O
import chebyshev_ref as R
import hmg_ref as H
import multigrid_ref as G


def round_planes(coef):
    """every entry rounded once to the nearest float and widened again (exact)"""
    return np.asarray(coef).astype(np.float32).astype(np.float64)


class Level(H.Level):
    """hmg_ref.Level (a multigrid_ref.Level on a mesh of cell size h) whose Poisson operator, inverse diagonal and Chebyshev bounds come
    from `planes` ([6][n_cells][n^3], lexicographic cells; None: the oracle's planes rounded through float32)"""

    def __init__(self, p, cells, h, quadrature, deform_amp, kappa, degree, smoothing_range, eig_its, planes=None):
        self.pr = O.Problem(p, cells, quadrature, h=h, deform_amp=deform_amp, kappa=kappa)
        self.coef64 = self.pr.coef
        self.pr.coef = round_planes(self.pr.coef) if planes is None else np.ascontiguousarray(planes, dtype=np.float64).reshape(self.pr.coef.shape)
        m = self.pr.mesh
        self.inv = 1.0 / O.operator_diagonal(m, self.pr.coef, self.pr.N, self.pr.D)
        v = R.start_vector(np.arange(m.n_dofs), m.constrained)
        self.min_est, self.max_est, self.cg_its = R.lanczos_estimate(self.pr.vmult, self.inv, v, eig_its)
        self.min_used, self.max_used = R.bounds(self.min_est, self.max_est, smoothing_range)
        self.degree = degree


class VCycle(G.VCycle):
    """hmg_ref.HybridVCycle (h_levels = 0: multigrid_ref.VCycle) with every level on float planes; planes: one array per level, or None"""

    def __init__(self, p, cells, quadrature=O.QUAD_GAUSS, deform_amp=0.0, kappa=O.kappa_none, h_levels=0, min_cells=4, planes=None,
                 smoother_degree=4, smoothing_range=20.0, eig_cg_n_iterations=10, coarse_degree=60, coarse_range=1000.0,
                 coarse_eig_cg_n_iterations=30):
        self.spec = H.hierarchy(p, cells, h_levels, min_cells)
        assert planes is None or len(planes) == len(self.spec), "one plane array per level"
        self.levels = []
        for lev, (q, c, h) in enumerate(self.spec):
            last = lev + 1 == len(self.spec)
            self.levels.append(Level(q, c, h, quadrature, deform_amp, kappa, coarse_degree if last else smoother_degree,
                                     coarse_range if last else smoothing_range, coarse_eig_cg_n_iterations if last else eig_cg_n_iterations,
                                     planes=None if planes is None else planes[lev]))
        self.transfers = [G.Transfer(fc, pf, pc) if pf != pc else H.GeometricTransfer(cc, pc)
                          for (pf, fc, _), (pc, cc, _) in zip(self.spec[:-1], self.spec[1:])]


def lexicographic_cells(mesh):
    """for a library BrickMesh (any cell order, one rank): the oracle's lexicographic index cx + n0 (cy + n1 cz) of every cell, from the
    global id of the cell's first local DoF (I, J, K) = p (cx, cy, cz)"""
    p = mesh.degree
    n0, n1, _ = (int(c) for c in mesh.cells)
    NX, NY = p * n0 + 1, p * n1 + 1
    l2g = np.asarray(mesh.l2g).reshape(mesh.n_cells, -1).astype(np.int64)
    g = np.asarray(mesh.global_ids).astype(np.int64)[l2g[:, 0]]
    I, J, K = g % NX, (g // NX) % NY, g // (NX * NY)
    assert not (I % p).any() and not (J % p).any() and not (K % p).any()
    return I // p + n0 * (J // p + n1 * (K // p))


def planes_to_lexicographic(mesh, planes):
    """planes [6][n_cells][n^3] in the mesh's own cell order -> the oracle's cell order"""
    planes = np.asarray(planes).reshape(6, mesh.n_cells, -1)
    out = np.empty_like(planes)
    out[:, lexicographic_cells(mesh)] = planes
    return out
