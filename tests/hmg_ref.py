"""numpy reference of the geometric (h) multigrid transfer and the hybrid p-then-h V-cycle (include/bp5.h:
bp5_mg_transfer_create_geometric, bp5_mg_*), on the oracle's lexicographic BrickMesh.  The 1-D factor of a direction holds M_s[a][b] =
phi_b(xi_a / 2 + s / 2) in rows p (2c + s) + a, columns p c + b; the global prolongation is the Kronecker product of the three factors,
applied by multigrid_ref.Transfer's sweeps.  The V-cycle is multigrid_ref.VCycle's recursion over multigrid_ref.Level /
Transfer, with the h-levels on O.Problem(..., h = 2^k h)."""
import numpy as np

import bp5_oracle as O
import multigrid_ref as G


def geometric_matrices(p):
    """[M_0, M_1], M_s[a][b] = phi_b^p(xi_a / 2 + s / 2) on the FE_Q (GLL) nodes; rows on a coarse node exact unit rows"""
    x, _ = O.gll_01(p + 1)
    out = []
    for s in (0, 1):
        xa = 0.5 * x + 0.5 * s
        M = np.ones((p + 1, p + 1))
        for b in range(p + 1):
            for m in range(p + 1):
                if m != b:
                    M[:, b] *= (xa - x[m]) / (x[b] - x[m])
        for a in range(p + 1):
            hit = np.nonzero(np.abs(xa[a] - x) < 1e-12)[0]
            if hit.size:
                M[a] = 0.0
                M[a, hit[0]] = 1.0
        out.append(M)
    return out


def geometric_prolongation_1d(p, n_coarse):
    """the 1-D factor along a direction of n_coarse coarse cells: rows p (2c + s) + a, columns p c + b hold M_s[a][b]"""
    Ms = geometric_matrices(p)
    P = np.zeros((2 * p * n_coarse + 1, p * n_coarse + 1))
    for c in range(n_coarse):
        for s in (0, 1):
            P[p * (2 * c + s):p * (2 * c + s) + p + 1, p * c:p * c + p + 1] = Ms[s]
    return P


class GeometricTransfer(G.Transfer):
    """P Z_c and Z_c P^T between the lexicographic degree-p meshes of 2 x cells_c and cells_c cells (Z_c: coarse Dirichlet entries 0)"""

    def __init__(self, cells_c, p):
        self.cells, self.pf, self.pc = tuple(2 * n for n in cells_c), p, p
        self.cells_c = tuple(cells_c)
        self.P1 = [geometric_prolongation_1d(p, n) for n in self.cells_c]
        self.shape_f = tuple(2 * p * n + 1 for n in self.cells_c[::-1])
        self.shape_c = tuple(p * n + 1 for n in self.cells_c[::-1])
        bc = np.zeros(self.shape_c, dtype=bool)
        bc[0], bc[-1], bc[:, 0], bc[:, -1], bc[:, :, 0], bc[:, :, -1] = True, True, True, True, True, True
        self.boundary_c = bc.ravel()


def coarsen(cells, min_cells=4, n_ranks=1):
    """BrickMesh.coarsen's rule: half the cells, or None (odd count, fewer than min_cells, or a slab split that does not nest)"""
    n2, R_ = cells[2], n_ranks
    if any(c % 2 or c // 2 < min_cells for c in cells):
        return None
    if any(n2 * r // R_ != 2 * ((n2 // 2) * r // R_) for r in range(R_ + 1)):
        return None
    return tuple(c // 2 for c in cells)


def hierarchy(p, cells, h_levels="max", min_cells=4, n_ranks=1):
    """[(degree, cells, h)] fine to coarse: p, p // 2, ..., 1 on cells (h = 1), then degree 1 on coarsened meshes"""
    out = [(q, tuple(cells), 1.0) for q in G.degrees(p)]
    while h_levels == "max" or len(out) - len(G.degrees(p)) < h_levels:
        c = coarsen(out[-1][1], min_cells, n_ranks)
        if c is None:
            break
        out.append((1, c, 2.0 * out[-1][2]))
    return out


class Level(G.Level):
    """multigrid_ref.Level on a mesh of cell size h (Poisson or Helmholtz operator)"""

    def __init__(self, p, cells, h, quadrature, deform_amp, kappa, degree, smoothing_range, eig_its, operator="poisson"):
        super().__init__(p, cells, quadrature, deform_amp, kappa, degree, smoothing_range, eig_its, h=h, operator=operator)


class HybridVCycle(G.VCycle):
    """PreconditionMG of bp5_mg_create on hierarchy(p, cells, h_levels): p-transfers between different degrees, geometric transfers
    between the degree-1 levels"""

    def __init__(self, p, cells, quadrature=O.QUAD_GAUSS, deform_amp=0.0, kappa=O.kappa_none, h_levels="max", min_cells=4,
                 smoother_degree=4, smoothing_range=20.0, eig_cg_n_iterations=10, coarse_degree=60, coarse_range=1000.0,
                 coarse_eig_cg_n_iterations=30, operator="poisson"):
        self.spec = hierarchy(p, cells, h_levels, min_cells)
        self.levels = []
        for lev, (q, c, h) in enumerate(self.spec):
            last = lev + 1 == len(self.spec)
            self.levels.append(Level(q, c, h, quadrature, deform_amp, kappa, coarse_degree if last else smoother_degree,
                                     coarse_range if last else smoothing_range, coarse_eig_cg_n_iterations if last else eig_cg_n_iterations,
                                     operator=operator))
        self.transfers = [G.Transfer(fc, pf, pc) if pf != pc else GeometricTransfer(cc, pc)
                          for (pf, fc, _), (pc, cc, _) in zip(self.spec[:-1], self.spec[1:])]
