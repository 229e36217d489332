"""Mesh surgery in numpy: user meshes that lie between the library's own generator (every block a lattice block) and a random numbering
(no block a lattice block).  A UserMesh starts from the flat arrays of a generator mesh or from the oracle's lexicographic brick and is
altered by operations that keep the discrete operator the same up to the DoF permutation `new_of_old` they accumulate (old id -> new id;
the ring, which identifies two node planes, is the one exception: its map is many to one).  `namespace()` is what MatrixFree.reinit
takes (the fields of _hanging_namespace in tests/test_gpu_parity.py plus cell_block_offsets), `oracle_mesh()` what the numpy oracle takes.

Local entry (i, j, k) of a cell sits at i + n (j + n k) of its local_to_global row."""
from types import SimpleNamespace

import numpy as np

import bp5_oracle as O


# ------------------------------------------------------------------ the 24 proper rotations of the local frame
def rotations():
    """the 24 signed permutation matrices of determinant +1"""
    out = []
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for signs in range(8):
            M = np.zeros((3, 3), dtype=np.int64)
            for r in range(3):
                M[r, perm[r]] = -1 if signs >> r & 1 else 1
            if round(np.linalg.det(M)) == 1:
                out.append(M)
    return out


ROT90_Z = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1]])        # R(i, j, k) = (j, p - i, k)
ROT180_X = np.array([[1, 0, 0], [0, -1, 0], [0, 0, -1]])      # R(i, j, k) = (i, p - j, p - k)
ROT120_DIAG = np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]])     # R(i, j, k) = (j, k, i)


def rotation_gather(p, R):
    """g with l2g_new[c, f] = l2g_old[c, g[f]]: entry (i, j, k) of the new frame is entry R(i, j, k) of the old one.  R acts on the cell's
    centred local coordinates 2 (i, j, k) - p as a signed permutation matrix; only det +1 keeps the Jacobian positive."""
    R = np.asarray(R, dtype=np.int64)
    if R.shape != (3, 3) or not np.array_equal(np.abs(R).sum(0), [1, 1, 1]) or not np.array_equal(np.abs(R).sum(1), [1, 1, 1]):
        raise ValueError("R must be a signed permutation matrix")
    if round(np.linalg.det(R)) != 1:
        raise ValueError("only proper rotations (det +1): a reflection turns the cell inside out")
    n = p + 1
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    new = np.stack([i.ravel(), j.ravel(), k.ravel()])                  # column f = (i, j, k) of flat index f
    old = (R @ (2 * new - p) + p) // 2
    return old[0] + n * (old[1] + n * old[2])


class UserMesh:
    def __init__(self, p, l2g, coords, constrained, block_offsets=None, cells=None):
        self.p, self.n = p, p + 1
        self.l2g = np.array(l2g, dtype=np.int64).reshape(-1, self.n ** 3)
        self.coords = np.array(coords, dtype=np.float64).reshape(-1, 3)
        self.constrained = np.unique(np.asarray(constrained, dtype=np.int64))
        self.block_offsets = None if block_offsets is None else np.array(block_offsets, dtype=np.int64)
        self.cells = cells
        self.new_of_old = np.arange(self.n_dofs, dtype=np.int64)

    # -------------------------------------------------------------- starting meshes
    @classmethod
    def from_generator(cls, mesh):
        """the arrays of a library mesh (pkg.BrickMesh on one rank), copied"""
        assert mesh.n_ghost == 0 and mesh.n_ranks == 1
        return cls(mesh.degree, mesh.l2g, mesh.coords, mesh.constrained, mesh.cell_block_offsets, mesh.cells)

    @classmethod
    def ring(cls, p, nx, ny, nz):
        """an nx x ny x nz lexicographic brick of unit cubes whose node planes x = 0 and x = L are identified, bent into the annulus
        (r cos t, r sin t, z), t = -2 pi x / L (the sign keeps the Jacobian positive), r = 1 + y; Dirichlet on the r and z boundaries.
        new_of_old maps the brick's lexicographic ids onto the ring's (the plane x = L onto the plane x = 0)."""
        b = O.BrickMesh(p, (nx, ny, nz))
        I, J, K = np.meshgrid(np.arange(b.NX), np.arange(b.NY), np.arange(b.NZ), indexing="ij")
        lex = I + b.NX * (J + b.NY * K)
        ring_id = (I % (b.NX - 1)) + (b.NX - 1) * (J + b.NY * K)
        new_of_old = np.empty(b.n_dofs, dtype=np.int64)
        new_of_old[lex.ravel()] = ring_id.ravel()
        keep = (I < b.NX - 1).ravel()
        x = np.empty(((b.NX - 1) * b.NY * b.NZ, 3))
        t = -2.0 * np.pi * b.coords[:, 0] / b.L[0]
        r = 1.0 + b.coords[:, 1]
        xyz = np.stack([r * np.cos(t), r * np.sin(t), b.coords[:, 2]], axis=-1)
        x[ring_id.ravel()[keep]] = xyz[lex.ravel()[keep]]
        bnd = ((J == 0) | (J == b.NY - 1) | (K == 0) | (K == b.NZ - 1)).ravel()
        m = cls(p, new_of_old[b.l2g.astype(np.int64)], x, ring_id.ravel()[bnd], None, (nx, ny, nz))
        m.new_of_old = new_of_old
        return m

    # -------------------------------------------------------------- properties
    @property
    def n_dofs(self):
        return self.coords.shape[0]

    @property
    def n_cells(self):
        return self.l2g.shape[0]

    @property
    def n_blocks(self):
        return 0 if self.block_offsets is None else self.block_offsets.size - 1

    @property
    def old_of_new(self):
        return np.argsort(self.new_of_old)

    def block_of_cell(self):
        return np.repeat(np.arange(self.n_blocks), np.diff(self.block_offsets))

    def dof_blocks(self):
        """(n_dofs, n_blocks) bool: block b holds DoF d"""
        out = np.zeros((self.n_dofs, self.n_blocks), dtype=bool)
        boc = self.block_of_cell()
        out[self.l2g.ravel(), np.repeat(boc, self.n ** 3)] = True
        return out

    def block_interior_dofs(self, b):
        """DoFs of block b in no other block and not on the domain boundary: the interior entity of a brick of a generator mesh (sorted)"""
        db = self.dof_blocks()
        mask = db[:, b] & (db.sum(1) == 1)
        mask[self.constrained] = False
        return np.nonzero(mask)[0]

    def shared_face_dofs(self, a, b):
        """DoFs in exactly the blocks a and b: the interior of the face two bricks meet in (sorted)"""
        db = self.dof_blocks()
        mask = db[:, a] & db[:, b] & (db.sum(1) == 2)
        mask[self.constrained] = False
        return np.nonzero(mask)[0]

    # -------------------------------------------------------------- operations
    def renumber(self, step):
        """step: current id -> new id, a permutation"""
        step = np.asarray(step, dtype=np.int64)
        assert np.array_equal(np.sort(step), np.arange(self.n_dofs))
        self.l2g = step[self.l2g]
        coords = np.empty_like(self.coords)
        coords[step] = self.coords
        self.coords = coords
        self.constrained = np.sort(step[self.constrained])
        self.new_of_old = step[self.new_of_old]
        return self

    def swap_dofs(self, a, b):
        step = np.arange(self.n_dofs, dtype=np.int64)
        step[a], step[b] = b, a
        return self.renumber(step)

    def shift_dofs(self, k):
        return self.renumber((np.arange(self.n_dofs, dtype=np.int64) + k) % self.n_dofs)

    def rotate_cells(self, cells, R):
        g = rotation_gather(self.p, R)
        cells = np.atleast_1d(np.asarray(cells, dtype=np.int64))
        self.l2g[cells] = self.l2g[cells][:, g]
        return self

    def permute_cells(self, order):
        """new cell c = current cell order[c]; the block boundaries stay where they are"""
        order = np.asarray(order, dtype=np.int64)
        assert np.array_equal(np.sort(order), np.arange(self.n_cells))
        self.l2g = self.l2g[order]
        return self

    def shuffle_within_blocks(self, rng):
        order = np.arange(self.n_cells)
        for b in range(self.n_blocks):
            sl = slice(self.block_offsets[b], self.block_offsets[b + 1])
            order[sl] = rng.permutation(order[sl])
        return self.permute_cells(order)

    def sort_block_cells(self, b, slowest=2):
        """the cells of block b in lexicographic order of their centroids, direction `slowest` slowest (cells of one layer differ by a cell
        size, far more than the deformation moves a centroid)"""
        c0, c1 = int(self.block_offsets[b]), int(self.block_offsets[b + 1])
        cen = self.coords[self.l2g[c0:c1]].mean(axis=1)
        size = np.ptp(self.coords[self.l2g[c0]], axis=0).max()
        q = np.rint((cen - cen.min(axis=0)) / size).astype(np.int64)
        order = np.arange(self.n_cells)
        order[c0:c1] = c0 + np.lexsort([q[:, d] for d in range(3) if d != slowest] + [q[:, slowest]])
        return self.permute_cells(order)

    def permute_blocks(self, order):
        """new block b = current block order[b], its cells in their order; cell_block_offsets rebuilt"""
        order = np.asarray(order, dtype=np.int64)
        assert np.array_equal(np.sort(order), np.arange(self.n_blocks))
        off = self.block_offsets
        cells = np.concatenate([np.arange(off[b], off[b + 1]) for b in order])
        self.l2g = self.l2g[cells]
        self.block_offsets = np.concatenate([[0], np.cumsum(np.diff(off)[order])])
        return self

    def regroup(self, offsets):
        offsets = np.asarray(offsets, dtype=np.int64)
        assert offsets[0] == 0 and offsets[-1] == self.n_cells and np.all(np.diff(offsets) > 0)
        self.block_offsets = offsets
        return self

    def constrain(self, dofs):
        self.constrained = np.union1d(self.constrained, np.asarray(dofs, dtype=np.int64))
        return self

    # -------------------------------------------------------------- what the library and the oracle take
    def namespace(self):
        nd, nc = self.n_dofs, self.n_cells
        return SimpleNamespace(degree=self.p, n=self.n, cells=self.cells, n_cells=nc, n_interior_cells=nc, n_owned=nd, n_ghost=0, n_local=nd, n_global_dofs=nd,
                               l2g=self.l2g.astype(np.uint32), coords=np.ascontiguousarray(self.coords), constrained=self.constrained.astype(np.uint32),
                               global_ids=np.arange(nd, dtype=np.uint64), n_neighbors=0, neighbor_rank=np.zeros(0, np.int32),
                               send_offsets=np.zeros(1, np.uint32), send_indices=np.zeros(0, np.uint32), recv_offsets=np.zeros(1, np.uint32),
                               cell_block_offsets=None if self.block_offsets is None else self.block_offsets.astype(np.uint32),
                               constraint_mask=None, rank=0, n_ranks=1)

    def build(self):
        """(namespace, new_of_old)"""
        return self.namespace(), self.new_of_old.copy()

    def oracle_mesh(self):
        return SimpleNamespace(p=self.p, n=self.n, n_cells=self.n_cells, n_dofs=self.n_dofs, l2g=self.l2g.astype(np.uint32), coords=self.coords.copy(),
                               constrained=self.constrained.astype(np.uint32))


class Reference:
    """the oracle on a UserMesh: Gauss(p+1) or GLL tables, the merged metric with the step-64 coefficient, operator, diagonal, right-hand side"""

    def __init__(self, um, quadrature=O.QUAD_GAUSS, kappa=O.kappa_step64):
        self.mesh = um.oracle_mesh()
        _, _, self.w, self.N, self.D = O.shape_tables(um.p, quadrature)
        self.kappa = kappa
        self.coef = O.merged_metric(self.mesh, self.N, self.D, self.w, kappa)

    def apply_cells(self, s):
        return O.apply_cells(self.mesh, self.coef, self.N, self.D, s)

    def vmult(self, s):
        return O.vmult(self.mesh, self.coef, self.N, self.D, s)

    def rhs(self):
        return O.assemble_rhs(self.mesh)

    def diagonal(self):
        return O.operator_diagonal(self.mesh, self.coef, self.N, self.D)

    def JxW(self):
        return O.jacobians(self.mesh, self.N, self.D, self.w)[1]


def dense_transfer(fine, coarse):
    """the p-transfer's prolongation assembled from the arrays of two UserMeshes with the same cells in the same local frames:
    P[l2g_f[c, a], l2g_c[c, b]] = (M x M x M)[a, b] cell by cell (the entries agree wherever cells overlap), columns of coarse Dirichlet
    DoFs zeroed.  Dense: for the few-cell meshes of the transfer tests."""
    from multigrid_ref import lagrange_matrix
    M = lagrange_matrix(fine.p, coarse.p)
    M3 = np.kron(M, np.kron(M, M))                     # rows i + nf (j + nf k), columns likewise: z slowest
    P = np.zeros((fine.n_dofs, coarse.n_dofs))
    for c in range(fine.n_cells):
        P[np.ix_(fine.l2g[c], coarse.l2g[c])] = M3
    P[:, coarse.constrained] = 0.0
    return P
