"""Numpy reference of the trilinear geometry mode (BP5_GEOM_TRILINEAR; deal.II MappingQ1): a cell is the trilinear image of its eight vertices.

`trilinearise` makes any mesh such a mesh, `deviation` is the library's acceptance measure, `vertex_metric` the closed form of the six planes from the
vertices alone -- written from the monomial coefficients of the map, not in the library's convex-combination form, so that the two do not share
their arithmetic.  The reference OPERATOR of the GPU tests is the oracle's ordinary degree-p one on the trilinearised coordinates: a degree-p mapping
reproduces a trilinear map exactly (tests/test_trilinear_cpu.py pins that against vertex_metric).

Vertex v = a + 2 b + 4 c of a cell is its corner (xi, eta, zeta) = (a, b, c), the local entry (a p, b p, c p)."""
import numpy as np

import bp5_oracle as O

AMP = 0.04
KAPPA = {0: O.kappa_none, 1: O.kappa_step64}


def vertex_entries(p):
    """local indices i + n (j + n k) of the eight corners, v = a + 2 b + 4 c"""
    n = p + 1
    return np.array([a * p + n * (b * p + n * c * p) for c in (0, 1) for b in (0, 1) for a in (0, 1)], dtype=np.int64)


def cell_vertices(mesh):
    """[n_cells][8][3]; mesh: anything with p, l2g [n_cells][n^3] and coords [n_dofs][3]"""
    l2g = np.asarray(mesh.l2g, dtype=np.int64).reshape(-1, (mesh.p + 1) ** 3)
    return np.asarray(mesh.coords)[l2g[:, vertex_entries(mesh.p)]]


def _phi(t):
    """[len(t)][2]: the two linear shape functions at t"""
    t = np.asarray(t, dtype=np.float64)
    return np.stack([1.0 - t, t], axis=-1)


def trilinear_image(V, t):
    """x(t_i, t_j, t_k) of every cell, [n_cells][len(t)^3][3] with the point index i + m (j + m k)"""
    F = _phi(t)
    Vc = V.reshape(-1, 2, 2, 2, 3)                                              # [cell][c][b][a][e]
    X = np.einsum("kc,jb,ia,zcbae->zkjie", F, F, F, Vc)
    return X.reshape(V.shape[0], -1, 3)


def trilinearise(um):
    """every cell's node coordinates become the trilinear image of its eight vertices (a UserMesh or an oracle mesh, changed in place and returned).
    Consistent across shared faces and edges: the image on a face depends on that face's four vertices only."""
    nodes = O.shape_tables(um.p, O.QUAD_GAUSS)[0]
    l2g = np.asarray(um.l2g, dtype=np.int64).reshape(-1, (um.p + 1) ** 3)
    X = trilinear_image(cell_vertices(um), nodes)
    coords = np.array(um.coords, dtype=np.float64)
    coords[l2g.ravel()] = X.reshape(-1, 3)
    back = coords[l2g] - X                                                      # cells that share a node agree on it to rounding
    assert np.abs(back).max() <= 1e-15 * max(1.0, np.abs(coords).max())
    um.coords = coords
    return um


def deviation(mesh):
    """per cell: the largest distance between a stored node and the trilinear image of its reference position, over the cell's shortest edge --
    what bp5_mf_set_geometry_mode(BP5_GEOM_TRILINEAR) compares with 1e-10"""
    nodes = O.shape_tables(mesh.p, O.QUAD_GAUSS)[0]
    l2g = np.asarray(mesh.l2g, dtype=np.int64).reshape(-1, (mesh.p + 1) ** 3)
    V = cell_vertices(mesh)
    dist = np.linalg.norm(np.asarray(mesh.coords)[l2g] - trilinear_image(V, nodes), axis=-1).max(axis=1)
    edges = [(v, v | 1 << d) for d in range(3) for v in range(8) if not v & 1 << d]
    shortest = np.min([np.linalg.norm(V[:, b] - V[:, a], axis=-1) for a, b in edges], axis=0)
    return dist / shortest


def vertex_metric(V, pts, w, kappa=O.kappa_none):
    """the six planes kappa(x_q) JxW K K^T of the cells with vertices V [n_cells][8][3] at the tensor points pts with weights w, in the oracle's
    layout [6][n_cells][qi + n (qj + n qk)] -- from the monomial form x = c0 + cx xi + cy eta + cz zeta + cxy xi eta + cxz xi zeta + cyz eta zeta +
    cxyz xi eta zeta"""
    Vc = V.reshape(-1, 2, 2, 2, 3)                                              # [cell][c][b][a][e]
    v = lambda a, b, c: Vc[:, c, b, a]
    c0 = v(0, 0, 0)
    cx, cy, cz = v(1, 0, 0) - c0, v(0, 1, 0) - c0, v(0, 0, 1) - c0
    cxy = v(1, 1, 0) - v(1, 0, 0) - v(0, 1, 0) + c0
    cxz = v(1, 0, 1) - v(1, 0, 0) - v(0, 0, 1) + c0
    cyz = v(0, 1, 1) - v(0, 1, 0) - v(0, 0, 1) + c0
    cxyz = v(1, 1, 1) - v(1, 1, 0) - v(1, 0, 1) - v(0, 1, 1) + v(1, 0, 0) + v(0, 1, 0) + v(0, 0, 1) - c0
    n = len(pts)
    zeta, eta, xi = [a.ravel() for a in np.meshgrid(pts, pts, pts, indexing="ij")]                  # q = qi + n (qj + n qk)
    W = (w[:, None, None] * w[None, :, None] * w[None, None, :]).ravel()
    e = lambda c: c[:, None, :]                                                 # [cell][1][e]
    s = lambda t: t[None, :, None]                                              # [1][q][1]
    x = e(c0) + e(cx) * s(xi) + e(cy) * s(eta) + e(cz) * s(zeta) + e(cxy) * s(xi * eta) + e(cxz) * s(xi * zeta) + e(cyz) * s(eta * zeta) + e(cxyz) * s(xi * eta * zeta)
    J = np.empty(x.shape + (3,))                                                # J[cell][q][e][d] = d x_e / d xi_d
    J[..., 0] = e(cx) + e(cxy) * s(eta) + e(cxz) * s(zeta) + e(cxyz) * s(eta * zeta)
    J[..., 1] = e(cy) + e(cxy) * s(xi) + e(cyz) * s(zeta) + e(cxyz) * s(xi * zeta)
    J[..., 2] = e(cz) + e(cxz) * s(xi) + e(cyz) * s(eta) + e(cxyz) * s(xi * eta)
    K = np.linalg.inv(J)
    G = np.einsum("cqdf,cqef->cqde", K, K)
    sc = np.abs(np.linalg.det(J)) * W[None] * kappa(x)
    assert n ** 3 == x.shape[1]
    return np.ascontiguousarray(np.stack([sc * G[:, :, d, f] for (d, f) in O.PLANE_PAIRS], axis=0))


def user_mesh(pkg, p, cells, amp=AMP, **brick):
    """the GPU tests' mesh: the generator's sine mesh with its coordinates trilinearised (tests/user_mesh.py: namespace() feeds the library,
    oracle_mesh() the oracle)"""
    from user_mesh import UserMesh
    return trilinearise(UserMesh.from_generator(pkg.BrickMesh(p, cells, deform_amp=amp, **brick)))
