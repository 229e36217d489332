"""tests/user_mesh.py pinned on the CPU: every operation of the mesh surgery keeps the discrete operator up to the DoF permutation it returns.

With A the oracle operator (merged metric with the step-64 coefficient, O.vmult) the check is A_altered(s[old_of_new])[new_of_old] ==
A_original(s) in relative l2, the oracle against itself, so the bound is rounding alone: the permuted operator sums the same products in
another order (cells in another order, sum factorisation along rotated axes).  Bound 1e-14, far below the operator tolerance 1e-13 of the GPU
tests that use these meshes.  Largest value measured per degree over all operations and compositions below (float64, numpy einsum):

    p = 2: 1.1e-16    p = 3: 5.4e-16    p = 4: 5.9e-16    p = 7: 3.8e-15

Also per operation: JxW > 0 at every quadrature point, the Dirichlet list is the image of the original one (plus what `constrain` added), the
blocks partition the cells.  The ring (the one operation that changes the operator): constants lie in the null space of the cell loop, and the
volume is that of the annulus."""
import math

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import multigrid_ref as G
import user_mesh as U

pkg = bp5_pkg.load()
TOL = 1e-14
CASES = {2: ((4, 4, 2), (2, 2, 2)), 3: ((4, 2, 2), (2, 2, 2)), 4: ((4, 2, 4), (2, 2, 2)), 7: ((2, 2, 2), (1, 2, 2))}   # p: cells, block
_cache, _worst = {}, {}


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _start(p):
    """(generator mesh, the oracle on its arrays, a source, A s): computed once per degree"""
    if p not in _cache:
        cells, block = CASES[p]
        g = pkg.BrickMesh(p, cells, h=0.25, deform_amp=0.03, cell_block=block, dof_numbering=1, cell_block_order=1)
        ref = U.Reference(U.UserMesh.from_generator(g))
        s = O.deterministic_src(g.n_owned, seed=5 + p)
        _cache[p] = (g, ref, s, ref.apply_cells(s))
    return _cache[p]


def _random_numbering(m, rng):
    return m.renumber(rng.permutation(m.n_dofs))


OPS = {
    "swap_dofs": lambda m, rng: m.swap_dofs(int(m.block_interior_dofs(0)[0]), int(m.block_interior_dofs(0)[-1])),
    "swap_dofs_across_entities": lambda m, rng: m.swap_dofs(int(m.block_interior_dofs(1)[0]), int(m.shared_face_dofs(0, 1)[0])),
    "shift_dofs": lambda m, rng: m.shift_dofs(m.n_dofs - sum(m.block_interior_dofs(b).size for b in range(m.n_blocks))),
    "rotate_cells_z90": lambda m, rng: m.rotate_cells([1], U.ROT90_Z),
    "rotate_cells_x180": lambda m, rng: m.rotate_cells([0, m.n_cells - 1], U.ROT180_X),
    "rotate_block": lambda m, rng: m.rotate_cells(np.arange(m.block_offsets[1], m.block_offsets[2]), U.ROT120_DIAG),
    "permute_cells": lambda m, rng: m.shuffle_within_blocks(rng),
    "permute_blocks": lambda m, rng: m.permute_blocks(np.arange(m.n_blocks)[::-1]),
    "regroup": lambda m, rng: m.regroup(np.concatenate([[0, m.block_offsets[1] - 1], m.block_offsets[2:]])),
    "constrain": lambda m, rng: m.constrain([m.block_interior_dofs(0)[0], m.shared_face_dofs(0, 1)[0]]),
    "rotate_1_4_and_renumber": lambda m, rng: _random_numbering(m.rotate_cells([1], U.ROT90_Z).rotate_cells([4], U.ROT180_X), rng),
    "everything": lambda m, rng: _random_numbering(m.permute_blocks(rng.permutation(m.n_blocks)).shuffle_within_blocks(rng), rng)
    .rotate_cells([0, 2, 3], U.ROT120_DIAG).shift_dofs(7).regroup([0, 3, m.n_cells - 2, m.n_cells]).constrain(np.setdiff1d(np.arange(m.n_dofs), m.constrained)[[0, -1]]),
}


@pytest.mark.parametrize("name", list(OPS))
@pytest.mark.parametrize("p", list(CASES))
def test_an_operation_keeps_the_operator_up_to_its_permutation(p, name):
    g, ref0, s, cells0 = _start(p)
    m = OPS[name](U.UserMesh.from_generator(g), np.random.default_rng(p))
    ns, new_of_old = m.build()
    old_of_new = np.argsort(new_of_old)
    assert np.array_equal(np.sort(new_of_old), np.arange(g.n_owned))
    # the Dirichlet list: ascending, unique, the image of the original list plus the added DoFs; same places in space
    c0 = np.asarray(g.constrained).astype(np.int64)
    c = ns.constrained.astype(np.int64)
    assert np.all(np.diff(c) > 0) and c[-1] < ns.n_local
    added = np.setdiff1d(c, new_of_old[c0])
    assert np.array_equal(np.union1d(new_of_old[c0], added), c) and added.size == (2 if name in ("constrain", "everything") else 0)
    assert np.array_equal(ns.coords[new_of_old], np.asarray(g.coords))
    # the blocks partition the cells, and the cells are the original cells (as DoF sets)
    off = ns.cell_block_offsets.astype(np.int64)
    assert off[0] == 0 and off[-1] == ns.n_cells == g.n_cells and np.all(np.diff(off) > 0)
    key = lambda l2g: sorted(tuple(sorted(row)) for row in np.asarray(l2g).astype(np.int64).tolist())
    assert key(old_of_new[ns.l2g.astype(np.int64)]) == key(g.l2g)
    # positive Jacobians, and the operator
    ref = U.Reference(m)
    assert ref.JxW().min() > 0.0
    old_added = old_of_new[added]
    want = cells0.copy()
    cc = np.concatenate([c0, old_added])
    want[cc] = s[cc]
    err = rel(ref.vmult(s[old_of_new])[new_of_old], want)
    _worst[p] = max(_worst.get(p, 0.0), err)
    print(f"surgery invariance p={p} {name}: {err:.2e} (largest so far at this degree {_worst[p]:.2e})")
    assert err <= TOL, (p, name, err)
    assert rel(ref.rhs()[new_of_old][~np.isin(np.arange(g.n_owned), cc)], ref0.rhs()[~np.isin(np.arange(g.n_owned), cc)]) <= TOL


def test_the_24_rotations_are_the_proper_ones_and_each_keeps_the_operator():
    Rs = U.rotations()
    assert len(Rs) == 24 and len({R.tobytes() for R in Rs}) == 24
    g, _, s, cells0 = _start(3)
    for R in Rs:
        gat = U.rotation_gather(3, R)
        assert np.array_equal(np.sort(gat), np.arange(64))
        m = U.UserMesh.from_generator(g).rotate_cells([2, 5], R)
        ref = U.Reference(m)
        assert ref.JxW().min() > 0.0 and rel(ref.apply_cells(s), cells0) <= TOL
    with pytest.raises(ValueError):
        U.rotation_gather(3, np.diag([1, 1, -1]))            # a reflection
    # the documented frames: ROT90_Z reads entry (j, p - i, k), ROT180_X entry (i, p - j, p - k)
    n, p = 4, 3
    f = lambda i, j, k: i + n * (j + n * k)
    assert U.rotation_gather(p, U.ROT90_Z)[f(1, 0, 2)] == f(0, p - 1, 2) and U.rotation_gather(p, U.ROT180_X)[f(1, 0, 2)] == f(1, p, p - 2)


def _circle_area(p, nx):
    """area enclosed by the degree-p GLL interpolant of the unit circle over nx equal arcs: nx / 2 * int_0^1 (x y' - y x') d xi with a quadrature
    that is exact for it, and the largest radial deviation of the interpolant from the circle"""
    nodes, _ = O.gll_01(p + 1)
    xi, w = O.gauss_01(2 * p + 2)
    N, D = O.lagrange_tables(nodes, xi)
    t = 2.0 * np.pi / nx * nodes
    x, y, dx, dy = N @ np.cos(t), N @ np.sin(t), D @ np.cos(t), D @ np.sin(t)
    fine = np.linspace(0.0, 1.0, 2001)
    Nf, _ = O.lagrange_tables(nodes, fine)
    return 0.5 * nx * float(w @ (x * dy - y * dx)), float(np.abs(np.hypot(Nf @ np.cos(t), Nf @ np.sin(t)) - 1.0).max())


@pytest.mark.parametrize("p,nx,ny,nz", [(2, 4, 1, 2), (3, 3, 1, 2), (4, 4, 1, 2), (4, 2, 1, 2), (2, 2, 1, 2), (7, 3, 2, 1)])
def test_ring(p, nx, ny, nz):
    m = U.UserMesh.ring(p, nx, ny, nz)
    ns, new_of_old = m.build()
    NX = p * nx + 1
    assert ns.n_local == (NX - 1) * (p * ny + 1) * (p * nz + 1) and new_of_old.size == NX * (p * ny + 1) * (p * nz + 1)
    lex = np.arange(new_of_old.size)
    assert np.array_equal(new_of_old[lex % NX == NX - 1], new_of_old[lex % NX == 0])          # the two planes are one
    assert np.unique(new_of_old).size == ns.n_local
    for c in range(m.n_cells):
        assert np.unique(m.l2g[c]).size == (p + 1) ** 3 - ((p + 1) ** 2 if nx == 1 else 0)
    r = np.hypot(ns.coords[:, 0], ns.coords[:, 1])
    on_bnd = (np.abs(r - 1.0) < 1e-12) | (np.abs(r - 1.0 - ny) < 1e-12) | (np.abs(ns.coords[:, 2]) < 1e-12) | (np.abs(ns.coords[:, 2] - nz) < 1e-12)
    assert np.array_equal(np.nonzero(on_bnd)[0], ns.constrained.astype(np.int64))
    ref = U.Reference(m)
    JxW = ref.JxW()
    assert JxW.min() > 0.0
    # the volume: exactly that of the interpolated annulus (the radial and axial maps are linear), and the true one within the interpolation
    # error: the interpolated circle stays within d of the unit circle and winds once, so its area lies in [pi (1 - d)^2, pi (1 + d)^2]
    area, d = _circle_area(p, nx)
    ring = ((1 + ny) ** 2 - 1) * nz
    print(f"ring p={p} nx={nx}: min JxW {JxW.min():.2e}, volume {JxW.sum():.4f} (annulus {math.pi * ring:.4f}), radial deviation {d:.1e}")
    assert abs(JxW.sum() - area * ring) <= 1e-12 * area * ring
    assert abs(JxW.sum() - math.pi * ring) <= (2 * d + d * d) * math.pi * ring
    # constants lie in the null space of the cell loop (nothing constrained there)
    s = O.deterministic_src(ns.n_local, seed=9)
    assert np.linalg.norm(ref.apply_cells(np.ones(ns.n_local))) <= 1e-12 * np.linalg.norm(ref.apply_cells(s))
    # symmetric: <A s, t> = <s, A t>
    t = O.deterministic_src(ns.n_local, seed=10)
    assert abs(ref.apply_cells(s) @ t - s @ ref.apply_cells(t)) <= 1e-12 * abs(ref.apply_cells(s) @ t)


def test_dense_transfer_is_the_lexicographic_one_and_follows_rotations():
    """dense_transfer (the reference of the GPU transfer test on rotated frames) against the sweep form of tests/multigrid_ref.py on the
    oracle's brick; rotating BOTH meshes' cells by one R changes nothing, rotating one of them does"""
    cells = (1, 1, 3)
    bf, bc = O.BrickMesh(4, cells), O.BrickMesh(2, cells)
    mk = lambda b: U.UserMesh(b.p, b.l2g, b.coords, b.constrained, None, cells)
    P = U.dense_transfer(mk(bf), mk(bc))
    T = G.Transfer(cells, 4, 2)
    rng = np.random.default_rng(3)
    ec, rf = rng.uniform(-1, 1, bc.n_dofs), rng.uniform(-1, 1, bf.n_dofs)
    assert rel(P @ ec, T.prolongate(ec)) <= 1e-14 and rel(P.T @ rf, T.restrict(rf)) <= 1e-14
    for R in (U.ROT90_Z, U.ROT180_X, U.ROT120_DIAG):
        both = U.dense_transfer(mk(bf).rotate_cells(np.arange(3), R), mk(bc).rotate_cells(np.arange(3), R))
        assert np.abs(both - P).max() <= 4e-16          # (the rows of M read backwards are M's mirror image up to rounding)
        one = U.dense_transfer(mk(bf).rotate_cells(np.arange(3), R), mk(bc))
        # (a quarter turn about the column's axis maps the five unconstrained coarse functions, which sit on the axis, onto themselves)
        assert np.allclose(one, P) == (R is U.ROT90_Z)
