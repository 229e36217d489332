"""The trilinear geometry mode (BP5_GEOM_TRILINEAR) without a GPU: the reference of tests/test_gpu_trilinear.py -- the oracle's ordinary degree-p
operator on trilinearised coordinates -- pinned outside itself against the closed-form vertex metric of tests/trilinear_ref.py, the test meshes shown
to be really deformed, and the acceptance measure of the mode on meshes it must refuse and meshes it must take."""
import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import trilinear_ref as T
from user_mesh import Reference, UserMesh

pkg = bp5_pkg.load()
AMP = T.AMP
# The sine displacement is a product of sin(2 pi x_d / L_d): it vanishes at every vertex of a mesh with one or two cells in some direction.  The
# trilinearised (3, 2, 2) and (13, 1, 1) meshes -- the launch-shape cases of the GPU parity test -- are therefore the UNDEFORMED bricks (still far from
# the sine mesh, whose inner nodes move); (3, 3, 3) is the smallest mesh whose cells keep skewed, non-parallel faces.
CELLS = (3, 2, 2)
SKEWED = (3, 3, 3)
QUADS = {"gauss": O.QUAD_GAUSS, "gll": O.QUAD_GLL}


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def sine_mesh(p, cells=CELLS, amp=AMP):
    return UserMesh.from_generator(pkg.BrickMesh(p, cells, deform_amp=amp))


@pytest.mark.parametrize("quad", sorted(QUADS))
@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_oracle_planes_equal_the_closed_form_vertex_metric(p, quad):
    """a degree-p mapping reproduces a trilinear map exactly: the oracle's six planes on the trilinearised nodes are the closed form from the eight
    vertices, to 1e-13, with either coefficient"""
    um = T.user_mesh(pkg, p, SKEWED)
    _, pts, w, _, _ = O.shape_tables(p, QUADS[quad])
    for kappa in (O.kappa_none, O.kappa_step64):
        got = Reference(um, QUADS[quad], kappa).coef
        want = T.vertex_metric(T.cell_vertices(um), pts, w, kappa)
        e = max(rel(got[c], want[c]) for c in range(3))
        eo = rel(got, want)
        print(f"p={p} {quad} {kappa.__name__}: diagonal planes {e:.2e}, all six {eo:.2e}")
        assert got.shape == want.shape and e <= 1e-13 and eo <= 1e-13


def test_the_p1_sine_mesh_is_trilinear_as_generated():
    um = sine_mesh(1)
    before = um.coords.copy()
    assert np.all(T.deviation(um) == 0.0)
    T.trilinearise(um)
    assert np.array_equal(um.coords, before)
    _, pts, w, _, _ = O.shape_tables(1, O.QUAD_GAUSS)
    a, b = Reference(sine_mesh(1)).coef, Reference(um).coef
    assert np.array_equal(a, b)


@pytest.mark.parametrize("cells", [CELLS, SKEWED])
@pytest.mark.parametrize("p", [2, 4])
def test_the_test_mesh_is_deformed_and_the_two_operators_differ(p, cells):
    """deform_amp = 0.04 moves the inner nodes of the sine mesh off the trilinear image: the two operators differ by more than 1e-3, so a kernel that
    read the sine mesh's nodes could not pass the GPU parity test; and on (3, 3, 3) K K^T varies inside a cell by more than a percent, so neither
    could one that took the cells for parallelepipeds"""
    sine, tri = sine_mesh(p, cells), T.user_mesh(pkg, p, cells)
    assert np.abs(sine.coords - tri.coords).max() > 1e-4
    src = O.deterministic_src(sine.n_dofs, seed=60 + p)
    a, b = Reference(sine, kappa=O.kappa_none).vmult(src), Reference(tri, kappa=O.kappa_none).vmult(src)
    print(f"p={p}: |A_sine s - A_tri s| / |A_tri s| = {rel(a, b):.2e}")
    assert rel(a, b) > 1e-3
    if cells != SKEWED:
        return
    G = Reference(tri, kappa=O.kappa_none).coef
    _, _, w, _, _ = O.shape_tables(p, O.QUAD_GAUSS)
    W = (w[:, None, None] * w[None, :, None] * w[None, None, :]).ravel()
    spread = np.ptp(G[0] / W, axis=1) / np.abs(G[0] / W).max(axis=1)
    assert spread.max() > 1e-2


@pytest.mark.parametrize("p", [2, 4, 8])
def test_the_deviation_measure_flags_the_sine_mesh(p):
    d = T.deviation(sine_mesh(p))
    print(f"p={p}: deviation of the sine mesh {d.min():.2e} .. {d.max():.2e} (threshold 1e-10)")
    assert d.max() > 1e-4 and d.min() > 1e-7               # orders of magnitude over 1e-10, in every cell


@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_the_deviation_measure_passes_affine_and_trilinearised_meshes(p):
    flat = sine_mesh(p, amp=0.0)
    assert T.deviation(flat).max() <= 1e-14
    sheared = sine_mesh(p, amp=0.0)
    sheared.coords = sheared.coords @ np.array([[1.0, 0.2, 0.0], [0.1, 0.9, 0.3], [0.0, -0.2, 1.1]]) + np.array([0.3, -0.1, 0.2])
    assert T.deviation(sheared).max() <= 1e-14
    for cells in (CELLS, (13, 1, 1), SKEWED):
        d = T.deviation(T.user_mesh(pkg, p, cells))
        print(f"p={p} {cells}: deviation of the trilinearised mesh {d.max():.2e}")
        assert d.max() <= 1e-14                            # rounding: four orders below the threshold
