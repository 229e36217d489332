"""One quantity, three setup kernels: rho(x_q) JxW at the quadrature points is the one plane of a mass handle (mass_plane_kernel), plane 6 of a
Helmholtz handle with the same coefficient (geometry_kernel) and plane 9 of the elasticity metric (elasticity_metric_kernel).  All three take
it from the same per-cell prologue (cell_point) by the same expression, so the three arrays agree -- to rounding, not to the bit: the compiler
fuses multiply-adds kernel by kernel, and at p = 8 one entry of mass_plane_kernel's plane differs from the other two in the last place (it did
before the prologue was shared, too: profiles/setup_refactor/README.md).  The bound is the one test_merged_metric holds the planes to against the oracle."""
import numpy as np
import pytest

import bp5_pkg

pytestmark = pytest.mark.gpu
pkg = bp5_pkg.load()


@pytest.mark.parametrize("p", [1, 3, 8])
def test_mass_plane_is_helmholtz_plane_6_is_elasticity_plane_9(p):
    mesh = pkg.BrickMesh(p, (3, 2, 2), deform_amp=0.04)
    N = mesh.n_cells * (p + 1) ** 3                      # entries of one plane; every handle here is plane-major, each plane in the pair layout
    mass = pkg.MassOperator(mesh, pkg.QUAD_GAUSS, 1).coef.cpu().numpy()[:N]
    helmholtz = pkg.HelmholtzOperator(mesh, pkg.QUAD_GAUSS, 1).coef.cpu().numpy()[6 * N:7 * N]
    elasticity = pkg.ElasticityOperator(mesh, pkg.QUAD_GAUSS, 1).coef.cpu().numpy()[9 * N:10 * N]
    assert mass.size == helmholtz.size == elasticity.size == N and np.all(mass > 0.0)
    bound = 1e-13 * np.abs(mass).max()
    for name, plane in (("Helmholtz plane 6", helmholtz), ("elasticity plane 9", elasticity)):
        err = np.abs(plane - mass).max()
        print(f"p = {p}: max |{name} - mass plane| = {err:.3e} ({np.count_nonzero(plane != mass)} of {N} entries differ), bound {bound:.3e}")
        assert err < bound
