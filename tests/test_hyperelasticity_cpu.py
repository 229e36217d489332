"""tests/hyperelasticity_ref.py pinned outside itself (no GPU): the residual is the gradient of the energy and the tangent the derivative of the
residual by central differences, the tangent at u = 0 is the linear elasticity operator, it is symmetric, a rigid rotation carries no stress
(where the linear operator does), a homogeneous stretch gives the closed-form energy and stress power.  Then the properties the GPU tests rely on:
how far the parity references move under input noise, the stability of the fixed-iteration CG references, and what the two Newton cases deliver.
p = 2 and 3 on (3, 2, 2) cells, deformed 0.04, step-64 kappa, both Lame pairs of elasticity_ref.LAME."""
import numpy as np
import pytest

import bp5_oracle as O
import elasticity_mg_ref as M
import elasticity_ref as E
import hyperelasticity_ref as H

CELLS, AMP = (3, 2, 2), 0.04
CASES = [(p, lame) for p in (2, 3) for lame in (0, 1)]
_cache = {}


def _problem(p, lame):
    if (p, lame) not in _cache:
        pr = H.Problem(p, CELLS, O.QUAD_GAUSS, deform_amp=AMP, kappa=O.kappa_step64, lam=E.LAME[lame][0], mu=E.LAME[lame][1])
        rng = np.random.default_rng(1)
        u = H.smooth_displacement(pr, 0.2)
        v, w = rng.uniform(-1, 1, u.shape), rng.uniform(-1, 1, u.shape)
        for a in (u, v, w):
            a.setflags(write=False)
        _cache[p, lame] = (pr, u, v, w)
    return _cache[p, lame]


# Central differences with step eps: truncation ~ eps^2, rounding ~ 1e-16 / eps.  Measured on these four cases (relative error of the directional
# derivative, eps = 1e-4, 3e-5, 1e-5, 3e-6, 1e-6, 3e-7):
#   energy -> <residual, v>:   1.6e-6 .. 2.4e-6, 1.3e-7 .. 2.1e-7, 8.6e-9 .. 2.4e-8, 7.8e-10 .. 2.0e-9, 1.0e-10 .. 6.8e-10, 1.3e-10 .. 1.7e-9
#   residual -> tangent(u, v): 9.0e-8 .. 9.4e-7, 8.1e-9 .. 8.4e-8, 9.0e-10 .. 9.4e-9, 8.2e-11 .. 8.4e-10, 2.4e-11 .. 9.0e-11, 3.8e-11 .. 7.6e-11
# Both curves are flattest at eps = 1e-6 (the eps^2 branch meets the rounding branch there): floors 6.8e-10 and 9.0e-11.  The bounds are 10 x those.
FD_EPS = 1e-6
GRADIENT_BOUND = 10 * 6.8e-10
TANGENT_BOUND = 10 * 9.0e-11


@pytest.mark.parametrize("p,lame", CASES)
def test_residual_is_the_gradient_of_the_energy(p, lame):
    pr, u, v, _ = _problem(p, lame)
    fd = (pr.energy(u + FD_EPS * v) - pr.energy(u - FD_EPS * v)) / (2 * FD_EPS)
    rv = float(np.sum(pr.residual_cells(u) * v))
    err = abs(fd - rv) / abs(rv)
    print(f"p={p} lame={E.LAME[lame]}: <residual, v> {rv:.12e}, central difference {fd:.12e}, relative {err:.2e}")
    assert err <= GRADIENT_BOUND


@pytest.mark.parametrize("p,lame", CASES)
def test_tangent_is_the_derivative_of_the_residual(p, lame):
    pr, u, v, _ = _problem(p, lame)
    fd = (pr.residual_cells(u + FD_EPS * v) - pr.residual_cells(u - FD_EPS * v)) / (2 * FD_EPS)
    tv = pr.tangent_cells(u, v)
    err = np.linalg.norm(fd - tv) / np.linalg.norm(tv)
    print(f"p={p} lame={E.LAME[lame]}: relative {err:.2e}")
    assert err <= TANGENT_BOUND


@pytest.mark.parametrize("p,lame", CASES)
def test_tangent_at_zero_is_the_linear_operator(p, lame):
    pr, u, v, _ = _problem(p, lame)
    lin = pr.apply_cells(v)
    err = np.linalg.norm(pr.tangent_cells(np.zeros_like(u), v) - lin) / np.linalg.norm(lin)
    print(f"p={p} lame={E.LAME[lame]}: {err:.2e}")
    assert err <= 1e-13
    assert np.linalg.norm(pr.tangent_cells(u, v) - lin) > 0.05 * np.linalg.norm(lin)        # ... and at max |grad u| = 0.2 it is a different one


@pytest.mark.parametrize("p,lame", CASES)
def test_tangent_is_symmetric(p, lame):
    """<w, T v> = <v, T w> to rounding: both are sums of ~ 3 n_dofs products whose errors are a few 1e-16 of |w| |T v| each (bound: 1e-13 of that)"""
    pr, u, v, w = _problem(p, lame)
    Tv, Tw = pr.tangent_cells(u, v), pr.tangent_cells(u, w)
    a, b = float(np.sum(w * Tv)), float(np.sum(v * Tw))
    scale = np.linalg.norm(w) * np.linalg.norm(Tv)
    print(f"p={p} lame={E.LAME[lame]}: {a:.15e} {b:.15e}, difference / (|w| |T v|) {abs(a - b) / scale:.2e}")
    assert abs(a - b) <= 1e-13 * scale and abs(a) > 1e-3 * scale


@pytest.mark.parametrize("p,lame", CASES)
def test_a_rigid_rotation_carries_no_stress(p, lame):
    """u = (R - I) X, R the rotation by 0.7 rad about (1, 2, 3) / sqrt(14); X is in the FE space, so F = R at every point and P = 0"""
    pr, _, _, _ = _problem(p, lame)
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(0.7) * Kx + (1 - np.cos(0.7)) * Kx @ Kx
    u = (R - np.eye(3)) @ pr.mesh.coords.T
    volume = float(np.sum(O.jacobians(pr.mesh, pr.N, pr.D, pr.w)[1]))
    bound = 1e-12 * pr.mu * volume ** (2.0 / 3.0)
    r, lin = np.linalg.norm(pr.residual_cells(u)), np.linalg.norm(pr.apply_cells(u))
    print(f"p={p} lame={E.LAME[lame]}: |residual| {r:.2e} (bound {bound:.2e}), |linear operator u| {lin:.2e}, volume {volume:.6f}")
    assert abs(volume - 12.0) < 1e-3
    assert r <= bound
    assert lin >= 1e6 * bound


@pytest.mark.parametrize("p", [2, 3])
def test_homogeneous_stretch_gives_the_closed_form_energy_and_stress(p):
    """u = (diag(1.2, 0.9, 1.1) - I) X on the undeformed mesh, kappa = 1: energy = volume Phi(F) and <residual, A X> = volume P : A for a fixed A
    (A X is in the FE space with gradient A).  Quadrature of constants: exact to rounding (1e-12 relative)"""
    lam, mu = E.LAME[0]
    pr = H.Problem(p, CELLS, O.QUAD_GAUSS, deform_amp=0.0, kappa=O.kappa_none, lam=lam, mu=mu)
    F = np.diag([1.2, 0.9, 1.1])
    A = np.array([[0.3, -0.2, 0.1], [0.05, 0.4, -0.3], [0.2, 0.1, -0.25]])
    X = pr.mesh.coords.T
    u = (F - np.eye(3)) @ X
    volume = 12.0
    e, e_ref = pr.energy(u), volume * float(H.phi(F, lam, mu))
    w, w_ref = float(np.sum(pr.residual_cells(u) * (A @ X))), volume * float(np.sum(H.piola(F, lam, mu) * A))
    print(f"p={p}: energy {e:.15e} (closed form {e_ref:.15e}), <residual, A X> {w:.15e} (closed form {w_ref:.15e})")
    assert abs(e - e_ref) <= 1e-12 * abs(e_ref) and abs(w - w_ref) <= 1e-12 * abs(w_ref)
    # the state of that field: B = F^-T, ln J = ln det F at every point
    st = pr.state(u)
    assert np.abs(st[:9] - np.linalg.inv(F).T.reshape(9, 1, 1)).max() <= 1e-14 and np.abs(st[9] - np.log(np.linalg.det(F))).max() <= 1e-14


def test_device_layout_is_the_inverse_of_coef_off():
    pr, u, _, _ = _problem(2, 0)
    n, st = pr.mesh.n, pr.state(u)
    dev = pr.to_device_layout(st).reshape(10, pr.mesh.n_cells, n ** 3)
    for qi, ab in ((0, 0), (1, 4), (2, 8), (2, 3)):
        assert np.array_equal(dev[:, :, E.coef_off(n, qi, ab)], st[:, :, qi + n * ab])


# ---- what tests/test_gpu_hyperelasticity.py relies on
def _gpu_parity_cells(p):
    return (5, 4, 4) if p <= 2 else (11, 2, 1)


@pytest.mark.parametrize("quad", [O.QUAD_GAUSS, O.QUAD_GLL])
@pytest.mark.parametrize("p", range(1, 9))
def test_parity_references_under_input_noise(p, quad):
    """The GPU parity test holds the residual and the state to the LARGER of 1e-13 (the tangent's tolerance) and 10 x the reference's own change
    under a relative 1e-16 perturbation of u (hyperelasticity_ref.input_noise_drift), per case and quantity.  Printed here; measured: residual
    4e-16 .. 3e-15 and B 2e-16 .. 3e-15 (1e-13 governs at every degree), ln J 2e-15 .. 7e-15 at p <= 5 (1e-13 governs) and 1.1e-14 and more from
    p = 6 (10 x the drift governs: the gradient matrix of a high degree amplifies the perturbation of u).  The drift stays within a decade of the
    tangent tolerance everywhere, else the comparison would say nothing"""
    pr = H.Problem(p, _gpu_parity_cells(p), quad, deform_amp=AMP, kappa=O.kappa_step64)
    u = H.smooth_displacement(pr, 0.2)
    d_r, d_b, d_j = H.input_noise_drift(pr, u)
    s0 = pr.state(u)
    print(f"p={p} quad={quad}: residual {d_r:.2e}, state B {d_b:.2e}, ln J {d_j:.2e} -> tolerances {max(1e-13, 10 * d_r):.1e} {max(1e-13, 10 * d_b):.1e} "
          f"{max(1e-13, 10 * d_j):.1e}; max |grad u| {H.max_grad(pr, u):.3f}, min J {np.exp(s0[9].min()):.3f}")
    assert 10 * max(d_r, d_b, d_j) <= 1e-12
    assert np.isfinite(s0).all() and np.abs(u[:, pr.constrained]).max() > 0


@pytest.mark.parametrize("name", ["p2", "p4"])
def test_fixed_iteration_cg_references_are_stable_under_operator_noise(name):
    """tests/test_gpu_hyperelasticity.py compares fixed-iteration solves on the tangent to 1e-11 per block -- without a preconditioner, with the
    Chebyshev polynomial and with the V-cycle of the linear operator: the references stay two decades below that under 1e-16 relative noise in
    every operator application"""
    pr, u, b, its = H.cg_case(name)
    p, cells = pr.mesh.p, pr.mesh.cells
    assert 0.19 < H.max_grad(pr, u) < 0.21 and not u[:, pr.constrained].any()
    plain = E.noise_drift(lambda v: pr.tangent(u, v), b, its)
    V = M.VCycle(p, cells)
    Lc = M.Level(p, cells, 1.0, O.QUAD_GAUSS, AMP, O.kappa_step64, E.LAME[0][0], E.LAME[0][1], 4, 20.0, 8)
    noise = [None]

    def A(v):
        y = pr.tangent(u, v)
        return y if noise[0] is None else noise[0](y)
    drifts = {"identity": plain}
    for label, P, set_noise in (("chebyshev", Lc.vmult, lambda nz: setattr(Lc, "noise", nz)), ("v-cycle", V.vmult, V.set_noise)):
        def both(nz, set_noise=set_noise):
            noise[0] = nz
            set_noise(nz)
        drifts[label] = M.drift(lambda P=P: M.pcg(A, P, b, its)[0], both)
    print(f"{name}: noise drift after {its} iterations {drifts}")
    assert max(drifts.values()) < 1e-13, drifts


def test_the_newton_case_is_nonlinear_and_converges_in_full_steps():
    """the load is scaled so that the reference alone converges in <= 8 full steps (no backtrack), reaches max |grad u| >= 0.1 and differs from the
    one-step linear solution by >= 1 % in l2"""
    pr, f, u, info = H.newton_case()
    lin, _, _ = E.cg(pr.vmult, f, 2000, tol=1e-12 * np.linalg.norm(f))
    g, d = H.max_grad(pr, u), np.linalg.norm(u - lin) / np.linalg.norm(u)
    print(f"{info}; max |grad u| {g:.3f}; distance to the linear solution {d:.3%}")
    assert info["status"] == "ok" and info["newton_iterations"] <= 8 and info["backtracks"] == 0
    assert g >= 0.1 and d >= 0.01
    h = info["history"]
    assert len(h) == info["newton_iterations"] + 1 and h[-1] <= 1e-10 * h[0] and all(b < a for a, b in zip(h, h[1:]))
    # no accepted step is a near tie (the GPU run has to take the same decisions)
    assert all(b < 0.5 * a for a, b in zip(h, h[1:]))


def test_the_backtracking_case_backtracks():
    """20 x the load: every one of the three steps halves alpha at least once; the decisions are no near ties"""
    pr, f, u, info = H.newton_case(True)
    print(info)
    assert info["backtracks"] >= 1 and info["newton_iterations"] == H.BACKTRACK_PARAMS["max_newton"] and info["status"] == "no_convergence"
    h = info["history"]
    assert all(b < 0.99 * a for a, b in zip(h, h[1:]))
