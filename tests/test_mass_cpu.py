"""The mass operator without a GPU: the numpy reference of tests/mass_ref.py pinned against quantities that do not come from it, the noise drift
of every fixed-iteration CG reference tests/test_gpu_mass.py compares against, and the public names of the feature."""
import os
import re

import numpy as np
import pytest

import bp5_oracle as O
import mass_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (p, cells, deformation, rho): the meshes the issue checked by hand
PINNED = [(2, (8, 8, 8), 0.0, O.kappa_none), (3, (3, 4, 5), 0.05, O.kappa_none), (4, (4, 4, 4), 0.05, O.kappa_step64)]
_cache = {}


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def problem(p, cells, amp, rho, quad=O.QUAD_GAUSS, dirichlet=True):
    key = (p, cells, amp, rho, quad, dirichlet)
    if key not in _cache:
        _cache[key] = M.Problem(p, cells, quad, deform_amp=amp, rho=rho, dirichlet=dirichlet)
    return _cache[key]


# ------------------------------------------------------------------ the CG references of the GPU tests (computed once, shared, never changed)
CG_ITERATIONS = 10


def config1_case():
    """BASELINE config 1 (p = 2, 8^3 unit cells) with rho = 1, b_i = int phi_i, no preconditioner: (problem, b, inverse diagonal or None)"""
    pr = problem(2, (8, 8, 8), 0.0, O.kappa_none)
    return pr, pr.rhs(), None


def step64_case():
    """p = 4, 4^3 deformed cells, rho = step-64's coefficient, Jacobi: the Dirichlet identity rows sit far from the mass spectrum, so the
    unpreconditioned iteration crawls and the inverse diagonal is part of the case"""
    pr = problem(4, (4, 4, 4), 0.05, O.kappa_step64)
    return pr, pr.rhs(), 1.0 / pr.diagonal()


BRICK_FREE = (2, (9, 8, 5), 0.2, 0.03)     # p, cells, h, deformation: the p = 2 brick mesh of the kernel-selection tests, no Dirichlet DoFs


def brick_free_case():
    """BP1 proper: no boundary condition, rho = 1, b = M u with a deterministic u, no preconditioner (the GPU test runs it on the block kernel
    with the dot products fused): (problem, b, None)"""
    key = ("brick_free",)
    if key not in _cache:
        p, cells, h, amp = BRICK_FREE
        pr = M.Problem(p, cells, h=h, deform_amp=amp, dirichlet=False)
        b = pr.vmult(O.deterministic_src(pr.mesh.n_dofs, seed=81))
        b.setflags(write=False)
        _cache[key] = (pr, b)
    return _cache[key] + (None,)


CG_CASES = {"config1": config1_case, "step64": step64_case}
SOLVERS = {"plain": O.cg_plain, "merged": O.cg_merged}


def cg_reference(case, solver):
    key = ("cg", case, solver)
    if key not in _cache:
        pr, b, inv = CG_CASES[case]()
        x, k, res = SOLVERS[solver](pr.vmult, b, CG_ITERATIONS, diag=inv)
        x.setflags(write=False)
        _cache[key] = (x, k, res)
    return _cache[key]


# ------------------------------------------------------------------ 1. the reference, pinned outside itself
@pytest.mark.parametrize("p,cells,amp,rho", PINNED)
def test_row_sums_are_the_right_hand_side(p, cells, amp, rho):
    """M 1 = (int phi_i): with rho = 1 the row sums of the mass matrix are O.assemble_rhs on the unconstrained rows"""
    pr = problem(p, cells, amp, O.kappa_none)
    got = pr.apply_cells(np.ones(pr.mesh.n_dofs))
    want = pr.rhs()
    free = np.ones(pr.mesh.n_dofs, bool)
    free[pr.mesh.constrained.astype(np.int64)] = False
    e = rel(got[free], want[free])
    print(f"p={p} {cells}: |M 1 - rhs| / |rhs| = {e:.2e}")
    assert e <= 1e-14


@pytest.mark.parametrize("p,cells,amp,rho", PINNED)
def test_energy_is_the_l2_norm(p, cells, amp, rho):
    pr = problem(p, cells, amp, O.kappa_none)
    u = O.deterministic_src(pr.mesh.n_dofs, seed=5)
    energy, l2 = u @ pr.apply_cells(u), O.l2_norm_solution(pr.mesh, u) ** 2
    print(f"p={p} {cells}: u M u = {energy:.15e}, |u|_L2^2 = {l2:.15e}")
    assert abs(energy - l2) <= 1e-13 * l2


@pytest.mark.parametrize("p,cells,amp,rho", PINNED)
def test_helmholtz_minus_laplace_is_the_mass_operator(p, cells, amp, rho):
    pr = problem(p, cells, amp, rho)
    lap = O.Problem(p, cells, O.QUAD_GAUSS, deform_amp=amp)               # (grad v, grad u), coefficient 1: the Laplace part of step-64's operator
    u = O.deterministic_src(pr.mesh.n_dofs, seed=6)
    want = O.apply_helmholtz_cells(pr.mesh, pr.N, pr.D, pr.w, u, coefficient=rho) - O.apply_cells(lap.mesh, lap.coef, lap.N, lap.D, u)
    e = rel(pr.apply_cells(u), want)
    print(f"p={p} {cells}: {e:.2e}")
    assert e <= 1e-12


TEXTBOOK_1D = {1: np.array([[2.0, 1.0], [1.0, 2.0]]) / 6.0,                                   # linear elements on [0, 1]
               2: np.array([[4.0, 2.0, -1.0], [2.0, 16.0, 2.0], [-1.0, 2.0, 4.0]]) / 30.0}     # quadratic, nodes 0, 1/2, 1


@pytest.mark.parametrize("p,h", [(1, 1.0), (1, 0.5), (2, 2.0), (2, 0.25)])
def test_cell_matrix_is_the_tensor_product_of_textbook_mass_matrices(p, h):
    """affine cube of edge h, rho = 1, Gauss(p+1) (exact there): the dense cell matrix is h^3 M1 x M1 x M1, local index i + n (j + n k)"""
    pr = problem(p, (1, 1, 1), 0.0, O.kappa_none, dirichlet=False) if h == 1.0 else M.Problem(p, (1, 1, 1), h=h, dirichlet=False)
    n3 = (p + 1) ** 3
    idx = pr.mesh.l2g[0].astype(np.int64)
    got = np.zeros((n3, n3))
    for s in range(n3):
        e = np.zeros(pr.mesh.n_dofs)
        e[idx[s]] = 1.0
        got[:, s] = pr.apply_cells(e)[idx]
    M1 = TEXTBOOK_1D[p]
    want = h ** 3 * np.kron(M1, np.kron(M1, M1))
    assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)


@pytest.mark.parametrize("p,cells,amp,rho", PINNED)
def test_collocated_operator_is_its_diagonal(p, cells, amp, rho):
    pr = problem(p, cells, amp, rho, quad=O.QUAD_GLL)
    u = O.deterministic_src(pr.mesh.n_dofs, seed=7)
    d = pr.diagonal()
    free = np.ones(pr.mesh.n_dofs, bool)
    free[pr.mesh.constrained.astype(np.int64)] = False
    assert rel(pr.apply_cells(u)[free], (d * u)[free]) <= 1e-14
    assert np.array_equal(pr.vmult(u)[~free], u[~free])


@pytest.mark.parametrize("p,cells,amp,rho", PINNED)
def test_diagonal_is_the_diagonal(p, cells, amp, rho):
    """a few entries of diag(M) through unit vectors"""
    pr = problem(p, cells, amp, rho)
    d = pr.diagonal()
    assert np.all(d[pr.mesh.constrained.astype(np.int64)] == 1.0)
    for i in np.random.default_rng(3).choice(pr.mesh.n_dofs, 12, replace=False):
        e = np.zeros(pr.mesh.n_dofs)
        e[i] = 1.0
        assert abs(pr.vmult(e)[i] - d[i]) <= 1e-13 * abs(d[i])


# ------------------------------------------------------------------ 2. noise drift of the fixed-iteration CG references
@pytest.mark.parametrize("solver", sorted(SOLVERS))
@pytest.mark.parametrize("case", sorted(CG_CASES))
def test_cg_references_do_not_amplify_rounding(case, solver):
    """a relative perturbation of 1e-16 per operator application moves the 10-iteration solution by less than 1e-13: the 1e-11 bound of the GPU
    comparison is two orders above what rounding can do to these references"""
    pr, b, inv = CG_CASES[case]()
    drift = M.noise_drift(pr.vmult, b, CG_ITERATIONS, inv_diag=inv, solver=SOLVERS[solver])
    x, k, res = cg_reference(case, solver)
    print(f"{case} / {solver}: drift {drift:.2e}, residual after {k} iterations {res:.3e} (|b| = {np.linalg.norm(b):.3e})")
    assert k == CG_ITERATIONS and drift < 1e-13


@pytest.mark.parametrize("solver", sorted(SOLVERS))
def test_cg_reference_without_dirichlet_dofs_does_not_amplify_rounding(solver):
    pr, b, inv = brick_free_case()
    drift = M.noise_drift(pr.vmult, b, CG_ITERATIONS, inv_diag=inv, solver=SOLVERS[solver])
    _, k, res = SOLVERS[solver](pr.vmult, b, CG_ITERATIONS)
    print(f"brick_free / {solver}: drift {drift:.2e}, residual after {k} iterations {res:.3e} (|b| = {np.linalg.norm(b):.3e})")
    assert k == CG_ITERATIONS and drift < 1e-13 and res > 1e-8 * np.linalg.norm(b)


def test_config1_is_far_from_converged_after_ten_iterations():
    """... so the fixed-count comparison compares iterates, not a converged solution"""
    pr, b, _ = config1_case()
    _, _, res = cg_reference("config1", "plain")
    assert 1e-3 < res / np.linalg.norm(b) < 1e-1


# ------------------------------------------------------------------ 3. - 5. the feature's public names
def test_python_mirror_names_the_operator():
    import bp5_pkg
    pkg = bp5_pkg.load()
    from deal_and_ceed_on_gpu_amd import _lib
    assert _lib.OP_MASS == 2 and pkg.OP_MASS == 2 and issubclass(pkg.MassOperator, pkg.PoissonOperator)


def test_header_names_the_operator():
    text = open(os.path.join(ROOT, "include", "bp5.h")).read()
    assert re.search(r"BP5_OP_MASS\s*=\s*2\b", text)


def test_examples_makefile_builds_the_bp1_example():
    text = open(os.path.join(ROOT, "examples", "Makefile")).read()
    assert re.search(r"^all:.*\bbp5_bp1\b", text, re.M) and re.search(r"^bp5_bp1:", text, re.M) and re.search(r"rm -f.*\bbp5_bp1\b", text)
