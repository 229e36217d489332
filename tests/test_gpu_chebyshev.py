"""PreconditionChebyshev and CG with a general preconditioner on the MI355X against the numpy reference (tests/chebyshev_ref.py on the
oracle's operator): vmult / step parity, the CG-Lanczos estimate, Chebyshev-PCG solutions native and through callbacks."""
import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import chebyshev_ref as R

pkg = bp5_pkg.load()
pytestmark = pytest.mark.gpu
Cheb = pkg.PreconditionChebyshev


def _t():
    import torch
    return torch


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _local_operator(A_global, perm):
    """the oracle operator in the GPU mesh's local numbering (local i == lexicographic perm[i])"""
    def A(v):
        full = np.zeros(v.size)
        full[perm] = v
        return A_global(full)[perm]
    return A


def _helmholtz(pr):
    c = pr.mesh.constrained.astype(np.int64)

    def A(s):
        d = O.apply_helmholtz_cells(pr.mesh, pr.N, pr.D, pr.w, s)
        d[c] = s[c]
        return d
    return A


class _PyOperator:
    """any operator with mf_data + vmult: reaches the library through the callback paths"""

    def __init__(self, op):
        self.op, self.mf_data = op, op.mf_data

    def vmult(self, dst, src):
        self.op.vmult(dst, src)


def _vmult_and_step_parity(op, A, n, seed, diagonal=True, bounds=(0.15, 2.1)):
    """diagonal False: no preconditioner (AdditionalData.preconditioner None = identity; the step kernel's builds without a diagonal)"""
    torch = _t()
    dev = "cuda:0"
    inv = op.compute_diagonal(invert=True)
    inv_np = inv.cpu().numpy()[:n] if diagonal else np.ones(n)
    src = O.deterministic_src(n, seed=seed)
    x0 = O.deterministic_src(n, seed=seed + 100)
    lo, hi = bounds
    for degree in (1, 2, 4, 6):
        ch = Cheb().initialize(op, Cheb.AdditionalData(degree=degree, max_eigenvalue=hi, min_eigenvalue=lo,
                                                       preconditioner=pkg.DiagonalMatrix(inv) if diagonal else None))
        assert ch.estimated_eigenvalues()["max_used"] == hi and ch.estimated_eigenvalues()["min_used"] == lo
        dst = torch.full((op.mf_data.n_local,), 7.0, dtype=torch.float64, device=dev)       # prior content is ignored
        s = op.initialize_dof_vector()
        s[:n] = torch.from_numpy(src)
        ch.vmult(dst, s)
        ref = R.vmult(A, inv_np, src, lo, hi, degree)
        err = _rel(dst.cpu().numpy()[:n], ref)
        assert err < 1e-12, (degree, err)
        x = op.initialize_dof_vector()
        x[:n] = torch.from_numpy(x0)
        ch.step(x, s)
        ref = R.step(A, inv_np, x0, src, lo, hi, degree)
        err = _rel(x.cpu().numpy()[:n], ref)
        assert err < 1e-12, ("step", degree, err)
        assert torch.equal(s[:n].cpu(), torch.from_numpy(src))                              # src untouched


@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("p,cells", [(1, (5, 4, 3)), (2, (4, 3, 3)), (4, (3, 2, 2)), (5, (2, 2, 2)), (8, (2, 1, 2))])
def test_vmult_and_step_match_numpy_pencil_kernel(p, cells, quad):
    """vmult and step at degree 1, 2, 4, 6 with fixed bounds, step-64 kappa, deformed mesh, Jacobi diagonal: 1e-12 relative."""
    pr = O.Problem(p, cells, quad, deform_amp=0.04, kappa=O.kappa_step64)
    mesh = pkg.BrickMesh(p, cells, deform_amp=0.04)
    op = pkg.PoissonOperator(mesh, quad, pkg.COEF_STEP64)
    _vmult_and_step_parity(op, pr.vmult, mesh.n_owned, seed=p)


def test_vmult_and_step_without_a_diagonal_on_an_odd_length():
    """The step kernel's four forms (vmult: 0, 2, 1; step: 3, 1) in the builds without a diagonal, on a vector of odd length (n_owned = 9 * 7 * 7:
    the kernel's scalar tail entry); with a diagonal the even-degree meshes above are odd lengths already.  The bounds are those of the UNSCALED
    operator (20 numpy power iterations), in the ratio of the other tests, so that the polynomial is as well conditioned as theirs: 1e-12."""
    p, cells = 2, (4, 3, 3)
    pr = O.Problem(p, cells, 0, deform_amp=0.04, kappa=O.kappa_step64)
    mesh = pkg.BrickMesh(p, cells, deform_amp=0.04)
    assert mesh.n_owned % 2 == 1
    v = O.deterministic_src(mesh.n_owned, seed=3)
    for _ in range(20):
        v = pr.vmult(v / np.linalg.norm(v))
    hi = 1.2 * np.linalg.norm(v)
    _vmult_and_step_parity(pkg.PoissonOperator(mesh, 0, pkg.COEF_STEP64), pr.vmult, mesh.n_owned, seed=11, diagonal=False, bounds=(hi / 14.0, hi))


@pytest.mark.parametrize("quad", [0, 1])
def test_vmult_and_step_match_numpy_block_kernel(quad):
    """The bench's kernel: brick-ordered mesh (partial bricks), block-assembled operator, a few bricks per workgroup."""
    cells = (6, 5, 9)
    pr = O.Problem(4, cells, quad, deform_amp=0.04, kappa=O.kappa_step64)
    mesh = pkg.BrickMesh(4, cells, deform_amp=0.04, cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1)
    op = pkg.PoissonOperator(mesh, quad, pkg.COEF_STEP64)
    op.mf_data.set_apply_variant(56)
    op.mf_data.set_block_workgroups(8)
    assert op.mf_data.get_apply_variant() == 56
    _vmult_and_step_parity(op, _local_operator(pr.vmult, mesh.global_ids.astype(np.int64)), mesh.n_owned, seed=40)


def test_vmult_and_step_match_numpy_helmholtz():
    """BP5_OP_HELMHOLTZ (step-64's operator, native fused kernel)."""
    p, cells = 3, (3, 3, 2)
    pr = O.Problem(p, cells, 0, h=0.25, deform_amp=0.04)
    mesh = pkg.BrickMesh(p, cells, h=0.25, deform_amp=0.04)
    op = pkg.HelmholtzOperator(mesh, 0, pkg.COEF_STEP64)
    _vmult_and_step_parity(op, _helmholtz(pr), mesh.n_owned, seed=33)


def test_estimate_matches_numpy_lanczos_and_bounds_the_spectrum():
    """The CG-Lanczos estimate equals numpy's on the same start vector and iteration count (1e-10); on a small mesh (729 DoFs, dense
    D^-1 A from columns of the oracle's vmult) max_est <= lambda_max (1 + 1e-12) and max_used >= lambda_max at 20 iterations."""
    torch = _t()
    p, cells = 2, (4, 4, 4)
    pr = O.Problem(p, cells, 0, deform_amp=0.05, kappa=O.kappa_step64)
    mesh = pkg.BrickMesh(p, cells, deform_amp=0.05)
    op = pkg.PoissonOperator(mesh, 0, pkg.COEF_STEP64)
    inv = op.compute_diagonal(invert=True)
    inv_ref = 1.0 / O.operator_diagonal(pr.mesh, pr.coef, pr.N, pr.D)
    assert _rel(inv.cpu().numpy(), inv_ref) < 1e-13
    v = R.start_vector(mesh.global_ids, mesh.constrained)
    for its, srange in ((8, 20.0), (20, 0.0), (5, 0.0)):
        ch = Cheb().initialize(op, Cheb.AdditionalData(degree=3, smoothing_range=srange, eig_cg_n_iterations=its, preconditioner=pkg.DiagonalMatrix(inv)))
        e = ch.estimated_eigenvalues()
        lo, hi, k = R.lanczos_estimate(pr.vmult, inv_ref, v, its)
        assert e["cg_its"] == k
        assert abs(e["min_est"] - lo) <= 1e-10 * lo and abs(e["max_est"] - hi) <= 1e-10 * hi, (e, lo, hi)
        mu, Mu = R.bounds(lo, hi, srange)
        assert abs(e["min_used"] - mu) <= 1e-10 * mu and abs(e["max_used"] - Mu) <= 1e-10 * Mu
    # dense D^-1 A on the free DoFs
    free = np.setdiff1d(np.arange(pr.mesh.n_dofs), pr.mesh.constrained.astype(np.int64))
    cols = np.zeros((pr.mesh.n_dofs, free.size))
    for j, f in enumerate(free):
        u = np.zeros(pr.mesh.n_dofs)
        u[f] = 1.0
        cols[:, j] = pr.vmult(u)
    Af = cols[free]
    s = np.sqrt(inv_ref[free])
    lam = np.linalg.eigvalsh(s[:, None] * Af * s[None, :])
    e = Cheb().initialize(op, Cheb.AdditionalData(degree=3, eig_cg_n_iterations=20, preconditioner=pkg.DiagonalMatrix(inv))).estimated_eigenvalues()
    assert e["max_est"] <= lam[-1] * (1 + 1e-12) and e["max_used"] >= lam[-1] and e["min_est"] >= lam[0] * (1 - 1e-12), (e, lam[0], lam[-1])
    print(f"lambda(D^-1 A) in [{lam[0]:.4f}, {lam[-1]:.4f}]; 20-step estimate [{e['min_est']:.4f}, {e['max_est']:.4f}]")


def test_estimate_is_the_same_for_every_numbering():
    """The start vector follows the global DoF id: a brick-major numbered mesh gives the lexicographic mesh's estimate."""
    cells = (6, 5, 9)
    ests = []
    for kw in (dict(), dict(cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1)):
        mesh = pkg.BrickMesh(4, cells, deform_amp=0.04, **kw)
        op = pkg.PoissonOperator(mesh, 0, pkg.COEF_STEP64)
        inv = op.compute_diagonal(invert=True)
        ests.append(Cheb().initialize(op, Cheb.AdditionalData(degree=2, preconditioner=pkg.DiagonalMatrix(inv))).estimated_eigenvalues())
    for key in ("min_est", "max_est"):
        assert abs(ests[0][key] - ests[1][key]) <= 1e-10 * ests[0][key], ests


def _pcg_case(p, cells, amp=0.05):
    pr = O.Problem(p, cells, 0, deform_amp=amp, kappa=O.kappa_step64)
    mesh = pkg.BrickMesh(p, cells, deform_amp=amp)
    op = pkg.PoissonOperator(mesh, 0, pkg.COEF_STEP64)
    inv = op.compute_diagonal(invert=True)
    return pr, mesh, op, inv


@pytest.mark.parametrize("path", ["native", "callback"])
def test_chebyshev_pcg_matches_numpy_at_a_fixed_iteration_count(path):
    """SolverCG + PreconditionChebyshev(degree 4, smoothing range 20, 8-step estimate), 12 iterations: the numpy PCG's iterate to 1e-11.
    callback: operator and preconditioner's operator are a Python object with vmult (bp5_vmult_fn callbacks throughout)."""
    torch = _t()
    pr, mesh, op, inv = _pcg_case(3, (4, 3, 3))
    A = op if path == "native" else _PyOperator(op)
    ch = Cheb().initialize(A, Cheb.AdditionalData(degree=4, smoothing_range=20.0, preconditioner=pkg.DiagonalMatrix(inv)))
    b = op.assemble_rhs()
    x = op.initialize_dof_vector()
    ctl = pkg.IterationNumberControl(12, 0.0)
    pkg.SolverCG(ctl).solve(A, x, b, ch)
    inv_ref = 1.0 / O.operator_diagonal(pr.mesh, pr.coef, pr.N, pr.D)
    lo, hi, _ = R.lanczos_estimate(pr.vmult, inv_ref, R.start_vector(mesh.global_ids, mesh.constrained), 8)
    mu, Mu = R.bounds(lo, hi, 20.0)
    xr, k, res = R.pcg(pr.vmult, lambda g: R.vmult(pr.vmult, inv_ref, g, mu, Mu, 4), pr.rhs(), 12)
    assert ctl.last_step() == k == 12
    err = _rel(x.cpu().numpy(), xr)
    assert err < 1e-11, err
    assert abs(ctl.last_value() - res) <= 1e-9 * res


def test_general_preconditioner_object_through_the_callback_is_bitwise_the_native_path():
    """Any object with vmult (no get_vector) is a preconditioner: a Python wrapper around the Chebyshev handle gives the native bits."""
    torch = _t()
    pr, mesh, op, inv = _pcg_case(3, (4, 3, 3))
    ch = Cheb().initialize(op, Cheb.AdditionalData(degree=3, smoothing_range=15.0, preconditioner=pkg.DiagonalMatrix(inv)))

    class Wrapped:
        def vmult(self, dst, src):
            ch.vmult(dst, src)

    b = op.assemble_rhs()
    xs = []
    for P in (ch, Wrapped()):
        x = op.initialize_dof_vector()
        pkg.SolverCG(pkg.IterationNumberControl(10, 0.0)).solve(op, x, b, P)
        xs.append(x.clone())
    assert torch.equal(xs[0], xs[1])


def test_chebyshev_pcg_cuts_iterations_and_is_independent_of_check_every():
    """p = 4, 6^3 cells, deform 0.05, step-64 kappa, tolerance 1e-10 ||b||: Chebyshev(4)-PCG takes <= 0.6x the iterations of
    Jacobi-PCG (the oracle: 147 against 43).  On the block kernel (owner stores, no atomics: bitwise reproducible) the result is bitwise
    the same for check_every 0, 1 and 3.  SolverCGFullMerge refuses a Chebyshev preconditioner."""
    torch = _t()
    pr, mesh, op, inv = _pcg_case(4, (6, 6, 6))
    b = op.assemble_rhs()
    tol = 1e-10 * float(torch.linalg.norm(b))
    cj = pkg.IterationNumberControl(1000, tol)
    xj = op.initialize_dof_vector()
    pkg.SolverCG(cj).solve(op, xj, b, pkg.DiagonalMatrix(inv))
    ch = Cheb().initialize(op, Cheb.AdditionalData(degree=4, smoothing_range=20.0, preconditioner=pkg.DiagonalMatrix(inv)))
    c = pkg.IterationNumberControl(1000, tol)
    x = op.initialize_dof_vector()
    pkg.SolverCG(c).solve(op, x, b, ch)
    assert c.last_value() <= tol
    print(f"Jacobi-PCG {cj.last_step()} iterations, Chebyshev(4)-PCG {c.last_step()} ({c.last_step() / cj.last_step():.2f}x); estimate {ch.estimated_eigenvalues()}")
    assert c.last_step() <= 0.6 * cj.last_step()
    assert _rel(x.cpu().numpy(), xj.cpu().numpy()) < 1e-8
    with pytest.raises(pkg.BP5Error):
        pkg.SolverCGFullMerge(pkg.IterationNumberControl(10, 0.0)).solve(op, op.initialize_dof_vector(), b, ch)
    # the same problem on the block kernel
    meshb = pkg.BrickMesh(4, (6, 6, 6), deform_amp=0.05, cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1)
    opb = pkg.PoissonOperator(meshb, 0, pkg.COEF_STEP64)
    opb.mf_data.set_apply_variant(56)
    invb = opb.compute_diagonal(invert=True)
    bb = opb.assemble_rhs()
    chb = Cheb().initialize(opb, Cheb.AdditionalData(degree=4, smoothing_range=20.0, preconditioner=pkg.DiagonalMatrix(invb)))
    xs, its = [], []
    for check in (0, 1, 3):
        cb = pkg.IterationNumberControl(1000, tol)
        xb = opb.initialize_dof_vector()
        pkg.SolverCG(cb, check_every=check).solve(opb, xb, bb, chb)
        xs.append(xb.clone())
        its.append(cb.last_step())
    assert its[0] == its[1] == its[2] and abs(its[0] - c.last_step()) <= 1
    assert all(torch.equal(xs[0], y) for y in xs[1:])
    perm = meshb.global_ids.astype(np.int64)
    assert _rel(xs[0].cpu().numpy(), x.cpu().numpy()[perm]) < 1e-9


def test_facade_example_matches_the_python_solve():
    """examples/bp5_chebyshev (step-37's solve on the C++ facade: operator, compute_diagonal(invert), PreconditionChebyshev, SolverCG)
    reports the iteration count, the bounds and the solution norm of the Python solve of the same problem."""
    import subprocess
    import os
    torch = _t()
    exe = os.path.join(bp5_pkg.ROOT, "examples", "bp5_chebyshev")
    txt = subprocess.run([exe, "3", "5", "4", "4", "0.05", "4", "20", "1e-9"], capture_output=True, text=True, timeout=300, check=True).stdout
    got = {l.split()[0]: l.split()[1:] for l in txt.splitlines() if l.strip()}
    pr, mesh, op, inv = _pcg_case(3, (5, 4, 4))
    ch = Cheb().initialize(op, Cheb.AdditionalData(degree=4, smoothing_range=20.0, preconditioner=pkg.DiagonalMatrix(inv)))
    b = op.assemble_rhs()
    x = op.initialize_dof_vector()
    x_norm_tol = 1e-9 * float(torch.linalg.norm(b[:mesh.n_owned]))
    ctl = pkg.SolverControl(10000, x_norm_tol)
    pkg.SolverCG(ctl).solve(op, x, b, ch)
    e = ch.estimated_eigenvalues()
    assert int(got["iterations"][0]) == ctl.last_step()
    assert abs(float(got["eigenvalue_bounds"][1]) - e["max_used"]) <= 1e-12 * e["max_used"]
    xn = float(torch.linalg.norm(x[:mesh.n_owned]))
    assert abs(float(got["solution_norm"][0]) - xn) <= 1e-10 * xn, (got, xn)


@pytest.mark.parametrize("check_every", [0, 7])
def test_preconditioned_solve_stops_working_once_converged(check_every):
    """With a tolerance far below max_iter the solve applies the operator and the preconditioner only for the iterations it needs (plus the
    host's lag in looking at the device's stop flag: two iterations with check_every = 0, up to check_every - 1 otherwise), not max_iter times."""
    pr, mesh, op, inv = _pcg_case(3, (4, 3, 3))
    calls = {"A": 0, "P": 0}
    ch = Cheb().initialize(op, Cheb.AdditionalData(degree=3, smoothing_range=20.0, preconditioner=pkg.DiagonalMatrix(inv)))

    class CountA(_PyOperator):
        def vmult(self, dst, src):
            calls["A"] += 1
            self.op.vmult(dst, src)

    class CountP:
        def vmult(self, dst, src):
            calls["P"] += 1
            ch.vmult(dst, src)

    b = op.assemble_rhs()
    x = op.initialize_dof_vector()
    ctl = pkg.IterationNumberControl(1000, 1e-9 * float(_t().linalg.norm(b)))
    pkg.SolverCG(ctl, check_every=check_every).solve(CountA(op), x, b, CountP())
    k = ctl.last_step()
    lag = 2 if check_every == 0 else check_every - 1
    assert 5 < k < 200 and ctl.last_value() <= ctl.tolerance
    assert k <= calls["A"] <= k + lag and k + 1 <= calls["P"] <= k + 1 + lag, (k, calls)
