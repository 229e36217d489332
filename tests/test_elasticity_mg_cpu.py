"""CPU checks of the elasticity preconditioners (bp5_elasticity_chebyshev_create, bp5_elasticity_mg_create, bp5_mg_transfer_*_components,
bp5_cg_solve_elasticity_preconditioned): the numpy composition the GPU tests compare against (tests/elasticity_mg_ref.py) is pinned OUTSIDE
itself -- the V-cycle is a symmetric positive operator, and CG with it, with Chebyshev(4) and with the block Jacobi diagonal needs the iteration
counts measured when the feature was proposed -- and every comparison tests/test_gpu_elasticity_mg.py makes is shown to be a stable one: the
drift under 1e-16 operator noise stays below 1e-13, and no Lanczos estimate whose step count is compared exactly stops near its threshold.
The library side that needs no device: symbols, prototypes, exports, the refusals that can be stated without a handle, the pinned Python
refusals."""
import ctypes as C

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import chebyshev_ref as CR
import elasticity_mg_ref as M
import elasticity_ref as E

pkg = bp5_pkg.load()
INVALID, UNSUPPORTED = 1, 5
SYMBOLS = ["bp5_elasticity_chebyshev_create", "bp5_elasticity_mg_create", "bp5_cg_solve_elasticity_preconditioned",
           "bp5_mg_transfer_prolongate_add_components", "bp5_mg_transfer_restrict_add_components"]
# (p, cells, Lame pair): CG iterations to 1e-8 ||b|| with the block Jacobi diagonal, Chebyshev(4) and the V-cycle (deformation 0.04, step-64 kappa,
# the right-hand side of elasticity_ref.cg_case, bp5_mg_params' defaults)
COUNTS = {(2, (4, 4, 4), 0): (49, 14, 6), (2, (4, 4, 4), 1): (81, 25, 9), (3, (3, 3, 2), 0): (55, 17, 7), (3, (3, 3, 2), 1): (90, 29, 15)}
_vc = {}


def _vcycle(p, cells, lame):
    if (p, cells, lame) not in _vc:
        _vc[p, cells, lame] = M.VCycle(p, cells, lam=E.LAME[lame][0], mu=E.LAME[lame][1])
    return _vc[p, cells, lame]


@pytest.mark.parametrize("p,cells,lame", [(2, (4, 4, 4), 1), (3, (3, 3, 2), 0)])
def test_v_cycle_is_symmetric_and_positive(p, cells, lame):
    V = _vcycle(p, cells, lame)
    pr = V.levels[0].pr
    u, w = pr.source(1), pr.source(2)
    Vu, Vw = V.vmult(u), V.vmult(w)
    a, b = np.sum(u * Vw), np.sum(w * Vu)
    print(f"p = {p} {cells}: u.Vw = {a:.16e}, w.Vu = {b:.16e}, relative difference {abs(a - b) / abs(a):.2e}")
    assert abs(a - b) <= 1e-13 * abs(a)
    assert np.sum(u * Vu) > 0 and np.sum(w * Vw) > 0


@pytest.mark.parametrize("p,cells,lame", sorted(COUNTS))
def test_iteration_counts_of_the_three_preconditioners(p, cells, lame):
    V = _vcycle(p, cells, lame)
    L0 = V.levels[0]
    b = M.rhs(L0.pr)
    tol = 1e-8 * np.linalg.norm(b)
    _, k_jacobi, _ = E.cg(L0.pr.vmult, b, 5000, tol=tol, inv_diag=L0.inv)
    Lc = M.Level(p, cells, 1.0, O.QUAD_GAUSS, M.AMP, O.kappa_step64, E.LAME[lame][0], E.LAME[lame][1], 4, 20.0, 10)
    _, k_cheb, _ = M.pcg(L0.pr.vmult, Lc.vmult, b, 5000, tol=tol)
    x, k_mg, res = M.pcg(L0.pr.vmult, V.vmult, b, 5000, tol=tol)
    print(f"p = {p} {cells} Lame {E.LAME[lame]}: Jacobi {k_jacobi}, Chebyshev(4) {k_cheb}, V-cycle {k_mg}")
    assert (k_jacobi, k_cheb, k_mg) == COUNTS[p, cells, lame]
    assert k_mg <= 15 and k_jacobi >= 5 * k_mg
    assert res <= tol and np.linalg.norm(b - L0.pr.vmult(x)) <= tol * (1 + 1e-6)


def _not_marginal(L, what):
    """the residual at the stopping step of the estimate and the one before it lie a factor >= 10 from the 1e-5 threshold"""
    last = L.residuals[-2:]
    print(f"{what}: degree {L.pr.mesh.p}, {L.cg_its} Lanczos steps, last relative residuals {last}")
    assert len(L.residuals) == L.cg_its
    for r in last:
        assert r >= 1e-4 or r <= 1e-6, (what, L.pr.mesh.p, L.residuals)


@pytest.mark.parametrize("name", sorted(M.VCYCLE_CASES))
def test_v_cycle_comparisons_of_the_gpu_tests_are_stable(name):
    """every level's cg_its is compared exactly and its bounds to 1e-10, the cycle's result to 1e-11"""
    V, s = M.vcycle_case(name)
    for lev, L in enumerate(V.levels):
        _not_marginal(L, f"{name} level {lev}")
    d = M.drift(lambda: V.vmult(s), V.set_noise)
    print(f"{name}: drift of the V-cycle under 1e-16 operator noise {d:.2e}")
    assert d < 1e-13


@pytest.mark.parametrize("p,degree,block_diagonal", M.CHEBYSHEV_CASES)
def test_chebyshev_comparisons_of_the_gpu_tests_are_stable(p, degree, block_diagonal):
    L, src, x0 = M.chebyshev_case(p, degree, block_diagonal)
    _not_marginal(L, f"Chebyshev p = {p}")

    def set_noise(noise):
        L.noise = noise
    dv = M.drift(lambda: L.vmult(src), set_noise)
    ds = M.drift(lambda: L.step(x0, src), set_noise)
    print(f"p = {p}, degree {degree}, block diagonal {block_diagonal}: drift vmult {dv:.2e}, step {ds:.2e}")
    assert dv < 1e-13 and ds < 1e-13


@pytest.mark.parametrize("name", sorted(M.SOLVE_CASES))
def test_five_iterations_of_v_cycle_pcg_are_stable(name):
    """the preconditioned solves of the GPU tests stop on a tolerance (count within one, solution to 1e-7); at a fixed count of five the
    solution moves by rounding only"""
    V, b = M.solve_case(name)
    A = V.levels[0].pr.vmult
    d = M.drift(lambda: M.pcg(V.levels[0].A, V.vmult, b, 5)[0], V.set_noise)
    print(f"{name}: drift of five V-cycle-PCG iterations {d:.2e}")
    assert d < 1e-13
    assert M.pcg(A, V.vmult, b, 5)[1] == 5


def test_start_vector_is_the_scalar_one_of_the_stacked_numbering():
    ids, con = np.arange(40), np.array([0, 7, 39])
    v = M.start_vector(ids, con)
    stacked = CR.start_vector((3 * ids[None, :] + np.arange(3)[:, None]).ravel(), []).reshape(3, -1)
    stacked[:, con] = 0.0
    assert np.array_equal(v, stacked) and v.min() == -5.0 and v.max() == 5.0


# ---- the library side that needs no device
def test_symbols_are_exported_and_listed():
    L = pkg.lib()
    for s in SYMBOLS:
        assert s in pkg.HEADER_SYMBOLS and hasattr(L, s) and s in L._protos, s
    assert len(L._protos["bp5_elasticity_chebyshev_create"][1]) == 8 and len(L._protos["bp5_elasticity_mg_create"][1]) == 9
    assert len(L._protos["bp5_cg_solve_elasticity_preconditioned"][1]) == 11
    assert len(L._protos["bp5_mg_transfer_prolongate_add_components"][1]) == len(L._protos["bp5_mg_transfer_restrict_add_components"][1]) == 6
    for name in ("ElasticityPreconditionChebyshev", "ElasticityPreconditionMG", "make_elasticity_mg_hierarchy"):
        assert hasattr(pkg, name), name
    for name in ("vmult", "step", "estimated_eigenvalues", "clear"):
        assert hasattr(pkg.ElasticityPreconditionChebyshev, name), name
    for name in ("vmult", "level_info", "clear"):
        assert hasattr(pkg.ElasticityPreconditionMG, name), name


def _buffers():
    """two 16-byte aligned host buffers: the refusals under test are decided before any pointer is dereferenced"""
    a = np.zeros(64 + 2)
    off = (-a.ctypes.data // 8) % 2
    return a.ctypes.data + 8 * off, a.ctypes.data + 8 * off + 8 * 32, a


def test_handle_free_refusals():
    from deal_and_ceed_on_gpu_amd import _lib
    L = pkg.lib()
    src, dst, keep = _buffers()
    null = C.c_void_p()
    vp = lambda p: C.c_void_p(p) if p else None
    prm, res = _lib.CGParams(_lib.CG_PLAIN, 10, 0.0, 0, 0), _lib.CGResult()
    cheb = _lib.ChebyshevParams(4, 20.0, 8, 0.0, 0.0, None)
    mgp = _lib.MGParams()
    L.bp5_mg_params_default(C.byref(mgp))
    out = C.c_void_p(0x77)
    never = _lib.VMULT_FN(lambda ctx, d, s: 1)
    pfn = C.cast(never, C.c_void_p)

    def chebyshev(lam=1.0, mu=1.0, ld=8, coef=src, inv=dst, p=cheb, o=out):
        st = L.bp5_elasticity_chebyshev_create(null, vp(coef), lam, mu, ld, vp(inv), C.byref(p) if p is not None else None, C.byref(o) if o is not None else None)
        return st, L.bp5_last_error().decode()

    def solve(lam=1.0, mu=1.0, ld=8, s=src, d=dst, p=prm, r=res, fn=pfn):
        st = L.bp5_cg_solve_elasticity_preconditioned(null, vp(src), lam, mu, ld, fn, None, vp(s), vp(d), C.byref(p) if p is not None else None,
                                                      C.byref(r) if r is not None else None)
        return st, L.bp5_last_error().decode()

    params = ((dict(ld=7), "even"), (dict(mu=0.0), "mu"), (dict(lam=-0.7, mu=1.0), "bulk"), (dict(lam=float("nan")), "finite"), (dict(), "null handle"))
    for kw, word in params + ((dict(inv=dst + 8), "aligned"), (dict(coef=None), "null"), (dict(p=None), "null"), (dict(o=None), "null")):
        st, msg = chebyshev(**kw)
        assert st == INVALID and word in msg and "elasticity" in msg, (kw, st, msg)
    assert not out.value or out.value == 0x77          # never a handle
    for kw, word in params + ((dict(d=dst + 8), "aligned"), (dict(s=None), "null"), (dict(d=src), "overlap"), (dict(fn=None), "null"), (dict(p=None), "null"),
                              (dict(r=None), "null"), (dict(p=_lib.CGParams(7, 10, 0.0, 0, 0)), "variant"), (dict(p=_lib.CGParams(_lib.CG_PLAIN, -1, 0.0, 0, 0)), "max_iter")):
        st, msg = solve(**kw)
        assert st == INVALID and word in msg and "elasticity" in msg, (kw, st, msg)

    # bp5_elasticity_mg_create: counts, null arrays, the layout and the parameters come before any level is looked at; then a null level
    one = (C.c_void_p * 1)(None)
    coefs = (C.c_void_p * 1)(src)

    def mg(n=1, mfs=one, cf=coefs, lam=1.0, mu=1.0, ld=8, p=mgp, o=out):
        st = L.bp5_elasticity_mg_create(n, mfs, cf, lam, mu, ld, None, C.byref(p) if p is not None else None, C.byref(o) if o is not None else None)
        return st, L.bp5_last_error().decode()
    bad = _lib.MGParams()
    L.bp5_mg_params_default(C.byref(bad))
    bad.smoother_degree = 0
    for kw, word in ((dict(n=0), "n_levels"), (dict(mfs=None), "null"), (dict(cf=None), "null"), (dict(p=None), "null"), (dict(o=None), "null"), (dict(n=2), "null"),
                     (dict(p=bad), "degrees"), (dict(ld=7), "even"), (dict(mu=-1.0), "mu"), (dict(lam=float("inf")), "finite"), (dict(), "null level")):
        st, msg = mg(**kw)
        assert st == INVALID and word in msg and "elasticity" in msg, (kw, st, msg)

    # the transfers on block vectors: a null transfer
    for fn in (L.bp5_mg_transfer_prolongate_add_components, L.bp5_mg_transfer_restrict_add_components):
        assert fn(null, 3, 8, vp(dst), 8, vp(src)) == INVALID and "null" in L.bp5_last_error().decode()
    del keep


def test_pinned_python_refusals_still_raise_unsupported():
    """PreconditionChebyshev, PreconditionMG, SolverCGFullMerge and SolverCG with any OTHER object refuse the elasticity operator as before
    (BP5Error 5, the same words), and SolverCGFullMerge refuses the new preconditioner classes too"""
    op = object.__new__(pkg.ElasticityOperator)
    op.mf_data = None
    with pytest.raises(pkg.BP5Error) as e:
        pkg.PreconditionChebyshev().initialize(op)
    assert e.value.status == UNSUPPORTED and "PreconditionChebyshev does not take the elasticity operator" in str(e.value)
    with pytest.raises(pkg.BP5Error) as e:
        pkg.PreconditionMG([op])
    assert e.value.status == UNSUPPORTED and "PreconditionMG does not take the elasticity operator" in str(e.value)

    class AnyPreconditioner:
        def vmult(self, dst, src):
            raise AssertionError("never applied")
    new_cheb = object.__new__(pkg.ElasticityPreconditionChebyshev)
    new_mg = object.__new__(pkg.ElasticityPreconditionMG)
    new_cheb._h = new_mg._h = None
    new_mg.transfers = []
    for solver, pre in ((pkg.SolverCG, AnyPreconditioner()), (pkg.SolverCG, object()), (pkg.SolverCG, pkg.PreconditionChebyshev()),
                        (pkg.SolverCGFullMerge, None), (pkg.SolverCGFullMerge, AnyPreconditioner()), (pkg.SolverCGFullMerge, new_cheb), (pkg.SolverCGFullMerge, new_mg)):
        with pytest.raises(pkg.BP5Error) as e:
            solver(pkg.IterationNumberControl(3, 0.0)).solve(op, None, None, pre)
        assert e.value.status == UNSUPPORTED and "elasticity: SolverCG with None / DiagonalMatrix only" in str(e.value), (solver.__name__, pre, str(e.value))
    # the new classes take nothing but the elasticity operator
    for fn in (lambda: pkg.ElasticityPreconditionChebyshev().initialize(object()), lambda: pkg.ElasticityPreconditionMG([object()]),
               lambda: pkg.ElasticityPreconditionMG([]), lambda: pkg.make_elasticity_mg_hierarchy(object())):
        with pytest.raises(pkg.BP5Error) as e:
            fn()
        assert e.value.status == INVALID
