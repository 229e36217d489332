"""The multigrid transfers and PreconditionMG at full size (1.4e8 fine DoFs, coarse levels above the 65 536 x 256 = 16 777 216 DoFs that
mg_combine covers in one grid-stride trip), on brick-ordered meshes as the benchmark uses them: the transfers against the numpy reference
(tests/multigrid_ref.py, tests/hmg_ref.py) through global_ids, the V-cycle's symmetry, bitwise reproducibility and MG-PCG's residual.
Each test prints its time and the process's peak host memory (run pytest with -s to see them)."""
import resource
import time

import numpy as np
import pytest

import bp5_pkg
import hmg_ref as H
import multigrid_ref as G

pkg = bp5_pkg.load()
pytestmark = pytest.mark.gpu
BRICKS = dict(cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1)
COMBINE_CAP = 65536 * 256      # coarse local DoFs mg_combine covers in its first grid-stride trip (bp5_device.hip: mg_combine)
BENCH_MG_ITERATIONS = 7        # MG-PCG on the p = 4 bench mesh (116 x 116 x 120 cells, tolerance 1e-8 ||b||), p-only and hybrid


def _t():
    import torch
    return torch


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _perm(op):
    m = op.mf_data.mesh
    return m.global_ids[:m.n_owned].astype(np.int64)


def _dev(v_lex, op):
    torch = _t()
    x = op.initialize_dof_vector()
    x[:op.mf_data.n_owned] = torch.from_numpy(np.ascontiguousarray(v_lex[_perm(op)])).to(x.device)
    return x


def _lex(x, op, n):
    out = np.zeros(n)
    out[_perm(op)] = x[:op.mf_data.n_owned].cpu().numpy()
    return out


def _report(name, t0):
    peak_gib = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20
    print(f"{name}: {time.time() - t0:.1f} s, peak host memory {peak_gib:.1f} GiB")


def _transfer_op(mesh):
    """the transfers read no metric: the affine geometry mode keeps the six planes (up to 22 GB here) out of device memory"""
    return pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_ONE, geometry=pkg.GEOM_AFFINE)


# the two 1.35e8-DoF meshes, generated once (about 20 s each on the host)
@pytest.fixture(scope="module")
def mesh_p4():
    return pkg.BrickMesh(4, (128, 128, 128), h=1.0 / 128, **BRICKS)


@pytest.fixture(scope="module")
def mesh_p2():
    return pkg.BrickMesh(2, (256, 256, 256), **BRICKS)


@pytest.mark.parametrize("pair", ["p4to2", "p2to1", "h2"])
def test_full_size_transfer_matches_numpy(pair, request):
    """p 4 -> 2 on 128^3 cells, p 2 -> 1 on 256^3 cells, geometric p = 2 from 256^3 to 128^3 cells: 1.35e8 fine DoFs, 257^3 = 1.70e7
    coarse DoFs, so the combine pass of the restriction takes a second trip over the coarse DoFs past COMBINE_CAP.  Those include free
    (non-Dirichlet) DoFs, checked here, so a skipped trip shows.  The small tests' assertions: 1e-13 relative, Dirichlet rows unchanged,
    <R r, e> = <r, P e>.  (Geometric p = 1 at this size would need 512^3 cells; its kernels get the partial-workgroup tests of
    test_gpu_preconditioner_setups.py, the combine pass is the same for every pair.)"""
    t0 = time.time()
    if pair == "p4to2":
        cells = (128, 128, 128)
        fine = _transfer_op(request.getfixturevalue("mesh_p4"))
        coarse = _transfer_op(pkg.BrickMesh(2, cells, h=1.0 / 128, **BRICKS))
        T = G.Transfer(cells, 4, 2)
    elif pair == "p2to1":
        cells = (256, 256, 256)
        fine = _transfer_op(request.getfixturevalue("mesh_p2"))
        coarse = _transfer_op(pkg.BrickMesh(1, cells, **BRICKS))
        T = G.Transfer(cells, 2, 1)
    else:
        fine = _transfer_op(request.getfixturevalue("mesh_p2"))
        coarse = _transfer_op(fine.mf_data.mesh.coarsen())
        assert coarse.mf_data.mesh.cells == (128, 128, 128)
        T = H.GeometricTransfer((128, 128, 128), 2)
    nf, nc = int(fine.mf_data.mesh.n_global_dofs), int(coarse.mf_data.mesh.n_global_dofs)
    assert nf == 513 ** 3 and nc == 257 ** 3 and coarse.mf_data.n_local > COMBINE_CAP
    bc = T.boundary_c
    past_cap = np.zeros(nc, dtype=bool)
    past_cap[_perm(coarse)[COMBINE_CAP:]] = True
    assert (past_cap & ~bc).sum() > 1000, (past_cap & ~bc).sum()
    tr = pkg.MGTwoLevelTransfer(fine, coarse, geometric=pair == "h2")
    rng = np.random.default_rng(17)
    ec, b0 = rng.uniform(-1, 1, nc), rng.uniform(-1, 1, nc)         # non-zero on the boundary too: Dirichlet DoFs count as 0
    x0 = rng.uniform(-1, 1, nf)
    x = _dev(x0, fine)
    tr.prolongate_and_add(x, _dev(ec, coarse))
    pe = _lex(x, fine, nf)
    del x
    pe -= x0
    del x0
    assert _rel(pe, T.prolongate(ec)) < 1e-13
    rf = rng.uniform(-1, 1, nf)
    b = _dev(b0, coarse)
    tr.restrict_and_add(b, _dev(rf, fine))
    got = _lex(b, coarse, nc)
    tr.clear()
    ref = T.restrict(rf)
    assert np.array_equal(got[bc], b0[bc])                          # Dirichlet rows unchanged
    assert _rel(got[~bc] - b0[~bc], ref[~bc]) < 1e-13
    tail = past_cap & ~bc                                            # the combine pass's second trip on its own
    assert _rel(got[tail] - b0[tail], ref[tail]) < 1e-13
    lhs, rhs = (got - b0) @ np.where(bc, 0.0, ec), rf @ pe
    assert abs(lhs - rhs) <= 1e-13 * np.abs(rf).sum() * np.abs(ec).max() * 8
    _report(f"transfer {pair}", t0)


@pytest.fixture(scope="module")
def hierarchy(mesh_p4):
    """the hybrid hierarchy of the p = 4 mesh (step-64 kappa) with apply variant 56 on every level; its first three levels are
    make_mg_hierarchy(fine)'s p-only hierarchy"""
    ops = pkg.make_mg_hierarchy(pkg.PoissonOperator(mesh_p4, pkg.QUAD_GAUSS, pkg.COEF_STEP64), h_levels="max")
    for o in ops:
        o.mf_data.set_apply_variant(56)
    assert [(o.mf_data.mesh.degree, o.mf_data.mesh.cells[0]) for o in ops] == [(4, 128), (2, 128), (1, 128), (1, 64), (1, 32), (1, 16), (1, 8),
                                                                                (1, 4)]
    assert ops[1].mf_data.n_local > COMBINE_CAP
    return ops


@pytest.mark.parametrize("h_levels", [0, "max"])
def test_full_size_v_cycle_properties(h_levels, hierarchy):
    """p = 4 on 128^3 cells (1.35e8 DoFs; the bench's brick order, h = 1/128, step-64 kappa), apply variant 56 on every level (bitwise
    reproducible operators), the p-only and the hybrid hierarchy: <u, MG v> = <MG u, v> and <u, MG u> > 0 on vectors that vanish on
    Dirichlet DoFs, two V-cycles give identical bits, and MG-PCG to 1e-8 ||b||: the recomputed ||A x - b|| matches the solver's residual,
    the count is the bench mesh's +-1."""
    torch = _t()
    t0 = time.time()
    ops = hierarchy if h_levels == "max" else hierarchy[:3]
    fine = ops[0]
    mg = pkg.PreconditionMG(ops)
    mf, n = fine.mf_data, fine.mf_data.n_owned
    g = torch.Generator(device="cuda:0").manual_seed(3)
    u = torch.rand(mf.n_local, dtype=torch.float64, device="cuda:0", generator=g) - 0.5
    v = torch.rand(mf.n_local, dtype=torch.float64, device="cuda:0", generator=g) - 0.5
    mf.set_constrained_values(0.0, u)
    mf.set_constrained_values(0.0, v)
    Mu, Mv, Mu2 = (fine.initialize_dof_vector() for _ in range(3))
    mg.vmult(Mu, u)
    mg.vmult(Mv, v)
    mg.vmult(Mu2, u)
    assert torch.equal(Mu, Mu2)
    uMv, vMu, uMu = (float(torch.dot(a[:n], b[:n])) for a, b in ((u, Mv), (v, Mu), (u, Mu)))
    assert uMu > 0
    sym = abs(uMv - vMu) / uMu
    assert sym < 1e-10, sym
    b = fine.assemble_rhs()
    tol = 1e-8 * float(torch.linalg.norm(b[:n]))
    x = fine.initialize_dof_vector()
    ctl = pkg.SolverControl(100, tol)
    pkg.SolverCG(ctl).solve(fine, x, b, mg)
    assert ctl.last_value() <= tol
    Ax = fine.initialize_dof_vector()
    fine.vmult(Ax, x)
    true_res = float(torch.linalg.norm((Ax - b)[:n]))
    assert abs(true_res - ctl.last_value()) < 1e-9 * ctl.initial_value(), (true_res, ctl.last_value())
    print(f"h_levels={h_levels}: {len(ops)} levels, symmetry {sym:.1e}, MG-PCG {ctl.last_step()} iterations")
    assert abs(ctl.last_step() - BENCH_MG_ITERATIONS) <= 1, ctl.last_step()
    mg.clear()
    _report(f"v-cycle h_levels={h_levels}", t0)
