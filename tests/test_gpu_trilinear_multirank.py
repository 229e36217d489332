"""The trilinear geometry mode (BP5_GEOM_TRILINEAR) on 2 ranks as processes on ONE GPU (the loopback build of test_gpu_multirank_loopback.py, every
transfer lagging behind its stream, receive buffers poisoned with NaN), with the one-rank run beside them: one distributed application in each
overlap mode, the inverse diagonal and ten Jacobi-CG iterations with both solvers, whose count and residual are the same on both ranks.  The
reference is the one-rank result, itself held to the numpy oracle on the undivided mesh.  Meshes the generator writes on any rank count and the mode
accepts: p = 1 on the sine mesh (trilinear as generated) and p = 4 on the undeformed mesh.  No new exchange code: the schedules are the atomic kernels'."""
import os

import numpy as np
import pytest

import bp5_oracle as O
from test_gpu_multirank_loopback import ROOT, _rel, _run_ranks

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "loopback", "worker_trilinear.py")
ITERATIONS = 10


def _union(ranks, key, nd):
    full = np.full(nd, np.nan)
    for z in ranks:
        full[z["gid"].astype(np.int64)] = z[key]
    assert not np.isnan(full).any()
    return full


@pytest.mark.parametrize("p,cells,amp_percent,kernel", [(1, (5, 5, 6), 5, "apply_pencil_trilinear_kernel<1,false,1,4,4>"),
                                                        (4, (3, 3, 4), 0, "apply_pencil_trilinear_kernel<4,false,4,25,1>")])
def test_trilinear_handles_across_ranks_match_one_rank(tmp_path, p, cells, amp_percent, kernel):
    world = 2
    pr = O.Problem(p, cells, O.QUAD_GAUSS, deform_amp=amp_percent / 100.0, kappa=O.kappa_step64)
    nd = pr.mesh.n_dofs
    runs = {}
    for w in (1, world):
        out = tmp_path / f"w{w}"
        out.mkdir()
        _run_ranks(w, [p, *cells, amp_percent, ITERATIONS], str(out), worker=WORKER, delay_us=300 if w > 1 else 0)
        runs[w] = [np.load(os.path.join(str(out), f"rank{r}.npz")) for r in range(w)]
    one, many = runs[1], runs[world]
    assert all(int(z["n_ghost"]) > 0 for z in many[1:])
    s = O.deterministic_src(nd, seed=47)
    assert _rel(_union(one, "vmult_0", nd), pr.vmult(s)) <= 1e-13                                        # the reference of this test, pinned outside the library
    for overlap in (0, 1, 2):
        e = _rel(_union(many, f"vmult_{overlap}", nd), _union(one, f"vmult_{overlap}", nd))
        print(f"p={p} overlap {overlap}: {e:.2e}")
        assert e <= 1e-13
    assert _rel(_union(many, "inv_diag", nd), _union(one, "inv_diag", nd)) <= 1e-13
    assert _rel(_union(many, "b", nd), _union(one, "b", nd)) <= 1e-13
    for name in ("plain", "merged"):
        e = _rel(_union(many, f"x_{name}", nd), _union(one, f"x_{name}", nd))
        print(f"p={p} {name}: {e:.2e} kernel {str(many[0]['kernel_' + name])} schedule {int(many[0]['sched_' + name])}")
        assert e <= 1e-11 and all(int(z[f"its_{name}"]) == ITERATIONS for z in one + many)
        assert all(str(z[f"kernel_{name}"]) == kernel and int(z[f"fused_{name}"]) == 0 for z in one + many)
        assert all(float(z[f"res_{name}"]) == float(many[0][f"res_{name}"]) for z in many)               # one all-reduced value on every rank
        ref_res = float(one[0][f"res_{name}"])
        assert abs(float(many[0][f"res_{name}"]) - ref_res) <= 1e-9 * ref_res
        assert all(int(z[f"sched_{name}"]) == 3 for z in many) and int(one[0][f"sched_{name}"]) == 0       # overlap on: the three-phase schedule
