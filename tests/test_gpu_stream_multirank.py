"""The loopback run of tests/test_gpu_multirank_loopback.py with every rank's handle on a busy non-blocking SIDE STREAM
(tests/loopback/worker_stream.py, tests/stream_harness.py): N processes on one GPU, lagging transfers whose receive buffers hold NaN until the
message has landed, and every call made while its inputs are still NaN behind a hold on the handle's stream.  The halo code takes two streams by
hand -- the handle's and its own communication stream, ordered by events in both directions -- and on the null stream neither a pack kernel on
the wrong stream nor a missing event shows.  The union over ranks against the oracle on the undivided mesh, to the tolerances of the loopback
test: 1e-13 operator, 1e-11 CG at a fixed iteration count."""
import os

import numpy as np
import pytest

import bp5_oracle as O
import bp5_pkg
import components_ref as R
from test_gpu_multirank_loopback import ROOT, _rel, _run_ranks

pytestmark = pytest.mark.gpu
pkg = bp5_pkg.load()
WORKER = os.path.join(ROOT, "tests", "loopback", "worker_stream.py")
ITERS = 8


@pytest.mark.parametrize("world,p,cells,block,numbering,variant,delay_us", [
    (2, 4, (8, 8, 12), (4, 4, 4), 1, 56, 400),   # the bench's configuration: block kernel, fused dot products, every exchange schedule
    (3, 2, (3, 3, 7), (0, 0, 0), 0, 0, 250),     # first / middle / last rank, ragged slabs, atomic pencil kernel (3-phase schedule)
])
def test_ranks_on_side_streams_match_the_undivided_problem(tmp_path, world, p, cells, block, numbering, variant, delay_us):
    _run_ranks(world, [p, *cells, *block, numbering, ITERS, variant], str(tmp_path), worker=WORKER, delay_us=delay_us)
    pr = O.Problem(p, cells, O.QUAD_GAUSS, deform_amp=0.03, kappa=O.kappa_step64)
    nd = pr.mesh.n_dofs
    ranks = [np.load(os.path.join(str(tmp_path), f"rank{r}.npz")) for r in range(world)]
    print("calibrated holds per rank (ms):", [float(z["hold_ms"]) for z in ranks])
    keys = [k for k in ranks[0].files if k[0] in "bAx"]
    full = {k: np.full(ranks[0][k].shape[:-1] + (nd,), np.nan) for k in keys}
    for z in ranks:
        gid = z["gid"].astype(np.int64)
        assert np.isnan(full["b"][gid]).all()                            # every DoF owned by exactly one rank
        for k in keys:
            full[k][..., gid] = z[k]
    assert not any(np.isnan(v).any() for v in full.values())
    b_ref = pr.rhs()
    assert _rel(full["b"], b_ref) < 1e-13
    A_ref = pr.vmult(O.deterministic_src(nd, seed=21))
    A3_ref = R.vmult(pr, np.stack([O.deterministic_src(nd, seed=21 + c) for c in range(3)]))
    for mode in (0, 1, 2):
        assert _rel(full[f"A{mode}"], A_ref) < 1e-13, mode
        assert max(_rel(full[f"A3_{mode}"][c], A3_ref[c]) for c in range(3)) < 1e-13, mode
    x_plain, _, res_plain = O.cg_plain(pr.vmult, b_ref, ITERS)
    x_merged, _, res_merged = O.cg_merged(pr.vmult, b_ref, ITERS)
    assert _rel(full["x_plain"], x_plain) < 1e-11
    for k in ("merged_unsplit", "merged_overlapped", "merged_default", "merged_unsplit_again"):
        assert _rel(full["x_" + k], x_merged) < 1e-11, k
    on_block_kernel = int(ranks[0]["variant"]) == 56
    assert on_block_kernel == (variant == 56)
    if on_block_kernel:        # fixed summation orders, the same kernels over the same workgroup ranges in every schedule: the same bits
        for k in ("merged_unsplit_again", "merged_overlapped", "merged_default"):
            assert np.array_equal(full["x_" + k], full["x_merged_unsplit"]), k
    for z in ranks:
        assert bool(z["fused_merged_unsplit"]) == on_block_kernel and bool(z["fused_merged_overlapped"]) == on_block_kernel
        assert int(z["sched_merged_unsplit"]) == 1 and int(z["sched_merged_overlapped"]) == (2 if on_block_kernel else 3)
        assert int(z["sched_merged_default"]) == (4 if on_block_kernel else 1)
        assert np.array_equal(z["norms"], ranks[0]["norms"])             # every rank sees the same all-reduced residual
    assert abs(ranks[0]["norms"][0] - res_plain) < 1e-9 * np.linalg.norm(b_ref)
    assert abs(ranks[0]["norms"][1] - res_merged) < 1e-9 * np.linalg.norm(b_ref)
    l2 = O.l2_norm_solution(pr.mesh, full["x_merged_default"])
    for z in ranks:
        assert abs(float(z["l2"]) - l2) < 1e-12 * l2
