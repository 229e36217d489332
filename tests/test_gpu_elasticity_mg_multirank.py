"""The block-vector multigrid transfers refuse a transfer whose handles have a communicator and neighbours (include/bp5.h:
bp5_mg_transfer_prolongate_add_components, bp5_mg_transfer_restrict_add_components): two ranks as processes on ONE GPU (the loopback build of
test_gpu_multirank_loopback.py), a p-transfer and a geometric one between handles that exchange halos.  Both entries, with one and with three
components, return BP5_ERR_UNSUPPORTED, bp5_last_error names the missing halo exchange and the neighbours, and the sentinel-filled block vectors
are not touched; the scalar entries of the same transfer handles work."""
import os

import numpy as np
import pytest

from test_gpu_multirank_loopback import ROOT, _run_ranks

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "loopback", "worker_transfer_components.py")
UNSUPPORTED = 5


def test_block_transfers_refuse_handles_with_neighbours(tmp_path):
    world = 2
    _run_ranks(world, [], str(tmp_path), worker=WORKER, timeout=120)
    ranks = [np.load(os.path.join(str(tmp_path), f"rank{r}.npz")) for r in range(world)]
    for r, z in enumerate(ranks):
        for name in ("p", "h"):
            assert (z[f"{name}_neighbors"] > 0).all(), (r, name, z[f"{name}_neighbors"])           # fine and coarse handle have a neighbour
            assert z[f"{name}_status"].tolist() == [UNSUPPORTED] * 4, (r, name, z[f"{name}_status"])
            for msg in z[f"{name}_messages"].tolist():
                assert "neighbours" in msg and "halo" in msg and "block vectors" in msg, (r, name, msg)
            assert bool(z[f"{name}_unchanged"]), (r, name, "a refused call wrote to a vector")
            assert float(z[f"{name}_scalar_norm"]) > 0.0
    assert all(int(z[f"{name}_ghosts"][0]) > 0 for z in ranks[1:] for name in ("p", "h"))           # the upper rank holds ghost DoFs
