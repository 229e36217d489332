"""One rank of an N-rank run ON ONE GPU (test infrastructure; started by tests/test_gpu_elasticity_mg_multirank.py with BP5_LIB =
libbp5_loopback.so, as tests/loopback/worker.py): the multigrid transfers on block vectors (bp5_mg_transfer_prolongate_add_components,
bp5_mg_transfer_restrict_add_components) REFUSE a transfer whose handles have a communicator and neighbours -- BP5_ERR_UNSUPPORTED, the reason
in bp5_last_error, no byte written -- for a p-transfer and for a geometric one, while the scalar entries of the same handles work.  What the
rank saw goes to rank<r>.npz.

  python tests/loopback/worker_transfer_components.py RANK WORLD PORT OUTDIR
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
SENTINEL = -7.25e30
EXTRA = 66


def main():
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    out = sys.argv[4]
    assert os.environ.get("BP5_LIB", "").endswith("libbp5_loopback.so"), "this worker must run on the loopback build"
    import torch
    import torch.distributed as dist
    import bp5_pkg
    pkg = bp5_pkg.load()
    L = pkg.lib()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        comm = pkg.Communicator.from_torch_distributed()

        def operator(mesh):
            return pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, comm=comm)

        def block(n):
            """(3, ld) tensor filled with the sentinel, rows and padding alike; ld = n rounded up to even + 66"""
            return torch.full((3, n + (n & 1) + EXTRA), SENTINEL, dtype=torch.float64, device="cuda:0")
        res = {}
        cases = []
        mesh_f = pkg.BrickMesh(2, (3, 2, 4), deform_amp=0.04, rank=rank, n_ranks=world)
        cases.append(("p", operator(mesh_f), operator(pkg.BrickMesh(1, (3, 2, 4), deform_amp=0.04, rank=rank, n_ranks=world)), False))
        mesh_g = pkg.BrickMesh(1, (4, 4, 4), deform_amp=0.04, rank=rank, n_ranks=world)
        cases.append(("h", operator(mesh_g), operator(mesh_g.coarsen(2)), True))
        for name, fine, coarse, geometric in cases:
            tr = pkg.MGTwoLevelTransfer(fine, coarse, geometric=geometric)
            res[f"{name}_neighbors"] = np.asarray([fine.mf_data.mesh.n_neighbors, coarse.mf_data.mesh.n_neighbors])
            res[f"{name}_ghosts"] = np.asarray([fine.mf_data.n_ghost, coarse.mf_data.n_ghost])
            xf, xc = block(fine.mf_data.n_local), block(coarse.mf_data.n_local)
            keep_f, keep_c = xf.clone(), xc.clone()
            pf, pc = C.c_void_p(xf.data_ptr()), C.c_void_p(xc.data_ptr())
            st, msgs = [], []
            for ncomp in (1, 3):
                st.append(L.bp5_mg_transfer_prolongate_add_components(tr.handle, ncomp, xf.shape[1], pf, xc.shape[1], pc))
                msgs.append(L.bp5_last_error().decode())
                st.append(L.bp5_mg_transfer_restrict_add_components(tr.handle, ncomp, xc.shape[1], pc, xf.shape[1], pf))
                msgs.append(L.bp5_last_error().decode())
            torch.cuda.synchronize()
            res[f"{name}_status"] = np.asarray(st)
            res[f"{name}_messages"] = np.asarray(msgs)
            res[f"{name}_unchanged"] = np.asarray(bool(torch.equal(xf, keep_f) and torch.equal(xc, keep_c)))
            # the scalar entries of the same handle serve these handles (their halo exchanges included): the refusal is the block entries' own
            sf, sc = fine.initialize_dof_vector(), coarse.initialize_dof_vector()
            sc.fill_(1.0)
            fine.mf_data.set_constrained_values(0.0, sf)
            tr.prolongate_and_add(sf, sc)
            torch.cuda.synchronize()
            res[f"{name}_scalar_norm"] = np.asarray(float(sf[:fine.mf_data.n_owned].norm()))
            tr.clear()
        np.savez(os.path.join(out, f"rank{rank}.npz"), **res)
        for _, fine, coarse, _ in cases:
            fine.mf_data.close()
            coarse.mf_data.close()
        comm.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
