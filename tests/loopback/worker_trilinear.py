"""One rank of an N-rank run ON ONE GPU of the trilinear geometry mode (BP5_GEOM_TRILINEAR; test infrastructure; started by
tests/test_gpu_trilinear_multirank.py with BP5_LIB = libbp5_loopback.so, as tests/loopback/worker.py): one distributed application of the operator
in each overlap mode, the inverse diagonal, and Jacobi-CG iterations with both solvers.  The rank's owned entries go to rank<r>.npz.

  python tests/loopback/worker_trilinear.py RANK WORLD PORT OUTDIR P NX NY NZ AMP_PERCENT ITERATIONS
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    out = sys.argv[4]
    p, nx, ny, nz, amp_percent, iterations = (int(a) for a in sys.argv[5:11])
    assert os.environ.get("BP5_LIB", "").endswith("libbp5_loopback.so"), "this worker must run on the loopback build"
    import torch
    import torch.distributed as dist
    import bp5_oracle as O          # deterministic input vectors only
    import bp5_pkg
    pkg = bp5_pkg.load()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        comm = pkg.Communicator.from_torch_distributed()
        mesh = pkg.BrickMesh(p, (nx, ny, nz), deform_amp=amp_percent / 100.0, rank=rank, n_ranks=world)
        op = pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_STEP64, comm=comm, geometry=pkg.GEOM_TRILINEAR)      # (the corners of ghost nodes included)
        assert op.coef is None
        no = mesh.n_owned
        gid = mesh.global_ids[:no].astype(np.int64)
        res = {"gid": gid, "n_ghost": np.asarray(mesh.n_ghost)}
        s_lex = O.deterministic_src(int(mesh.n_global_dofs), seed=47)            # non-zero on the boundary: the Dirichlet copy is part of the check
        src = op.initialize_dof_vector()
        src[:no] = torch.from_numpy(s_lex[gid]).cuda()
        for overlap in (0, 1, 2):                                                # unsplit; the three-phase schedule of the atomic kernels; the library's choice
            op.mf_data.set_overlap(overlap)
            dst = op.initialize_dof_vector()
            dst.fill_(float("nan"))
            op.vmult(dst, src)                                                   # bp5_apply_distributed
            res[f"vmult_{overlap}"] = dst[:no].cpu().numpy()
            assert float(src[no:].abs().max()) == 0.0 if mesh.n_ghost else True  # the ghosts of src are zero again
        op.mf_data.set_overlap(1)
        inv = op.compute_diagonal(invert=True)
        res["inv_diag"] = inv[:no].cpu().numpy()
        b = op.assemble_rhs()
        res["b"] = b[:no].cpu().numpy()
        for name, solver in (("plain", pkg.SolverCG), ("merged", pkg.SolverCGFullMerge)):
            ctl = pkg.IterationNumberControl(iterations, 0.0)
            x = op.initialize_dof_vector()
            x.fill_(float("nan"))
            solver(ctl).solve(op, x, b, pkg.DiagonalMatrix(inv))
            res[f"x_{name}"] = x[:no].cpu().numpy()
            res[f"its_{name}"] = np.asarray(ctl.last_step())
            res[f"res_{name}"] = np.asarray(ctl.last_value())
            res[f"sched_{name}"] = np.asarray(int(ctl.exchange_schedule))
            res[f"fused_{name}"] = np.asarray(int(ctl.dot_products_fused))
            res[f"kernel_{name}"] = np.asarray(ctl.apply_kernel)
        np.savez(os.path.join(out, f"rank{rank}.npz"), **res)
        op.mf_data.close()
        comm.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
