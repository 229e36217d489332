"""One rank of an N-rank run ON ONE GPU of the mass operator (BP5_OP_MASS; test infrastructure; started by tests/test_gpu_mass_multirank.py with
BP5_LIB = libbp5_loopback.so, as tests/loopback/worker.py): one distributed application, the inverse diagonal, ten Jacobi-CG iterations with
both solvers and a tolerance stop.  The rank's owned entries go to rank<r>.npz.

  python tests/loopback/worker_mass.py RANK WORLD PORT OUTDIR P NX NY NZ BX BY BZ NUMBERING VARIANT OVERLAP ITERATIONS STOP_TOL
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
    p, nx, ny, nz, bx, by, bz, numbering, variant, overlap, iterations = (int(a) for a in sys.argv[5:16])
    stop_tol = float(sys.argv[16])
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
        mesh = pkg.BrickMesh(p, (nx, ny, nz), deform_amp=0.05, rank=rank, n_ranks=world, cell_block=(bx, by, bz), dof_numbering=numbering,
                             cell_block_order=1 if numbering == 1 else 0)
        op = pkg.MassOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_STEP64, comm=comm)
        op.mf_data.set_apply_variant(variant)
        op.mf_data.set_overlap(overlap)
        no = mesh.n_owned
        gid = mesh.global_ids[:no].astype(np.int64)
        res = {"gid": gid, "n_ghost": np.asarray(mesh.n_ghost)}
        s_lex = O.deterministic_src(int(mesh.n_global_dofs), seed=47)            # non-zero on the boundary: the Dirichlet copy is part of the check
        src = op.initialize_dof_vector()
        src[:no] = torch.from_numpy(s_lex[gid]).cuda()
        dst = op.initialize_dof_vector()
        dst.fill_(float("nan"))
        op.vmult(dst, src)                                                       # bp5_apply_distributed
        res["vmult"] = dst[:no].cpu().numpy()
        inv = op.compute_diagonal(invert=True)
        res["inv_diag"] = inv[:no].cpu().numpy()
        b = op.assemble_rhs()
        res["b"] = b[:no].cpu().numpy()
        for name, solver in (("plain", pkg.SolverCG), ("merged", pkg.SolverCGFullMerge)):
            for key, ctl in ((f"x_{name}", pkg.IterationNumberControl(iterations, 0.0)), (f"xtol_{name}", pkg.IterationNumberControl(200, stop_tol))):
                x = op.initialize_dof_vector()
                x.fill_(float("nan"))
                solver(ctl).solve(op, x, b, pkg.DiagonalMatrix(inv))
                res[key] = x[:no].cpu().numpy()
                res["its_" + key] = np.asarray(ctl.last_step())
                res["res_" + key] = np.asarray(ctl.last_value())
                res["sched_" + key] = np.asarray(int(ctl.exchange_schedule))
                res["fused_" + key] = np.asarray(int(ctl.dot_products_fused))
                res["kernel_" + key] = np.asarray(ctl.apply_kernel)
        np.savez(os.path.join(out, f"rank{rank}.npz"), **res)
        op.mf_data.close()
        comm.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
