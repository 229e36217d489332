"""One rank of an N-rank run of PreconditionChebyshev and the preconditioned CG ON ONE GPU (test infrastructure; started by
tests/test_gpu_chebyshev_multirank.py with BP5_LIB = libbp5_loopback.so, as tests/loopback/worker.py).  The estimate (all-reduced CG-Lanczos
on the global-id start vector), vmult / step (distributed operator applications on the Chebyshev work vectors), Chebyshev-PCG at a fixed
iteration count natively and through the Python callbacks, and at a tolerance.  The rank's owned entries go to rank<r>.npz.

  python tests/loopback/worker_chebyshev.py RANK WORLD PORT OUTDIR P NX NY NZ BX BY BZ NUMBERING VARIANT ITERS ABS_TOL
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
    p, nx, ny, nz, bx, by, bz, numbering, variant, iters = (int(a) for a in sys.argv[5:15])
    tol = float(sys.argv[15])
    assert os.environ.get("BP5_LIB", "").endswith("libbp5_loopback.so"), "this worker must run on the loopback build"
    import torch
    import torch.distributed as dist
    import bp5_oracle as O          # deterministic input vectors only
    import bp5_pkg
    pkg = bp5_pkg.load()
    Cheb = pkg.PreconditionChebyshev
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        comm = pkg.Communicator.from_torch_distributed()
        mesh = pkg.BrickMesh(p, (nx, ny, nz), deform_amp=0.05, rank=rank, n_ranks=world, cell_block=(bx, by, bz), dof_numbering=numbering,
                             cell_block_order=1 if numbering == 1 else 0)
        op = pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_STEP64, comm=comm)
        op.mf_data.set_apply_variant(variant)
        no = mesh.n_owned
        gid = mesh.global_ids[:no].astype(np.int64)
        res = {"gid": gid, "n_ghost": np.asarray(mesh.n_ghost)}
        inv = op.compute_diagonal(invert=True)
        res["inv"] = inv[:no].cpu().numpy()
        ch = Cheb().initialize(op, Cheb.AdditionalData(degree=4, smoothing_range=20.0, preconditioner=pkg.DiagonalMatrix(inv)))
        e = ch.estimated_eigenvalues()
        for k in ("min_est", "max_est", "min_used", "max_used", "cg_its"):
            res["est_" + k] = np.asarray(e[k])
        # vmult and step on vectors that are non-zero on the boundary too
        s_lex = O.deterministic_src(int(mesh.n_global_dofs), seed=31)
        x_lex = O.deterministic_src(int(mesh.n_global_dofs), seed=32)
        src = op.initialize_dof_vector()
        src[:no] = torch.from_numpy(s_lex[gid]).cuda()
        dst = op.initialize_dof_vector()
        dst.fill_(float("nan"))                       # prior content (ghost range included) is ignored
        ch.vmult(dst, src)
        res["vmult"] = dst[:no].cpu().numpy()
        x = op.initialize_dof_vector()
        x[:no] = torch.from_numpy(x_lex[gid]).cuda()
        ch.step(x, src)
        res["step"] = x[:no].cpu().numpy()
        b = op.assemble_rhs()

        class PyOperator:                             # reaches the library through the bp5_vmult_fn callbacks
            mf_data = op.mf_data

            def vmult(self, d, s):
                op.vmult(d, s)

        for key, A in (("native", op), ("callback", PyOperator())):
            P = ch if key == "native" else Cheb().initialize(A, Cheb.AdditionalData(degree=4, smoothing_range=20.0, preconditioner=pkg.DiagonalMatrix(inv)))
            c = pkg.IterationNumberControl(iters, 0.0)
            x = op.initialize_dof_vector()
            pkg.SolverCG(c).solve(A, x, b, P)
            res["x_" + key] = x[:no].cpu().numpy()
        for check in (0, 1):
            c = pkg.IterationNumberControl(500, tol)
            x = op.initialize_dof_vector()
            pkg.SolverCG(c, check_every=check).solve(op, x, b, ch)
            res[f"x_tol{check}"] = x[:no].cpu().numpy()
            res[f"its_tol{check}"] = np.asarray(c.last_step())
        np.savez(os.path.join(out, f"rank{rank}.npz"), **res)
        ch.clear()
        op.mf_data.close()
        comm.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
