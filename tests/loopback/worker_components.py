"""One rank of an N-rank run of the BLOCK-VECTOR path on one GPU (test infrastructure; started by tests/test_gpu_components_multirank.py
through _run_ranks with BP5_LIB = libbp5_loopback.so).  Only the Python mirror is used -- op.vmult and SolverCG.solve on 2-D tensors -- so
what runs is what the dispatch on PoissonOperator.distributed selects: bp5_apply_components_distributed and
bp5_cg_solve_components_distributed, with the exchange of the block vector between DIFFERENT ranks in every operator application.  The rank's
owned entries go to rank<r>.npz; the parent compares the union over ranks with tests/components_ref.py on the undivided mesh.

  python tests/loopback/worker_components.py RANK WORLD PORT OUTDIR P NX NY NZ DEFORM COEFFICIENT COMPONENTS ITERS WITH_DIAG OVERLAPS [STOP_TOL]
    COMPONENTS, OVERLAPS: comma-separated lists (component counts; overlap modes of the fixed-iteration solves)
    STOP_TOL > 0: one more solve, of the first component count, that stops on this absolute tolerance
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    p, nx, ny, nz = (int(a) for a in sys.argv[5:9])
    deform, coefficient = float(sys.argv[9]), int(sys.argv[10])
    components = [int(a) for a in sys.argv[11].split(",")]
    iters, with_diag = int(sys.argv[12]), int(sys.argv[13]) != 0
    overlaps = [int(a) for a in sys.argv[14].split(",")]
    stop_tol = float(sys.argv[15]) if len(sys.argv) > 15 else 0.0
    assert os.environ.get("BP5_LIB", "").endswith("libbp5_loopback.so"), "this worker must run on the loopback build"
    import torch
    import torch.distributed as dist
    import bp5_oracle as O          # deterministic input vectors only
    import bp5_pkg
    import components_ref as R      # the right-hand sides' modulation only
    pkg = bp5_pkg.load()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        comm = pkg.Communicator.from_torch_distributed()
        mesh = pkg.BrickMesh(p, (nx, ny, nz), deform_amp=deform, rank=rank, n_ranks=world)
        op = pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, coefficient, comm=comm)
        assert op.distributed
        no, nl = mesh.n_owned, mesh.n_owned + mesh.n_ghost
        gid = mesh.global_ids[:no].astype(np.int64)
        n_global = int(mesh.n_global_dofs)
        res = {"gid": mesh.global_ids[:no], "n_ghost": np.asarray(mesh.n_ghost)}
        b = op.assemble_rhs()[:no].cpu().numpy()
        inv = op.compute_diagonal(invert=True) if with_diag else None
        precond = pkg.DiagonalMatrix(inv) if with_diag else pkg.DiagonalMatrix()

        def rhs(nc):
            """components_ref.rhs_blocks evaluated at the global ids: b (1 + 0.5 sin(0.37 (c + 1) i)), i the GLOBAL DoF index"""
            full = np.zeros(n_global)
            full[gid] = b
            B = op.initialize_block_vector(nc)
            B[:, :no] = torch.from_numpy(R.rhs_blocks(full, nc)[:, gid]).cuda()
            return B

        for nc in components:
            # the operator on vectors with non-zero boundary values, every exchange schedule
            src = op.initialize_block_vector(nc)
            for c in range(nc):
                src[c, :no] = torch.from_numpy(O.deterministic_src(n_global, seed=21 + c)[gid]).cuda()
            for mode in (0, 1, 2):
                op.mf_data.set_overlap(mode)
                dst = torch.full_like(src, float("nan"))
                s_in = src.clone()
                op.vmult(dst, s_in)
                assert torch.equal(s_in, src)                    # ghosts of src zeroed again, nothing else touched
                if mesh.n_ghost:
                    assert float(dst[:, no:nl].abs().max()) == 0.0
                res[f"A{mode}_{nc}"] = dst[:, :no].cpu().numpy()
            B = rhs(nc)
            for mode in overlaps:
                op.mf_data.set_overlap(mode)
                x = torch.full_like(B, float("nan"))
                ctl = pkg.IterationNumberControl(iters, 0.0)
                pkg.SolverCG(ctl).solve(op, x, B, precond)
                res[f"x{mode}_{nc}"] = x[:, :no].cpu().numpy()
                res[f"its{mode}_{nc}"] = np.asarray(int(ctl.last_step()))
                res[f"res{mode}_{nc}"] = np.asarray(float(ctl.last_value()))
                res[f"sched{mode}_{nc}"] = np.asarray(int(ctl.exchange_schedule))
                res[f"kernel{mode}_{nc}"] = np.asarray(ctl.apply_kernel)
        if stop_tol > 0.0:
            # tolerance stop across the ranks: every rank sees the same all-reduced residual, the device-side flag fires on all of them in the
            # same iteration and freezes the iterate (check_every = 3: the host looks now and then)
            nc = components[0]
            B = rhs(nc)
            for mode in (0, 1):
                op.mf_data.set_overlap(mode)
                x = op.initialize_block_vector(nc)
                ctl = pkg.SolverControl(400, stop_tol)
                pkg.SolverCG(ctl, check_every=3).solve(op, x, B, precond)
                res[f"x_stop{mode}"] = x[:, :no].cpu().numpy()
                res[f"its_stop{mode}"] = np.asarray(int(ctl.last_step()))
                res[f"res_stop{mode}"] = np.asarray(float(ctl.last_value()))
        np.savez(os.path.join(out, f"rank{rank}.npz"), **res)
        op.mf_data.synchronize()
        op.mf_data.close()
        comm.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
