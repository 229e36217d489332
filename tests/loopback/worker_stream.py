"""One rank of an N-rank run ON ONE GPU with the rank's handle on a busy NON-BLOCKING SIDE STREAM (test infrastructure; started by
tests/test_gpu_stream_multirank.py through _run_ranks with BP5_LIB = libbp5_loopback.so).  Every call goes through the protocol of
tests/stream_harness.py: the working inputs hold NaN, the stream is held, the producers of the good inputs are enqueued behind the hold, the
call is made while the hold lasts, the result is cloned on the stream.  What the library enqueues on another stream than the handle's -- or
on its communication stream without an event from the handle's stream in front -- runs ahead of the producers and sends, packs or reads NaN.
The rank's owned entries go to rank<r>.npz; the parent compares the union over ranks with the oracle on the undivided mesh.

  python tests/loopback/worker_stream.py RANK WORLD PORT OUTDIR P NX NY NZ BX BY BZ NUMBERING ITERS VARIANT
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
    p, nx, ny, nz, bx, by, bz, numbering, iters, variant = (int(a) for a in sys.argv[5:15])
    assert os.environ.get("BP5_LIB", "").endswith("libbp5_loopback.so"), "this worker must run on the loopback build"
    import torch
    import torch.distributed as dist
    import bp5_oracle as O          # deterministic input vectors only
    import bp5_pkg
    import stream_harness as SH
    pkg = bp5_pkg.load()
    nan = float("nan")
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        S = SH.side_stream()
        SH.calibrate()
        with torch.cuda.stream(S):
            comm = pkg.Communicator.from_torch_distributed()
            blocked = numbering == 1 and bx > 2
            mesh = pkg.BrickMesh(p, (nx, ny, nz), deform_amp=0.03, rank=rank, n_ranks=world, cell_block=(bx, by, bz), dof_numbering=numbering,
                                 cell_block_order=1 if blocked else 0)
            op = pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_STEP64, comm=comm)
            assert op.distributed and op.mf_data.stream == S.cuda_stream != 0
            op.mf_data.set_apply_variant(variant)
            no, nl = mesh.n_owned, mesh.n_owned + mesh.n_ghost
            gid = mesh.global_ids[:no].astype(np.int64)
            n_global = int(mesh.n_global_dofs)
            res = {"gid": mesh.global_ids[:no], "variant": np.asarray(op.mf_data.get_apply_variant()), "hold_ms": np.asarray(SH.calibrate()["measured_ms"])}

            def vector(owned, rows=None):
                """(working tensor, staging tensor): owned entries given, ghosts zero; rows: a block vector, the sentinel in its padding"""
                if rows is None:
                    good = torch.zeros(nl, dtype=torch.float64, device="cuda:0")
                    good[:no] = torch.from_numpy(np.ascontiguousarray(owned)).cuda()
                else:
                    good = torch.full((rows, nl + (nl & 1) + 66), SH.SENTINEL, dtype=torch.float64, device="cuda:0")
                    good[:, :nl] = 0.0
                    good[:, :no] = torch.from_numpy(np.ascontiguousarray(owned)).cuda()
                return torch.empty_like(good), good

            def nan_like(t, rows=None):
                pre = torch.full_like(t, nan)
                if rows is not None:
                    pre[:, nl:] = SH.SENTINEL
                return torch.empty_like(t), pre

            # the right-hand side: no input, its zero-fill, cell kernel, compress(add) and Dirichlet rows all behind the hold
            _, b = SH.run(S, [], [], op.assemble_rhs)
            res["b"] = b[:no].cpu().numpy()
            b_w, b_good = torch.empty_like(b), b.clone()
            # the distributed operator, every exchange schedule
            src_w, src_good = vector(O.deterministic_src(n_global, seed=21)[gid])
            dst, dst_pre = nan_like(src_w)
            for mode in (0, 1, 2):
                op.mf_data.set_overlap(mode)
                (got,), _ = SH.run(S, [(src_w, src_good)], [(dst, dst_pre)], lambda: op.vmult(dst, src_w))
                res[f"A{mode}"] = got[:no].cpu().numpy()
            # the three-component operator (one message per neighbour and direction)
            s3_w, s3_good = vector(np.stack([O.deterministic_src(n_global, seed=21 + c)[gid] for c in range(3)]), rows=3)
            d3, d3_pre = nan_like(s3_w, rows=3)
            for mode in (0, 1, 2):
                op.mf_data.set_overlap(mode)
                (got,), _ = SH.run(S, [(s3_w, s3_good)], [(d3, d3_pre)], lambda: op.vmult(d3, s3_w))
                assert bool((got[:, nl:] == SH.SENTINEL).all())
                res[f"A3_{mode}"] = got[:, :no].cpu().numpy()
            # solvers
            x, x_pre = nan_like(b_w)
            x_pre[no:] = 0.0
            norms = []

            def solve(Solver, overlap, key):
                op.mf_data.set_overlap(overlap)
                ctl = pkg.IterationNumberControl(iters, 0.0)
                (got,), _ = SH.run(S, [(b_w, b_good)], [(x, x_pre)], lambda: Solver(ctl).solve(op, x, b_w, pkg.DiagonalMatrix()))
                res["x_" + key] = got[:no].cpu().numpy()
                res["fused_" + key] = np.asarray(bool(ctl.dot_products_fused))
                res["sched_" + key] = np.asarray(int(ctl.exchange_schedule))
                norms.append(ctl.last_value())
                return got

            solve(pkg.SolverCG, 2, "plain")
            solve(pkg.SolverCGFullMerge, 0, "merged_unsplit")
            solve(pkg.SolverCGFullMerge, 1, "merged_overlapped")
            xs = solve(pkg.SolverCGFullMerge, 2, "merged_default")
            solve(pkg.SolverCGFullMerge, 0, "merged_unsplit_again")
            res["norms"] = np.asarray(norms)
            # the ghosted L2 norm: its argument produced behind the hold, its ghosts refreshed inside and zeroed again
            u_w, u_good = torch.empty_like(xs), xs.clone()
            u_good[no:] = 0.0
            _, l2 = SH.run(S, [(u_w, u_good)], [], lambda: op.l2_norm_solution(u_w))
            res["l2"] = np.asarray(l2)
            np.savez(os.path.join(out, f"rank{rank}.npz"), **res)
            op.mf_data.synchronize()
            op.mf_data.close()
            comm.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
