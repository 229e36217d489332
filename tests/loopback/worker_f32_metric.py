"""One rank of an N-rank run ON ONE GPU of the operator and the multigrid preconditioner on FP32 metric planes (bp5_mf_set_metric_precision;
test infrastructure; started by tests/test_gpu_f32_metric_multirank.py with BP5_LIB = libbp5_loopback.so, as tests/loopback/worker.py):
one distributed application of the FP32-plane operator, then the mixed-precision MG-PCG -- outer operator FP64, every level of
make_mg_hierarchy(metric_precision="float32") on float planes.  The rank's owned entries, and every level's planes read back from the
library with the lexicographic index of each cell, go to rank<r>.npz.

  python tests/loopback/worker_f32_metric.py RANK WORLD PORT OUTDIR P NX NY NZ BX BY BZ NUMBERING VARIANT REL_TOL H_LEVELS COARSE_DEGREE
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    out = sys.argv[4]
    p, nx, ny, nz, bx, by, bz, numbering, variant = (int(a) for a in sys.argv[5:14])
    rel_tol = float(sys.argv[14])
    h_levels = sys.argv[15] if sys.argv[15] == "max" else int(sys.argv[15])
    coarse_degree = int(sys.argv[16])
    assert os.environ.get("BP5_LIB", "").endswith("libbp5_loopback.so"), "this worker must run on the loopback build"
    import torch
    import torch.distributed as dist
    import bp5_oracle as O          # deterministic input vectors only
    import bp5_pkg
    import f32_metric_ref as F      # cell order only
    pkg = bp5_pkg.load()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        comm = pkg.Communicator.from_torch_distributed()
        mesh = pkg.BrickMesh(p, (nx, ny, nz), deform_amp=0.05, rank=rank, n_ranks=world, cell_block=(bx, by, bz), dof_numbering=numbering,
                             cell_block_order=1 if numbering == 1 else 0)
        outer = pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_STEP64, comm=comm)
        ops = pkg.make_mg_hierarchy(outer, h_levels=h_levels, metric_precision="float32")
        assert ops[0] is not outer and ops[0].mf_data.mesh is mesh
        for o in [outer] + ops:
            o.mf_data.set_apply_variant(variant)
        op = ops[0]
        no = mesh.n_owned
        gid = mesh.global_ids[:no].astype(np.int64)
        res = {"gid": gid, "n_ghost": np.asarray([o.mf_data.n_ghost for o in ops]), "degrees": np.asarray([o.mf_data.mesh.degree for o in ops]),
               "cells": np.asarray([o.mf_data.mesh.cells for o in ops]), "precision": np.asarray([o.mf_data.get_metric_precision() for o in ops])}
        for lev, o in enumerate(ops):
            m = o.mf_data.mesh
            res[f"planes{lev}"] = o.mf_data.coef_reference_layout(o.coef).cpu().numpy().reshape(6, m.n_cells, -1)
            res[f"cell_lex{lev}"] = F.lexicographic_cells(m)
        s_lex = O.deterministic_src(int(mesh.n_global_dofs), O.BrickMesh(p, (nx, ny, nz)).constrained, seed=43)
        src = op.initialize_dof_vector()
        src[:no] = torch.from_numpy(s_lex[gid]).cuda()
        dst = op.initialize_dof_vector()
        dst.fill_(float("nan"))
        op.vmult(dst, src)                                           # bp5_apply_distributed on float planes
        res["vmult"] = dst[:no].cpu().numpy()
        mg = pkg.PreconditionMG(ops, pkg.PreconditionMG.AdditionalData(coarse_degree=coarse_degree))
        for lev, d in enumerate(mg.level_info()):
            for k in ("min_est", "max_est", "min_used", "max_used", "cg_its"):
                res[f"l{lev}_{k}"] = np.asarray(d[k])
        b = outer.assemble_rhs()
        bnorm = float(torch.linalg.norm(b[:no])) ** 2
        t = torch.tensor([bnorm], dtype=torch.float64)
        dist.all_reduce(t)
        ctl = pkg.SolverControl(200, rel_tol * float(t.item()) ** 0.5)
        x = outer.initialize_dof_vector()
        pkg.SolverCG(ctl).solve(outer, x, b, mg)                     # outer operator FP64, preconditioner on float planes
        res["x"] = x[:no].cpu().numpy()
        res["its"] = np.asarray(ctl.last_step())
        np.savez(os.path.join(out, f"rank{rank}.npz"), **res)
        mg.clear()
        for o in [outer] + ops:
            o.mf_data.close()
        comm.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
