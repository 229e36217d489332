#!/usr/bin/env python3
"""Block-vector operator behind the halo exchange (bp5_apply_components_distributed) on the slab a rank > 0 owns in an N-rank run of the bench
workload, in ONE process with alternating legs and HIP events (the method of tools/bench_components.py).  The exchange is real RCCL traffic
with the rank as its own neighbour (tools/halo_overhead_self.py): one message out and one in per exchange, like a middle rank.  Not an xGMI
measurement: it shows what the library's own exchange kernels, the RCCL groups and the split into ranges cost on one device.

  (a) one bp5_apply_components_distributed, unsplit (overlap off)
  (b) the same, three-phase (overlap on)
  (c) NC calls of bp5_apply_distributed on the atomic pencil kernel, unsplit   -- NC exchanges each way, the metric read NC times
  (d) one bp5_apply_components on the communicator-free twin of the slab       -- the cell kernel without any exchange

usage: python tools/bench_components_halo.py [--cells 116 116 120] [--ranks 8] [--rank 3] [--nc 3] [--json FILE]
Reported per leg: median / min / max ms over the rounds; then (a) - (d), the cost of the exchange, and (a) / (c)."""
import argparse
import ctypes as C
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bp5_pkg

pkg = bp5_pkg.load()
ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, nargs=3, default=[116, 116, 120], help="cells of the WHOLE problem (the slab of --rank of --ranks is cut from it)")
ap.add_argument("--ranks", type=int, default=8)
ap.add_argument("--rank", type=int, default=3)
ap.add_argument("--degree", type=int, default=4)
ap.add_argument("--nc", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--json", default=None)
a = ap.parse_args()


def consistent_self_glue(m1):
    """send indices of a self-neighbour exchange: every ghost DoF glued to an owned DoF of the SAME Dirichlet status (tools/halo_overhead_self.py)"""
    no, ng = m1.n_owned, m1.n_ghost
    con = np.zeros(no + ng, bool)
    con[m1.constrained.astype(np.int64)] = True
    free_owned, dir_owned = np.nonzero(~con[:no])[0][::-1], np.nonzero(con[:no])[0][::-1]
    ghost_con = con[no:]
    send = np.zeros(ng, np.uint32)
    send[ghost_con] = dir_owned[:int(ghost_con.sum())]
    send[~ghost_con] = free_owned[:int((~ghost_con).sum())]
    return send


p, nc = a.degree, a.nc
nx, ny, nz = a.cells
m1 = pkg.BrickMesh(p, (nx, ny, nz), h=1.0 / nx, rank=a.rank, n_ranks=a.ranks)
no, ng = m1.n_owned, m1.n_ghost
nl = no + ng
mesh = SimpleNamespace(degree=p, n=p + 1, cells=(nx, ny, nz), n_cells=m1.n_cells, n_interior_cells=m1.n_interior_cells, n_owned=no, n_ghost=ng, n_local=nl,
                       n_global_dofs=no, l2g=m1.l2g, coords=m1.coords, global_ids=m1.global_ids, constrained=m1.constrained, n_neighbors=1,
                       neighbor_rank=np.zeros(1, np.int32), send_offsets=np.asarray([0, ng], np.uint32), send_indices=consistent_self_glue(m1),
                       recv_offsets=np.asarray([0, ng], np.uint32), cell_block_offsets=None, rank=0, n_ranks=1, h=1.0 / nx, deform_amp=0.0)
comm = pkg.Communicator(0, 1)
op = pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_STEP64, comm=comm)
twin = pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS, pkg.COEF_STEP64)            # the same cells and numbering, no communicator: no exchange
twin.coef = op.coef
L, h, ht = pkg.lib(), op.mf_data.handle, twin.mf_data.handle
ptr = lambda t: C.c_void_p(t.data_ptr())
src, dst = op.initialize_block_vector(nc), op.initialize_block_vector(nc)
ld = src.shape[1]
src[:, :no] = torch.rand((nc, no), dtype=torch.float64, device="cuda") - 0.5
rows = [(src[c, :nl], dst[c, :nl]) for c in range(nc)]


def ok(st):
    if st != 0:
        raise RuntimeError(L.bp5_last_error().decode())


def components(overlap):
    def f():
        ok(L.bp5_mf_set_overlap(h, overlap))
        ok(L.bp5_apply_components_distributed(h, ptr(op.coef), nc, ld, ptr(src), ptr(dst), 1))
    return f


def scalar():
    ok(L.bp5_mf_set_overlap(h, 0))
    for s, d in rows:
        ok(L.bp5_apply_distributed(h, ptr(op.coef), ptr(s), ptr(d), 1))


def no_exchange():
    ok(L.bp5_apply_components(ht, ptr(op.coef), nc, ld, ptr(src), ptr(dst), 1))


legs = [("a components, unsplit", components(0)), ("b components, three-phase", components(1)), ("c scalar pencil x NC, unsplit", scalar),
        ("d components, no exchange", no_exchange)]
times = {name: [] for name, _ in legs}
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
for rnd in range(a.rounds + 1):                      # round 0 warms up
    for name, fn in legs:
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(a.reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        if rnd:
            times[name].append(ev[0].elapsed_time(ev[1]) / a.reps)
ctl = pkg.IterationNumberControl(1, 0.0)
op.mf_data.set_cg_fusion(False)
pkg.SolverCG(ctl).solve(op, op.initialize_dof_vector(), rows[0][0].clone(), pkg.DiagonalMatrix())
scalar_kernel = ctl.apply_kernel
print(f"p={p} slab of rank {a.rank} of {a.ranks} of {a.cells}: cells={m1.n_cells} interior={m1.n_interior_cells} owned DoFs={no} ghosts={ng} NC={nc} "
      f"message {nc * ng * 8 / 1e6:.2f} MB each way; scalar leg: {scalar_kernel}")
out = dict(p=p, cells=a.cells, rank=a.rank, ranks=a.ranks, n_cells=int(m1.n_cells), n_interior=int(m1.n_interior_cells), n_owned=int(no), n_ghost=int(ng), nc=nc,
           rounds=a.rounds, reps=a.reps, scalar_kernel=scalar_kernel, legs=[])
med = {}
for name, _ in legs:
    t = np.array(times[name])
    med[name] = float(np.median(t))
    print(f"  ({name}): median {med[name]:.3f} ms  min {t.min():.3f} max {t.max():.3f} ({len(t)} rounds x {a.reps})")
    out["legs"].append(dict(leg=name, median_ms=med[name], min_ms=float(t.min()), max_ms=float(t.max())))
ma, mb, mc, md = (med[name] for name, _ in legs)
out.update(exchange_ms=ma - md, a_over_c=ma / mc, b_over_a=mb / ma)
print(f"  (a) - (d) = {ma - md:.3f} ms: the exchange (two RCCL groups, four exchange kernels, ghost zeroing)   (a) / (c) = {ma / mc:.3f}   (b) / (a) = {mb / ma:.3f}")
if a.json:
    with open(a.json, "a") as f:
        f.write(json.dumps(out) + "\n")
op.mf_data.synchronize()
