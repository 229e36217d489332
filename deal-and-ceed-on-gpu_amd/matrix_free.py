"""Host-side mirror of the reference's operator/solver interface for the BP5 path, on top of the
C ABI (include/bp5.h).  Names, argument meaning and error behaviour follow the reference:

  MatrixFree ............. CUDAWrappers::MatrixFree<3,double> as used at bp5/step-64.cu:234-275
  PoissonOperator ........ bp5/step-64.cu:198-276 (vmult, initialize_dof_vector, do_zero_out)
  DiagonalMatrix ......... bp5/step-64.cu:428-432 (get_vector)
  IterationNumberControl . bp5/step-64.cu:443-445 (last_step)
  SolverCG ............... deal.II SolverCG, call site bp5/step-64.cu:446-453
  SolverCGFullMerge ...... bp5/solver.h:16-30,343-542 (x-update schedule fixed)
  PreconditionChebyshev .. deal.II PreconditionChebyshev<Operator, Vector, DiagonalMatrix> (Chebyshev-Jacobi, include/bp5.h)
  MGTwoLevelTransfer ..... deal.II MGTwoLevelTransfer (p-transfer between FE_Q(p) and FE_Q(p/2) on the same cells; geometric
                           transfer between 2:1 meshes of one degree, reinit_geometric_transfer)
  PreconditionMG ......... deal.II PreconditionMG / Multigrid: V-cycle with Chebyshev smoothers (step-37), p-coarsening, then optional
                           h-coarsening at degree 1 (step-75's global coarsening)

Vectors are torch float64 CUDA tensors of n_owned + n_ghost entries (torch is plumbing for
device memory / streams / the process group only -- no torch op is on the hot path).

Block vectors (deal.II BlockVector over one scalar DoFHandler; CEED BP6): a contiguous 2-D tensor of shape (n_components, ld), component c
in row c laid out like a scalar vector, ld = n_local rounded up to even (initialize_block_vector).  PoissonOperator.vmult and
SolverCG.solve take them (bp5_apply_components, bp5_cg_solve_components; their *_distributed twins on more than one rank); everything else
refuses them with status 5."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import BP5Error, CG_MERGED, CG_PLAIN, COEF_ONE, QUAD_GAUSS


def _torch():
    import torch
    return torch


def _ptr(t, n_min=0):
    torch = _torch()
    if t is None:
        return None
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
        raise BP5Error(1, "expected a contiguous float64 CUDA tensor")
    if t.numel() < n_min:
        raise BP5Error(1, f"vector has {t.numel()} entries, need {n_min}")
    return C.c_void_p(t.data_ptr())


class Communicator:
    """RCCL communicator, one rank per GPU.  The 128-byte unique id is created on rank 0 and
    broadcast by the host (here: torch.distributed, any backend)."""

    def __init__(self, rank=0, n_ranks=1, unique_id=None):
        L = _lib.lib()
        if unique_id is None:
            buf = C.create_string_buffer(_lib.UNIQUE_ID_BYTES)
            _lib.check(L.bp5_comm_unique_id(buf))
            unique_id = buf.raw
        self.rank, self.n_ranks = rank, n_ranks
        self._h = C.c_void_p()
        _lib.check(L.bp5_comm_create(C.c_char_p(unique_id), rank, n_ranks, C.byref(self._h)))

    @classmethod
    def from_torch_distributed(cls):
        import torch.distributed as dist
        rank, n = dist.get_rank(), dist.get_world_size()
        box = [None]
        if rank == 0:
            buf = C.create_string_buffer(_lib.UNIQUE_ID_BYTES)
            _lib.check(_lib.lib().bp5_comm_unique_id(buf))
            box[0] = buf.raw
        dist.broadcast_object_list(box, src=0)
        return cls(rank, n, box[0])

    def close(self):
        if self._h:
            _lib.lib().bp5_comm_destroy(self._h)
            self._h = C.c_void_p()


class MatrixFree:
    """== CUDAWrappers::MatrixFree<3,double>; reinit uploads the flat per-cell arrays."""

    def __init__(self):
        self._h = None
        self.mesh = None
        self.stream = None

    def reinit(self, mesh, quadrature=QUAD_GAUSS, coefficient=COEF_ONE, device=0, stream=None, comm=None):
        """== mf_data.reinit(mapping, dof_handler, constraints, quad, additional_data),
        bp5/step-64.cu:234-248."""
        torch = _torch()
        L = _lib.lib()
        self.mesh, self.quadrature, self.coefficient, self.device = mesh, quadrature, coefficient, device
        if stream is None:
            stream = torch.cuda.current_stream(device).cuda_stream
        stream = int(getattr(stream, "cuda_stream", stream))          # a torch stream or a raw hipStream_t; 0: the null stream
        d = _lib.MFDesc()
        d.dim, d.degree, d.quadrature, d.coefficient = 3, mesh.degree, quadrature, coefficient
        d.n_cells, d.n_interior_cells, d.n_owned, d.n_ghost = mesh.n_cells, mesh.n_interior_cells, mesh.n_owned, mesh.n_ghost
        keep = [np.ascontiguousarray(mesh.l2g, dtype=np.uint32), np.ascontiguousarray(mesh.coords, dtype=np.float64),
                np.ascontiguousarray(mesh.constrained, dtype=np.uint32), np.ascontiguousarray(mesh.neighbor_rank, dtype=np.int32),
                np.ascontiguousarray(mesh.send_offsets, dtype=np.uint32), np.ascontiguousarray(mesh.send_indices, dtype=np.uint32),
                np.ascontiguousarray(mesh.recv_offsets, dtype=np.uint32)]
        d.local_to_global_host, d.node_coords_host, d.constrained_host = keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data
        d.n_constrained = keep[2].size
        d.n_neighbors = int(mesh.n_neighbors)
        d.neighbor_rank_host, d.send_offsets_host = keep[3].ctypes.data, keep[4].ctypes.data
        d.send_indices_host, d.recv_offsets_host = keep[5].ctypes.data, keep[6].ctypes.data
        d.device, d.stream = device, stream
        blocks = getattr(mesh, "cell_block_offsets", None)
        if blocks is not None:
            keep.append(np.ascontiguousarray(blocks, dtype=np.uint32))
            d.n_cell_blocks, d.cell_block_offsets_host = keep[-1].size - 1, keep[-1].ctypes.data
        cmask = getattr(mesh, "constraint_mask", None)      # hanging-node masks of 2:1 refined meshes (BP5_HANG_* bits)
        if cmask is not None:
            keep.append(np.ascontiguousarray(cmask, dtype=np.uint32))
            d.constraint_mask_host = keep[-1].ctypes.data
        h = C.c_void_p()
        _lib.check(L.bp5_mf_create(C.byref(d), C.byref(h)))
        self._h = h
        self.stream = stream
        self.n_owned, self.n_ghost, self.n_local = mesh.n_owned, mesh.n_ghost, mesh.n_owned + mesh.n_ghost
        self.comm = comm
        if comm is not None:
            _lib.check(L.bp5_mf_set_comm(h, comm._h))
        return self

    # -- handle plumbing
    @property
    def handle(self):
        if not self._h:
            raise BP5Error(1, "MatrixFree.reinit has not been called")
        return self._h

    def close(self):
        if self._h:
            _lib.lib().bp5_mf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _lib.check(_lib.lib().bp5_mf_sync(self.handle))

    def set_stream(self, stream):
        """bp5_mf_set_stream: every later call on this handle enqueues on `stream` (a torch.cuda.Stream or a raw hipStream_t as an int; 0: the
        null stream; None is refused -- in reinit it means torch's current stream, and a handle is never moved silently).  The caller orders the new stream behind the work already enqueued on the old one.  The classes here
        allocate and fill with torch, so `stream` should be torch's current stream whenever they are used (`with torch.cuda.stream(s):`).
        Objects built on the handle (PreconditionChebyshev, PreconditionMG, transfers) follow it: they hold no stream of their own; the
        levels of one PreconditionMG must be moved together."""
        if stream is None:
            raise BP5Error(1, "set_stream: pass a stream, or 0 for the null stream")
        stream = int(getattr(stream, "cuda_stream", stream))
        _lib.check(_lib.lib().bp5_mf_set_stream(self.handle, C.c_void_p(stream)))
        self.stream = stream

    def set_geometry_mode(self, mode):
        """BP5_GEOM_MERGED6 (reference representation, default), BP5_GEOM_AFFINE (affine meshes) or BP5_GEOM_TRILINEAR (straight-sided
        meshes, deal.II's MappingQ1: the metric from the cells' vertices inside the operator kernel)."""
        _lib.check(_lib.lib().bp5_mf_set_geometry_mode(self.handle, int(mode)))

    def set_overlap(self, mode=True):
        """== AdditionalData::overlap_communication_computation (bp5/step-64.cu:241): True / 1 on, False / 0 off, 2 = the
        library decides by the slab's size (default)."""
        _lib.check(_lib.lib().bp5_mf_set_overlap(self.handle, int(mode)))

    def set_cg_fusion(self, on=True):
        """SolverCGFullMerge: dot products inside the block kernel's write-out (default) or as a separate kernel."""
        _lib.check(_lib.lib().bp5_mf_set_cg_fusion(self.handle, 1 if on else 0))

    def set_apply_variant(self, v):
        _lib.check(_lib.lib().bp5_mf_set_apply_variant(self.handle, int(v)))

    def set_operator(self, op):
        """OP_POISSON (bp5/step-64.cu:147-194, default), OP_HELMHOLTZ (step-64/step-64.cu:154-160,201-219: seven planes) or OP_MASS
        (MatrixFreeOperators::MassOperator, CEED BP1: one plane)."""
        _lib.check(_lib.lib().bp5_mf_set_operator(self.handle, int(op)))

    METRIC_PRECISION = {"float64": 0, "float32": 1}   # bp5.h: BP5_METRIC_*

    def set_metric_precision(self, precision):
        """"float64" (default) or "float32": storage type of the merged-metric planes (bp5_mf_set_metric_precision; arithmetic and vectors
        stay double).  Before coef_size / evaluate_coefficients.  The coef tensor of a float32 handle is opaque: float64 storage of
        ceil(6 n_cells n^3 / 2) entries that holds the floats; coef_reference_layout widens them."""
        if precision not in self.METRIC_PRECISION:
            raise BP5Error(1, f"metric precision must be 'float64' or 'float32', not {precision!r}")
        _lib.check(_lib.lib().bp5_mf_set_metric_precision(self.handle, self.METRIC_PRECISION[precision]))

    def get_metric_precision(self):
        v = C.c_int()
        _lib.check(_lib.lib().bp5_mf_get_metric_precision(self.handle, C.byref(v)))
        return "float32" if v.value == 1 else "float64"

    def set_block_workgroups(self, n):
        _lib.check(_lib.lib().bp5_mf_set_block_workgroups(self.handle, int(n)))

    def set_streaming(self, policy):
        """1: non-temporal accesses to once-used data (metric planes; v, x in the update kernel), 0: ordinary, -1: by local size (default)."""
        _lib.check(_lib.lib().bp5_mf_set_streaming(self.handle, int(policy)))

    TUNE = {"lattice_indices": 0, "early_gather": 1, "combine_signal": 2, "boundary_first": 3, "fold_small": 4, "update_unroll": 5,
            "update_flat": 6, "update_nt": 7, "combine_wg_per_cu": 8, "interior_stores": 9, "ghost_combine_on_comm": 10, "face_carry": 11, "fused_update": 12}   # bp5.h: BP5_TUNE_*

    def set_tuning(self, knob, value):
        """Per-handle A/B knob (bp5.h BP5_TUNE_*; same bits for every setting); knob by name or number."""
        _lib.check(_lib.lib().bp5_mf_set_tuning(self.handle, int(self.TUNE.get(knob, knob)), int(value)))

    def get_tuning(self, knob):
        v = C.c_int()
        _lib.check(_lib.lib().bp5_mf_get_tuning(self.handle, int(self.TUNE.get(knob, knob)), C.byref(v)))
        return v.value

    def wait_value_available(self):
        """True when the in-launch stream wait-value schedules passed the handle's self-check (bp5.h)."""
        v = C.c_int()
        _lib.check(_lib.lib().bp5_mf_wait_value_available(self.handle, C.byref(v)))
        return bool(v.value)

    def block_plan_info(self):
        """(n_blocks, max_runs, packed_indices) of the block kernel's plan."""
        nb, mr, pk = C.c_uint32(), C.c_uint32(), C.c_int()
        _lib.check(_lib.lib().bp5_mf_block_plan_info(self.handle, C.byref(nb), C.byref(mr), C.byref(pk)))
        return nb.value, mr.value, bool(pk.value)

    def block_plan_lattice(self):
        """number of the block plan's LATTICE blocks (closed-form indices: no per-DoF index stream)"""
        n = C.c_uint32()
        _lib.check(_lib.lib().bp5_mf_block_plan_lattice(self.handle, C.byref(n)))
        return n.value

    def block_plan_carry(self):
        """(faces the plan can carry in LDS from block to block, brick-surface DoFs, brick-surface DoFs in the combine tables of the last block launch)"""
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _lib.check(_lib.lib().bp5_mf_block_plan_carry(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def get_apply_variant(self):
        """The kernel variant a whole-range application resolves to (what 0 = default means here)."""
        v = C.c_int()
        _lib.check(_lib.lib().bp5_mf_get_apply_variant(self.handle, C.byref(v)))
        return v.value

    # -- reference API
    def initialize_dof_vector(self, vec=None):
        """== mf_data.initialize_dof_vector(vec), bp5/step-64.cu:214: owned + ghost storage."""
        torch = _torch()
        return torch.zeros(self.n_local, dtype=torch.float64, device=f"cuda:{self.device}")

    def initialize_block_vector(self, n_components):
        """Zero-filled block vector: contiguous (n_components, ld) with ld = n_local rounded up to even (include/bp5.h: block vectors)."""
        torch = _torch()
        if not 1 <= int(n_components) <= _lib.MAX_COMPONENTS:
            raise BP5Error(1, f"n_components must be 1 .. {_lib.MAX_COMPONENTS}, not {n_components!r}")
        return torch.zeros((int(n_components), self.n_local + (self.n_local & 1)), dtype=torch.float64, device=f"cuda:{self.device}")

    def coef_size(self):
        n = C.c_size_t()
        _lib.check(_lib.lib().bp5_mf_coef_size(self.handle, C.byref(n)))
        return n.value

    def evaluate_coefficients(self, coef=None):
        """== mf_data.evaluate_coefficients(JacobianFunctor), bp5/step-64.cu:256-258."""
        torch = _torch()
        if coef is None:
            coef = torch.empty(max(self.coef_size(), 1), dtype=torch.float64, device=f"cuda:{self.device}")
        _lib.check(_lib.lib().bp5_mf_compute_merged_metric(self.handle, _ptr(coef, self.coef_size())))
        return coef

    def coef_reference_layout(self, coef):
        """The planes in the reference layout [c][cell][q], as doubles (float32 planes widened: the operator the kernels apply)."""
        torch = _torch()
        if self.get_metric_precision() == "float32":      # the opaque tensor holds floats: one double per entry comes back
            out = torch.empty(6 * self.mesh.n_cells * (self.mesh.degree + 1) ** 3, dtype=torch.float64, device=coef.device)
        else:
            out = torch.empty_like(coef)
        _lib.check(_lib.lib().bp5_mf_metric_to_reference_layout(self.handle, _ptr(coef, self.coef_size()), _ptr(out)))
        return out

    def cell_loop(self, coef, src, dst, cell_begin=0, cell_end=None):
        """== mf_data.cell_loop(LocalPoissonOperator, src, dst), bp5/step-64.cu:274 (one range)."""
        if cell_end is None:
            cell_end = self.mesh.n_cells
        _lib.check(_lib.lib().bp5_apply_cells(self.handle, _ptr(coef), _ptr(src, self.n_local), _ptr(dst, self.n_local),
                                              cell_begin, cell_end))

    def copy_constrained_values(self, src, dst):
        _lib.check(_lib.lib().bp5_copy_constrained(self.handle, _ptr(src, self.n_local), _ptr(dst, self.n_local)))

    def set_constrained_values(self, value, dst):
        _lib.check(_lib.lib().bp5_set_constrained(self.handle, float(value), _ptr(dst, self.n_local)))

    # -- halo exchange of a block vector (2-D tensor): one message per neighbour and direction, whatever n_components is
    def update_ghost_values_block(self, v):
        """== BlockVector::update_ghost_values()"""
        nc, ld = _block_args(self, v)
        _lib.check(_lib.lib().bp5_halo_gather_components(self.handle, nc, ld, _ptr(v)))

    def compress_add_block(self, v):
        """== BlockVector::compress(VectorOperation::add); ghosts zero afterwards"""
        nc, ld = _block_args(self, v)
        _lib.check(_lib.lib().bp5_halo_scatter_add_components(self.handle, nc, ld, _ptr(v)))

    def zero_out_ghosts_block(self, v):
        """== BlockVector::zero_out_ghosts()"""
        nc, ld = _block_args(self, v)
        _lib.check(_lib.lib().bp5_halo_zero_ghosts_components(self.handle, nc, ld, _ptr(v)))

    def get_data(self, color=0):
        d = _lib.MFData()
        _lib.check(_lib.lib().bp5_mf_get_data(self.handle, color, C.byref(d)))
        return d


class PoissonOperator:
    """== BP5::PoissonOperator<3,fe_degree>, bp5/step-64.cu:198-276."""

    def __init__(self, mesh, quadrature=QUAD_GAUSS, coefficient=COEF_ONE, device=0, comm=None, stream=None, geometry=0, metric_precision="float64"):
        if metric_precision not in MatrixFree.METRIC_PRECISION:       # (before a handle exists: nothing to release)
            raise BP5Error(1, f"metric precision must be 'float64' or 'float32', not {metric_precision!r}")
        self.mf_data = MatrixFree().reinit(mesh, quadrature, coefficient, device, stream, comm)
        self.geometry = geometry
        self.metric_precision = metric_precision
        if metric_precision != "float64":         # "float32": float planes, double arithmetic (MatrixFree.set_metric_precision)
            self.mf_data.set_metric_precision(metric_precision)
        if geometry in (_lib.GEOM_AFFINE, _lib.GEOM_TRILINEAR):   # per-cell metric + one scalar plane / the cells' vertices: no 6-plane array at all
            self.mf_data.set_geometry_mode(geometry)
            self.coef = None
        else:
            self.coef = self.mf_data.evaluate_coefficients()
        self.n_owned_cells = mesh.n_cells
        self.do_zero_out = True                      # bp5/step-64.cu:223,232
        self.distributed = comm is not None and comm.n_ranks > 1

    def initialize_dof_vector(self, vec=None):
        return self.mf_data.initialize_dof_vector(vec)

    def initialize_block_vector(self, n_components):
        return self.mf_data.initialize_block_vector(n_components)

    def vmult(self, dst, src):
        """dst = [0 +] A src; dst[c] = src[c] on Dirichlet DoFs (bp5/step-64.cu:263-276).  Block vectors (2-D tensors): the same on every
        component with one pass over the metric (bp5_apply_components; on more than one rank bp5_apply_components_distributed, which
        brings the halo exchange of the block vector)."""
        L, mf = _lib.lib(), self.mf_data
        dst, src = _vals(dst), _vals(src)
        if _is_block(dst) or _is_block(src):
            nc, ld = _block_args(mf, dst, src)
            fn = L.bp5_apply_components_distributed if self.distributed else L.bp5_apply_components
            _lib.check(fn(mf.handle, _ptr(self.coef), nc, ld, _ptr(src), _ptr(dst), 1 if self.do_zero_out else 0))
            return
        fn = L.bp5_apply_distributed if self.distributed else L.bp5_apply
        _lib.check(fn(mf.handle, _ptr(self.coef), _ptr(src, mf.n_local), _ptr(dst, mf.n_local), 1 if self.do_zero_out else 0))

    def compute_diagonal(self, invert=False):
        """diag(A_eff) (1 on Dirichlet DoFs) or, with invert=True, the Jacobi preconditioner vector for
        DiagonalMatrix (the `diag` the reference's solver kernels multiply by, bp5/solver.h:68,100,131,170)."""
        d = self.initialize_dof_vector()
        _lib.check(_lib.lib().bp5_compute_diagonal(self.mf_data.handle, _ptr(self.coef), _ptr(d), 1 if invert else 0))
        return d

    def assemble_rhs(self):
        b = self.initialize_dof_vector()
        _lib.check(_lib.lib().bp5_assemble_rhs(self.mf_data.handle, _ptr(b)))
        return b

    def l2_norm_solution(self, u):
        r = C.c_double()
        _lib.check(_lib.lib().bp5_l2_norm_solution(self.mf_data.handle, _ptr(u, self.mf_data.n_local), C.byref(r)))
        return r.value


class HelmholtzOperator(PoissonOperator):
    """== Step64::HelmholtzOperator<3,fe_degree>, step-64/step-64.cu:233-305: (grad v, grad u) + (v, a(x) u) with
    a = 10 / (0.05 + 2 |x|^2) (VaryingCoefficientFunctor, :99-118) as the library's native fused kernel
    (bp5_mf_set_operator(BP5_OP_HELMHOLTZ)): `coef` holds the six merged planes and the mass plane a JxW.  vmult, the solvers
    (cg.solve(A, x, b, P): the PoissonOperator branch of Solver.solve -- same handle, same entry points) and the halo exchange
    are the ones of the Poisson operator."""

    def __init__(self, mesh, quadrature=QUAD_GAUSS, coefficient=1, device=0, comm=None, stream=None):
        self.mf_data = MatrixFree().reinit(mesh, quadrature, coefficient, device, stream, comm)
        self.mf_data.set_operator(_lib.OP_HELMHOLTZ)
        self.geometry = 0
        self.metric_precision = "float64"
        self.coef = self.mf_data.evaluate_coefficients()
        self.n_owned_cells = mesh.n_cells
        self.do_zero_out = True
        self.distributed = comm is not None and comm.n_ranks > 1


class MassOperator(PoissonOperator):
    """== MatrixFreeOperators::MassOperator<3,fe_degree> (CEED BP1): (v, rho(x) u) as the library's native mass kernel
    (bp5_mf_set_operator(BP5_OP_MASS)): `coef` holds ONE plane, rho JxW, rho = `coefficient` (COEF_ONE by default).  vmult,
    compute_diagonal, assemble_rhs, l2_norm_solution, the solvers (the PoissonOperator branch of Solver.solve) and the halo exchange
    are the ones of the Poisson operator; block vectors are refused (BP5Error 5)."""

    def __init__(self, mesh, quadrature=QUAD_GAUSS, coefficient=COEF_ONE, device=0, comm=None, stream=None):
        self.mf_data = MatrixFree().reinit(mesh, quadrature, coefficient, device, stream, comm)
        self.mf_data.set_operator(_lib.OP_MASS)
        self.geometry = 0
        self.metric_precision = "float64"
        self.coef = self.mf_data.evaluate_coefficients()
        self.n_owned_cells = mesh.n_cells
        self.do_zero_out = True
        self.distributed = comm is not None and comm.n_ranks > 1


class ElasticityOperator:
    """Linear elasticity on three-component block vectors (deal.II step-8 / step-18; the CEED "solids" mini-app):
    a(v, u) = int kappa [ lam (div v)(div u) + 2 mu eps(v) : eps(u) ] as the library's native coupled kernel (bp5_elasticity_*, include/bp5.h).
    `coef` holds the operator's TEN planes (K and kappa JxW); vectors are (3, ld) tensors; all three components are clamped on the mesh's
    Dirichlet set.  SolverCG.solve(op, x, b, DiagonalMatrix(block inverse diagonal or None)) runs bp5_cg_solve_elasticity; SolverCGFullMerge,
    PreconditionChebyshev and PreconditionMG refuse it (BP5Error 5): its preconditioners are ElasticityPreconditionChebyshev and
    ElasticityPreconditionMG, which SolverCG.solve takes.  Not a PoissonOperator: nothing scalar is offered."""

    n_components = 3

    def __init__(self, mesh, quadrature=QUAD_GAUSS, coefficient=COEF_ONE, lam=1.0, mu=1.0, device=0, stream=None):
        torch = _torch()
        self.lam, self.mu = float(lam), float(mu)
        self.mf_data = MatrixFree().reinit(mesh, quadrature, coefficient, device, stream, None)
        n = C.c_size_t()
        _lib.check(_lib.lib().bp5_elasticity_coef_size(self.mf_data.handle, C.byref(n)))
        self.coef = torch.empty(max(n.value, 2), dtype=torch.float64, device=f"cuda:{device}")
        _lib.check(_lib.lib().bp5_elasticity_compute_metric(self.mf_data.handle, _ptr(self.coef)))
        self.n_owned_cells = mesh.n_cells
        self.do_zero_out = True
        self.distributed = False

    def initialize_block_vector(self):
        return self.mf_data.initialize_block_vector(3)

    def _args(self, *vectors):
        nc, ld = _block_args(self.mf_data, *vectors)
        if nc != 3:
            raise BP5Error(1, f"elasticity: block vectors of three components expected, got {nc}")
        return ld

    def vmult(self, dst, src):
        """dst = [0 +] A src on (3, ld) tensors; dst_c = src_c on Dirichlet DoFs (bp5_elasticity_apply)."""
        dst, src = _vals(dst), _vals(src)
        ld = self._args(dst, src)
        _lib.check(_lib.lib().bp5_elasticity_apply(self.mf_data.handle, _ptr(self.coef), self.lam, self.mu, ld, _ptr(src), _ptr(dst), 1 if self.do_zero_out else 0))

    def cell_loop(self, src, dst, cell_begin=0, cell_end=None):
        """dst += A src over the cells [cell_begin, cell_end), no Dirichlet copy (bp5_elasticity_apply_cells)."""
        ld = self._args(dst, src)
        cell_end = self.n_owned_cells if cell_end is None else cell_end
        _lib.check(_lib.lib().bp5_elasticity_apply_cells(self.mf_data.handle, _ptr(self.coef), self.lam, self.mu, ld, _ptr(src), _ptr(dst), cell_begin, cell_end))

    def compute_diagonal(self, invert=False):
        """the three diagonals as a (3, ld) tensor (1 on Dirichlet DoFs); invert=True: the block Jacobi preconditioner for DiagonalMatrix"""
        d = self.initialize_block_vector()
        _lib.check(_lib.lib().bp5_elasticity_compute_diagonal(self.mf_data.handle, _ptr(self.coef), self.lam, self.mu, d.shape[1], _ptr(d), 1 if invert else 0))
        return d

    def assemble_rhs(self):
        """the scalar load vector b_i = int phi_i (bp5_assemble_rhs): a body force f is b_c = f_c * assemble_rhs()"""
        b = self.mf_data.initialize_dof_vector()
        _lib.check(_lib.lib().bp5_assemble_rhs(self.mf_data.handle, _ptr(b)))
        return b

    def l2_norm_solution(self, u):
        """the L2 norm of ONE component (a 1-D view of its block)"""
        r = C.c_double()
        _lib.check(_lib.lib().bp5_l2_norm_solution(self.mf_data.handle, _ptr(u, self.mf_data.n_local), C.byref(r)))
        return r.value


class HyperelasticityOperator:
    """Finite-strain compressible neo-Hookean elasticity on three-component block vectors (the CEED "solids" mini-app's ElasFSInitialNH1F; deal.II
    step-44 / step-72): Phi(F) = lam / 2 (ln J)^2 - mu ln J + mu / 2 (tr F^T F - 3) as the library's native residual and tangent kernels
    (bp5_hyperelasticity_*, include/bp5.h).  residual(r, u) evaluates F_int(u) and stores the state (B = F^-T and ln J at every quadrature point);
    vmult(dst, src) is the tangent AT THAT STATE.  `linear` is the ElasticityOperator on the same handle and geometry planes -- the tangent at u = 0:
    build ElasticityPreconditionChebyshev / ElasticityPreconditionMG from it and hand them to SolverCG.solve(op, x, b, P)
    (bp5_cg_solve_hyperelasticity; None = no preconditioner) or NewtonSolver.solve(op, u, f_ext, P)."""

    n_components = 3

    def __init__(self, mesh, quadrature=QUAD_GAUSS, coefficient=COEF_ONE, lam=1.0, mu=1.0, device=0, stream=None):
        torch = _torch()
        self.linear = ElasticityOperator(mesh, quadrature, coefficient, lam, mu, device, stream)
        self.lam, self.mu, self.mf_data, self.coef = self.linear.lam, self.linear.mu, self.linear.mf_data, self.linear.coef
        n = C.c_size_t()
        _lib.check(_lib.lib().bp5_hyperelasticity_state_size(self.mf_data.handle, C.byref(n)))
        self.state = torch.zeros(max(n.value, 2), dtype=torch.float64, device=f"cuda:{device}")
        self.n_owned_cells = mesh.n_cells
        self.do_zero_out = True
        self.distributed = False
        self.residual(self.initialize_block_vector(), self.initialize_block_vector())      # the state of u = 0: vmult is the linear operator until residual is called

    def initialize_block_vector(self):
        return self.mf_data.initialize_block_vector(3)

    def assemble_rhs(self):
        """the scalar load vector b_i = int phi_i (bp5_assemble_rhs): a body force f is b_c = f_c * assemble_rhs()"""
        return self.linear.assemble_rhs()

    def _args(self, *vectors):
        nc, ld = _block_args(self.mf_data, *vectors)
        if nc != 3:
            raise BP5Error(1, f"hyperelasticity: block vectors of three components expected, got {nc}")
        return ld

    def residual(self, r, u):
        """r = [0 +] F_int(u) on (3, ld) tensors, r_c = 0 on Dirichlet DoFs; stores the state of u (bp5_hyperelasticity_residual)."""
        r, u = _vals(r), _vals(u)
        ld = self._args(r, u)
        _lib.check(_lib.lib().bp5_hyperelasticity_residual(self.mf_data.handle, _ptr(self.coef), _ptr(self.state), self.lam, self.mu, ld, _ptr(u), _ptr(r),
                                                           1 if self.do_zero_out else 0))

    def vmult(self, dst, src):
        """dst = [0 +] T(state) src; dst_c = src_c on Dirichlet DoFs (bp5_hyperelasticity_apply)."""
        dst, src = _vals(dst), _vals(src)
        ld = self._args(dst, src)
        _lib.check(_lib.lib().bp5_hyperelasticity_apply(self.mf_data.handle, _ptr(self.coef), _ptr(self.state), self.lam, self.mu, ld, _ptr(src), _ptr(dst),
                                                        1 if self.do_zero_out else 0))

    def cell_loop(self, src, dst, cell_begin=0, cell_end=None):
        """dst += T(state) src over the cells [cell_begin, cell_end), no Dirichlet copy (bp5_hyperelasticity_apply_cells)."""
        ld = self._args(dst, src)
        cell_end = self.n_owned_cells if cell_end is None else cell_end
        _lib.check(_lib.lib().bp5_hyperelasticity_apply_cells(self.mf_data.handle, _ptr(self.coef), _ptr(self.state), self.lam, self.mu, ld, _ptr(src), _ptr(dst),
                                                              cell_begin, cell_end))


def _refuse_elasticity(who, A):
    if isinstance(A, (ElasticityOperator, HyperelasticityOperator)):
        raise BP5Error(5, f"{who} does not take the elasticity operator: SolverCG with None / DiagonalMatrix does")


class Vector:
    """The part of LinearAlgebra::distributed::Vector<double, MemorySpace::CUDA> the reference's path uses
    (bp5/solver.h:369-382,417-421,511,528; bp5/step-64.cu:349,366-367,431-432,445,449,467), over a torch CUDA
    tensor (owned entries, then ghosts) and the library's BLAS-1 / halo entry points.  Solvers and operators
    accept either this class or the bare tensor (`.values`)."""

    def __init__(self, mf=None):
        self.mf, self.values = mf, None
        if mf is not None:
            self.reinit(mf)

    def reinit(self, other, omit_zeroing_entries=False):
        """reinit(MatrixFree) == initialize_dof_vector; reinit(Vector) == same layout as `other`."""
        mf = other.mf if isinstance(other, Vector) else other
        if self.values is None or self.mf is not mf:
            self.mf = mf
            self.values = mf.initialize_dof_vector()
        elif not omit_zeroing_entries:
            self.assign(0.0)
        return self

    def assign(self, s):
        """== operator=(scalar)"""
        _lib.check(_lib.lib().bp5_vec_fill(self.mf.handle, _ptr(self.values), float(s), self.mf.n_local))
        return self

    def all_zero(self):
        z = C.c_int()
        _lib.check(_lib.lib().bp5_vec_all_zero(self.mf.handle, _ptr(self.values), self.local_size(), C.byref(z)))
        return bool(z.value)

    def add(self, a, v):
        _lib.check(_lib.lib().bp5_vec_axpy(self.mf.handle, _ptr(self.values), float(a), _ptr(v.values), self.local_size()))

    def equ(self, a, v):
        _lib.check(_lib.lib().bp5_vec_equ(self.mf.handle, _ptr(self.values), float(a), _ptr(v.values), self.local_size()))

    def sadd(self, s, a, v):
        _lib.check(_lib.lib().bp5_vec_sadd(self.mf.handle, _ptr(self.values), float(s), float(a), _ptr(v.values), self.local_size()))

    def l2_norm(self):
        r = C.c_double()
        _lib.check(_lib.lib().bp5_vec_l2_norm(self.mf.handle, _ptr(self.values), self.local_size(), C.byref(r)))
        return r.value

    def get_values(self):
        return self.values

    def local_size(self):
        return self.mf.mesh.n_owned

    def size(self):
        return int(self.mf.mesh.n_global_dofs)

    def import_(self, host_values):
        """== import(ReadWriteVector, VectorOperation::insert): host values of the owned range."""
        torch = _torch()
        h = torch.as_tensor(host_values, dtype=torch.float64)
        if h.numel() != self.local_size():
            raise BP5Error(1, "import: need the owned range")
        self.values[:self.local_size()].copy_(h)

    def update_ghost_values(self):
        _lib.check(_lib.lib().bp5_halo_gather(self.mf.handle, _ptr(self.values)))

    def update_ghost_values_start(self):
        _lib.check(_lib.lib().bp5_halo_gather_start(self.mf.handle, _ptr(self.values)))

    def update_ghost_values_finish(self):
        _lib.check(_lib.lib().bp5_halo_gather_finish(self.mf.handle, _ptr(self.values)))

    def compress_start(self):
        """== compress_start(VectorOperation::add)"""
        _lib.check(_lib.lib().bp5_halo_scatter_add_start(self.mf.handle, _ptr(self.values)))

    def compress_finish(self):
        _lib.check(_lib.lib().bp5_halo_scatter_add_finish(self.mf.handle, _ptr(self.values)))

    def compress_add(self):
        """== compress(VectorOperation::add)"""
        _lib.check(_lib.lib().bp5_halo_scatter_add(self.mf.handle, _ptr(self.values)))

    def zero_out_ghosts(self):
        _lib.check(_lib.lib().bp5_halo_zero_ghosts(self.mf.handle, _ptr(self.values)))


def _vals(v):
    return v.values if isinstance(v, Vector) else v


def _is_block(t):
    """a block vector: a 2-D tensor (n_components, ld)"""
    return getattr(t, "dim", None) is not None and t.dim() == 2


def _refuse_blocks(who, *vectors):
    if any(_is_block(_vals(v)) for v in vectors):
        raise BP5Error(5, f"{who} does not take block vectors (2-D tensors): PoissonOperator.vmult and SolverCG with a DiagonalMatrix do")


def _block_args(mf, *vectors):
    """(n_components, ld) of block vectors of one shape, checked against the handle's layout"""
    shapes = {tuple(v.shape) for v in vectors}
    if len(shapes) != 1 or not all(_is_block(v) for v in vectors):
        raise BP5Error(1, f"block vectors of one shape (n_components, ld) expected, got {sorted(tuple(v.shape) for v in vectors)}")
    nc, ld = vectors[0].shape
    if ld < mf.n_local:
        raise BP5Error(1, f"block vector has ld = {ld}, need at least n_local = {mf.n_local}")
    return int(nc), int(ld)


class DiagonalMatrix:
    """== DiagonalMatrix<Vector>; `None` vector == identity (the reference sets it to 1,
    bp5/step-64.cu:432, and still streams it; here identity costs no bytes)."""

    def __init__(self, vector=None):
        self._v = vector

    def get_vector(self):
        return self._v


class SolverControl:
    def __init__(self, max_steps=100, tolerance=1e-10):
        self.max_steps, self.tolerance = int(max_steps), float(tolerance)
        self._last_step, self._last_value, self._initial_value = 0, float("nan"), float("nan")
        self.solve_ms = self.apply_ms_avg = self.operator_ms_avg = 0.0
        self.apply_launches = 0
        self.dot_products_fused = False
        self.exchange_schedule, self.apply_kernel, self.phase_ms = 0, "", [0.0] * 8

    def last_step(self):
        return self._last_step

    def last_value(self):
        return self._last_value

    def initial_value(self):
        return self._initial_value


class IterationNumberControl(SolverControl):
    """Stops at max_steps or when the residual drops below tolerance, reports success either way
    (bp5/step-64.cu:443-445)."""


class _DeviceArray:
    """__cuda_array_interface__ carrier: lets torch alias device memory the library owns (the solvers' work vectors)."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}


def _callback(obj, mf, failure):
    """bp5_vmult_fn that runs obj.vmult(dst, src) on torch views of the library's device vectors (owned + ghost length).  It enqueues
    on the current stream; no exception may cross the C boundary: it is kept in `failure` and status 1 is returned."""
    torch = _torch()

    def view(p):
        return torch.as_tensor(_DeviceArray(p, mf.n_local), device=f"cuda:{mf.device}")

    def callback(_ctx, dst, src):
        try:
            obj.vmult(view(dst), view(src))
            return 0
        except Exception as e:         # noqa: BLE001
            failure.append(e)
            return 1

    return _lib.VMULT_FN(callback)


def _even_ld(mf):
    return mf.n_local + (mf.n_local & 1)


def _global_ids(mf):
    ids = getattr(mf.mesh, "global_ids", None)
    return np.ascontiguousarray(ids[:mf.n_owned], dtype=np.uint64) if ids is not None else None


class _NativePreconditioner:
    """A preconditioner that lives in the library: the handle, its end, and the (callback pointer, context) pair the C solvers take.
    Subclasses: _VMULT / _DESTROY (the C entries), _NO_HANDLE (what a missing handle means), _vectors (the vector shape they accept)."""

    _failure = ()                    # (exceptions of a Python operator callback: PreconditionChebyshev only)

    @property
    def handle(self):
        if not self._h:
            raise BP5Error(1, self._NO_HANDLE.format(type(self).__name__))
        return self._h

    def _native(self):
        return C.cast(getattr(_lib.lib(), self._VMULT), C.c_void_p), self.handle

    def _vectors(self, dst, src):
        """the pointers of scalar vectors (owned + ghost); block vectors are refused"""
        n = self.mf_data.n_local
        _refuse_blocks(type(self).__name__, dst, src)
        return _ptr(_vals(dst), n), _ptr(_vals(src), n)

    def _run(self, fn, dst, src):
        pdst, psrc = self._vectors(dst, src)
        status = fn(self.handle, pdst, psrc)
        if self._failure:
            raise self._failure.pop(0)
        _lib.check(status)

    def clear(self):
        if self._h:
            getattr(_lib.lib(), self._DESTROY)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.clear()
        except Exception:
            pass


def _elasticity_vectors(pre, op, dst, src):
    """_vectors of the elasticity preconditioners: (3, ld) tensors of the ld `pre` was initialised for"""
    dst, src = _vals(dst), _vals(src)
    if op._args(dst, src) != pre.ld:
        raise BP5Error(1, f"elasticity: the preconditioner was initialised for ld = {pre.ld}, the vectors have {dst.shape[1]}")
    return _ptr(dst), _ptr(src)


class _ChebyshevBase(_NativePreconditioner):
    _VMULT, _DESTROY, _NO_HANDLE = "bp5_chebyshev_vmult", "bp5_chebyshev_destroy", "{}.initialize has not been called"

    def __init__(self):
        self._h = None
        self._keep = []

    def _create(self, A, data, keep, create):
        """the end of initialize(): create(prm, h) is the subclass's C create call; `keep` lives as long as the handle"""
        mf = A.mf_data
        self.A, self.mf_data, self.data = A, mf, data
        ids = _global_ids(mf)
        prm = _lib.ChebyshevParams(data.degree, data.smoothing_range, data.eig_cg_n_iterations, data.max_eigenvalue, data.min_eigenvalue,
                                   ids.ctypes.data if ids is not None else None)
        h = C.c_void_p()
        status = create(prm, h)
        if self._failure:
            raise self._failure[0]
        _lib.check(status)
        self._h = h
        self._keep = keep
        return self

    def vmult(self, dst, src):
        """dst = P src (dst's prior content ignored; the elasticity class: on (3, ld) tensors); enqueued on the handle's stream."""
        self._run(_lib.lib().bp5_chebyshev_vmult, dst, src)

    def step(self, dst, src):
        """Smoother: dst improved from its current value by `degree` Chebyshev steps on A dst = src."""
        self._run(_lib.lib().bp5_chebyshev_step, dst, src)

    def estimated_eigenvalues(self):
        """dict(min_est, max_est, min_used, max_used, cg_its): the CG-Lanczos estimate and the bounds the polynomial uses."""
        v = [C.c_double() for _ in range(4)]
        k = C.c_int()
        _lib.check(_lib.lib().bp5_chebyshev_eigenvalues(self.handle, *[C.byref(x) for x in v], C.byref(k)))
        return dict(min_est=v[0].value, max_est=v[1].value, min_used=v[2].value, max_used=v[3].value, cg_its=k.value)

    def clear(self):
        super().clear()
        self._keep = []


class PreconditionChebyshev(_ChebyshevBase):
    """== PreconditionChebyshev<Operator, Vector, DiagonalMatrix> (deal.II): a Chebyshev polynomial of degree `degree` in D^-1 A on the
    eigenvalue bounds of D^-1 A, estimated at initialize() by a few CG-Lanczos steps (bp5_chebyshev_create, include/bp5.h).  vmult is
    degree-1 operator applications and degree pointwise step launches, with no dot product: only the operator's halo exchanges.

    A: a PoissonOperator / HelmholtzOperator (its coef, natively) or any object with `mf_data` and `vmult(dst, src)` (through a
    callback).  AdditionalData.preconditioner: a DiagonalMatrix holding the INVERSE diagonal (compute_diagonal(invert=True)), None = identity."""

    class AdditionalData:
        def __init__(self, degree=1, smoothing_range=0.0, eig_cg_n_iterations=8, max_eigenvalue=0.0, min_eigenvalue=0.0, preconditioner=None):
            self.degree, self.smoothing_range, self.eig_cg_n_iterations = int(degree), float(smoothing_range), int(eig_cg_n_iterations)
            self.max_eigenvalue, self.min_eigenvalue = float(max_eigenvalue), float(min_eigenvalue)
            self.preconditioner = preconditioner

    def initialize(self, A, data=None):
        self.clear()
        _refuse_elasticity(type(self).__name__, A)
        data = data if data is not None else PreconditionChebyshev.AdditionalData()
        mf = A.mf_data
        inv = _vals(data.preconditioner.get_vector()) if data.preconditioner is not None else None
        self._failure = []
        if isinstance(A, PoissonOperator):
            coef, cb = _ptr(A.coef), None
        else:
            coef, cb = None, _callback(A, mf, self._failure)
        return self._create(A, data, [inv, cb], lambda prm, h: _lib.lib().bp5_chebyshev_create(
            mf.handle, coef, C.cast(cb, C.c_void_p) if cb is not None else None, None, _ptr(inv, mf.n_owned) if inv is not None else None, C.byref(prm), C.byref(h)))


class MGTwoLevelTransfer:
    """== MGTwoLevelTransfer (deal.II matrix-free global-coarsening transfer) between two operators of degrees pf >= 2 and
    pc = max(1, pf // 2) on the same cells (bp5_mg_transfer_*, include/bp5.h); geometric=True: == reinit_geometric_transfer between two
    operators of one degree in 1..4 on a 2:1 pair of BrickMeshes (BrickMesh.coarsen), the parent map from BrickMesh.parent_cells
    (bp5_mg_transfer_create_geometric).  prolongate_and_add: dst_f += P src_c; restrict_and_add: dst_c += P^T src_f (Dirichlet rows of
    dst_c unchanged).  Vectors: owned + ghost storage of their operator."""

    def __init__(self, fine_op, coarse_op, geometric=False):
        self._h = None
        self.fine, self.coarse, self.geometric = fine_op, coarse_op, bool(geometric)
        h = C.c_void_p()
        if self.geometric:
            parent, child = fine_op.mf_data.mesh.parent_cells(coarse_op.mf_data.mesh)
            _lib.check(_lib.lib().bp5_mg_transfer_create_geometric(fine_op.mf_data.handle, coarse_op.mf_data.handle, parent.ctypes.data,
                                                                   child.ctypes.data, C.byref(h)))
        else:
            _lib.check(_lib.lib().bp5_mg_transfer_create(fine_op.mf_data.handle, coarse_op.mf_data.handle, C.byref(h)))
        self._h = h

    @property
    def handle(self):
        if not self._h:
            raise BP5Error(1, "MGTwoLevelTransfer has been cleared")
        return self._h

    def prolongate_and_add(self, dst, src):
        _lib.check(_lib.lib().bp5_mg_transfer_prolongate_add(self.handle, _ptr(_vals(dst), self.fine.mf_data.n_local),
                                                             _ptr(_vals(src), self.coarse.mf_data.n_local)))

    def restrict_and_add(self, dst, src):
        _lib.check(_lib.lib().bp5_mg_transfer_restrict_add(self.handle, _ptr(_vals(dst), self.coarse.mf_data.n_local),
                                                           _ptr(_vals(src), self.fine.mf_data.n_local)))

    def _components(self, fine_v, coarse_v):
        fine_v, coarse_v = _vals(fine_v), _vals(coarse_v)
        (ncf, ldf), (ncc, ldc) = _block_args(self.fine.mf_data, fine_v), _block_args(self.coarse.mf_data, coarse_v)
        if ncf != ncc:
            raise BP5Error(1, f"block vectors of one component count expected, got {ncf} (fine) and {ncc} (coarse)")
        return ncf, ldf, _ptr(fine_v), ldc, _ptr(coarse_v)

    def prolongate_and_add_components(self, dst, src):
        """dst_f += P src_c block by block on (n_components, ld) tensors, one launch (bp5_mg_transfer_prolongate_add_components)"""
        nc, ldf, pf, ldc, pc = self._components(dst, src)
        _lib.check(_lib.lib().bp5_mg_transfer_prolongate_add_components(self.handle, nc, ldf, pf, ldc, pc))

    def restrict_and_add_components(self, dst, src):
        """dst_c += P^T src_f block by block on (n_components, ld) tensors (bp5_mg_transfer_restrict_add_components)"""
        nc, ldf, pf, ldc, pc = self._components(src, dst)
        _lib.check(_lib.lib().bp5_mg_transfer_restrict_add_components(self.handle, nc, ldc, pc, ldf, pf))

    def clear(self):
        if self._h:
            _lib.lib().bp5_mg_transfer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.clear()
        except Exception:
            pass


def mg_coarse_degrees(degree):
    """The p-multigrid hierarchy p, p // 2, ..., 1 (fine to coarse)."""
    degrees = [int(degree)]
    while degrees[-1] > 1:
        degrees.append(max(1, degrees[-1] // 2))
    return degrees


def _check_h_levels(who, h_levels):
    if h_levels != "max" and (isinstance(h_levels, bool) or not isinstance(h_levels, int) or h_levels < 0):
        raise BP5Error(1, f"{who}: h_levels must be an int >= 0 or 'max', not {h_levels!r}")


def _mg_levels(top, h_levels, min_cells, level):
    """[top, ...]: below `top`, level(mesh) at the degrees p // 2, ..., 1 on top's cells, then up to h_levels times on the coarsened mesh of the one above"""
    from .mesh import BrickMesh
    m = top.mf_data.mesh
    ops = [top]
    for p in mg_coarse_degrees(m.degree)[1:]:
        ops.append(level(BrickMesh(p, m.cells, h=m.h, deform_amp=m.deform_amp, rank=m.rank, n_ranks=m.n_ranks, cell_block=m.cell_block,
                                   dof_numbering=m.dof_numbering, cell_block_order=m.cell_block_order)))
    n_h = 0
    while h_levels == "max" or n_h < h_levels:
        coarse = ops[-1].mf_data.mesh.coarsen(min_cells)
        if coarse is None:
            break
        ops.append(level(coarse))
        n_h += 1
    return ops


def make_mg_hierarchy(fine_op, h_levels=0, min_cells=4, metric_precision=None):
    """The operators of the multigrid levels below fine_op (a PoissonOperator on a BrickMesh): the same operator class, cells, block order
    and numbering scheme, coefficient, quadrature, geometry mode, device, stream and communicator at degrees p // 2, ..., 1; then, at
    degree 1, up to
    h_levels geometric levels (an int, or "max": as many as the mesh allows), each on BrickMesh.coarsen(min_cells) of the one above
    (half the cells per direction, twice h, the same domain), stopping where coarsen returns None.  h_levels = 0 (default): the p-levels
    only.  Returns [fine_op, ...].
    metric_precision = None (default): nothing changes -- the coarse levels are built with FP64 planes whatever fine_op's own planes are (a
    fine_op that is itself float32 gets FP64 levels below it; pass "float32" for an all-float hierarchy).  "float32": EVERY level operator keeps its metric planes as floats (deal.II's
    mixed-precision multigrid, step-37 / step-75, as far as the planes go: arithmetic and vectors stay double) -- level 0 included, which
    is then NOT fine_op but a new float32 twin of it on the same mesh object, quadrature, coefficient, stream and communicator.  The caller
    keeps fine_op as the outer CG's operator (the solution is then the FP64 solution) and passes the returned list to PreconditionMG."""
    _check_h_levels("make_mg_hierarchy", h_levels)
    mf = fine_op.mf_data
    stream = mf.stream                # the levels share fine_op's stream (bp5_mg_create refuses anything else), whatever torch's current one is

    geometry = dict(geometry=fine_op.geometry) if fine_op.geometry else {}     # (HelmholtzOperator: six-plane geometry only)
    if metric_precision is not None:
        if metric_precision not in MatrixFree.METRIC_PRECISION:
            raise BP5Error(1, f"make_mg_hierarchy: metric_precision must be None, 'float64' or 'float32', not {metric_precision!r}")
        if type(fine_op) is not PoissonOperator:
            raise BP5Error(5, "make_mg_hierarchy: metric_precision needs a PoissonOperator")
        geometry["metric_precision"] = metric_precision

    def level(mesh):
        return type(fine_op)(mesh, mf.quadrature, mf.coefficient, device=mf.device, comm=mf.comm, stream=stream, **geometry)

    top = fine_op if metric_precision in (None, getattr(fine_op, "metric_precision", "float64")) else level(mf.mesh)
    return _mg_levels(top, h_levels, min_cells, level)


class _MGBase(_NativePreconditioner):
    _VMULT, _DESTROY, _NO_HANDLE = "bp5_mg_vmult", "bp5_mg_destroy", "{} has been cleared"

    def _initialize(self, operators, data, ld=None):
        """initialize() of both classes: the checks, the transfers, the parameters; _level_arguments and _c_create are the subclass's"""
        name = type(self).__name__
        self.clear()
        data = data if data is not None else PreconditionMG.AdditionalData()
        ops = list(operators)
        self._check_operators(ops)
        # bp5_mg_create checks the handles themselves, but the transfers it takes are built first, and bp5_mg_transfer_create refuses such a
        # pair with words of its own: the same refusal here, in bp5_mg_create's words (from MatrixFree.stream, which set_stream keeps current)
        if len({o.mf_data.stream for o in ops}) > 1:
            raise BP5Error(1, f"{name}: the levels must share one stream (MatrixFree.set_stream moves each of them)")
        self._level_arguments(ops, ld)
        self.operators, self.data, self.mf_data = ops, data, ops[0].mf_data
        self.transfers = [MGTwoLevelTransfer(f, c, geometric=f.mf_data.mesh.degree == c.mf_data.mesh.degree) for f, c in zip(ops[:-1], ops[1:])]
        ids = [_global_ids(o.mf_data) for o in ops]
        id_ptrs = (C.c_void_p * len(ops))(*[a.ctypes.data if a is not None else None for a in ids])
        prm = _lib.MGParams(data.smoother_degree, data.smoothing_range, data.eig_cg_n_iterations, data.coarse_degree, data.coarse_range,
                            data.coarse_eig_cg_n_iterations, C.cast(id_ptrs, C.c_void_p))
        n = len(ops)
        mfs = (C.c_void_p * n)(*[o.mf_data.handle.value for o in ops])
        coefs = (C.c_void_p * n)(*[o.coef.data_ptr() if o.coef is not None else None for o in ops])
        trs = (C.c_void_p * max(n - 1, 1))(*[t.handle.value for t in self.transfers])
        h = C.c_void_p()
        _lib.check(self._c_create(n, mfs, coefs, trs, C.byref(prm), C.byref(h)))
        self._h = h
        return self

    def _check_operators(self, ops):
        if not ops or not all(isinstance(o, self._OPERATOR) for o in ops):
            raise BP5Error(1, f"{type(self).__name__} needs a list of {self._OPERATOR.__name__}s, fine to coarse")

    def _level_arguments(self, ops, ld):
        pass

    def vmult(self, dst, src):
        """dst = V src: one V-cycle (dst's prior content ignored; the elasticity class: on (3, ld) tensors); enqueued on the operators' stream."""
        self._run(_lib.lib().bp5_mg_vmult, dst, src)

    def level_info(self):
        """Per level, fine to coarse: dict(degree, cells, n_owned, n_global_dofs, min_est, max_est, min_used, max_used, cg_its,
        chebyshev_degree); cells: the level mesh's global cells per direction (None if its mesh does not say)."""
        out = []
        for lev, o in enumerate(self.operators):
            v = _lib.MGLevel()
            _lib.check(_lib.lib().bp5_mg_level_info(self.handle, lev, C.byref(v)))
            cells = getattr(o.mf_data.mesh, "cells", None)
            out.append(dict(degree=v.degree, cells=tuple(int(c) for c in cells) if cells is not None else None, n_owned=v.n_owned, n_global_dofs=int(o.mf_data.mesh.n_global_dofs), min_est=v.min_est,
                            max_est=v.max_est, min_used=v.min_used, max_used=v.max_used, cg_its=v.cg_its, chebyshev_degree=v.chebyshev_degree))
        return out

    def clear(self):
        super().clear()
        for t in self.transfers:
            t.clear()
        self.transfers = []


class PreconditionMG(_MGBase):
    """== PreconditionMG<dim, Vector, MGTransferMatrixFree> around Multigrid (V-cycle) with PreconditionChebyshev smoothers and a
    Chebyshev coarse solver (step-37), coarsening in the polynomial degree and then in the mesh (bp5_mg_*, include/bp5.h).  operators:
    PoissonOperators from fine to coarse, degrees p, max(1, p // 2), ..., 1 on the same cells, then optionally degree-1 levels on
    2:1 coarser BrickMeshes (make_mg_hierarchy builds them).  A pair of different degrees gets the p-transfer, a pair of equal degrees
    the geometric one.  vmult is one symmetric V-cycle,
    enqueued on the operators' stream without a host synchronisation; SolverCG.solve passes it natively (bp5_mg_vmult)."""

    _OPERATOR = PoissonOperator

    class AdditionalData:
        def __init__(self, smoother_degree=4, smoothing_range=20.0, eig_cg_n_iterations=10, coarse_degree=60, coarse_range=1000.0,
                     coarse_eig_cg_n_iterations=30):
            self.smoother_degree, self.smoothing_range, self.eig_cg_n_iterations = int(smoother_degree), float(smoothing_range), int(eig_cg_n_iterations)
            self.coarse_degree, self.coarse_range = int(coarse_degree), float(coarse_range)
            self.coarse_eig_cg_n_iterations = int(coarse_eig_cg_n_iterations)

    def __init__(self, operators, data=None):
        self._h = None
        self.transfers = []
        self.initialize(operators, data)

    def initialize(self, operators, data=None):
        return self._initialize(operators, data)

    def _check_operators(self, ops):
        for o in ops:
            _refuse_elasticity(type(self).__name__, o)
        super()._check_operators(ops)

    def _c_create(self, n, mfs, coefs, trs, prm, h):
        return _lib.lib().bp5_mg_create(n, mfs, coefs, trs, prm, h)


class ElasticityPreconditionChebyshev(_ChebyshevBase):
    """== PreconditionChebyshev<ElasticityOperator, BlockVector, DiagonalMatrix>: the Chebyshev polynomial of PreconditionChebyshev for an
    ElasticityOperator on (3, ld) tensors (bp5_elasticity_chebyshev_create, include/bp5.h).  AdditionalData: PreconditionChebyshev's, its
    preconditioner a DiagonalMatrix holding the BLOCK inverse diagonal (ElasticityOperator.compute_diagonal(invert=True)) or None = identity.
    ld: the row length of the vectors vmult / step will see -- default: the inverse diagonal's, else n_local rounded up to even (what
    initialize_block_vector gives).  SolverCG.solve(op, x, b, this) runs bp5_cg_solve_elasticity_preconditioned with bp5_chebyshev_vmult."""

    AdditionalData = PreconditionChebyshev.AdditionalData

    def initialize(self, A, data=None, ld=None):
        self.clear()
        if not isinstance(A, ElasticityOperator):
            raise BP5Error(1, f"{type(self).__name__} needs an ElasticityOperator (PreconditionChebyshev takes the scalar operators)")
        data = data if data is not None else PreconditionChebyshev.AdditionalData()
        mf = A.mf_data
        inv = _vals(data.preconditioner.get_vector()) if data.preconditioner is not None else None
        if inv is not None and not (_is_block(inv) and inv.shape[0] == 3):
            raise BP5Error(1, f"elasticity: the inverse diagonal is a block vector of shape (3, ld), got {tuple(inv.shape)}")
        self.ld = int(ld) if ld is not None else (int(inv.shape[1]) if inv is not None else _even_ld(mf))
        if inv is not None and int(inv.shape[1]) != self.ld:
            raise BP5Error(1, f"elasticity: the inverse diagonal has ld = {inv.shape[1]}, the preconditioner ld = {self.ld}")
        return self._create(A, data, [inv], lambda prm, h: _lib.lib().bp5_elasticity_chebyshev_create(
            mf.handle, _ptr(A.coef), A.lam, A.mu, self.ld, _ptr(inv), C.byref(prm), C.byref(h)))

    def _vectors(self, dst, src):
        return _elasticity_vectors(self, self.A, dst, src)


def make_elasticity_mg_hierarchy(fine_op, h_levels=0, min_cells=4):
    """The ElasticityOperators of the multigrid levels below fine_op (on a BrickMesh): the same lam, mu, quadrature, coefficient, device and
    stream at degrees p // 2, ..., 1 on the same cells, then at the last degree up to h_levels geometric levels (an int, or "max") on
    BrickMesh.coarsen(min_cells) of the one above -- make_mg_hierarchy's rule.  Returns [fine_op, ...] for ElasticityPreconditionMG."""
    if not isinstance(fine_op, ElasticityOperator):
        raise BP5Error(1, "make_elasticity_mg_hierarchy needs an ElasticityOperator")
    _check_h_levels("make_elasticity_mg_hierarchy", h_levels)
    mf = fine_op.mf_data

    def level(mesh):
        return ElasticityOperator(mesh, mf.quadrature, mf.coefficient, lam=fine_op.lam, mu=fine_op.mu, device=mf.device, stream=mf.stream)

    return _mg_levels(fine_op, h_levels, min_cells, level)


class ElasticityPreconditionMG(_MGBase):
    """== PreconditionMG<dim, BlockVector, MGTransferMatrixFree> for ElasticityOperators, fine to coarse (make_elasticity_mg_hierarchy builds
    them): PreconditionMG's V-cycle -- Chebyshev smoothers on the block inverse diagonals, the fused residual restriction, the scalar transfer
    handles on all three blocks, the coarse polynomial -- on (3, ld) tensors (bp5_elasticity_mg_create, include/bp5.h).  ld: the row length of
    the vectors vmult will see (default: n_local of the fine level rounded up to even).  SolverCG.solve(op, x, b, this) runs
    bp5_cg_solve_elasticity_preconditioned with bp5_mg_vmult."""

    _OPERATOR = ElasticityOperator
    AdditionalData = PreconditionMG.AdditionalData

    def __init__(self, operators, data=None, ld=None):
        self._h = None
        self.transfers = []
        self.initialize(operators, data, ld)

    def initialize(self, operators, data=None, ld=None):
        return self._initialize(operators, data, ld)

    def _level_arguments(self, ops, ld):
        if len({(o.lam, o.mu) for o in ops}) > 1:
            raise BP5Error(1, f"{type(self).__name__}: the levels must share lam and mu")
        self.ld = int(ld) if ld is not None else _even_ld(ops[0].mf_data)

    def _c_create(self, n, mfs, coefs, trs, prm, h):
        return _lib.lib().bp5_elasticity_mg_create(n, mfs, coefs, self.operators[0].lam, self.operators[0].mu, self.ld, trs, prm, h)

    def _vectors(self, dst, src):
        return _elasticity_vectors(self, self.operators[0], dst, src)


class _SolverBase:
    variant = CG_PLAIN

    def __init__(self, control, check_every=0, profile=False):
        self.control, self.check_every, self.profile = control, check_every, profile

    def solve(self, A, x, b, preconditioner=None):
        """== cg.solve(A, x, b, preconditioner), bp5/step-64.cu:450-453,492-495.  x0 = 0.
        A PoissonOperator runs entirely inside bp5_cg_solve; any other object with `mf_data` (vector layout, stream) and
        `vmult(dst, src)` is solved through bp5_cg_solve_operator -- the solvers need nothing of A but vmult
        (bp5/solver.h:25-30,377,475).  The preconditioner: None / DiagonalMatrix (the solvers' diag), a PreconditionChebyshev (native:
        bp5_cg_solve_preconditioned with bp5_chebyshev_vmult), a PreconditionMG (native: bp5_mg_vmult), or any other object with vmult(dst, src) (through a callback; SolverCG only).
        An ElasticityOperator: None / DiagonalMatrix (bp5_cg_solve_elasticity), or an ElasticityPreconditionChebyshev / ElasticityPreconditionMG
        (bp5_cg_solve_elasticity_preconditioned with their native vmult; SolverCG only); anything else is refused (BP5Error 5)."""
        mf = A.mf_data
        x, b = _vals(x), _vals(b)
        if isinstance(A, HyperelasticityOperator):
            return self._solve_hyperelasticity(A, x, b, preconditioner)
        general = preconditioner is not None and not hasattr(preconditioner, "get_vector")
        # the elasticity preconditioners (SolverCG): bp5_cg_solve_elasticity_preconditioned with their native vmult
        el_precond = (isinstance(A, ElasticityOperator) and self.variant == CG_PLAIN
                      and isinstance(preconditioner, (ElasticityPreconditionChebyshev, ElasticityPreconditionMG)))
        if isinstance(A, ElasticityOperator) and (self.variant != CG_PLAIN or general) and not el_precond:      # (one status for the class, whatever else is wrong)
            raise BP5Error(5, "elasticity: SolverCG with None / DiagonalMatrix only")
        if general and not hasattr(preconditioner, "vmult"):
            raise BP5Error(1, "the preconditioner needs get_vector() (diagonal) or vmult(dst, src)")
        if general and self.variant != CG_PLAIN:
            raise BP5Error(1, f"{type(self).__name__} takes a diagonal preconditioner only (None or DiagonalMatrix); use SolverCG")
        prm = _lib.CGParams(self.variant, self.control.max_steps, self.control.tolerance, self.check_every,
                            int(self.profile))   # False / True / 2 (phase stamps)
        res = _lib.CGResult()
        failure = []
        native = isinstance(A, PoissonOperator)
        if el_precond:
            ld = A._args(x, b)
            if ld != preconditioner.ld:
                raise BP5Error(1, f"elasticity: the preconditioner was initialised for ld = {preconditioner.ld}, the vectors have {ld}")
            status = _lib.lib().bp5_cg_solve_elasticity_preconditioned(mf.handle, _ptr(A.coef), A.lam, A.mu, ld, *preconditioner._native(), _ptr(b), _ptr(x),
                                                                       C.byref(prm), C.byref(res))
        elif isinstance(A, ElasticityOperator):
            # the coupled three-component system: ONE Krylov space, a BLOCK inverse diagonal (bp5_cg_solve_elasticity)
            ld = A._args(x, b)
            diag = _vals(preconditioner.get_vector()) if preconditioner is not None else None
            if diag is not None and tuple(diag.shape) != tuple(x.shape):
                raise BP5Error(1, f"elasticity: the inverse diagonal is a block vector of shape {tuple(x.shape)}, got {tuple(diag.shape)}")
            status = _lib.lib().bp5_cg_solve_elasticity(mf.handle, _ptr(A.coef), A.lam, A.mu, ld, _ptr(diag) if diag is not None else None, _ptr(b), _ptr(x),
                                                        C.byref(prm), C.byref(res))
        elif _is_block(x) or _is_block(b):
            # the stacked system diag(A, ..., A) x = b: ONE Krylov space for all components (bp5_cg_solve_components[_distributed])
            if self.variant != CG_PLAIN or general or not native:
                raise BP5Error(5, "block vectors (2-D tensors): SolverCG on a PoissonOperator with None / DiagonalMatrix only")
            nc, ld = _block_args(mf, x, b)
            diag = _vals(preconditioner.get_vector()) if preconditioner is not None else None
            fn = _lib.lib().bp5_cg_solve_components_distributed if A.distributed else _lib.lib().bp5_cg_solve_components
            status = fn(mf.handle, _ptr(A.coef), nc, ld, _ptr(diag, mf.n_owned) if diag is not None else None, _ptr(b), _ptr(x), C.byref(prm), C.byref(res))
        elif general:
            if isinstance(preconditioner, (PreconditionChebyshev, PreconditionMG)):
                pfn, pctx = preconditioner._native()
            else:
                pcb = _callback(preconditioner, mf, failure)
                pfn, pctx = C.cast(pcb, C.c_void_p), None
            acb = None if native else _callback(A, mf, failure)
            status = _lib.lib().bp5_cg_solve_preconditioned(mf.handle, _ptr(A.coef) if native else None,
                                                            C.cast(acb, C.c_void_p) if acb is not None else None, None, pfn, pctx,
                                                            _ptr(b, mf.n_local), _ptr(x, mf.n_local), C.byref(prm), C.byref(res))
            if isinstance(preconditioner, PreconditionChebyshev) and preconditioner._failure:
                failure.append(preconditioner._failure.pop(0))
        else:
            diag = _vals(preconditioner.get_vector()) if preconditioner is not None else None
            dptr = _ptr(diag, mf.n_owned) if diag is not None else None
            if native:
                status = _lib.lib().bp5_cg_solve(mf.handle, _ptr(A.coef), dptr, _ptr(b, mf.n_local), _ptr(x, mf.n_local), C.byref(prm), C.byref(res))
            else:
                cb = _callback(A, mf, failure)
                status = _lib.lib().bp5_cg_solve_operator(mf.handle, cb, None, dptr, _ptr(b, mf.n_local), _ptr(x, mf.n_local), C.byref(prm), C.byref(res))
        if failure:
            raise failure[0]
        return self._finish(res, status)

    def _solve_hyperelasticity(self, A, x, b, preconditioner):
        """the tangent at A's stored state (bp5_cg_solve_hyperelasticity): None, or an elasticity preconditioner of A.linear with its native vmult"""
        ld = A._args(x, b)
        pfn, pctx = _elasticity_precond(preconditioner, ld)
        prm = _lib.CGParams(self.variant, self.control.max_steps, self.control.tolerance, self.check_every, int(self.profile))
        res = _lib.CGResult()
        status = _lib.lib().bp5_cg_solve_hyperelasticity(A.mf_data.handle, _ptr(A.coef), _ptr(A.state), A.lam, A.mu, ld, pfn, pctx, _ptr(b), _ptr(x), C.byref(prm),
                                                         C.byref(res))
        return self._finish(res, status)

    def _finish(self, res, status):
        c = self.control
        c._last_step, c._last_value, c._initial_value = res.iterations, res.residual, res.initial_residual
        c.solve_ms, c.apply_ms_avg, c.apply_launches = res.solve_ms, res.apply_ms_avg, res.apply_launches
        c.operator_ms_avg = res.operator_ms_avg
        c.dot_products_fused = bool(res.dot_products_fused)
        c.exchange_schedule, c.apply_kernel, c.phase_ms = res.exchange_schedule, res.apply_kernel.decode(), list(res.phase_ms)
        _lib.check(status)
        return res


class SolverCG(_SolverBase):
    variant = CG_PLAIN


def _elasticity_precond(preconditioner, ld):
    """(callback, context) of the preconditioners the hyperelastic solves take: None (identity), ElasticityPreconditionChebyshev, ElasticityPreconditionMG"""
    if preconditioner is None:
        return None, None
    if not isinstance(preconditioner, (ElasticityPreconditionChebyshev, ElasticityPreconditionMG)):
        raise BP5Error(5, "hyperelasticity: the preconditioner is None, an ElasticityPreconditionChebyshev or an ElasticityPreconditionMG (of op.linear)")
    if ld != preconditioner.ld:
        raise BP5Error(1, f"hyperelasticity: the preconditioner was initialised for ld = {preconditioner.ld}, the vectors have {ld}")
    return preconditioner._native()


class NewtonSolver:
    """Newton's method with backtracking on F_int(u) = f_ext for a HyperelasticityOperator (bp5_hyperelasticity_newton, include/bp5.h).
    control: SolverControl(max Newton steps, absolute tolerance on ||r||); cg_control: SolverControl(max CG iterations per step, unused tolerance --
    every tangent solve runs to cg_rel_tol ||r||).  After solve: newton_iterations, total_cg_iterations, backtracks, residual_history."""

    def __init__(self, control, cg_control, rel_tol=1e-10, cg_rel_tol=1e-12, max_backtracks=8, check_every=0):
        self.control, self.cg_control = control, cg_control
        self.rel_tol, self.cg_rel_tol, self.max_backtracks, self.check_every = rel_tol, cg_rel_tol, max_backtracks, check_every
        self.newton_iterations = self.total_cg_iterations = self.backtracks = 0
        self.residual_history = []

    def solve(self, op, u, f_ext, preconditioner=None):
        """u: the start vector (its Dirichlet values are the prescribed displacement) -> the solution.  Raises BP5Error 7 (no convergence) or
        6 (backtracking exhausted); the counters and the history are set either way."""
        if not isinstance(op, HyperelasticityOperator):
            raise BP5Error(1, "NewtonSolver needs a HyperelasticityOperator")
        u, f_ext = _vals(u), _vals(f_ext)
        ld = op._args(u, f_ext)
        pfn, pctx = _elasticity_precond(preconditioner, ld)
        cg = _lib.CGParams(CG_PLAIN, self.cg_control.max_steps, 0.0, self.check_every, 0)
        prm = _lib.NewtonParams(self.control.max_steps, self.control.tolerance, self.rel_tol, cg, self.cg_rel_tol, self.max_backtracks)
        res = _lib.NewtonResult()
        status = _lib.lib().bp5_hyperelasticity_newton(op.mf_data.handle, _ptr(op.coef), _ptr(op.state), op.lam, op.mu, ld, pfn, pctx, _ptr(f_ext), _ptr(u),
                                                       C.byref(prm), C.byref(res))
        self.newton_iterations, self.total_cg_iterations, self.backtracks = res.newton_iterations, res.total_cg_iterations, res.backtracks
        self.residual_history = list(res.residual_history[:min(res.newton_iterations + 1, 32)])
        self.control._last_step, self.control._last_value = res.newton_iterations, self.residual_history[-1] if self.residual_history else 0.0
        _lib.check(status)
        return res


class SolverCGFullMerge(_SolverBase):
    variant = CG_MERGED
