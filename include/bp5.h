/* bp5.h -- C ABI of the MI355X-native BP5 matrix-free operator + CG hot path.
 *
 * This is the drop-in boundary: every entry point below replaces one piece of the reference's
 * (peterrum/deal-and-ceed-on-gpu) hot path, cited as file:line under the reference root.  The
 * reference has no FFI of its own (it is C++ calling deal.II templates); a maintainer binds
 * these symbols from the C++ host code as shown in INTEGRATION.md, or uses the header-only
 * facade include/bp5_dealii_facade.hpp which re-creates the deal.II class names on top of them.
 *
 * Conventions
 *   - every function returns an int status (BP5_OK == 0); no exception crosses the boundary
 *     (the reference throws: AssertThrow/AssertCuda, bp5/solver.h:396-397,539-540);
 *   - pointers are DEVICE pointers unless the parameter name ends in `_host`;
 *   - handles are opaque, one per device; calls on one handle are not thread-safe;
 *   - all device work is enqueued on the handle's stream (bp5_mf_set_stream) and is
 *     asynchronous unless stated otherwise; nothing allocates inside the hot loop; the only other
 *     stream the library uses is the handle's own communication stream (RCCL halo traffic that
 *     overlaps compute), ordered against the handle's stream by events in both directions;
 *   - FP64 arithmetic, 32-bit DoF indices (types::global_dof_index, bp5/fe_evaluation_gl.h:84);
 *   - vectors are plain arrays of n_owned + n_ghost doubles, owned range first
 *     (LinearAlgebra::distributed::Vector<double, MemorySpace::CUDA>, bp5/step-64.cu:321-323).
 */
#ifndef BP5_H
#define BP5_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------ */
/* status codes                                                                                */
enum {
  BP5_OK = 0,
  BP5_ERR_INVALID = 1,        /* bad argument / unsupported degree                             */
  BP5_ERR_HIP = 2,            /* a HIP runtime call failed (AssertCuda, bp5/solver.h:396-397)  */
  BP5_ERR_NO_DEVICE = 3,      /* no gfx950 device visible: there is NO CPU fallback            */
  BP5_ERR_RCCL = 4,           /* an RCCL call failed                                           */
  BP5_ERR_UNSUPPORTED = 5,    /* e.g. a cell block that does not fit in LDS for a forced variant */
  BP5_ERR_BREAKDOWN = 6,      /* CG breakdown: p.Ap == 0 or NaN (ExcDivideByZero, solver.h:501)*/
  BP5_ERR_NO_CONVERGENCE = 7  /* SolverControl::NoConvergence, bp5/solver.h:539-540            */
};
const char *bp5_strerror(int status);
const char *bp5_last_error(void); /* detail of the last failure on this thread */

enum { BP5_QUAD_GAUSS = 0, /* QGauss<1>(p+1), bp5/step-64.cu:246 (reference default) */
       BP5_QUAD_GLL = 1,   /* QGaussLobatto<1>(p+1), bp5/step-64.cu:244 (COLLOCATION) */
       BP5_QUAD_GAUSS_OVER = 2 /* QGauss<1>(p+2): CEED BP1 - BP4; the n_q_points_1d = p + 2 of FEEvaluationGL<dim, p, n_q_points_1d, n_components>,
                                  bp5/fe_evaluation_gl.h:28.  See "over-integration" at bp5_mf_create */ };

enum { BP5_COEF_ONE = 0,   /* kappa == 1: the reference folds only JxW, bp5/step-64.cu:107-113 */
       BP5_COEF_STEP64 = 1 /* kappa = 10/(0.05+2|x|^2), step-64/step-64.cu:117 */ };

#define BP5_MAX_DEGREE 8

/* ------------------------------------------------------------------------------------------ */
/* host-only helpers (run without a GPU)                                                       */

/* Quadrature points per direction: Q = degree + 1 for BP5_QUAD_GAUSS and BP5_QUAD_GLL, degree + 2 for BP5_QUAD_GAUSS_OVER.
 * BP5_ERR_INVALID for a degree outside 1..BP5_MAX_DEGREE or an unknown quadrature id. */
int bp5_quadrature_points_1d(int degree, int quadrature, int *n_q);

/* 1-D data of FE_Q(degree) on GLL nodes with the chosen quadrature, all on [0,1]:
 * nodes[n], pts[Q], w[Q], N[q*n+i] = phi_i(x_q), D[q*n+i] = phi_i'(x_q), n = degree+1, q < Q = bp5_quadrature_points_1d
 * (Q == n but for BP5_QUAD_GAUSS_OVER, whose tables are rectangular: (n + 1) x n entries each).  Bitwise (anti)symmetric under
 * x -> 1 - x: N[q][i] == N[Q-1-q][n-1-i], D[q][i] == -D[Q-1-q][n-1-i].
 * Replaces the shape_values/shape_gradients tables MatrixFree::reinit builds
 * (call site bp5/step-64.cu:243-248). */
int bp5_shape_tables(int degree, int quadrature, double *nodes_host, double *pts_host, double *w_host,
                     double *N_host, double *D_host);

/* Structured hex-mesh generator standing in for GridGenerator::subdivided_hyper_rectangle +
 * refine_global + DoFHandler::distribute_dofs + zero Dirichlet constraints
 * (bp5/step-64.cu:341-358, 629-663); slab partition along z replaces the p4est partition. */
typedef struct bp5_mesh bp5_mesh;
typedef struct {
  int degree;          /* p */
  uint32_t cells[3];   /* global number of cells per direction */
  double h;            /* cell side (reference: 2^-refine) */
  double deform_amp;   /* 0 = cubes; >0 = smooth boundary-preserving sine displacement */
  int rank, n_ranks;   /* z-slab decomposition; interface planes owned by the lower rank */
  uint32_t cell_block[3]; /* cells are emitted block by block (bx x by x bz cells, x fastest inside a
                             block) so that consecutive cells form compact bricks; 0 = plain
                             lexicographic order */
  int dof_numbering;   /* 0: lexicographic I + NX (J + NY K) over the owned range;
                          1: block-major (needs cell_block): the DoFs strictly inside a cell block are
                             numbered contiguously, then block faces, edges, vertices -- every entity
                             contiguous.  A brick's gather/scatter then touches a few long runs instead
                             of many short rows.  global_ids_host always gives the lexicographic id.
                          2: the owned DoFs strictly INSIDE a cell first, cell after cell in the order the cells are handed over
                             ((p-1)^3 consecutive DoFs per cell, x fastest), then all other owned DoFs as in 0 (as in 1 where
                             cell_block is given).  bp5_mf_create recognises this property of a mesh (whoever numbered it) and the
                             pencil kernel of p >= 5 then stores cell-interior entries plainly instead of adding them atomically:
                             they share no cache line with an atomically updated DoF (half the atomics at p = 8). */
  int cell_block_order; /* order of the cells inside a block: 0 lexicographic (x fastest); 1 parity class by
                             parity class ((x&1, y&1, z&1) relative to the block corner, lexicographic inside a
                             class): consecutive cells then share no DoF, which is the order the block-assembled
                             kernel walks them in (its passes read consecutive cells) and spreads the atomics of
                             the pencil kernel */
} bp5_mesh_desc;

typedef struct {
  int degree;
  uint32_t n_cells;           /* locally owned cells                                            */
  uint32_t n_interior_cells;  /* cells [0,n_interior_cells) touch no ghost DoF                  */
  uint32_t n_owned, n_ghost;  /* local DoFs: owned first, then ghosts                           */
  uint64_t n_global_dofs;
  uint32_t global_dofs_per_dir[3];
  const uint32_t *local_to_global_host; /* [n_cells*(p+1)^3], local indices, i + n(j + n k)     */
  const double *node_coords_host;       /* [n_owned+n_ghost][3]                                 */
  const uint64_t *global_ids_host;      /* [n_owned+n_ghost] lexicographic global DoF id        */
  const uint32_t *constrained_host;     /* local indices of Dirichlet DoFs (owned + ghost)      */
  uint32_t n_constrained;
  /* halo plan (Utilities::MPI::Partitioner): per neighbour, owned indices to send for the
   * ghost gather, and the contiguous ghost range received from it */
  int n_neighbors;
  const int *neighbor_rank_host;        /* [n_neighbors]                                        */
  const uint32_t *send_offsets_host;    /* [n_neighbors+1] into send_indices                    */
  const uint32_t *send_indices_host;    /* owned local indices                                  */
  const uint32_t *recv_offsets_host;    /* [n_neighbors+1] offsets into the ghost range         */
  uint32_t n_cell_blocks;               /* cell blocks: block b = cells [off[b], off[b+1])       */
  const uint32_t *cell_block_offsets_host; /* [n_cell_blocks+1]                                  */
} bp5_mesh_view;

int bp5_mesh_create_brick(const bp5_mesh_desc *desc, bp5_mesh **out);
int bp5_mesh_view_get(const bp5_mesh *mesh, bp5_mesh_view *out);
void bp5_mesh_destroy(bp5_mesh *mesh);

/* Parent map of a 2:1 pair of brick meshes (the geometric multigrid transfer, bp5_mg_transfer_create_geometric): for every locally
 * owned cell k of `fine`, in handle order, parent_cell_host[k] = the local index of the coarse cell that contains it and
 * child_host[k] = its position in that parent, cx | cy << 1 | cz << 2 (cx = 1: the upper half in x).  Correct for every cell order the
 * generator emits (lexicographic, bricks, class-major, the ghost-touching layer last on ranks > 0).  The pair must have the same
 * degree, deform_amp, rank and n_ranks, fine cells = 2 x coarse cells in every direction and fine h = coarse h / 2, and the coarse
 * z-slab split must hold the parents of every rank's fine cells: floor(n2 r / R) == 2 floor((n2 / 2) r / R) for all r (n2 = fine
 * layers, R = n_ranks; e.g. 120 layers on 8 ranks fail: there is no repartitioning).  Otherwise BP5_ERR_INVALID with the reason in
 * bp5_last_error.  Host only (no GPU).  parent_cell_host, child_host: [fine n_cells]. */
int bp5_mesh_parent_cells(const bp5_mesh *fine, const bp5_mesh *coarse, uint32_t *parent_cell_host, uint8_t *child_host);

/* ------------------------------------------------------------------------------------------ */
/* device + vectors                                                                            */
int bp5_device_count(int *count);
int bp5_vec_alloc(size_t n, double **out);            /* hipMalloc, zero-filled                 */
int bp5_vec_free(double *v);
int bp5_copy_h2d(void *dst, const void *src_host, size_t bytes);   /* synchronous               */
int bp5_copy_d2h(void *dst_host, const void *src, size_t bytes);   /* synchronous               */

/* ------------------------------------------------------------------------------------------ */
/* matrix-free engine: CUDAWrappers::MatrixFree<3,double> as the reference uses it             */
typedef struct bp5_mf bp5_mf;

typedef struct {
  int dim;                 /* must be 3                                                         */
  int degree;              /* 1..BP5_MAX_DEGREE                                                 */
  int quadrature;          /* BP5_QUAD_*                                                        */
  int coefficient;         /* BP5_COEF_*                                                        */
  uint32_t n_cells, n_interior_cells, n_owned, n_ghost;
  const uint32_t *local_to_global_host;
  const double *node_coords_host;       /* MappingQGeneric(degree) through the FE_Q nodes,
                                           bp5/step-64.cu:234                                   */
  const uint32_t *constrained_host;
  uint32_t n_constrained;
  int n_neighbors;
  const int *neighbor_rank_host;
  const uint32_t *send_offsets_host, *send_indices_host, *recv_offsets_host;
  int device;              /* HIP device ordinal                                                */
  void *stream;            /* hipStream_t; NULL = the HIP default (null) stream                 */
  /* optional: groups of consecutive cells that one workgroup assembles in LDS (compact bricks give
   * the fewest DoFs shared between groups); NULL = the library groups 64 consecutive cells      */
  uint32_t n_cell_blocks;
  const uint32_t *cell_block_offsets_host; /* [n_cell_blocks+1], first 0, last n_cells           */
  /* optional: hanging-node constraints of 2:1 refined meshes, one mask per cell (BP5_HANG_* below); NULL = conforming mesh.
   * == MatrixFree::Data::constraint_mask as consumed by resolve_hanging_nodes, bp5/fe_evaluation_gl.h:150-151,167-168 */
  const uint32_t *constraint_mask_host;   /* [n_cells]                                          */
} bp5_mf_desc;

/* constraint_mask bits of a fine cell that touches coarser cells ("hanging" faces / edges of 2:1 refined meshes):
 *   BP5_HANG_FACE_d   the face normal to direction d lies on a coarser neighbour (any subset: cells on the rim of a refined
 *                     region have one, at its edges two, at its corners three);
 *   BP5_HANG_EDGE_d   the edge along d lies on a coarser cell's edge although neither face through it is constrained
 *                     (re-entrant corners of the refined region);
 *   BP5_HANG_SIDE_e   position of the cell in its parent along e (0 / 1): constrained faces normal to e sit at xi_e = that side,
 *                     a constrained edge along d at the corner (SIDE_e1, SIDE_e2) of the two other directions;
 *   BP5_HANG_HALF_d   the same position, as selector of the interpolation ALONG d: the cell covers the upper half [1/2, 1] of
 *                     the coarse face / edge (else the lower half).  (A cell with one constrained face may name only the SIDE
 *                     of the normal and the HALF of the two tangential directions; where both are used they must agree.)
 * local_to_global of the (p+1)^2 entries ON a constrained face names the COARSE face's DoFs in the same orientation, the p+1
 * entries on a constrained edge the coarse edge's.  Gathers (read_dof_values, and the node coordinates of the geometry) apply,
 * per direction d, the 1-D matrix I_h[a][b] = phi_b(xi_a / 2 + h / 2), h = HALF_d, to every cell-local line along d that lies on
 * a constrained face tangential to d or on the constrained edge along d; scatters (distribute_local_to_global, RHS
 * assembly) apply the adjoint.  (deal.II's own bit layout is not part of the reference repository; this one is the library's.) */
enum { BP5_HANG_FACE_X = 1, BP5_HANG_FACE_Y = 2, BP5_HANG_FACE_Z = 4,
       BP5_HANG_SIDE_X = 8, BP5_HANG_SIDE_Y = 16, BP5_HANG_SIDE_Z = 32,
       BP5_HANG_HALF_X = 64, BP5_HANG_HALF_Y = 128, BP5_HANG_HALF_Z = 256,
       BP5_HANG_EDGE_X = 512, BP5_HANG_EDGE_Y = 1024, BP5_HANG_EDGE_Z = 2048 };

/* == MatrixFree::reinit(mapping, dof_handler, constraints, quad, additional_data),
 *    bp5/step-64.cu:234-248.  Uploads the flat arrays; computes nothing yet.
 *
 * Over-integration, desc->quadrature == BP5_QUAD_GAUSS_OVER: Q = p + 2 Gauss points per direction on n = p + 1 nodes (CEED BP1 - BP4; deal.II's
 * FEEvaluation<dim, p, n_q_points_1d = p + 2>, the ordinary way to over-integrate a deformed geometry or a variable coefficient).  On affine cells
 * with a constant coefficient the operator equals the Gauss(p+1) one to rounding; on deformed cells or with BP5_COEF_STEP64 it does not.
 *   operators       BP5_OP_POISSON (CEED BP3) and BP5_OP_MASS (bp5_mf_set_operator; CEED BP1), as kernels of their own: apply_pencil_q_kernel and
 *                   apply_pencil_mass_q_kernel, Q^2 lanes per cell, rectangular Q x n contractions, atomic scatter (not bitwise reproducible);
 *                   bp5_mf_get_apply_variant reports 0, the pencil kernel, on every mesh -- also on cell bricks where a p + 1 handle resolves to 56;
 *   metric array    bp5_mf_coef_size = planes * n_cells * Q^3 doubles (6 planes, or 1 for the mass operator), each plane in the pair layout of
 *                   bp5_mf_compute_merged_metric TAKEN AT Q: coef[c*n_cells*Q^3 + cell*Q^3 + off_Q(qi, qj + Q*qk)], off_Q the formula there with Q for n
 *                   (lane ab = qj + Q qk owns the x-pencil qi = 0 .. Q-1); bp5_mf_metric_to_reference_layout returns [c][cell][qi + Q (qj + Q qk)];
 *   entry points    everything that is operator-agnostic works with the same dst contracts: bp5_mf_compute_merged_metric, bp5_apply (zero_dst 0 / 1),
 *                   bp5_apply_cells (accumulates, ragged ranges), bp5_apply_distributed (the atomic kernels' unsplit and three-phase schedules),
 *                   bp5_copy_constrained, bp5_compute_diagonal (also inverted), bp5_cg_solve in both variants (separate dot-product kernels:
 *                   bp5_cg_result.dot_products_fused is 0), bp5_cg_solve_operator, bp5_cg_solve_preconditioned, bp5_chebyshev_*; n_constrained == 0 is
 *                   fine (BP1 has no boundary condition).  bp5_assemble_rhs and bp5_l2_norm_solution keep their own Gauss(p+1) tables: their definition;
 *   refusals        BP5_ERR_UNSUPPORTED, decided before any launch and in either call order, bp5_last_error names the "quadrature": BP5_OP_HELMHOLTZ,
 *                   hanging-node masks (by bp5_mf_create itself), BP5_GEOM_AFFINE, BP5_METRIC_F32, every apply variant other than 0,
 *                   bp5_apply_components* and bp5_cg_solve_components* (block vectors: CEED BP2 / BP4), bp5_mf_get_data, bp5_mg_create with such a
 *                   level.  The facade's MatrixFree::reinit refuses the id too (its device-side FEEvaluation holds n_q_points_1d == p + 1):
 *                   examples/bp5_bp3.hip shows a native operator class over this descriptor. */
int bp5_mf_create(const bp5_mf_desc *desc, bp5_mf **out);
int bp5_mf_destroy(bp5_mf *mf);
int bp5_mf_set_stream(bp5_mf *mf, void *hip_stream);
int bp5_mf_sync(bp5_mf *mf); /* hipStreamSynchronize */

/* Which operator the handle applies (bp5_apply*, bp5_cg_solve, all exchange schedules, fused dot products):
 *   BP5_OP_POISSON    (default) LocalPoissonOperator, bp5/step-64.cu:147-194:  (grad v, kappa grad u), six merged planes;
 *   BP5_OP_HELMHOLTZ  step-64's LocalHelmholtzOperator + HelmholtzOperatorQuad (step-64/step-64.cu:154-160,201-219):
 *                     (grad v, grad u) + (v, a(x) u) -- evaluate(true, true), submit_value(a * get_value()) +
 *                     submit_gradient(get_gradient()), integrate(true, true) -- as a native fused kernel: the value path costs one
 *                     more 1-D contraction each way and one more plane.  The metric array then holds SEVEN planes: the six merged
 *                     planes JxW K K^T (coefficient 1) and the mass plane a(x_q) JxW, a = the handle's BP5_COEF_* function
 *                     (VaryingCoefficientFunctor, step-64/step-64.cu:99-118, with JxW folded in): G = 7 doubles per q-point.
 *                     Conforming meshes, BP5_GEOM_MERGED6; apply variants 0 (pencil kernel) and 56 (block kernel on cell bricks).
 *   BP5_OP_MASS       the mass operator (v, rho(x) u): CEED BP1, deal.II's MatrixFreeOperators::MassOperator -- evaluate(values),
 *                     submit_value(rho * get_value()), integrate(values) -- L2 projection and every explicit time step, as a native kernel
 *                     of its own (apply_pencil_mass_kernel): six 1-D contractions per cell with Gauss quadrature, none under GLL
 *                     collocation, where the operator is diagonal.  The metric array holds ONE plane, rho(x_q) JxW, rho = the handle's
 *                     BP5_COEF_* function, in the pair layout of the other planes: G = 1 double per q-point.  Every entry point of the
 *                     other operators takes such a handle with the same dst contracts (bp5_apply, bp5_apply_cells,
 *                     bp5_apply_distributed, bp5_copy_constrained, bp5_compute_diagonal, both bp5_cg_solve variants,
 *                     bp5_cg_solve_preconditioned, bp5_chebyshev_*), also with n_constrained == 0 (BP1 has no boundary condition).
 *                     Conforming meshes, BP5_GEOM_MERGED6, double planes, apply variants 0 (pencil kernel) and 56 (block kernel on cell
 *                     bricks, packed indices): BP5_ERR_UNSUPPORTED for hanging-node masks, BP5_GEOM_AFFINE, BP5_METRIC_F32 -- in
 *                     either order of the two calls --, every other apply variant and block vectors.
 * Set before bp5_mf_coef_size / bp5_mf_compute_merged_metric (afterwards, between operators of different plane counts: BP5_ERR_INVALID). */
enum { BP5_OP_POISSON = 0, BP5_OP_HELMHOLTZ = 1, BP5_OP_MASS = 2 };
int bp5_mf_set_operator(bp5_mf *mf, int op);
/* Storage precision of the merged-metric planes (per handle, like bp5_mf_set_operator):
 *   BP5_METRIC_F64  (default) the planes are doubles;
 *   BP5_METRIC_F32  the planes are FLOATS: half the bytes of the stream the operator kernels live on (p = 4, unfused application on lattice
 *                   bricks: 16 + 24 r instead of 16 + 48 r bytes per DoF, r = cell entries per DoF).  All arithmetic and all vectors stay
 *                   double: a kernel widens each entry where it uses it.  bp5_mf_compute_merged_metric computes every entry in double exactly
 *                   as for double planes and rounds it ONCE, to nearest, when it stores it.  The operator applied is then the FP64 operator
 *                   of the ROUNDED planes: an O(1e-8) relative perturbation of the FP64 operator, always symmetric, positive definite as long
 *                   as rounding keeps every 3 x 3 tensor SPD (any cell whose metric condition number is far below 1e7; not checked at run
 *                   time).  Meant for the level operators of a multigrid preconditioner under an FP64 outer CG (deal.II step-37 / step-75).
 * The `coef` buffer of such a handle is OPAQUE: every entry point keeps its `const double *coef` signature and reads the buffer as the
 * handle says (bp5_apply, bp5_apply_cells, bp5_apply_distributed, bp5_compute_diagonal, bp5_cg_solve, bp5_cg_solve_preconditioned,
 * bp5_chebyshev_create, bp5_mg_create -- whose levels may mix precisions: each level brings its own handle and coef).  bp5_mf_coef_size
 * returns ceil(6 n_cells (p+1)^3 / 2), the doubles that hold the floats, so allocation through bp5_vec_alloc keeps working;
 * bp5_mf_metric_to_reference_layout returns DOUBLES (the floats widened, exactly): a host sees exactly the operator the kernels apply.
 * Set before bp5_mf_coef_size / bp5_mf_compute_merged_metric (afterwards: BP5_ERR_INVALID).  BP5_ERR_UNSUPPORTED for handles with
 * hanging-node masks, BP5_OP_HELMHOLTZ and BP5_GEOM_AFFINE (which has no six-plane stream to shrink) -- in either order of the two calls --
 * and for apply variants other than 0 and 56.  Variant 0 resolves to the block kernel under the conditions of double planes (packed indices
 * needed at every degree), else to the degree's PLAIN atomic pencil kernel -- not always the kernel a double-plane handle runs by default:
 * p = 1, 3 without cell blocks run the x-row team kernel there, and p >= 5 on a mesh that numbers cell-interior DoFs first
 * (bp5_mesh_desc.dof_numbering = 2) the pencil build with plain interior stores; neither has a float-plane build.
 * Fused CG dot products (bp5_mf_set_cg_fusion) do not exist for float planes: both solvers run their separate dot-product kernels
 * (the path Jacobi-preconditioned merged CG takes) and bp5_cg_result.dot_products_fused is 0.  The block kernel reads float planes with
 * ordinary loads (bp5_mf_set_streaming has no effect on them; same bits either way). */
enum { BP5_METRIC_F64 = 0, BP5_METRIC_F32 = 1 };
int bp5_mf_set_metric_precision(bp5_mf *mf, int precision);
int bp5_mf_get_metric_precision(const bp5_mf *mf, int *precision);
/* number of doubles of the merged-metric array: 6 * n_cells * (p+1)^3  (bp5/step-64.cu:253-254); 7 planes for BP5_OP_HELMHOLTZ, 1 plane
 * (n_cells * (p+1)^3) for BP5_OP_MASS;
 * BP5_METRIC_F32: ceil(6 * n_cells * (p+1)^3 / 2);
 * BP5_QUAD_GAUSS_OVER: 6 * n_cells * (p+2)^3, or n_cells * (p+2)^3 for BP5_OP_MASS */
int bp5_mf_coef_size(const bp5_mf *mf, size_t *n_doubles);

/* == mf_data.evaluate_coefficients(JacobianFunctor), bp5/step-64.cu:84-114,256-258:
 *    coef_c = kappa * JxW * (K K^T)_c, c in {00,11,22,01,02,12}.
 *    Device layout (this library's own; the reference's is [c][cell][q]; bp5_mf_metric_to_reference_layout converts):
 *      coef[c*n_cells*nq + cell*nq + off(qi, qj + n*qk)],   n = p+1, nq = n^3, ab = qj + n*qk,
 *      off(qi, ab) = (qi/2)*2n^2 + 2ab + (qi&1)  for qi < 2(n/2);   (n/2)*2n^2 + ab  for the last qi of odd n
 *    i.e. per cell the x-pencils of the n^2 (qj,qk) positions, stored as pairs (qi, qi+1) position after position:
 *    the kernels fetch 16 bytes per lane and a wave's load is one contiguous run.
 *    BP5_METRIC_F32: the SAME index formula over an array of floats (`coef` reinterpreted as float *): the pair layout with float entries,
 *    a lane fetches 8 bytes per load, a wave's load is one contiguous run of n^2 * 8 bytes per cell.  (A layout of quads (qi .. qi+3) that
 *    keeps 16-byte loads -- 12 instead of 18 metric load instructions per lane and cell at p = 4 -- has not been built: DESIGN 7e.) */
int bp5_mf_compute_merged_metric(bp5_mf *mf, double *coef);
/* Geometry representation used by bp5_apply / bp5_cg_solve:
 *   BP5_GEOM_MERGED6  the reference's six stored planes per q-point (G = 6 doubles per q-point), `coef`
 *                     from bp5_mf_compute_merged_metric -- the default;
 *   BP5_GEOM_AFFINE   for meshes whose cells are all affine (the reference's meshes always are: congruent
 *                     cubes, bp5/step-64.cu:656-663): K K^T is constant per cell, so the library keeps six
 *                     doubles per CELL and one scalar plane kappa*JxW per q-point (G = 1).  Same operator,
 *                     same results to rounding; the `coef` argument of apply/solve is then ignored.
 *                     Fails with BP5_ERR_UNSUPPORTED if K K^T varies by more than 1e-10 (relative) inside a cell.
 *   BP5_GEOM_TRILINEAR for straight-sided hex meshes, every cell the trilinear image of its eight vertices (deal.II's
 *                     default mapping MappingQ1 / MappingQGeneric(1); what hex mesh generators write): the library
 *                     keeps 24 doubles per CELL (its corners, the local entries (0|p, 0|p, 0|p)) and the operator
 *                     kernel apply_pencil_trilinear_kernel computes kappa JxW K K^T at every q-point from them
 *                     (G = 0: no plane is read).  Same operator, same results to rounding; the `coef` argument of
 *                     apply / solve / diagonal / preconditioner entries may be NULL and is not read.  Runs
 *                     bp5_apply, bp5_apply_cells, bp5_apply_distributed, bp5_compute_diagonal, every bp5_cg_solve*
 *                     entry of scalar vectors (dot_products_fused = 0), bp5_chebyshev_create and bp5_mg_create levels.
 *                     Fails with BP5_ERR_UNSUPPORTED "mesh is not trilinear" if a node lies further than 1e-10 (relative
 *                     to the cell's shortest edge) from the trilinear image of its reference position; the handle
 *                     then stays in its previous mode.  BP5_ERR_UNSUPPORTED naming "trilinear", decided before any
 *                     launch and in either order of the two calls: BP5_OP_HELMHOLTZ, BP5_OP_MASS, BP5_QUAD_GAUSS_OVER,
 *                     hanging-node masks, BP5_METRIC_F32, every apply variant other than 0 (bp5_mf_get_apply_variant
 *                     reports 0 on brick meshes too), bp5_mf_get_data, bp5_apply_components* / bp5_cg_solve_components*
 *                     and the bp5_elasticity_* entries. */
enum { BP5_GEOM_MERGED6 = 0, BP5_GEOM_AFFINE = 1, BP5_GEOM_TRILINEAR = 2 };
int bp5_mf_set_geometry_mode(bp5_mf *mf, int mode);
/* permute to the reference layout [c][cell][qi + n(qj + n qk)] (tests / interop); coef_ref: 6 n_cells (p+1)^3 DOUBLES in either precision
 * (BP5_OP_HELMHOLTZ: 7 planes; BP5_OP_MASS: the one plane as [cell][q]; BP5_QUAD_GAUSS_OVER: [c][cell][qi + Q (qj + Q qk)], Q = p + 2) */
int bp5_mf_metric_to_reference_layout(bp5_mf *mf, const double *coef, double *coef_ref);

/* MatrixFree::Data mirror (bp5/fe_evaluation_gl.h:112-120, bp5/step-64.cu:94-97):
 * the unmerged geometry inv_jacobian (9 SoA planes) and JxW with deal.II's padding.
 * Arrays are created on first request. */
typedef struct {
  const uint32_t *local_to_global; /* [n_cells*padding_length]                                  */
  const double *inv_jacobian;      /* [9][n_cells*padding_length], plane d*3+e = d xi_d/d x_e   */
  const double *JxW;               /* [n_cells*padding_length]                                  */
  const double *q_points;          /* [3][n_cells*padding_length]                               */
  const uint32_t *constraint_mask; /* [n_cells], BP5_HANG_* bits (all zero on conforming meshes) */
  uint32_t n_cells, padding_length, row_start;
  int use_coloring;
} bp5_mf_data;
int bp5_mf_get_data(bp5_mf *mf, int color, bp5_mf_data *out);

/* == PoissonOperator::vmult(dst, src), bp5/step-64.cu:263-276:
 *    [dst = 0 if zero_dst] ; dst += sum_cells P^T B^T S B P src ; dst[c] = src[c] on Dirichlet DoFs.
 *    Single-rank form (no halo exchange). */
int bp5_apply(bp5_mf *mf, const double *coef, const double *src, double *dst, int zero_dst);
/* pieces, for hosts that overlap the halo exchange themselves (MatrixFree::cell_loop,
 * bp5/step-64.cu:274): cell range [cell_begin, cell_end) only, no zeroing, no Dirichlet copy */
int bp5_apply_cells(bp5_mf *mf, const double *coef, const double *src, double *dst, uint32_t cell_begin,
                    uint32_t cell_end);
/* (with cell blocks: ranges that are unions of whole blocks keep the block-assembled kernel -- DoFs shared with
 * blocks outside the range are then added atomically; [0, n_interior_cells) of bp5_mesh_create_brick is such a range) */
/* == mf_data.copy_constrained_values(src, dst), bp5/step-64.cu:275 */
int bp5_copy_constrained(bp5_mf *mf, const double *src, double *dst);
/* == MatrixFree::set_constrained_values(val, dst) [upstream] */
int bp5_set_constrained(bp5_mf *mf, double value, double *dst);

/* Block vectors (deal.II BlockVector over ONE scalar DoFHandler; CEED BP6 = BP5 with three components): n_components local vectors in
 * one allocation, component c at v + c * ld, each block laid out like a scalar vector (owned entries, then ghosts).  ld >= n_owned +
 * n_ghost and even, the base pointer 16-byte aligned (every block then is); entries [n_owned + n_ghost, ld) of a block are padding:
 * never read, never written.  Index plans, the Dirichlet set and the diagonal stay per scalar DoF and are shared by all components. */
#define BP5_MAX_COMPONENTS 8
/* dst_c = [0 +] A src_c ; dst_c[constrained] = src_c[constrained], c = 0 .. n_components-1: bp5_apply on every block, with ONE pass over the
 * metric planes and local_to_global (FEEvaluation<dim,p,n_q,n_components> on a BlockVector; the reference asserts n_components == 1:
 * bp5/fe_evaluation_gl.h:137,165).  One kernel of its own (apply_pencil_components_kernel) for every n_components, 1 included; it scatters
 * with atomics: not bitwise reproducible.  Refused before any launch (reason in bp5_last_error) -- BP5_ERR_INVALID: null pointer,
 * n_components outside 1..BP5_MAX_COMPONENTS, ld < n_owned + n_ghost, odd ld, misaligned base, overlapping src / dst;
 * BP5_ERR_UNSUPPORTED: FP32-metric, Helmholtz, hanging-node and affine-geometry handles, a handle with a communicator and neighbours
 * (a rank-local mesh with ghost DoFs but no communicator is fine: the ghost slots are just entries of the block). */
int bp5_apply_components(bp5_mf *mf, const double *coef, int n_components, size_t ld, const double *src, double *dst, int zero_dst);

/* kernel variant selection for the fused operator (tuning / A-B tests):
 * 0 = library default: the measured best kernel for the degree, the geometry mode and the way the
 * cells were handed over (a mesh given in cell blocks runs the block-assembled kernel at p = 4) */
int bp5_mf_set_apply_variant(bp5_mf *mf, int variant);
/* cap on the persistent grid of the block-assembled kernel (0 = sized from the CU count; tuning / tests: a small cap
 * makes every workgroup walk several blocks even on a small mesh) */
int bp5_mf_set_block_workgroups(bp5_mf *mf, int max_workgroups);
/* cache policy for the data a CG iteration touches ONCE (the metric planes in the p = 4 lattice block kernel; v and x in the merged solver's
 * update kernel; results are the same bits either way): 1 = non-temporal accesses, so that this data does not evict the vectors that are
 * reused (p, r) from the 256 MB memory-side cache (-6 % per CG iteration at 1e7 DoFs, +1 % at 1e8), 0 = ordinary accesses,
 * -1 = chosen from the local size (default: non-temporal up to 2.4e7 local DoFs) */
int bp5_mf_set_streaming(bp5_mf *mf, int policy);
/* Per-handle tuning / A-B knobs (results are the same bits for every setting; two handles of one process may differ).  The
 * environment variables named below are read ONCE, by bp5_mf_create, as the handle's initial values -- nothing on the apply or
 * solve path reads the environment.
 *   BP5_TUNE_LATTICE_INDICES   (env BP5_LATTICE_INDICES, default 1) closed-form indices for lattice blocks; 0 keeps the packed
 *                              u16 stream.  Set before the block plan is built (first apply / solve / bp5_mf_block_plan_*).
 *   BP5_TUNE_EARLY_GATHER      (env BP5_EARLY_GATHER, default 1) fused merged CG across ranks: the ghost gather of the new search
 *                              direction travels under the update kernel (0: after it).
 *   BP5_TUNE_COMBINE_SIGNAL    (env BP5_COMBINE_SIGNAL, default 0) default exchange schedule with ONE combine launch: the ghost rows
 *                              first, the exchange released mid-launch by a stream wait-value (needs the capability below).
 *   BP5_TUNE_BOUNDARY_FIRST    (env BP5_BOUNDARY_FIRST = signal | launches, default 1 = signal) boundary-first schedule inside one
 *                              launch (stream wait-value) or as two launches (0).  The in-launch form is used only when the device
 *                              reports hipDeviceAttributeCanUseStreamWaitValue AND a producer / consumer self-check, run once when the
 *                              handle creates its communication stream, has seen the waiting stream released while the producing kernel
 *                              was still running (on plain device memory the runtime implements the wait by polling; if that ever
 *                              stops working mid-kernel the library falls back to two launches by itself).
 *   BP5_TUNE_FOLD_SMALL        (env BP5_FOLD_SMALL, default 1) merged CG on the atomic kernels: zero-fill and Dirichlet copy folded
 *                              into the neighbouring launches.
 *   BP5_TUNE_UPDATE_UNROLL     (env BP5_UPDATE_UNROLL, 1 | 2 | 4, default 1) 16-byte accesses per lane, stream and loop trip of the merged
 *                              solver's update kernels.
 *   BP5_TUNE_UPDATE_FLAT       (env BP5_UPDATE_FLAT, default 1) streaming kernels without a reduction (update kernels, vector updates)
 *                              are launched with ONE trip per workgroup instead of a capped grid-stride grid: the stores of a capped
 *                              grid drift apart and lose 15-35 % of the HBM write rate (profiles/r4: hbm_sweep).
 *   BP5_TUNE_UPDATE_NT         (env BP5_UPDATE_NT, -1 | 0 | 1, default -1) non-temporal accesses to v and x in the update kernels:
 *                              -1 = the library's default (on at every size: -0.9 % per iteration at 1e8 DoFs, -1.2 % at 1e7).
 *   BP5_TUNE_COMBINE_WG_PER_CU (env BP5_COMBINE_WG_PER_CU, 0 ... 32, default 16) workgroups per CU of the fused solver's combine pass (a fixed grid that walks
 *                              the tiles of brick-surface DoFs, one dot-product column per workgroup); 0 = as many workgroups as columns are free
 *                              (rounds 2-3).  The dot products are summed over another column layout (rounding-level differences), v is the same bits.
 *   BP5_TUNE_GHOST_COMBINE_ON_COMM (env BP5_GHOST_COMBINE_ON_COMM, default 0) default exchange schedule (overlap 2): the ghost-row window of the combine pass on the
 *                              communication stream (in front of the send) instead of the compute stream, so that the owned-row window starts right behind the brick kernel.
 *   BP5_TUNE_INTERIOR_STORES   (env BP5_INTERIOR_STORES, default 1) atomic pencil kernel of p >= 5 on a mesh whose cell-interior DoFs are numbered ahead of all
 *                              others (bp5_mesh_desc.dof_numbering = 2; detected at bp5_mf_create): plain stores for the (p-1)^3 entries a cell owns alone.
 *   BP5_TUNE_FACE_CARRY        (env BP5_FACE_CARRY, default 1) block kernel on lattice bricks (p = 4): the interior of the face two CONSECUTIVE bricks of one
 *                              workgroup's range share stays in LDS from the first brick's write-out to the second's, which stores the sum as an owner store;
 *                              the combine pass of that launch skips those DoFs.  v is the same bits as without (a + b == b + a); the fused dot products are
 *                              summed over other workgroups (rounding-level differences, reproducible run to run).
 *   BP5_TUNE_FUSED_UPDATE      (env BP5_FUSED_UPDATE, -1 | 0 | 1, default -1) merged CG with fused dot products on one rank, p = 4, lattice bricks, DoFs numbered
 *                              brick by brick (bp5_mesh_desc.dof_numbering = 1): the block kernel applies the solver's vector update to the interior DoFs of every
 *                              brick right before it processes the brick, and the update launch shrinks to the brick surfaces -- p and r are read back while they
 *                              are still in the memory-side cache.  Same bits as the separate update; on such a solve p, r and x are updated by the OPERATOR launch.
 *                              1 = wherever the plan qualifies (anything else takes the separate update silently), -1 = only above 2.4e7 local DoFs (where the
 *                              vectors do not fit that cache from one launch to the next: -3 % per iteration at 1e8 DoFs, profiles/fused_update), 0 = off.
 *                              Such a launch reads the metric non-temporally unless bp5_mf_set_streaming says 0. */
enum { BP5_TUNE_LATTICE_INDICES = 0, BP5_TUNE_EARLY_GATHER = 1, BP5_TUNE_COMBINE_SIGNAL = 2, BP5_TUNE_BOUNDARY_FIRST = 3,
       BP5_TUNE_FOLD_SMALL = 4, BP5_TUNE_UPDATE_UNROLL = 5, BP5_TUNE_UPDATE_FLAT = 6, BP5_TUNE_UPDATE_NT = 7, BP5_TUNE_COMBINE_WG_PER_CU = 8,
       BP5_TUNE_INTERIOR_STORES = 9, BP5_TUNE_GHOST_COMBINE_ON_COMM = 10, BP5_TUNE_FACE_CARRY = 11, BP5_TUNE_FUSED_UPDATE = 12,
       BP5_TUNE_COUNT = 13 };
int bp5_mf_set_tuning(bp5_mf *mf, int knob, int value);
int bp5_mf_get_tuning(const bp5_mf *mf, int knob, int *value);
/* 1 when the in-launch stream wait-value schedules are available on this handle (capability + self-check, see BP5_TUNE_BOUNDARY_FIRST);
 * creates the handle's communication stream if it does not exist yet */
int bp5_mf_wait_value_available(bp5_mf *mf, int *available);
/* facts about the block kernel's plan for this handle (builds it): number of cell blocks, longest run-length list of a
 * block, and whether the packed one-u16-per-DoF index form is available (<= 128 runs per block; brick-major numbering
 * gives ~30, a slab's boundary bricks with their ghost rows ~70) -- every rank of a multi-GPU run should report 1 */
int bp5_mf_block_plan_info(bp5_mf *mf, uint32_t *n_blocks, uint32_t *max_runs, int *packed_indices);
/* ... and how many of its cell blocks are LATTICE blocks: full boxes of cells whose DoFs are numbered entity by entity (what a brick-major
 * numbering produces; recognised topologically and verified entry by entry when the plan is built).  For those the kernel computes every
 * entry's list slot and DoF in closed form from the cell's position in its block and reads no per-DoF index at all (the packed stream of
 * the other blocks costs 2 bytes per cell-local DoF); the results are bitwise the same either way. */
int bp5_mf_block_plan_lattice(bp5_mf *mf, uint32_t *n_lattice_blocks);
/* ... and the face carry (BP5_TUNE_FACE_CARRY): faces the plan found that a workgroup may keep in LDS from one block to the next, the plan's
 * brick-surface (shared) DoFs, and how many of those the combine pass of the LAST block-kernel launch on this handle had in its tables
 * (== n_shared when that launch carried nothing). */
int bp5_mf_block_plan_carry(bp5_mf *mf, uint32_t *n_faces, uint32_t *n_shared, uint32_t *n_shared_last_launch);
/* the variant a whole-range application resolves to (what "0" means for this handle) */
int bp5_mf_get_apply_variant(bp5_mf *mf, int *effective);

/* diag(A_eff) of the operator bp5_apply applies (1 on Dirichlet DoFs), or its reciprocal when invert != 0: the
 * Jacobi preconditioner for the `diag` slot every solver kernel of the reference already threads through
 * (bp5/solver.h:68,100,131,170; bp5/step-64.cu:428-432 fills it with ones).  Setup-time, matrix-free
 * (sum-factorised, no element matrices); ghost contributions are sent to their owners when a communicator is set.
 * diag: owned + ghost storage, ghost entries are left zero.  BP5_OP_HELMHOLTZ: the mass term is included.
 * BP5_OP_MASS: diag_i = sum_cells sum_q (N.N x N.N x N.N) rho JxW (under GLL collocation the whole operator). */
int bp5_compute_diagonal(bp5_mf *mf, const double *coef, double *diag, int invert);

/* b_i = int phi_i with Gauss(p+1), constrained rows 0 (assemble_rhs, bp5/step-64.cu:372-418) */
int bp5_assemble_rhs(bp5_mf *mf, double *b);
/* ||u_h||_L2 by Gauss(p+1) quadrature (output_results, bp5/step-64.cu:602-616); synchronous.  With a communicator and
 * neighbours the ghost range of u is refreshed from its owners first (the reference integrates a ghosted copy,
 * ghost_solution_host) and zeroed again afterwards -- the owned entries are never written. */
int bp5_l2_norm_solution(bp5_mf *mf, const double *u, double *result_host);

/* ------------------------------------------------------------------------------------------ */
/* vector BLAS-1 used by the solvers (LinearAlgebra::distributed::Vector surface,
 * bp5/solver.h:369-382,417-421,511,528).  n = number of OWNED entries.                        */
int bp5_vec_fill(bp5_mf *mf, double *v, double value, size_t n);
int bp5_vec_axpy(bp5_mf *mf, double *y, double a, const double *x, size_t n);              /* y += a x   (add)  */
int bp5_vec_equ(bp5_mf *mf, double *y, double a, const double *x, size_t n);               /* y  = a x   (equ)  */
int bp5_vec_sadd(bp5_mf *mf, double *y, double s, double a, const double *x, size_t n);    /* y = s y + a x     */
int bp5_vec_dot(bp5_mf *mf, const double *x, const double *y, size_t n, double *result_host); /* synchronous, local */
/* Vector::l2_norm() / Vector::all_zero() (bp5/solver.h:369-382, bp5/step-64.cu:467): over the first n (= owned)
 * entries of every rank -- one on-stream RCCL all-reduce when a communicator is attached; synchronous */
int bp5_vec_l2_norm(bp5_mf *mf, const double *x, size_t n, double *result_host);
int bp5_vec_all_zero(bp5_mf *mf, const double *x, size_t n, int *result_host);

/* ------------------------------------------------------------------------------------------ */
/* communication: one rank per GPU, RCCL over xGMI                                             */
typedef struct bp5_comm bp5_comm;
#define BP5_UNIQUE_ID_BYTES 128
int bp5_comm_unique_id(char *id_host /*[BP5_UNIQUE_ID_BYTES]*/);    /* rank 0; broadcast by the host */
int bp5_comm_create(const char *id_host, int rank, int n_ranks, bp5_comm **out);
int bp5_comm_destroy(bp5_comm *comm);
int bp5_mf_set_comm(bp5_mf *mf, bp5_comm *comm);
/* sum-allreduce of n doubles in place on the handle's stream
 * (replaces cudaMemcpy D2H + MPI_Allreduce, bp5/solver.h:488-494) */
int bp5_comm_allreduce_sum(bp5_mf *mf, double *buf, size_t n);
/* == src.update_ghost_values_start/finish, dst.compress_start/finish(add), zero_out_ghosts
 *    (inside cell_loop, bp5/step-64.cu:274).
 *    *_start: the owners' values are packed on the handle's stream, then the RCCL send/recv group runs on the handle's own
 *    communication stream (ordered by events); *_finish: the handle's stream waits for the transfer (scatter-add: and adds
 *    the received contributions to the owned entries, ghosts zeroed).  Work enqueued on the handle's stream between a start
 *    and its finish overlaps the transfer; it must not touch the entries in flight (gather: the ghost range of v;
 *    scatter-add: the ghost range of v and nothing else).  One exchange of each kind may be in flight per handle.
 *    bp5_halo_gather / bp5_halo_scatter_add = start immediately followed by finish. */
int bp5_halo_gather_start(bp5_mf *mf, double *v);
int bp5_halo_gather_finish(bp5_mf *mf, double *v);
int bp5_halo_scatter_add_start(bp5_mf *mf, double *v);
int bp5_halo_scatter_add_finish(bp5_mf *mf, double *v);
int bp5_halo_gather(bp5_mf *mf, double *v);
int bp5_halo_scatter_add(bp5_mf *mf, double *v);
int bp5_halo_zero_ghosts(bp5_mf *mf, double *v);
/* == MatrixFree::AdditionalData::overlap_communication_computation (bp5/step-64.cu:241).  mode 1: on (the reference's setting);
 *    0: off -- the exchange stays on the handle's stream and the cell loop runs unsplit; 2 (default): the library decides.
 *    Solvers on the block kernel (fused dot products), mode 1: BOUNDARY-FIRST -- every workgroup of the (single) launch walks its share
 *    of the ghost-touching bricks first and counts itself in; the communication stream waits for the count (hipStreamWaitValue64),
 *    combines the ghost rows and sends them to their owners while the same launch works through the interior bricks.  Mode 2 there:
 *    one launch, then the ghost rows of the combine pass, the exchange on the communication stream UNDER the owned rows of the combine
 *    pass (a transfer that runs beside the bandwidth-bound brick kernel is slow and slows it; profiles/r3).  In every mode the ghost
 *    gather of the search direction travels under the vector update, and the results are bitwise the same.
 *    bp5_apply_distributed and the atomic kernels use the three-phase split (interior, boundary, interior): automatic from 1e6
 *    interior cells on -- it costs three launches and four cross-stream dependencies per application (profiles/r2, r3 READMEs) */
int bp5_mf_set_overlap(bp5_mf *mf, int mode);
/* distributed vmult == PoissonOperator::vmult on more than one rank (bp5/step-64.cu:263-276 with the cell_loop of :274).
 *    With the overlapped schedule (bp5_mf_set_overlap): ghost gather started; first part of the interior cells [0, n_interior_cells) underneath it; gather finished; the cells
 *    that touch ghosts; ghost contributions sent to their owners (atomic kernels: under the rest of the interior cells; the
 *    block kernel: after its single combine pass, which completes the ghost entries) and added; ghosts of src zeroed;
 *    Dirichlet copy.  Same kernels and, with the block kernel, bitwise the same result as the unsplit application (gather,
 *    all cells, scatter-add on the handle's stream), which is what runs when the overlap policy says off. */
int bp5_apply_distributed(bp5_mf *mf, const double *coef, double *src, double *dst, int zero_dst);

/* The same on block vectors (layout as for bp5_apply_components: component c at v + c * ld, ld even and >= n_owned + n_ghost, base 16-byte
 * aligned, entries [n_owned + n_ghost, ld) of a block never read, never written).  The ghost ranges of a block vector are n_components
 * strided pieces, so every exchange goes through staging buffers of the handle (grown on demand) in which a neighbour's message is
 * contiguous and holds all components, [neighbour][component][entry]: ONE send and ONE receive per neighbour and direction in one RCCL
 * group, zero-length messages skipped; the number of launches and of RCCL calls does not depend on n_components.  Stream choice as for the
 * scalar calls (bp5_mf_set_overlap).  Refused before any launch: the layout errors of bp5_apply_components (BP5_ERR_INVALID); a handle
 * without neighbours is not an error (nothing to exchange).
 * == BlockVector::update_ghost_values() (per block: src.update_ghost_values, bp5/step-64.cu:274): every block's ghost range receives
 *    its owners' values */
int bp5_halo_gather_components(bp5_mf *mf, int n_components, size_t ld, double *v);
/* == BlockVector::compress(VectorOperation::add) (per block: dst.compress(add) inside cell_loop, bp5/step-64.cu:274): the ghost
 *    contributions of every block are added to the owners' entries, neighbour after neighbour in the fixed order of bp5_halo_scatter_add
 *    (bitwise reproducible); every block's ghost range is zero afterwards */
int bp5_halo_scatter_add_components(bp5_mf *mf, int n_components, size_t ld, double *v);
/* == BlockVector::zero_out_ghosts() [upstream; the reference's cell_loop leaves src without ghost values, bp5/step-64.cu:274] */
int bp5_halo_zero_ghosts_components(bp5_mf *mf, int n_components, size_t ld, double *v);
/* bp5_apply_distributed on every block == PoissonOperator::vmult on a BlockVector on more than one rank (bp5/step-64.cu:263-276; the
 *    reference asserts n_components == 1: bp5/fe_evaluation_gl.h:137,165): ghosts of src gathered; apply_pencil_components_kernel over the
 *    cells; dst scatter-added; ghosts of src zeroed again; Dirichlet copy on every block.  Overlap off, or auto below 1e6 interior cells:
 *    unsplit, all on the handle's stream.  Overlap on: the three-phase schedule of bp5_apply_distributed for atomic kernels -- the gather
 *    in flight under the first half of the interior cells, the cells that touch ghosts, the ghost contributions on their way under the
 *    rest of the interior cells.  Refusals: those of bp5_apply_components except the communicator one; a handle without a communicator or
 *    without neighbours does what bp5_apply_components does. */
int bp5_apply_components_distributed(bp5_mf *mf, const double *coef, int n_components, size_t ld, double *src, double *dst, int zero_dst);

/* ------------------------------------------------------------------------------------------ */
/* Krylov solvers                                                                              */
enum { BP5_CG_PLAIN = 0,  /* deal.II SolverCG (bp5/step-64.cu:446-453): the parity target      */
       BP5_CG_MERGED = 1  /* SolverCGFullMerge (bp5/solver.h:343-542), x schedule fixed         */ };

typedef struct {
  int variant;       /* BP5_CG_*                                                                */
  int max_iter;      /* IterationNumberControl(max_iter, abs_tol), bp5/step-64.cu:443-445       */
  double abs_tol;    /* stop when ||r|| <= abs_tol                                              */
  int check_every;   /* host looks at the device-side convergence flag every k iterations
                        (0 = only at the end); the iterate is frozen on device at convergence
                        either way, so the result does not depend on it                         */
  int profile;       /* 1 = bracket every operator launch with HIP events; 2 = also stamp the phases of every
                        iteration (bp5_cg_result.phase_ms; diagnostic: the stamps themselves cost a few us) */
} bp5_cg_params;

typedef struct {
  int iterations;          /* SolverControl::last_step()                                        */
  double residual;         /* last ||r||                                                        */
  double initial_residual;
  double solve_ms;         /* HIP-event time of the whole solve on the stream                   */
  double apply_ms_avg;     /* profile=1: average duration of one launch of the cell kernel alone  */
  int apply_launches;
  double operator_ms_avg;  /* profile=1: zero-fill + cell kernel + combine pass (one A*x without halo) */
  int dot_products_fused;  /* 1: the solve formed its dot products inside the operator kernels (bp5_mf_set_cg_fusion) */
  int exchange_schedule;   /* halo exchange of the operator applications: 0 none (one rank), 1 unsplit (gather, all cells, scatter-add),
                              2 boundary-first (ghost-touching bricks, exchange on the communication stream under the interior bricks),
                              3 three-phase (atomic kernels / separate dot products: interior, boundary, interior),
                              4 all bricks in one launch, ghost rows combined first, exchange under the owned-row combine pass    */
  char apply_kernel[96];   /* the operator kernel the solve launched last, as a profiler prints it (e.g.
                              "apply_block_kernel<4,false,32,1,1337344>"): what rocprofv3 rows belong to this solve               */
  /* profile=2, BP5_CG_MERGED: average HIP-event time of the phases of one iteration on the handle's stream (ms), BP5_PHASE_* */
  double phase_ms[8];
} bp5_cg_result;
enum { BP5_PHASE_UPDATE = 0,      /* vector update (+ packing / starting the ghost gather of the new search direction)       */
       BP5_PHASE_GATHER_WAIT = 1, /* stream waits for the ghost values (exposed part of the gather)                          */
       BP5_PHASE_OPERATOR = 2,    /* cell kernels + combine pass (boundary-first: + ghost-row combine, exchange start)        */
       BP5_PHASE_EXCHANGE = 3,    /* exposed part of the scatter-add exchange + unpack (unsplit: the whole exchange)          */
       BP5_PHASE_REDUCE = 4,      /* local reduction of the partial sums                                                      */
       BP5_PHASE_ALLREDUCE = 5,   /* RCCL all-reduce of the 7 sums                                                            */
       BP5_PHASE_CONTROL = 6,     /* scalar step (alpha, beta, stopping test)                                                 */
       BP5_PHASE_ITERATION = 7    /* whole iteration                                                                          */ };

/* == cg.solve(A, x, b, preconditioner) with DiagonalMatrix (bp5/step-64.cu:446-453,488-495).
 *    diag may be NULL (== 1, bp5/step-64.cu:432).  x is overwritten (x0 = 0, bp5/step-64.cu:449).
 *    Returns BP5_OK also when max_iter is reached (IterationNumberControl reports success). */
int bp5_cg_solve(bp5_mf *mf, const double *coef, const double *diag, const double *b, double *x,
                 const bp5_cg_params *params, bp5_cg_result *result_host);

/* The same solvers for ANY operator: cg.solve(A, x, b, preconditioner) uses nothing of A but A.vmult(dst, src)
 * (bp5/solver.h:25-30,377,475; the reference solves step-64's Helmholtz operator with them, step-64/step-64.cu:505-530).
 * The callback must ENQUEUE dst = A src on the handle's stream (no host synchronisation needed), define every owned entry
 * of dst (Dirichlet rows included), may use the ghost range of src and dst as scratch, and returns BP5_OK or an error code
 * (which aborts the solve and is returned).  `mf` supplies the vector layout (n_owned), the stream, the communicator for
 * the dot products and the work vectors; b, x, diag as for bp5_cg_solve. */
typedef int (*bp5_vmult_fn)(void *ctx, double *dst, double *src);
int bp5_cg_solve_operator(bp5_mf *mf, bp5_vmult_fn vmult, void *ctx, const double *diag, const double *b, double *x,
                          const bp5_cg_params *params, bp5_cg_result *result_host);

/* SolverCG (bp5/step-64.cu:446-453) on the stacked system diag(A, ..., A) x = b of a block vector (bp5_apply_components; CEED BP6): ONE
 * Krylov space -- alpha, beta and the stop test (||g||_2 of the stacked residual against abs_tol, capped by max_iter) are shared by all
 * components, so the iterates differ from n_components separate solves unless the right-hand sides coincide.  The BP5_CG_PLAIN recurrence
 * of bp5_cg_solve; inv_diag (n_owned entries, or NULL == 1) is applied to every block; dot products run over the owned entries of all
 * blocks in a fixed order.  Refusals as for bp5_apply_components; params->variant: an unknown value is BP5_ERR_INVALID, BP5_CG_MERGED
 * (known, not offered on block vectors) BP5_ERR_UNSUPPORTED.  The work vectors (3 n_components ld doubles) belong to the handle. */
int bp5_cg_solve_components(bp5_mf *mf, const double *coef, int n_components, size_t ld, const double *inv_diag, const double *b, double *x,
                            const bp5_cg_params *params, bp5_cg_result *result_host);
/* ... on more than one rank (cg.solve on a BlockVector with MPI, bp5/step-64.cu:446-453): the same recurrence, still ONE Krylov space,
 * with the halo exchange inside every operator application (bp5_apply_components_distributed) and d.h, g.g and g.z all-reduced where
 * bp5_cg_solve all-reduces them (replaces cudaMemcpy D2H + MPI_Allreduce, bp5/solver.h:488-494), the initial reduction included: every
 * rank gets the same iteration count and residual.  Stop rule, check_every, breakdown status and result fields as on one rank;
 * result->exchange_schedule is 1 (unsplit) or 3 (three-phase), 0 without neighbours.  Refusals as for bp5_cg_solve_components except the
 * communicator one. */
int bp5_cg_solve_components_distributed(bp5_mf *mf, const double *coef, int n_components, size_t ld, const double *inv_diag, const double *b,
                                        double *x, const bp5_cg_params *params, bp5_cg_result *result_host);

/* ---- Linear elasticity: a(v, u) = int kappa(x) [ lambda (div v)(div u) + 2 mu eps(v) : eps(u) ] dx, eps(u) = (grad u + grad u^T) / 2, on
 * three-component block vectors over the handle's ONE scalar DoF layout (layout as for bp5_apply_components with n_components = 3) -- the
 * operator that couples the components at the quadrature points (deal.II step-8 / step-18: FEEvaluation<dim, p, n_q, dim> with
 * get_symmetric_gradient / submit_symmetric_gradient; the "solids" mini-app of CEED).  lambda, mu: constant Lame parameters, by value;
 * kappa: the handle's BP5_COEF_* function, scaling both; Dirichlet: all three components clamped on the handle's constrained set
 * (n_constrained == 0 is legal: the six rigid-body modes are then the null space).  With K[d][e] = d xi_d / d x_e (bp5_mf_get_data's
 * inv_jacobian), ghat_c the reference gradient of component c and s = kappa JxW, a quadrature point computes
 *   G[c][e] = sum_d K[d][e] ghat_c[d],  sigma[c][e] = lambda tr(G) delta_ce + mu (G[c][e] + G[e][c]),  t_c[d] = s sum_e K[d][e] sigma[c][e].
 * The entries sit beside the handle's others and change none of them: the same handle goes on serving bp5_apply with its own array.
 * Refused before any launch, bp5_last_error names "elasticity" -- BP5_ERR_INVALID: null pointer (coef included), odd ld, misaligned base (checked
 * before the handle is looked at), src == dst or overlapping (bp5_cg_solve_elasticity: also inv_diag overlapping x), mu <= 0, lambda + 2/3 mu <= 0 or a non-finite parameter, ld < n_owned + n_ghost;
 * BP5_ERR_UNSUPPORTED: BP5_QUAD_GAUSS_OVER, a Helmholtz or mass handle, hanging-node masks, BP5_GEOM_AFFINE, BP5_METRIC_F32, a handle with a
 * communicator and neighbours (a rank-local slab with ghosts and no communicator is fine). */
/* Doubles of the operator's metric array: TEN planes, plane-major, each n_cells * (p+1)^3 in the pair layout of the merged metric --
 * planes 0..8 K[d][e] at 3 d + e, plane 9 kappa(x_q) JxW.  An array of its own: the handle's plane count (bp5_mf_coef_size) is not touched.
 * (replaces MatrixFree::reinit's inverse_jacobian / JxW for the vector-valued FEEvaluation) */
int bp5_elasticity_coef_size(const bp5_mf *mf, size_t *n_doubles);
/* Fills it (one setup kernel; replaces MatrixFree::reinit with update_gradients | update_JxW_values and the coefficient evaluation). */
int bp5_elasticity_compute_metric(bp5_mf *mf, double *coef);
/* dst = [0 +] A src, dst_c = src_c on Dirichlet DoFs: per-block zero-fill, ONE kernel launch for the three components
 * (apply_pencil_elasticity_kernel, the degree's default pencil shape, both quadratures), the Dirichlet copy.  Scatter by atomics: not
 * bitwise reproducible.  Entries [n_owned + n_ghost, ld) are never read or written.  (replaces ElasticityOperator::vmult: cell_loop with
 * FEEvaluation<dim, p, n_q, dim>::evaluate / submit_symmetric_gradient / integrate; CEED solids: ApplyJacobian of the linear problem) */
int bp5_elasticity_apply(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, const double *src, double *dst, int zero_dst);
/* dst += A src over the cells [cell_begin, cell_end) (any range, also ragged against the kernel's teams; empty: nothing is launched); no
 * zero-fill, no Dirichlet copy.  (replaces one colour of MatrixFree::cell_loop) */
int bp5_elasticity_apply_cells(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, const double *src, double *dst, uint32_t cell_begin,
                               uint32_t cell_end);
/* The three diagonals as one block vector (they differ per component): diag_a[i] = sum_cells sum_q s [ (lambda + mu) (d_a phi_i)^2 +
 * mu |grad phi_i|^2 ], 1 on Dirichlet DoFs; invert != 0: the reciprocals (owned entries) -- bp5_compute_diagonal's convention, block by
 * block.  (replaces MatrixFreeOperators::Base::compute_diagonal of the vector-valued operator) */
int bp5_elasticity_compute_diagonal(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, double *diag, int invert);
/* SolverCG on A x = b: the BP5_CG_PLAIN recurrence of bp5_cg_solve_components with the coupled application as operator step and a BLOCK
 * inverse diagonal (inv_diag: three blocks ld apart as bp5_elasticity_compute_diagonal returns them, or NULL == identity).  One Krylov space,
 * the stop rule on the stacked ||g||_2; check_every, breakdown status and result fields as there (dot_products_fused == 0); BP5_CG_MERGED:
 * BP5_ERR_UNSUPPORTED.  (replaces SolverCG<BlockVector>::solve(A, x, b, PreconditionJacobi) of step-8) */
int bp5_cg_solve_elasticity(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, const double *inv_diag, const double *b, double *x,
                            const bp5_cg_params *params, bp5_cg_result *result_host);

/* SolverCG on A x = b with ANY preconditioner: the BP5_CG_PLAIN recurrence of bp5_cg_solve_preconditioned on the stacked three-component system.
 * precond (bp5_vmult_fn shape) enqueues z = P g on three-block vectors of the same ld on the handle's stream: bp5_chebyshev_vmult with a handle of
 * bp5_elasticity_chebyshev_create, bp5_mg_vmult with a handle of bp5_elasticity_mg_create (both created with this ld), or any callback; it defines
 * the owned entries of every block of z and never touches [n_owned + n_ghost, ld).  One Krylov space; g.g and g.z run over the owned entries of all
 * blocks in a fixed order; stop rule, check_every (0: the host's lagged look at the stop flag, as bp5_cg_solve_preconditioned), breakdown status and
 * result fields as bp5_cg_solve_elasticity.  z (3 ld doubles) belongs to the handle, beside g, d, h.  Refusals: those of bp5_cg_solve_elasticity
 * (BP5_CG_MERGED: BP5_ERR_UNSUPPORTED), a null precond BP5_ERR_INVALID.
 * (replaces SolverCG<BlockVector>::solve(A, x, b, PreconditionChebyshev / PreconditionMG) of step-8 with step-37's preconditioners) */
int bp5_cg_solve_elasticity_preconditioned(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, bp5_vmult_fn precond, void *precond_ctx,
                                           const double *b, double *x, const bp5_cg_params *params, bp5_cg_result *result_host);

/* ---- Finite-strain hyperelasticity: the compressible neo-Hookean material of the CEED "solids" mini-app (ElasFSInitialNH1F) and Holzapfel,
 *   Phi(F) = lambda / 2 (ln J)^2 - mu ln J + mu / 2 (tr F^T F - 3),   F = I + grad_x u,   J = det F,   B = F^-T,
 *   first Piola stress  P  = mu (F - B) + lambda ln J B,
 *   its tangent         dP = mu G + (mu - lambda ln J) B G^T B + lambda (B : G) B     for an increment with G = grad_x du,
 * on the vectors, the handle and the TEN geometry planes of the linear elasticity entries above (coef: bp5_elasticity_compute_metric's array;
 * kappa scales the energy: s = kappa JxW).  At F = I the tangent is the operator of bp5_elasticity_apply; it is symmetric (it comes from a
 * potential).  A quadrature point computes G[c][e] = sum_d K[d][e] ghat_c[d] and t_c[d] = s sum_e K[d][e] T[c][e], T = P (residual) or dP (tangent).
 * state: ten planes of n_cells (p+1)^3 doubles, plane-major, each in the pair layout of the metric planes -- planes 0..8 B[c][e] at 3 c + e,
 * plane 9 ln J.  The residual WRITES it, the tangent only READS it (no inverse, determinant or logarithm in the tangent's quadrature-point function):
 * a tangent application belongs to the u of the last residual call on that array.  A point with J <= 0 yields NaN in the state and in r: documented,
 * not trapped (bp5_hyperelasticity_newton backtracks on a non-finite norm).
 * One rank, conforming meshes, FP64 planes, constant lambda and mu.  Refused before any launch and in either call order, bp5_last_error names
 * "hyperelasticity": everything bp5_elasticity_apply refuses, with the same status (the trilinear geometry mode among them), and a null state
 * (BP5_ERR_INVALID).  The entries sit beside the handle's others and change none of them. */
/* Doubles of the state array: 10 n_cells (p+1)^3. */
int bp5_hyperelasticity_state_size(const bp5_mf *mf, size_t *n_doubles);
/* r = [0 +] F_int(u), r_c = 0 on Dirichlet DoFs in every block, and the state of u is stored.  u may carry non-zero values on Dirichlet DoFs (a
 * prescribed displacement).  Per-block zero-fill, ONE launch of apply_pencil_hyperelasticity_kernel<.., residual> (the degree's default pencil
 * shape, both quadratures), the Dirichlet zeros.  Scatter by atomics: not bitwise reproducible.  Entries [n_owned + n_ghost, ld) are never read or
 * written.  (replaces CEED solids' ElasFSInitialNH1F residual QFunction; deal.II step-44's assemble_system_rhs) */
int bp5_hyperelasticity_residual(bp5_mf *mf, const double *coef, double *state, double lambda, double mu, size_t ld, const double *u, double *r, int zero_dst);
/* dst = [0 +] T(state) src, the tangent at the stored state; dst_c = src_c on Dirichlet DoFs.  ONE launch of
 * apply_pencil_hyperelasticity_kernel<.., tangent>.  (replaces CEED solids' ElasFSInitialNH1F_dF Jacobian QFunction; deal.II step-44's tangent matrix
 * assembly, applied matrix-free as in step-72) */
int bp5_hyperelasticity_apply(bp5_mf *mf, const double *coef, const double *state, double lambda, double mu, size_t ld, const double *src, double *dst, int zero_dst);
/* dst += T(state) src over the cells [cell_begin, cell_end) (any range, also ragged against the kernel's teams; empty: nothing is launched); no
 * zero-fill, no Dirichlet step: the contract of bp5_elasticity_apply_cells.  (replaces one colour of MatrixFree::cell_loop on the tangent) */
int bp5_hyperelasticity_apply_cells(bp5_mf *mf, const double *coef, const double *state, double lambda, double mu, size_t ld, const double *src, double *dst,
                                    uint32_t cell_begin, uint32_t cell_end);
/* SolverCG on T(state) x = b: the BP5_CG_PLAIN recurrence of bp5_cg_solve_elasticity_preconditioned with the tangent as operator step.  precond ==
 * NULL: identity; otherwise any bp5_vmult_fn on three-block vectors of this ld -- intended: bp5_chebyshev_vmult / bp5_mg_vmult with handles of
 * bp5_elasticity_chebyshev_create / bp5_elasticity_mg_create on the same handle and ld, i.e. the LINEAR operator as preconditioner of the tangent.
 * Stop rule, check_every, breakdown status and result fields as there (dot_products_fused == 0); BP5_CG_MERGED: BP5_ERR_UNSUPPORTED.
 * (replaces the linear solve inside CEED solids' SNES / step-44's solve_linear_system) */
int bp5_cg_solve_hyperelasticity(bp5_mf *mf, const double *coef, const double *state, double lambda, double mu, size_t ld, bp5_vmult_fn precond, void *precond_ctx,
                                 const double *b, double *x, const bp5_cg_params *params, bp5_cg_result *result_host);

/* Newton's method with backtracking on F_int(u) = f_ext (replaces CEED solids' SNES with a line search; deal.II step-44's solve_nonlinear_timestep).
 * From the given u (Dirichlet values as prescribed; they stay):
 *   r = f_ext - F_int(u), Dirichlet rows 0;   stop on ||r|| <= max(abs_tol, rel_tol ||r_0||);
 *   T(state) delta = r by bp5_cg_solve_hyperelasticity with cg (its abs_tol is REPLACED by cg_rel_tol ||r||; a solve that ends at cg.max_iter is used
 *   as it is) and the given preconditioner;
 *   u_new = u + alpha delta, alpha = 1, halved while the new ||r|| is non-finite or not smaller than the old (at most max_backtracks halvings);
 *   the accepted residual has refilled the state.
 * Synchronous; ONE norm per residual (the stacked l2 norm over the owned entries of all blocks).  residual_history[k]: ||r|| after k steps (k = 0:
 * the start), the first 32.  status / return value: BP5_OK, BP5_ERR_NO_CONVERGENCE after max_newton steps (u: the last accepted iterate),
 * BP5_ERR_BREAKDOWN when backtracking is exhausted (u: the last accepted iterate, the state refilled for it), the inner solve breaks down or the residual of the start vector is not finite.
 * The work vectors (delta, the trial u and r: 9 ld doubles) belong to the handle.  Refusals: those of bp5_cg_solve_hyperelasticity; max_newton < 0,
 * max_backtracks < 0, a negative or non-finite tolerance, u overlapping f_ext: BP5_ERR_INVALID. */
typedef struct {
  int max_newton;
  double abs_tol, rel_tol;
  bp5_cg_params cg;
  double cg_rel_tol;
  int max_backtracks;
} bp5_newton_params;
typedef struct {
  int newton_iterations;        /* accepted steps */
  int total_cg_iterations;
  double residual_history[32];
  int backtracks;               /* halvings of alpha over all steps */
  int status;                   /* the return value */
} bp5_newton_result;
int bp5_hyperelasticity_newton(bp5_mf *mf, const double *coef, double *state, double lambda, double mu, size_t ld, bp5_vmult_fn precond, void *precond_ctx,
                               const double *f_ext, double *u, const bp5_newton_params *params, bp5_newton_result *result_host);

/* BP5_CG_MERGED on the packed block kernel (cell bricks, one rank's cells, diag == NULL): by default the operator's
 * write-out and combine pass also form the v-dependent dot products of update_b (bp5/solver.h:142-311: p.v, v.v, r.v, r.r)
 * and write the Dirichlet rows, so the separate pass over p, r, v and the copy_constrained launch disappear.  Same
 * arithmetic, different summation order (still fixed: bitwise reproducible).  BP5_CG_PLAIN on that kernel takes d.h (its one
 * dot product with the operator's result; any diag) from it the same way: the sum over the cells of the quadrature-point
 * energy, so the pass over d and h disappears.  0 switches back to the separate kernels. */
int bp5_mf_set_cg_fusion(bp5_mf *mf, int on);

/* cg.solve(A, x, b, preconditioner) with ANY preconditioner: z = P g is the caller's callback (bp5_vmult_fn shape: enqueue
 * dst = P src on the handle's stream, every owned entry of dst defined, ghost ranges usable as scratch).  A is the library's
 * operator (coef, vmult == NULL) or any operator through its callback (vmult != NULL; coef then ignored).  BP5_CG_PLAIN only
 * (BP5_CG_MERGED: BP5_ERR_INVALID -- its recurrence has no place for a preconditioner application).  Per iteration: h = A d,
 * d.h, x += alpha d, g += alpha h, z = P g, g.g and g.z in ONE all-reduce, d = beta d - z.  The preconditioner runs in every
 * iteration the host enqueues (up to the host's look at the convergence flag); once the device has stopped the solve its output
 * is ignored, so the result is bitwise the same for every check_every.  Neither the operator nor the preconditioner is gated on the
 * device's stop flag, so with check_every = 0 the host looks at the flag itself, two iterations behind the work it has enqueued (an
 * asynchronous copy per iteration; the queue never drains): at most two iterations' applications run after convergence, never max_iter.
 * precond may be bp5_chebyshev_vmult with its handle. */
int bp5_cg_solve_preconditioned(bp5_mf *mf, const double *coef, bp5_vmult_fn vmult, void *ctx, bp5_vmult_fn precond, void *precond_ctx,
                                const double *b, double *x, const bp5_cg_params *params, bp5_cg_result *result_host);

/* ------------------------------------------------------------------------------------------ */
/* PreconditionChebyshev<Operator, Vector, DiagonalMatrix> (deal.II): a Chebyshev polynomial in D^-1 A with D^-1 = inv_diag
 * (NULL: identity), on the spectrum bounds [min_used, max_used] of D^-1 A, theta / delta = their midpoint / half-width:
 *   vmult (dst = P src, x_0 = 0):   x_1 = D^-1 src / theta;
 *                                   x_{k+1} = x_k + f1_k (x_k - x_{k-1}) + f2_k D^-1 (src - A x_k),  k = 1 .. degree-1,
 *                                   rho_0 = delta / theta, rho_k = 1 / (2 theta / delta - rho_{k-1}), f1_k = rho_k rho_{k-1},
 *                                   f2_k = 2 rho_k / delta;   1 - lambda p(lambda) = T_degree((theta - lambda)/delta) / T_degree(theta/delta)
 *   step  (dst improved from its current value x_0): x_1 = x_0 + D^-1 (src - A x_0) / theta, then the same recurrence: degree operator
 *                                   applications.
 * Each step is ONE launch of a pointwise kernel (48 bytes per DoF: x, x_old, src, t = A x_k, diag read, x_new written into x_old's
 * buffer; 40 without diag); the scalars are kernel arguments (known on the host at create): vmult and step enqueue on the handle's
 * stream and never synchronise the host.  No dot product and no all-reduce: only the operator's halo exchanges.
 * The operator is applied in overwrite mode (zero_dst = 1, Dirichlet copy), with neighbours as bp5_apply_distributed; A is the
 * library's operator (coef, vmult == NULL) or any operator through its callback. */
typedef struct {
  int degree;              /* >= 1; degree 1 == dst = D^-1 src / theta (Jacobi); degree-1 operator applications per vmult       */
  double smoothing_range;  /* > 1: min_used = max_used / smoothing_range; <= 1: min_used = min(0.9 max_used, min_est)          */
  int eig_cg_n_iterations; /* CG-Lanczos steps of the estimate (deal.II default 8); the estimate stops early at ||r|| <= 1e-5 ||v|| */
  double max_eigenvalue, min_eigenvalue; /* both > 0: used as given (min_used, max_used), no estimate                          */
  const uint64_t *start_ids_host; /* [n_owned] global DoF ids (bp5_mesh_view.global_ids_host) for the estimate's start vector
                                     v_i = (id mod 11) - 5 (0 on Dirichlet DoFs): the same vector on every rank count; NULL = the
                                     local index                                                                              */
} bp5_chebyshev_params;
typedef struct bp5_chebyshev bp5_chebyshev;
/* Setup (synchronous): unless both bounds are given, Jacobi-PCG (D^-1 = inv_diag) on A x = v, x_0 = 0, eig_cg_n_iterations steps,
 * its alpha / beta history copied to the host once at the end; Lanczos tridiagonal T_kk = 1/alpha_k + beta_{k-1}/alpha_{k-1},
 * T_{k,k+1} = sqrt(beta_k)/alpha_k; min_est / max_est = its extreme eigenvalues; max_used = 1.2 max_est.  Dot products are
 * all-reduced when a communicator is set.  inv_diag must stay valid for the life of the handle. */
int bp5_chebyshev_create(bp5_mf *mf, const double *coef, bp5_vmult_fn vmult, void *ctx, const double *inv_diag,
                         const bp5_chebyshev_params *params, bp5_chebyshev **out);
int bp5_chebyshev_eigenvalues(const bp5_chebyshev *c, double *min_est, double *max_est, double *min_used, double *max_used, int *cg_its);
int bp5_chebyshev_vmult(void *c, double *dst, double *src);          /* bp5_vmult_fn shape: dst = P src, dst's prior content ignored */
int bp5_chebyshev_step(bp5_chebyshev *c, double *dst, double *src);  /* smoother: dst improved from its current value              */
int bp5_chebyshev_destroy(bp5_chebyshev *c);
/* PreconditionChebyshev<ElasticityOperator, BlockVector, DiagonalMatrix> (deal.II step-8's operator under step-37's smoother): the same polynomial
 * for the elasticity operator of bp5_elasticity_apply (coef: its ten planes; lambda, mu by value) on three-block vectors ld apart.  inv_diag: a
 * BLOCK inverse diagonal as bp5_elasticity_compute_diagonal(..., invert = 1) returns it (three blocks ld apart), or NULL = identity; it must stay
 * valid for the life of the handle.  The result is an ordinary bp5_chebyshev: bp5_chebyshev_vmult, _step, _eigenvalues and _destroy take it, its
 * vectors are then three-block vectors of the ld given here (entries [n_owned + n_ghost, ld) never read, never written); each step is ONE launch of
 * the pointwise kernel (chebyshev_step_kernel: the component is the second grid dimension; a scalar handle launches it with one) and one
 * bp5_elasticity_apply.  The estimate is Jacobi-PCG on the stacked system (one Krylov space, the block diagonal) from the start vector
 * v_c[i] = ((3 id_i + c) mod 11) - 5, 0 on Dirichlet DoFs, id from params->start_ids_host (NULL: the local index).  Refusals: those of
 * bp5_elasticity_apply (bp5_last_error names "elasticity"), and bp5_chebyshev_create's on params. */
int bp5_elasticity_chebyshev_create(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, const double *inv_diag,
                                    const bp5_chebyshev_params *params, bp5_chebyshev **out);
/* all eigenvalues of the symmetric tridiagonal matrix (diag[n], offdiag[n-1]), ascending; Sturm-sequence bisection on the host
 * (no LAPACK, no GPU) */
int bp5_tridiagonal_eigenvalues(int n, const double *diag, const double *offdiag, double *eig_ascending_host);

/* ------------------------------------------------------------------------------------------ */
/* p-multigrid: deal.II MGTwoLevelTransfer (matrix-free global-coarsening transfer), Multigrid and PreconditionMG with Chebyshev
 * smoothers (step-37), coarsening in the polynomial degree on the same cells.
 *
 * Transfer between a fine handle of degree pf >= 2 and a coarse handle of degree pc = max(1, pf / 2) on the SAME cells in the same
 * order AND the same local frames (two bp5_mesh_create_brick meshes that differ only in degree, or two user meshes whose cell c lists
 * its entries along the same three axes in both), the same communicator and stream.  Checked at create (BP5_ERR_INVALID, the reason
 * names the first offending cell): the cells' corner DoFs pair up one to one, and corner (i, j, k) of every cell has the same coordinates
 * in both handles to 1e-12 of the cell's size -- the pairing alone cannot tell a column of cells that one handle lists turned about its
 * axis.  M[a][b] = phi_b^pc(xi_a^pf) (FE_Q nodes of bp5_shape_tables; its end rows exact unit vectors); P = M x M x M cell by cell,
 * with the coarse Dirichlet DoFs taken as 0:
 *   prolongate_add  dst_f += P src_c: each cell interpolates its coarse values to its fine nodes; every owned fine DoF is written by ONE
 *                   cell (the first in handle order that holds it): no atomics, no race.  With neighbours the coarse ghosts are gathered
 *                   first (src_c's ghost range is written); dst_f's ghost range is not touched.
 *   restrict_add    dst_c += P^T src_f, Dirichlet rows of dst_c unchanged: each cell forms M^T x M^T x M^T of w (.) src_f, w = 1 / (number
 *                   of cells that hold the DoF, counted over all ranks at create), into a slot array; one combine pass sums the slots of
 *                   each coarse DoF in cell order (bitwise reproducible).  With neighbours: src_f's ghosts gathered first, dst_c's ghost
 *                   range sent to its owners and added (then zeroed).
 * Conforming meshes only (a handle with hanging-node masks: BP5_ERR_INVALID).  Vectors: owned + ghost storage of their handle.
 * Create is synchronous; the applications enqueue on the handles' stream. */
typedef struct bp5_mg_transfer bp5_mg_transfer;
int bp5_mg_transfer_create(bp5_mf *fine, bp5_mf *coarse, bp5_mg_transfer **out);
int bp5_mg_transfer_prolongate_add(bp5_mg_transfer *t, double *dst_fine, double *src_coarse);
int bp5_mg_transfer_restrict_add(bp5_mg_transfer *t, double *dst_coarse, double *src_fine);
int bp5_mg_transfer_destroy(bp5_mg_transfer *t);
/* The same transfers on block vectors (MGTwoLevelTransfer<dim, BlockVector>: prolongate_and_add / restrict_and_add block by block), on the SAME
 * scalar transfer handles, p-transfers and geometric ones: index lists, writer masks and weights are per scalar DoF and shared by all components.
 * Component c of the fine vector at v + c * ld_fine, of the coarse vector at v + c * ld_coarse (layout as for bp5_apply_components: each ld even and
 * >= n_owned + n_ghost of its level, bases 16-byte aligned, entries [n_owned + n_ghost, ld) never read, never written).  ONE launch per direction
 * serves all components (mg_prolongate_kernel and mg_combine_kernel, the kernels of the scalar entries, which launch them with one component;
 * mg_restrict_components_kernel, the block form of the scalar entries' mg_restrict_kernel): a thread reads its index, writer-mask bit and weight
 * once and runs the components one after the other through the same LDS tile; per component the floating-point operations and their order do not
 * depend on the component count, and are those of the scalar restriction kernel, so every block holds the bits
 * bp5_mg_transfer_prolongate_add / _restrict_add give on that block alone.  Slots are [component][cell][(pc+1)^3]; a call with more components than any before it on the handle grows them
 * (bp5_elasticity_mg_create reserves three).  n_components: 1 .. BP5_MAX_COMPONENTS.  Refused before any launch -- BP5_ERR_INVALID: null pointer,
 * n_components out of range, an odd or too small ld, a misaligned base; BP5_ERR_UNSUPPORTED: a transfer whose handles have a communicator and
 * neighbours (no block halo exchange here). */
int bp5_mg_transfer_prolongate_add_components(bp5_mg_transfer *t, int n_components, size_t ld_fine, double *dst_fine, size_t ld_coarse, double *src_coarse);
int bp5_mg_transfer_restrict_add_components(bp5_mg_transfer *t, int n_components, size_t ld_coarse, double *dst_coarse, size_t ld_fine, double *src_fine);

/* Geometric (h) transfer at one degree p in 1..4 (deal.II MGTwoLevelTransfer::reinit_geometric_transfer, step-75's h-levels): the
 * coarse handle's cells are the parents of the fine handle's, 8 children each (bp5_mesh_parent_cells gives the map: parent_cell_host[k],
 * child_host[k] = cx | cy << 1 | cz << 2 of fine cell k).  M_s[a][b] = phi_b^p(xi_a / 2 + s / 2), s = 0, 1, on the FE_Q nodes of
 * bp5_shape_tables; rows where a fine node coincides with a coarse node are exact unit rows.  Fine cell k interpolates its parent's
 * coarse values with M_cx x M_cy x M_cz.  Everything else is the p-transfer's scheme above: prolongate_add writes each owned fine DoF
 * from one cell (writer mask); restrict_add forms w (.) src_f (w = 1 / cells holding the DoF, all ranks) per fine cell into slots that
 * one combine pass sums in cell order (no atomics, bitwise reproducible); coarse Dirichlet DoFs are read as 0 and get no slots; the same
 * halo gather and scatter-add with neighbours.  The handle works with bp5_mg_transfer_prolongate_add / _restrict_add / _destroy and
 * in bp5_mg_create chains (mixed with p-transfers).  Device data: one Dirichlet-masked coarse index list per coarse cell and one
 * 32-bit word per fine cell (parent << 3 | child).  Checked at create (BP5_ERR_INVALID): equal degrees in 1..4; same communicator,
 * stream and device; no hanging-node masks; every coarse cell has exactly 8 children with distinct child codes and every parent index
 * is a local coarse cell; the fine corner each child shares with its parent has the parent's corner coordinates to 1e-12 of the
 * parent's size (catches a wrong map).  Create is synchronous. */
int bp5_mg_transfer_create_geometric(bp5_mf *fine, bp5_mf *coarse, const uint32_t *parent_cell_host, const uint8_t *child_host,
                                     bp5_mg_transfer **out);

/* PreconditionMG: one symmetric V-cycle per vmult.  Levels fine (0) to coarse (n_levels - 1), mfs[l] / coefs[l] the level's handle and
 * merged metric, transfers[l] between level l and l + 1 (n_levels - 1 of them; p-transfers and geometric transfers in any mix, e.g.
 * step-75's p = 4, 2, 1 on the fine cells, then p = 1 on cells / 2, cells / 4).  At create every level gets its inverse diagonal
 * (bp5_compute_diagonal) and a Chebyshev-Jacobi polynomial (bp5_chebyshev_create: smoother_degree on [max_used / smoothing_range,
 * max_used]; the coarsest level: coarse_degree on [max_used / coarse_range, max_used], a fixed polynomial, so the cycle is a fixed
 * symmetric linear operator as CG needs).  vmult (dst = V src, dst's prior content ignored), level l from x_l = 0:
 *   l = coarsest:  x_l = coarse polynomial (src_l)
 *   else           x_l = smoother vmult (src_l)                       pre-smoothing from zero
 *                  src_{l+1} = P^T (w (.) (src_l - A_l x_l)), Dirichlet rows 0   (fused: the fine residual is never stored)
 *                  x_{l+1} = V_{l+1}(src_{l+1}); x_l += P x_{l+1}; x_l = smoother step (x_l, src_l)   post-smoothing
 * Everything is enqueued on the fine handle's stream (all handles share it): no host synchronisation and no all-reduce; the halo
 * exchanges of the levels run one after the other on the one communicator. */
typedef struct {
  int smoother_degree;         /* default 4                                                                                  */
  double smoothing_range;      /* default 20                                                                                 */
  int eig_cg_n_iterations;     /* CG-Lanczos steps of each smoother's estimate (default 10)                                  */
  int coarse_degree;           /* Chebyshev degree of the coarse solver (default 60)                                         */
  double coarse_range;         /* its max_used / min_used (default 1000)                                                     */
  int coarse_eig_cg_n_iterations; /* CG-Lanczos steps of the coarse estimate (default 30)                                   */
  const uint64_t *const *start_ids_host; /* [n_levels] per level the global DoF ids of the owned DoFs (bp5_chebyshev_params); NULL:
                                            the local index                                                                  */
} bp5_mg_params;
typedef struct {
  int n_levels, degree;
  uint32_t n_owned;            /* owned DoFs of this rank on the level                                                      */
  double min_est, max_est, min_used, max_used; /* the level's Chebyshev estimate and the bounds its polynomial uses            */
  int cg_its, chebyshev_degree;
} bp5_mg_level;
typedef struct bp5_mg bp5_mg;
void bp5_mg_params_default(bp5_mg_params *params);
int bp5_mg_create(int n_levels, bp5_mf *const *mfs, const double *const *coefs, bp5_mg_transfer *const *transfers, const bp5_mg_params *params,
                  bp5_mg **out);
/* PreconditionMG for the elasticity operator (deal.II step-8's operator under step-37 / step-75's hybrid multigrid): the V-cycle above, step for
 * step, on three-block vectors.  mfs[l] / coefs[l]: the level's handle and its TEN elasticity planes (bp5_elasticity_compute_metric); lambda, mu the
 * same on every level; transfers[l]: the scalar transfer handles between the levels (p-transfers and geometric ones in any mix), used through
 * bp5_mg_transfer_*_components; ld: the stride of the level-0 vectors bp5_mg_vmult will see (level vectors below have their own even ld).  Every
 * level gets its three inverse diagonals (bp5_elasticity_compute_diagonal) and a polynomial of bp5_elasticity_chebyshev_create; the residual
 * restriction is fused (b - A x is never stored); nothing allocates inside vmult.  The result is an ordinary bp5_mg for bp5_mg_vmult (three-block
 * vectors of this ld), bp5_mg_level_info and bp5_mg_destroy.  Refused before any launch, bp5_last_error names "elasticity": everything
 * bp5_elasticity_apply refuses, for every level; levels on different streams (BP5_ERR_INVALID, "stream"); a level without Dirichlet DoFs
 * (BP5_ERR_UNSUPPORTED, "Dirichlet": the coarse polynomial is no solver for a singular level). */
int bp5_elasticity_mg_create(int n_levels, bp5_mf *const *mfs, const double *const *coefs, double lambda, double mu, size_t ld,
                             bp5_mg_transfer *const *transfers, const bp5_mg_params *params, bp5_mg **out);
int bp5_mg_vmult(void *mg, double *dst, double *src); /* bp5_vmult_fn shape: plugs into bp5_cg_solve_preconditioned */
int bp5_mg_level_info(const bp5_mg *mg, int level, bp5_mg_level *out);
int bp5_mg_destroy(bp5_mg *mg);

/* event helpers so a host in another language can time on the handle's stream */
typedef struct bp5_event bp5_event;
int bp5_event_create(bp5_event **out);
int bp5_event_record(bp5_mf *mf, bp5_event *ev);
int bp5_event_elapsed_ms(bp5_event *start, bp5_event *stop, double *ms_host); /* synchronises on stop */
int bp5_event_destroy(bp5_event *ev);

#ifdef __cplusplus
}
#endif
#endif /* BP5_H */
