// Shared by the device translation units of libbp5, in this order: the handle (bp5_mf); what an apply variant number means (decode_variant) and
// what one operator application carries (ApplyCall); one launcher per kernel family (launch_apply_t: pencil, launch_apply_components_t,
// launch_block_t, launch_team_t, launch_march_t), which share apply_args and zero_dst; the list of builds of the default block kernel and its
// resolver (DefaultBlockBuilds, launch_block_default: variant 56 of every operator class); and the per-degree dispatch apply_degree_impl.
// bp5_device.hip holds the C ABI; bp5_apply_pN.hip instantiate apply_degree_impl<N> and apply_components_degree_impl<N> (one translation unit
// per degree so that `make -j` compiles them side by side).
#pragma once
#include "bp5_internal.hpp"
#include "bp5_kernels.hpp"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <tuple>
#include <vector>

using namespace bp5;

#define HIP_TRY(expr)                                                                                              \
  do {                                                                                                             \
    hipError_t e_ = (expr);                                                                                        \
    if (e_ != hipSuccess)                                                                                          \
      return fail(e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice ? BP5_ERR_NO_DEVICE : BP5_ERR_HIP,         \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                                              \
  } while (0)
#define NCCL_TRY(expr)                                                                                             \
  do {                                                                                                             \
    ncclResult_t r_ = (expr);                                                                                      \
    if (r_ != ncclSuccess) return fail(BP5_ERR_RCCL, std::string(#expr) + ": " + ncclGetErrorString(r_));         \
  } while (0)
#define BP5_TRY(expr)                                                                                              \
  do {                                                                                                             \
    int s_ = (expr);                                                                                               \
    if (s_ != BP5_OK) return s_;                                                                                   \
  } while (0)
#define KERNEL_CHECK() HIP_TRY(hipGetLastError())

struct bp5_comm {
  ncclComm_t comm = nullptr;
  int rank = 0, n_ranks = 1;
};
struct bp5_event {
  hipEvent_t ev = nullptr;
};

constexpr size_t STREAMING_MAX_DOFS = 24000000; // see bp5_mf_set_streaming (include/bp5.h)
struct bp5_mf {
  int degree = 0, quadrature = 0, coefficient = 0, n = 0, n3 = 0, device = 0;
  // quadrature points per direction and per cell: n and n3 but on a BP5_QUAD_GAUSS_OVER handle (n + 1 points per direction), whose metric planes,
  // tables and kernels are its own (the bp5_overint unit): Poisson and mass operator, pencil kernels, conforming mesh, six double planes or one
  int nq = 0, nq3 = 0;
  bool overint() const { return quadrature == BP5_QUAD_GAUSS_OVER; }
  uint32_t n_cells = 0, n_interior = 0, n_owned = 0, n_ghost = 0, n_constrained = 0;
  int apply_variant = 0, n_cus = 0, geometry_mode = 0, march_max_steps = 32;
  int operator_kind = 0; // BP5_OP_POISSON | BP5_OP_HELMHOLTZ (seven planes: six merged + the mass plane a JxW) | BP5_OP_MASS (one plane: rho JxW)
  mutable int coef_planes_committed = 0; // planes of the metric array the caller has sized (bp5_mf_coef_size) or filled: set_operator may not change the count afterwards
  static int planes_of(int op) { return op == BP5_OP_HELMHOLTZ ? 7 : op == BP5_OP_MASS ? 1 : 6; }
  int n_planes() const { return planes_of(operator_kind); }
  // BP5_METRIC_F64 | BP5_METRIC_F32 (bp5_mf_set_metric_precision): entry type of the merged-metric planes behind every `coef` argument.  F32: the
  // same pair layout with float entries (coef_plane_stride / coef_cell_stride then count floats), read by the BLK_F32M builds of the pencil
  // and block kernel; fixed once the array has been sized or filled (coef_planes_committed)
  int metric_precision = BP5_METRIC_F64;
  bool f32_metric() const { return metric_precision == BP5_METRIC_F32; }
  int block_max_wg = 0; // 0: persistent grid sized from the CU count; > 0: cap (tests force several blocks per workgroup)
  int streaming = -1; // bp5_mf_set_streaming: -1 chosen by size, 0 ordinary accesses, 1 non-temporal accesses to once-used data
  int auto_team = -1;  // -1 not decided; 1: the x-row team plan could be built (p = 1, 3 default)
  int auto_block = -1; // -1 not decided; 1: the caller's cell blocks fit three block-kernel workgroups per CU
  double *d_scalar_plane = nullptr, *d_gcell = nullptr;
  double *d_vertices = nullptr; // BP5_GEOM_TRILINEAR: [n_cells][24], each cell's eight corners (bp5_mf_set_geometry_mode allocates it on first use)
  bool trilinear() const { return geometry_mode == BP5_GEOM_TRILINEAR; }
  hipStream_t stream = nullptr;
  bool own_stream = false;
  Tables tab, tab_gauss;
  // device arrays
  uint32_t *d_l2g = nullptr, *d_constrained = nullptr, *d_send_idx = nullptr;
  uint32_t *d_constrained_bits = nullptr; // bit i: DoF i is a Dirichlet DoF (owned range; the solver's dot-product kernel applies the copy)
  double *d_coords = nullptr, *d_tab = nullptr, *d_tab_gauss = nullptr;
  // Data mirror (lazy)
  uint32_t *d_l2g_padded = nullptr, *d_constraint_mask = nullptr;
  // hanging nodes (2:1 refinement): per-cell masks and the two 1-D interpolation matrices [2][n*n]; has_hanging: some mask != 0
  // layout of the six metric planes: plane-major [c][cell][q] (round 1) or cell-major [cell][c][q] (one contiguous 48 n^3-byte chunk per cell)
  uint64_t coef_plane_stride = 0, coef_cell_stride = 0;
  bool has_hanging = false;
  uint32_t *d_hang_mask = nullptr;
  double *d_hang_I = nullptr;
  double *d_inv_jac = nullptr, *d_JxW = nullptr, *d_qpoints = nullptr;
  uint32_t pad = 0;
  // halo plan
  std::vector<int> neighbors;
  std::vector<uint32_t> send_off, recv_off;
  double *d_sendbuf = nullptr, *d_recvbuf = nullptr;
  uint8_t *d_send_dirichlet = nullptr; // per send index: the owner DoF is a Dirichlet DoF
  bp5_comm *comm = nullptr;
  // halo exchange on its own stream (overlap with interior cells): created on first use
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_halo[4] = {nullptr, nullptr, nullptr, nullptr}; // packed / gathered / ghosts ready / received
  int overlap = 2;            // MatrixFree::AdditionalData::overlap_communication_computation (bp5/step-64.cu:241): 0 off, 1 on, 2 auto
  bool overlap_now = false;   // the decision for the exchange in flight (set by *_start)
  bool cg_fusion = true;      // SolverCGFullMerge: dot products inside the block kernel's write-out when the plan allows
  // ApplyCall::signal: a block launch counts the workgroups whose first part is written out at *d_signal (monotonic: signal_target = the
  // count after the last launch), so that the communication stream can wait for the ghost rows mid-kernel
  unsigned long long *d_signal = nullptr;
  uint64_t signal_target = 0;
  int wait_value_ok = -1;     // -1 not probed; 1: hipDeviceAttributeCanUseStreamWaitValue AND the producer / consumer self-check saw a mid-kernel release
  int can_wait_value = -1;    // wait_value_ok and not switched off by BP5_TUNE_BOUNDARY_FIRST = 0
  // per-handle tuning / A-B knobs (bp5.h: BP5_TUNE_*): initial values from the environment, read once by bp5_mf_create
  int tune[BP5_TUNE_COUNT] = {1, 1, 0, 1, 1, 1, 1, -1, 16, 1, 0, 1, -1};
  bool cell_interiors_first = false; // the mesh numbers the DoFs strictly inside a cell ahead of all others, cell after cell, x fastest (bp5_mesh_desc.dof_numbering = 2)
  // solver workspace
  double *d_partials = nullptr, *d_sc = nullptr, *d_scalar = nullptr;
  int *d_st = nullptr;
  double *ws_g = nullptr, *ws_d = nullptr, *ws_h = nullptr, *d_evec = nullptr;
  char *ws_base = nullptr;
  double *ws_z = nullptr;     // preconditioner output of bp5_cg_solve_preconditioned (allocated on first use)
  double *wsc_base = nullptr; // bp5_cg_solve_components: g, d, h as block vectors (3 n_components ld doubles), grown on demand
  size_t wsc_cap = 0;         // ... doubles allocated
  double *wsz_base = nullptr; // bp5_cg_solve_elasticity_preconditioned: z = P g as a block vector (n_components ld doubles), grown on demand
  size_t wsz_cap = 0;
  double *wsn_base = nullptr; // bp5_hyperelasticity_newton: delta, the trial u and r as block vectors (9 ld doubles), grown on demand
  size_t wsn_cap = 0;
  // halo exchange of block vectors: four staging buffers in one allocation, grown on demand -- gather send / scatter receive (n_components
  // send_off.back() doubles each), gather receive / scatter send (n_components n_ghost each); a neighbour's message is contiguous and holds
  // all components, [neighbour][component][entry].  d_hc_off: send_off, then recv_off, for the kernels that place an entry in its message
  double *hc_base = nullptr;
  size_t hc_cap = 0;
  uint32_t *d_hc_off = nullptr;
  // bp5_cg_solve_preconditioned with check_every = 0: the stop flag of iteration k copied to h_done[k % 3] behind ev_done[k % 3]
  int *h_done = nullptr; // pinned
  hipEvent_t ev_done[3] = {nullptr, nullptr, nullptr};
  unsigned long long *d_stamps = nullptr;
  double *h_sc = nullptr; // pinned
  int *h_st = nullptr;    // pinned
  std::vector<hipEvent_t> ev_pool;
  hipEvent_t ev_solve[2] = {nullptr, nullptr}; // start / stop of a solve (owned by the handle: no leak on error paths)
  char last_apply_kernel[96] = ""; // the operator kernel launched last, named as a profiler prints it (bp5_cg_result.apply_kernel)
  // profile == 2: stamps at the phase boundaries of every merged-CG iteration (bp5_cg_result.phase_ms); the events are a cache, which of
  // them a solve recorded is the solve's own business (SolveState)
  struct PhaseProfile {
    static constexpr int MARKS = 8, MAX_ITERS = 64;
    std::vector<hipEvent_t> ev;   // [MAX_ITERS][MARKS]
  } phase;
  // team plans of the team-assembled kernel, keyed by cells per team
  std::vector<uint32_t> h_l2g;
  struct DevPlan {
    uint32_t *off = nullptr, *dofs = nullptr, *sh_dof = nullptr, *sh_off = nullptr, *sh_slot = nullptr;
    uint16_t *pos = nullptr;
    uint8_t *cell_round = nullptr, *team_rounds = nullptr;
    double *partial = nullptr;
    uint32_t *cell_off = nullptr, *pass_cell = nullptr, *pass_off = nullptr, *run_off = nullptr, *runs = nullptr, *gidx = nullptr;
    uint16_t *packed = nullptr;
    // lattice form of the packed indices (structured bricks: every cell-local DoF's list slot and DoF follow in closed form from the cell's
    // position in its brick -- no per-DoF index stream at all): per block 64 words (bp5_kernels.hpp: BLOCK_LATTICE_WORDS), per cell its position
    uint32_t *lattice = nullptr;
    uint16_t *cell_pos = nullptr;
    uint32_t n_lattice_blocks = 0;
    // fused vector update (BP5_TUNE_FUSED_UPDATE): the interior runs of the lattice blocks are disjoint, cover exactly the DoFs [0, upd_n_int),
    // hold no Dirichlet DoF and nothing another block touches (get_plan_raw: interior_runs_cover); 0: the plan does not qualify
    uint32_t upd_n_int = 0;
    std::vector<double> h_cost;                       // [n_groups+1] prefix sum of the estimated cost of the blocks (pass units)
    // block ranges of the persistent workgroups, one device array per (n_wg, first block, end block) ever launched: the
    // interior / boundary ranges of the overlapped schedule alternate, nothing is freed or re-uploaded inside a solve
    std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>, uint32_t *> *wg_blocks = nullptr; // key: n_wg, first, end, first block of part 0 (0: one part)
    uint32_t *cr_start = nullptr, *cr_dof0 = nullptr, *cr_soff = nullptr, *cr_slots = nullptr, *cr_tile = nullptr; // run-length combine
    // face carry (BP5_TUNE_FACE_CARRY; bp5_kernels.hpp: BLOCK_CARRY_MAX): which faces stay in LDS depends on the workgroups' block ranges, so the
    // combine tables WITHOUT the carried faces are kept per partition (the key of wg_blocks); a block launch hands the tables its combine
    // pass must use to its caller (ApplyCall::combine_tables).  cr_last_launch: the same pointer kept for bp5_mf_block_plan_carry to report
    // (NULL: the plan's own, every shared DoF) -- a diagnostic, no launch reads it
    struct CombineTables { uint32_t *start = nullptr, *dof0 = nullptr, *soff = nullptr, *slots = nullptr, *tile = nullptr; uint32_t n_shared = 0, n_shared_owned = 0; };
    std::vector<uint32_t> h_cr_start, h_cr_dof0, h_cr_soff, h_cr_slots; // host form of cr_* (runs, not DoFs: small)
    std::vector<uint32_t> h_carry_dof, h_carry_len;                      // [n_groups] first DoF / DoF count of the face block g can hand to block g + 1 (0: none)
    std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>, CombineTables> *cr_carry = nullptr;
    const CombineTables *cr_last_launch = nullptr;
    uint32_t n_shared = 0, n_groups = 0, max_list = 0, max_runs = 0;
    uint32_t n_shared_owned = 0; // shared DoFs are listed in ascending order: ordinals [0, n_shared_owned) are owned DoFs, the rest ghosts
    bool covers_all = false;
  };
  std::vector<bool> h_constrained;   // per local DoF: Dirichlet DoF (run tables carry the flag)
  std::vector<uint32_t> h_block_off; // caller-provided cell blocks (may be empty)
  struct DevMarch { uint32_t *team_off = nullptr, *entries = nullptr; uint32_t n_teams = 0; };
  std::map<int, DevMarch> march_plans; // keyed by cells per team
  std::map<int, DevPlan> plans;
  size_t n_local() const { return (size_t)n_owned + n_ghost; }
  bool has_neighbors() const { return comm && !neighbors.empty(); } // operator applications carry the halo exchange (tests: a self neighbour)
};

// Fused CG dot products (SolverCGFullMerge on the block kernel) of ONE operator application: the solver owns it, the launches advance it
struct FuseState {
  const double *p = nullptr, *r = nullptr;
  uint32_t n_cols = 0;        // columns of d_partials written so far (block kernel workgroups, then the combine pass, then the unpack kernels)
  bool ghosts_zeroed = false; // the exchange's unpack kernel has zeroed the ghost ranges of v and p
  // the launch also applies the merged solver's vector update to the brick interiors (BLK_UPD; cg_solve_merged decided that the plan qualifies)
  int upd_mode = 0;           // 0: no; 1 / 2: cgm_update_one<1 / 2>
  double *upd_x = nullptr;
  const double *upd_diag = nullptr;
};
// What an apply variant number means (include/bp5.h: bp5_mf_set_apply_variant), the ONE place that knows the ranges: 1xx = variant xx with the
// global-atomic scatter, 0-6 pencil shapes, 10-14 team kernel, 48-63 block kernel (56 its default shape, the others A/B siblings and older shapes),
// 70-72 z-marching, 90 the pencil kernel of hanging-node meshes; anything else is a timing-only build (libbp5_timing.so) or unknown
enum VariantFamily { VARIANT_PENCIL, VARIANT_TEAM, VARIANT_MARCH, VARIANT_BLOCK, VARIANT_BLOCK_SIBLING, VARIANT_HANGING_PENCIL, VARIANT_OTHER };
struct VariantInfo {
  VariantFamily family;
  bool atomic_scatter;    // 1xx: the team kernel with the global-atomic scatter (A/B tests)
  bool shared_by_atomics; // 54 / 55: brick-surface DoFs by atomics
  bool csr_combine;       // 48: per-DoF CSR combine kernel instead of the run-length one
  bool overwrites;        // owner stores + combine pass define every entry of dst: no zero-fill needed (team and block kernels, not 1xx)
};
constexpr VariantInfo decode_variant(int v)
{
  const int b = v % 100;
  const VariantFamily f = b <= 6 ? VARIANT_PENCIL : b >= 10 && b <= 14 ? VARIANT_TEAM : b == 56 ? VARIANT_BLOCK : b >= 48 && b <= 63 ? VARIANT_BLOCK_SIBLING
                        : b >= 70 && b <= 72 ? VARIANT_MARCH : b == 90 ? VARIANT_HANGING_PENCIL : VARIANT_OTHER;
  return {f, v >= 100, b == 54 || b == 55, b == 48, v < 100 && (f == VARIANT_TEAM || f == VARIANT_BLOCK || f == VARIANT_BLOCK_SIBLING)};
}

// What ONE operator application is asked to do, and what its launches report back.  It lives on the caller's stack and travels by
// reference down launch_apply -> apply_degree_impl -> launch_*_t -> launch_combine: nothing of it is kept on the handle.
enum { EXCHANGE_NONE = 0, EXCHANGE_BOUNDARY_FIRST = 1, EXCHANGE_GHOST_ROWS_FIRST = 2 };
struct ApplyCall {
  uint32_t c0 = 0, c1 = 0;     // cell range
  bool overwrite = false;      // the launch must leave dst = A src (no prior zeroing by the caller); otherwise dst += A src
  // dst is all zero where this launch starts although overwrite is false: the caller (or the solver's update kernel) has just zero-filled it.  Builds
  // that STORE an entry instead of adding to it (PEN_INTERIOR_STORES) need overwrite or this; an accumulating call on the caller's dst has neither
  bool dst_known_zero = false;
  int variant = 0;             // resolved apply variant: launch_apply takes it from effective_variant(handle, range) ...
  bool keep_variant = false;   // ... unless the caller fixed it (phased applications: ONE kernel family for every range)
  // the switches a variant implies (decode_variant), for every degree and operator; their only readers are the p = 4 block / team launches and
  // the combine pass behind them (other degrees, Helmholtz and hanging-node meshes reject 48, 54, 55 before any launch).  csr_combine holds for
  // the immediate AND a deferred pass
  bool atomic_scatter = false, shared_by_atomics = false, csr_combine = false;
  void set_variant(int v)
  {
    const VariantInfo d = decode_variant(v);
    variant = v; atomic_scatter = d.atomic_scatter; shared_by_atomics = d.shared_by_atomics; csr_combine = d.csr_combine;
  }
  // block kernel
  uint32_t b0 = 0, b1 = 0;     // block range of [c0, c1) (0,0 = all blocks; filled in by the dispatch)
  bool combine_later = false;  // cell ranges: partial slab now, ONE combine pass (per window) launched by the caller after the last range
  // launches over ALL bricks of a slab with ghosts: two parts per workgroup (its share of the ghost-touching bricks, then its interior
  // bricks); signal: the launch counts the workgroups whose first part is written out (bp5_mf::d_signal)
  bool two_parts = false, signal = false;
  // fused dot products across ranks, where the exchange is enqueued: boundary-first -- the ghost-touching bricks run first, one combine pass
  // per window, the exchange travels under the interior bricks; ghost-rows-first -- all bricks in one launch, the ghost rows combined first,
  // the exchange under the owned-row combine
  int exchange = EXCHANGE_NONE;
  FuseState *fuse = nullptr;   // fused CG dot products (NULL: not fusing)
  hipEvent_t mark_event = nullptr; // profiling: recorded once before the combine pass (= end of the dominant kernel) ...
  bool mark_recorded = false;      // ... out: it was
  const bp5_mf::DevPlan::CombineTables *combine_tables = nullptr; // out: the tables the last block launch chose for its combine pass (NULL: the plan's own)
};

// Lanes per cell of the block-assembled kernel's default shape (one transpose tile per cell used field after field; when the lanes
// of a cell sit in one wave -- LPC divides 64 -- the tile exchanges are wave-local, else they use the workgroup barrier).
// Cells per pass = 256 / LPC.
// p = 2, 5, 8 (round 3): n^2 = 9 / 36 / 81 lanes per cell -- cells span waves, so the tile exchanges go through the workgroup barrier,
// but 28 / 7 / 3 cells share a pass and hardly a lane idles (round 2: 16 / 64 / 128 lanes per cell, 44 / 44 / 37 % idle).  Same-box A/B
// at the config-4 sizes (profiles/r3 i_*): p = 2 18.1 against 17.7 GDoF/s, p = 5 (6x4x2 bricks) 25.5 against 23.1, p = 8 23.2 against
// 19.7.  The macros are the A/B knobs (-DBP5_LPC_P2=16 -DBP5_LPC_P5=64 -DBP5_LPC_P8=128 rebuilds round 2's shapes).
#ifndef BP5_LPC_P2
#define BP5_LPC_P2 9
#endif
#ifndef BP5_LPC_P5
#define BP5_LPC_P5 36
#endif
#ifndef BP5_LPC_P8
#define BP5_LPC_P8 81
#endif
constexpr int block_lpc(int degree) { return degree == 1 ? 4 : degree == 2 ? BP5_LPC_P2 : degree == 3 ? 16 : degree == 4 ? 32 : degree == 5 ? BP5_LPC_P5 : degree == 6 || degree == 7 ? 64 : degree == 8 ? BP5_LPC_P8 : 0; }
inline int block_cpt(const bp5_mf *mf) { return block_lpc(mf->degree) ? 256 / block_lpc(mf->degree) : 8; }

template <typename T>
inline int upload(T **dptr, const T *host, size_t count)
{
  HIP_TRY(hipMalloc((void **)dptr, std::max<size_t>(count, 1) * sizeof(T)));
  if (count) HIP_TRY(hipMemcpy(*dptr, host, count * sizeof(T), hipMemcpyHostToDevice));
  return BP5_OK;
}

// defined in bp5_device.hip
// key > 0: uniform teams of `key` cells (team kernel); key < 0: cell blocks walked in passes of
// -key cells (block kernel) -- the caller's blocks if given, else groups of `default_block` cells
int get_plan_raw(bp5_mf *mf, int key, bp5_mf::DevPlan **dpo, int default_block = 64);
int get_plan(bp5_mf *mf, int cpt, bp5::TeamPlan &tp, bp5_mf::DevPlan **dpo);
// window: COMBINE_ALL every shared row; COMBINE_GHOST / COMBINE_OWNED only the rows of ghost / owned DoFs (the boundary-first exchange
// schedule completes the ghost rows before the interior bricks run); the windows need the run-length form of the pass
enum { COMBINE_ALL = 0, COMBINE_GHOST = 1, COMBINE_OWNED = 2, COMBINE_GHOST_THEN_OWNED = 3 }; // 3: one launch, ghost rows first + signal (fused solves)
// on_comm_stream: the pass runs on the communication stream (between a wait and the send) instead of the compute stream
int launch_combine(bp5_mf *mf, ApplyCall &call, bp5_mf::DevPlan *dp, double *dst, bool set, int window = COMBINE_ALL, bool on_comm_stream = false);
// combine tables of one workgroup partition without the faces its workgroups carry from brick to brick (wb: the block ranges as uploaded for the kernel)
int build_carry_tables(bp5_mf *mf, bp5_mf::DevPlan *dp, const std::vector<uint32_t> &wb, uint32_t n_wg, bool two_parts, bp5_mf::DevPlan::CombineTables *out);
// [c0,c1) == union of whole cell blocks [b0,b1) of the caller's blocking?
bool block_aligned(const bp5_mf *mf, uint32_t c0, uint32_t c1, uint32_t *b0, uint32_t *b1);
// CU count of the handle's device (cached; 0 if the query fails)
int device_cus(bp5_mf *mf);
// Non-temporal accesses to the data a CG iteration touches once (the operator's metric planes; v and x in the update kernel) keep it from evicting
// the vectors that ARE reused (p, r) from the 256 MB memory-side cache: a gain while those fit there (-6 % per iteration at 1e7 DoFs), a small loss
// beyond (+1 % at 1e8; profiles/r3/README.md, x_*)
inline bool streaming_accesses(const bp5_mf *mf) { return mf->streaming >= 0 ? mf->streaming != 0 : mf->n_local() <= STREAMING_MAX_DOFS; }

// ------------------------------------------------------------------------------------ operator launches
// 1-D tables as the kernels read them: the (anti)symmetric half of N and D (p <= 4), or their even-odd split (mv_even_odd)
template <int n>
inline void pack_even_odd(const double *M, bool anti, double *out)
{
  constexpr int c = (n + 1) / 2, h = n / 2, m = (n - 1) / 2;
  for (int q = 0; q < n; ++q)
    for (int i = 0; i < h; ++i) {
      const double E = 0.5 * (M[q * n + i] + M[q * n + n - 1 - i]), O = 0.5 * (M[q * n + i] - M[q * n + n - 1 - i]);
      if (q < c) out[q * h + i] = anti ? O : E;
      if (q < h) out[c * h + q * h + i] = anti ? E : O;
    }
  if (n & 1)
    for (int q = 0; q < c; ++q) out[c * h + h * h + q] = M[q * n + m];
}
template <int n>
inline void fill_shape(ShapeArg<n> &sh, const bp5_mf *mf)
{
  memcpy(sh.N, mf->tab.N, sizeof(sh.N));
  memcpy(sh.D, mf->tab.D, sizeof(sh.D));
  if constexpr (n >= EO_MIN_N) {
    pack_even_odd<n>(mf->tab.N, false, sh.N);
    pack_even_odd<n>(mf->tab.D, true, sh.D);
  }
}

// The over-integrated handle (BP5_QUAD_GAUSS_OVER), defined in overint/bp5_overint.hip -- a translation unit of its own, off the per-degree units:
// the operator (refuses every variant but the pencil kernel and every class but Poisson and mass), the planes, the diagonal (contributions of the
// cells; the caller has zeroed diag) and the permutation to the reference layout
int overint_apply(bp5_mf *mf, ApplyCall &call, const double *coef, const double *src, double *dst);
int overint_compute_metric(bp5_mf *mf, double *coef);
int overint_diagonal(bp5_mf *mf, const double *coef, double *diag);
int overint_to_reference_layout(bp5_mf *mf, const double *coef, double *coef_ref);
// the reason an over-integrated handle refuses something with (BP5_ERR_UNSUPPORTED)
inline int overint_refuse(const char *what) { return fail(BP5_ERR_UNSUPPORTED, std::string("Gauss(p+2) quadrature (BP5_QUAD_GAUSS_OVER): ") + what); }

// The trilinear handle (BP5_GEOM_TRILINEAR), defined in trilinear/bp5_trilinear.hip -- a translation unit of its own, off the per-degree units, in a
// directory of its own (its ISA is kept beside it): the operator (refuses every variant but the pencil kernel and every class but Poisson; reads no
// metric array), the setup launch (the cells' corners and the per-cell deviation from their trilinear image) and the diagonal (contributions of the
// cells; the caller has zeroed diag)
int trilinear_apply(bp5_mf *mf, ApplyCall &call, const double *src, double *dst);
int trilinear_setup(bp5_mf *mf, double *vertices, double *deviation);
int trilinear_diagonal(bp5_mf *mf, double *diag);
// the reason a trilinear handle refuses something with (BP5_ERR_UNSUPPORTED)
inline int trilinear_refuse(const char *what) { return fail(BP5_ERR_UNSUPPORTED, std::string("trilinear geometry mode (BP5_GEOM_TRILINEAR): ") + what); }

// Linear elasticity (bp5_elasticity_*), defined in elasticity/bp5_elasticity.hip -- a translation unit of its own, off the per-degree units, in a
// directory of its own (its ISA is kept beside it): the ten planes, the coupled three-component operator over the cells [c0, c1) (accumulates;
// an empty range launches nothing) and the cells' contributions to the three diagonals (the caller has zeroed diag).  The callers have
// validated handle, layout and parameters.
int elasticity_compute_metric(bp5_mf *mf, double *coef);
int elasticity_apply_cells(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, const double *src, double *dst, uint32_t c0, uint32_t c1);
int elasticity_diagonal(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, double *diag);

// Neo-Hookean hyperelasticity (bp5_hyperelasticity_*), defined in hyperelasticity/bp5_hyperelasticity.hip -- likewise a translation unit and a
// directory of its own: the residual (fills the ten state planes) and the tangent at the stored state over the cells [c0, c1), on the elasticity
// operator's ten geometry planes (both accumulate; an empty range launches nothing).  The callers have validated handle, layout and parameters.
int hyperelasticity_residual_cells(bp5_mf *mf, const double *coef, double *state, double lambda, double mu, size_t ld, const double *u, double *r, uint32_t c0,
                                   uint32_t c1);
int hyperelasticity_apply_cells(bp5_mf *mf, const double *coef, const double *state, double lambda, double mu, size_t ld, const double *src, double *dst, uint32_t c0,
                                uint32_t c1);

// The pointwise and transfer kernels of every vector shape (the Chebyshev step and the multigrid transfers of scalar and of block vectors, the dot
// product of block vectors), defined in blockvec/bp5_blockvec.hip -- a translation unit of its own, the only one that instantiates them.
// n_components blocks ld apart, a scalar vector n_components = 1 (ld is then not read); the callers have validated handles and layouts.
struct MgComponentsArgs { // the device tables of one transfer (bp5_mg_transfer), by value
  int pf = 0;
  bool geometric = false;
  const double *M = nullptr, *w = nullptr;
  const uint32_t *cidx = nullptr, *pcode = nullptr, *fidx = nullptr, *wmask = nullptr, *coff = nullptr, *cslot = nullptr;
  uint32_t n_cells = 0;
  hipStream_t stream = nullptr;
};
// partial sums of x.y, component = grid.y, in the columns cg_dh_kernel uses
int blockvec_dot(hipStream_t s, dim3 grid, const double *x, const double *y, size_t n, size_t ld, double *partials);
// one Chebyshev step (form 0..3 of chebyshev_step_kernel) on all blocks in one launch; diag == NULL: identity; diag_ld: 0 shared, ld block diagonal
int blockvec_chebyshev_step(hipStream_t s, int form, unsigned grid_x, int n_components, bool nt, double *x_new, const double *x, const double *x_old, const double *src,
                            const double *t, const double *diag, size_t n, size_t ld, size_t diag_ld, double f1, double f2);
// dst_f += P src_c ; slots = per-cell shares of P^T (w (.) (b - tv)) (tv == NULL: of w (.) b), [component][cell][NC^3] ; the combine pass
int blockvec_mg_prolongate(const MgComponentsArgs &a, int n_components, size_t ld_c, const double *src, size_t ld_f, double *dst);
int blockvec_mg_restrict(const MgComponentsArgs &a, int n_components, size_t ld_f, const double *b, const double *tv, size_t slot_stride, double *slots);
int blockvec_mg_combine(const MgComponentsArgs &a, int n_components, const double *slots, size_t slot_stride, uint32_t n_owned, uint32_t n, size_t ld, double *dst, bool add);

// What every operator launch takes from the handle (affine builds read ONE scalar plane, cells n^3 entries apart); the launcher adds range and team counts
inline ApplyArgs apply_args(const bp5_mf *mf, bool affine, const double *coef, const double *src, double *dst)
{
  ApplyArgs a{};
  a.l2g = mf->d_l2g; a.coef = coef; a.src = src; a.dst = dst;
  a.plane_stride = mf->coef_plane_stride; a.cell_stride = affine ? (uint64_t)mf->n3 : mf->coef_cell_stride;
  a.gcell = mf->d_gcell; a.n_cells_total = mf->n_cells;
  a.hang_mask = mf->d_hang_mask; a.hang_I = mf->d_hang_I;
  return a;
}
inline int zero_dst(bp5_mf *mf, double *dst) // ahead of a launch that accumulates (atomic scatter; owner stores that do not reach every entry)
{
  HIP_TRY(hipMemsetAsync(dst, 0, mf->n_local() * sizeof(double), mf->stream));
  return BP5_OK;
}

// The ONE switch on the degree: f(std::integral_constant<int, P>{}) for P = 1..8.  A caller templated on n = P + 1 writes P() + 1.
template <class F>
inline int for_degree(int degree, F &&f, const char *unsupported = "unsupported degree")
{
  switch (degree) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
  }
  return fail(BP5_ERR_INVALID, unsupported);
}

// The pencil launch shape: cells [c0, c1) in teams of CPT cells, TPB teams of TW waves per workgroup, the workgroups dealt out to the 8 XCDs
// (the kernels undo the dealing with teams_per_xcd).  Fills the range and team counts of a; the launcher adds its own LDS size.
struct PencilLaunch { dim3 grid, block; };
template <int CPT, int TW, int TPB>
inline PencilLaunch pencil_launch(ApplyArgs &a, uint32_t c0, uint32_t c1)
{
  a.cell_begin = c0; a.cell_end = c1;
  a.n_teams = (c1 - c0 + CPT - 1) / CPT;
  const uint32_t nblk = (a.n_teams + TPB - 1) / TPB;
  a.teams_per_xcd = (nblk + 7) / 8;
  return {dim3(a.teams_per_xcd * 8), dim3(64 * TW * TPB)};
}

// grid of a setup launch (one cell per workgroup, grid-stride beyond the cap; an empty handle still launches one)
inline uint32_t cell_grid(const bp5_mf *mf, uint32_t cap) { return std::min<uint32_t>(std::max<uint32_t>(mf->n_cells, 1), cap); }

// The degree's default pencil launch: p <= 3 four one-wave teams per workgroup, p >= 4 one four-wave team; n^2 lanes per cell, every plane prefetched.
// Users: variant 0 of every operator class (interior stores at p >= 5; hanging + affine included) and the block-vector kernel
template <int DEG>
struct DefaultPencil {
  static constexpr int TW = DEG <= 3 ? 1 : 4, LPC = (DEG + 1) * (DEG + 1), TPB = DEG <= 3 ? 4 : 1;
  static constexpr bool PF = true;
};

// overwrite: the launch must leave dst = A src; the kernel accumulates with atomics, so dst is zeroed first
template <int P, bool COLL, int TW, int LPC, int TPB, bool PF, int ABL = 0>
inline int launch_apply_t(bp5_mf *mf, ApplyCall &, const double *coef, const double *src, double *dst, uint32_t c0, uint32_t c1, bool overwrite)
{
  constexpr int n = P + 1;
  constexpr int CPT = 64 * TW / LPC;
  using L = LdsLayout<n, LPC>;
  if ((ABL & BLK_HANG) && !mf->has_hanging) return fail(BP5_ERR_INVALID, "the hanging-node build needs constraint masks");
  if (overwrite) BP5_TRY(zero_dst(mf, dst));
  ApplyArgs a = apply_args(mf, (ABL & BLK_AFFINE) != 0, coef, src, dst);
  const PencilLaunch pl = pencil_launch<CPT, TW, TPB>(a, c0, c1);
  ShapeArg<n> sh;
  fill_shape(sh, mf);
  const size_t lds = (size_t)TPB * CPT * L::CS * sizeof(double);
  snprintf(mf->last_apply_kernel, sizeof(mf->last_apply_kernel), "apply_pencil_kernel<%d,%s,%d,%d,%d,%s,%d>", P, COLL ? "true" : "false", TW, LPC, TPB, PF ? "true" : "false", ABL);
  hipLaunchKernelGGL((apply_pencil_kernel<P, COLL, TW, LPC, TPB, PF, ABL>), pl.grid, pl.block, lds, mf->stream, a,
                     sh);
  KERNEL_CHECK();
  return BP5_OK;
}

// bp5_apply_components: cells [c0, c1) (non-empty), every component through ONE pass over the metric planes and local_to_global (the caller
// has validated the layout and zeroed dst where asked; the phases of bp5_apply_components_distributed launch one range each)
template <int P, bool COLL, int TW, int LPC, int TPB>
inline int launch_apply_components_t(bp5_mf *mf, const double *coef, int n_components, size_t ld, const double *src, double *dst, uint32_t c0, uint32_t c1)
{
  constexpr int n = P + 1;
  constexpr int CPT = 64 * TW / LPC;
  using L = LdsLayout<n, LPC>;
  ApplyArgs a = apply_args(mf, false, coef, src, dst);
  const PencilLaunch pl = pencil_launch<CPT, TW, TPB>(a, c0, c1);
  ComponentArgs ca{(uint32_t)n_components, (uint64_t)ld};
  ShapeArg<n> sh;
  fill_shape(sh, mf);
  const size_t lds = (size_t)TPB * CPT * L::CS * sizeof(double);
  snprintf(mf->last_apply_kernel, sizeof(mf->last_apply_kernel), "apply_pencil_components_kernel<%d,%s,%d,%d,%d>", P, COLL ? "true" : "false", TW, LPC, TPB);
  hipLaunchKernelGGL((apply_pencil_components_kernel<P, COLL, TW, LPC, TPB>), pl.grid, pl.block, lds, mf->stream, a, ca, sh);
  KERNEL_CHECK();
  return BP5_OK;
}
// BP5_OP_MASS: cells [c0, c1) through the mass pencil kernel (atomic scatter: an overwriting launch zero-fills dst first)
template <int P, bool COLL, int TW, int LPC, int TPB>
inline int launch_apply_mass_t(bp5_mf *mf, const double *coef, const double *src, double *dst, uint32_t c0, uint32_t c1, bool overwrite)
{
  constexpr int n = P + 1;
  constexpr int CPT = 64 * TW / LPC;
  if (overwrite) BP5_TRY(zero_dst(mf, dst));
  ApplyArgs a = apply_args(mf, false, coef, src, dst);
  const PencilLaunch pl = pencil_launch<CPT, TW, TPB>(a, c0, c1);
  ShapeArg<n> sh;
  fill_shape(sh, mf);
  const size_t lds = COLL ? 0 : (size_t)TPB * CPT * mass_tile_stride<n, LPC>() * sizeof(double); // one field per cell slot (collocation: pointwise, no tile)
  snprintf(mf->last_apply_kernel, sizeof(mf->last_apply_kernel), "apply_pencil_mass_kernel<%d,%s,%d,%d,%d>", P, COLL ? "true" : "false", TW, LPC, TPB);
  hipLaunchKernelGGL((apply_pencil_mass_kernel<P, COLL, TW, LPC, TPB>), pl.grid, pl.block, lds, mf->stream, a, sh);
  KERNEL_CHECK();
  return BP5_OK;
}
// the degree's default pencil shape, both quadratures
template <int DEG>
int apply_components_degree_impl(bp5_mf *mf, const double *coef, int n_components, size_t ld, const double *src, double *dst, uint32_t c0, uint32_t c1)
{
  using DP = DefaultPencil<DEG>;
  if (c1 <= c0) return BP5_OK;
  if (mf->quadrature == BP5_QUAD_GLL) return launch_apply_components_t<DEG, true, DP::TW, DP::LPC, DP::TPB>(mf, coef, n_components, ld, src, dst, c0, c1);
  return launch_apply_components_t<DEG, false, DP::TW, DP::LPC, DP::TPB>(mf, coef, n_components, ld, src, dst, c0, c1);
}

// LDS bytes of one block-kernel workgroup: transpose tiles of the cell slots (two per slot where the cells span waves: BlockPass::PP),
// the brick's accumulator (and its staged src: ABL & BLK_STAGE), two run tables and two lattice tables.  The ONE formula: the launcher
// sizes the launch with it and the library's automatic kernel choice (effective_variant) counts workgroups per CU with it.
template <int P, bool COLL, int LPC, int ABL>
constexpr size_t block_lds_bytes(uint32_t max_list)
{
  return ((size_t)(256 / LPC) * (size_t)BlockPass<P, COLL, LPC, SC_OWNER_SET, ABL>::TILE_CS + ((ABL & BLK_STAGE) ? 2 : 1) * (size_t)max_list) * sizeof(double) +
         ((ABL & BLK_RUNS) ? (4 * BLOCK_MAX_RUNS + 2 * BLOCK_LATTICE_WORDS) * sizeof(uint32_t) : 0) + ((ABL & BLK_CARRY) ? 2 * BLOCK_CARRY_MAX * sizeof(double) : 0);
}
// ... of the default shape of a degree (sequential tiles, metric loaded in its own pass, run-length write-out, packed indices; the
// Helmholtz, hanging-node, fused-CG and lattice builds have the same tiles)
inline size_t block_default_lds_bytes(int degree, uint32_t max_list)
{
  constexpr int D = BLK_DEFAULT;
  switch (degree) {
    case 1: return block_lds_bytes<1, false, block_lpc(1), D>(max_list);
    case 2: return block_lds_bytes<2, false, block_lpc(2), D>(max_list);
    case 3: return block_lds_bytes<3, false, block_lpc(3), D>(max_list);
    case 4: return block_lds_bytes<4, false, block_lpc(4), D>(max_list);
    case 5: return block_lds_bytes<5, false, block_lpc(5), D>(max_list);
    case 6: return block_lds_bytes<6, false, block_lpc(6), D>(max_list);
    case 7: return block_lds_bytes<7, false, block_lpc(7), D>(max_list);
    case 8: return block_lds_bytes<8, false, block_lpc(8), D>(max_list);
  }
  return ~(size_t)0;
}

// workgroups per CU the BLK_MASS build of a degree is compiled for and launched with (block_wg_per_cu), for the library's automatic kernel choice
inline int mass_block_wg_per_cu(int degree)
{
  constexpr int M = BLK_DEFAULT | BLK_MASS;
  switch (degree) {
    case 1: return block_wg_per_cu<1, M>();
    case 2: return block_wg_per_cu<2, M>();
    case 3: return block_wg_per_cu<3, M>();
    case 4: return block_wg_per_cu<4, M>();
    case 5: return block_wg_per_cu<5, M>();
    case 6: return block_wg_per_cu<6, M>();
    case 7: return block_wg_per_cu<7, M>();
    case 8: return block_wg_per_cu<8, M>();
  }
  return 2;
}

// block-assembled kernel; falls back to the team kernel path when the range is partial
template <int P, bool COLL, int LPC, int ABL = 0>
inline int launch_block_t(bp5_mf *mf, ApplyCall &call, const double *coef, const double *src, double *dst, bool overwrite)
{
  constexpr int n = P + 1;
  constexpr int CPT = 256 / LPC;
  bp5_mf::DevPlan *dp = nullptr;
  BP5_TRY(get_plan_raw(mf, -CPT, &dp));
  const size_t lds = block_lds_bytes<P, COLL, LPC, ABL>(dp->max_list);
  if ((ABL & BLK_RUNS) && dp->max_runs > (uint32_t)BLOCK_MAX_RUNS) return fail(BP5_ERR_UNSUPPORTED, "too many runs per block for the run-length write-out");
  if ((ABL & BLK_PACK) && !dp->packed) return fail(BP5_ERR_UNSUPPORTED, "more than 128 runs per block: packed indices unavailable");
  if ((ABL & BLK_LATT) && !(dp->lattice && dp->n_lattice_blocks == dp->n_groups)) return fail(BP5_ERR_INVALID, "the lattice build needs a plan of lattice blocks only");
  if (lds > 160 * 1024) return fail(BP5_ERR_UNSUPPORTED, "cell block does not fit in LDS; pass smaller cell blocks");
  BlockPlan bp{}; // value-initialised: a field this launcher forgets is null, not garbage
  bp.pass_cell = dp->pass_cell; bp.pass_off = dp->pass_off; bp.off = dp->off; bp.dofs = dp->dofs; bp.pos = dp->pos; bp.gidx = dp->gidx;
  bp.packed = dp->packed;
  bp.lattice = dp->lattice; bp.cell_pos = dp->cell_pos;
  bp.cell_round = dp->cell_round; bp.blk_rounds = dp->team_rounds; bp.partial = dp->partial; bp.n_blocks = dp->n_groups;
  bp.run_off = dp->run_off; bp.runs = dp->runs; bp.max_list = dp->max_list;
  // a block-aligned cell range: only these blocks run, accumulate mode; DoFs shared with other blocks go to dst by
  // atomics (the partial slab + combine pass needs every block of the plan in the launch)
  const bool sub_range = call.b1 > call.b0 && (call.b0 != 0 || call.b1 != dp->n_groups);
  bp.blk_begin = sub_range ? call.b0 : 0;
  if (sub_range) bp.n_blocks = call.b1 - call.b0;
  // ... unless the caller runs ALL blocks in several range launches and one combine pass after the last one
  // (call.combine_later: the overlapped halo schedule): then every launch is the ordinary owner-store kernel
  const bool atomic_shared = call.shared_by_atomics || (sub_range && !call.combine_later);
  if (sub_range && overwrite && !call.combine_later) return fail(BP5_ERR_INVALID, "a cell range cannot overwrite dst");
  // persistent grid: two workgroups per CU (LDS budget), a multiple of 8 for the XCD mapping
  if (!device_cus(mf)) return fail(BP5_ERR_HIP, "hipGetDeviceProperties: no CU count");
  constexpr int wg_reg = block_wg_per_cu<P, ABL>(); // what the registers allow (launch bounds of the kernel) ...
  const int wg_per_cu = std::max(1, std::min<int>(wg_reg, (int)(160 * 1024 / std::max<size_t>(lds, 1)))); // ... and what the LDS of this plan allows
  uint32_t n_wg = (uint32_t)(mf->n_cus * wg_per_cu);
  if (mf->block_max_wg > 0) n_wg = std::min<uint32_t>(n_wg, (uint32_t)mf->block_max_wg);
  n_wg = std::max<uint32_t>(8, std::min<uint32_t>(n_wg, (bp.n_blocks + 7) / 8 * 8) / 8 * 8);
  bp.n_wg = n_wg;
  { // block ranges of the persistent workgroups: equal shares of the estimated COST (thin or partial bricks are cheaper per
    // block but dearer per cell than full ones), cached
    const uint32_t B0 = bp.blk_begin, B1 = bp.blk_begin + bp.n_blocks;
    // two parts (whole-range launches on a slab whose ghost-touching bricks come last, [Bs, B1)): every workgroup takes an equal share
    // of the ghost-touching bricks first, then interior bricks up to an equal share of the TOTAL cost
    uint32_t Bs = 0, bs0_ = 0;
    const bool two_parts = call.two_parts && !sub_range && mf->n_interior > 0 && mf->n_interior < mf->n_cells && block_aligned(mf, 0, mf->n_interior, &bs0_, &Bs) && Bs > B0 && Bs < B1;
    if (!dp->wg_blocks) dp->wg_blocks = new std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>, uint32_t *>;
    auto key = std::make_tuple(n_wg, B0, B1, two_parts ? Bs : 0u);
    auto itw = dp->wg_blocks->find(key);
    auto make_ranges = [&]() {
      const std::vector<double> &pc = dp->h_cost;
      std::vector<uint32_t> wb((two_parts ? 2 : 1) * (size_t)(n_wg + 1));
      if (!two_parts) {
        const double c0 = pc[B0], total = pc[B1] - c0;
        for (uint32_t w = 0; w <= n_wg; ++w)
          wb[w] = (uint32_t)(std::lower_bound(pc.begin() + B0, pc.begin() + B1 + 1, c0 + total * w / n_wg - 1e-9) - pc.begin());
        wb[0] = B0; wb[n_wg] = B1;
      } else {
        uint32_t *wa = wb.data(), *wi = wb.data() + n_wg + 1; // part 0: [Bs, B1), part 1: [B0, Bs)
        const double ca = pc[Bs], ta = pc[B1] - ca, ci = pc[B0], ti = pc[Bs] - ci;
        for (uint32_t w = 0; w <= n_wg; ++w) {
          wa[w] = (uint32_t)(std::lower_bound(pc.begin() + Bs, pc.begin() + B1 + 1, ca + ta * w / n_wg - 1e-9) - pc.begin());
          if (w == 0) wa[w] = Bs;
          if (w == n_wg) wa[w] = B1;
          const double want = (ta + ti) * w / n_wg - (pc[wa[w]] - ca); // interior cost the workgroups before w should hold
          wi[w] = (uint32_t)(std::lower_bound(pc.begin() + B0, pc.begin() + Bs + 1, ci + std::max(want, 0.0) - 1e-9) - pc.begin());
          if (w > 0) wi[w] = std::max(wi[w], wi[w - 1]);
        }
        wi[0] = B0; wi[n_wg] = Bs;
      }
      return wb;
    };
    if (itw == dp->wg_blocks->end()) {
      const std::vector<uint32_t> wb = make_ranges();
      uint32_t *dev = nullptr;
      BP5_TRY(upload(&dev, wb.data(), wb.size()));
      itw = dp->wg_blocks->emplace(key, dev).first;
    }
    bp.wg_block = itw->second;
    // face carry: whole-range owner-store launches of a carry build whose plan found faces to carry; the combine pass of THIS launch then
    // takes the tables of this partition (call.combine_tables), every other launch the plan's own
    call.combine_tables = nullptr;
    if constexpr ((ABL & BLK_CARRY) != 0) {
      if (mf->tune[BP5_TUNE_FACE_CARRY] && !sub_range && !atomic_shared && dp->cr_tile && !call.csr_combine && !dp->h_carry_len.empty()) {
        if (!dp->cr_carry) dp->cr_carry = new std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>, bp5_mf::DevPlan::CombineTables>;
        auto itc = dp->cr_carry->find(key);
        if (itc == dp->cr_carry->end()) {
          bp5_mf::DevPlan::CombineTables ct;
          BP5_TRY(build_carry_tables(mf, dp, make_ranges(), n_wg, two_parts, &ct));
          itc = dp->cr_carry->emplace(key, ct).first;
        }
        if (itc->second.n_shared < dp->n_shared) { // (equal: no face of this partition can be carried)
          call.combine_tables = &itc->second;
          bp.carry = 1u;
        }
      }
    }
    dp->cr_last_launch = call.combine_tables;
    bp.n_parts = two_parts ? 2u : 1u;
    bp.signal = nullptr;
    if (call.signal) {
      if (!two_parts || !mf->d_signal) return fail(BP5_ERR_INVALID, "boundary-first signal: the launch has no separate ghost-touching part");
      bp.signal = mf->d_signal;
    }
  }
  bp.cg_r = call.fuse ? call.fuse->r : nullptr; bp.dot_partials = mf->d_partials; bp.n_owned = mf->n_owned; bp.cg_state = mf->d_st;
  if constexpr ((ABL & BLK_UPD) != 0) { // the vector update of the brick interiors: one-part whole-range launches of a merged solve on a plan that qualifies
    if (!call.fuse || !call.fuse->upd_mode || !call.fuse->r || !dp->upd_n_int || sub_range || bp.n_parts != 1 || mf->n_ghost)
      return fail(BP5_ERR_INVALID, "the fused-update build needs a one-rank merged solve on a plan whose brick interiors are numbered first");
    bp.upd_p = const_cast<double *>(src); bp.upd_r = const_cast<double *>(call.fuse->r); bp.upd_v = dst; bp.upd_x = call.fuse->upd_x;
    bp.upd_diag = call.fuse->upd_diag; bp.upd_sc = mf->d_sc; bp.upd_mode = (uint32_t)call.fuse->upd_mode; bp.upd_end = dp->upd_n_int & ~1u;
  }
  bp.stamps = nullptr;
  if (ABL & BLK_STAMPS) {
    if (!mf->d_stamps) HIP_TRY(hipMalloc((void **)&mf->d_stamps, 4096 * 16 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(mf->d_stamps, 0, 4096 * 16 * sizeof(unsigned long long), mf->stream));
    bp.stamps = mf->d_stamps;
  }
  ApplyArgs a = apply_args(mf, (ABL & BLK_AFFINE) != 0, coef, src, dst);
  a.cell_begin = 0; a.cell_end = mf->n_cells; a.n_teams = dp->n_groups; a.teams_per_xcd = 0;
  if ((ABL & BLK_HANG) && !mf->has_hanging) return fail(BP5_ERR_INVALID, "the hanging-node build needs constraint masks");
  ShapeArg<n> sh;
  fill_shape(sh, mf);
  const bool set = overwrite && dp->covers_all;
  if (overwrite && !set) BP5_TRY(zero_dst(mf, dst));
  if (bp.signal && atomic_shared) return fail(BP5_ERR_INVALID, "boundary-first signal: owner-store launches only");
  const dim3 grid(n_wg), block(256);
  snprintf(mf->last_apply_kernel, sizeof(mf->last_apply_kernel), "apply_block_kernel<%d,%s,%d,%d,%d>", P, COLL ? "true" : "false", LPC,
           atomic_shared ? (set ? SC_OWNER_SET_ATOMIC : SC_OWNER_ADD_ATOMIC) : (set ? SC_OWNER_SET : SC_OWNER_ADD), ABL);
  if constexpr ((ABL & BLK_FUSE) != 0) { // fused CG dot products: overwrite mode, every DoF touched; the whole range in one launch, or
    // (boundary-first exchange schedule) in block ranges that together cover it, with ONE deferred combine pass
    if (!set || atomic_shared || (sub_range && !call.combine_later) || (call.combine_later && call.exchange == EXCHANGE_NONE) || !call.fuse)
      return fail(BP5_ERR_INVALID, "fused dot products need overwrite launches that cover the whole range");
    if (call.fuse->n_cols + n_wg > (uint32_t)PARTIAL_STRIDE / 2) return fail(BP5_ERR_UNSUPPORTED, "too many workgroups for the partial-sum rows");
    bp.dot_col0 = call.fuse->n_cols;
    call.fuse->n_cols += n_wg;
  }
  if constexpr ((ABL & BLK_FUSE) == 0) if (atomic_shared) {
    // brick-surface DoFs by atomics: zero exactly those first (SET mode), no partial slab / combine
    if (set && dp->n_shared) {
      hipLaunchKernelGGL(zero_indexed_kernel, dim3((dp->n_shared + 255) / 256), dim3(256), 0, mf->stream, dp->sh_dof, dp->n_shared, dst);
      KERNEL_CHECK();
    }
    if (set) {
      auto kern = apply_block_kernel<P, COLL, LPC, SC_OWNER_SET_ATOMIC, ABL>;
      HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(kern, grid, block, lds, mf->stream, a, bp, sh);
    } else {
      auto kern = apply_block_kernel<P, COLL, LPC, SC_OWNER_ADD_ATOMIC, ABL>;
      HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(kern, grid, block, lds, mf->stream, a, bp, sh);
    }
    KERNEL_CHECK();
    return BP5_OK;
  }
  if (set) {
    auto kern = apply_block_kernel<P, COLL, LPC, SC_OWNER_SET, ABL>;
    HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, grid, block, lds, mf->stream, a, bp, sh);
  } else if constexpr ((ABL & BLK_FUSE) == 0) {
    auto kern = apply_block_kernel<P, COLL, LPC, SC_OWNER_ADD, ABL>;
    HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, grid, block, lds, mf->stream, a, bp, sh);
  }
  KERNEL_CHECK();
  if (bp.signal) mf->signal_target += n_wg; // the launch was accepted: every workgroup counts itself in once; the caller waits for this value
  if (ABL & BLK_STAMPS) { // diagnostic build: print the per-phase cycle shares (never quote its run time)
    HIP_TRY(hipStreamSynchronize(mf->stream));
    std::vector<unsigned long long> hs((size_t)n_wg * 16);
    HIP_TRY(hipMemcpy(hs.data(), mf->d_stamps, hs.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    double tot[9] = {0};
    for (uint32_t w = 0; w < n_wg; ++w) for (int k = 0; k < 9; ++k) tot[k] += (double)hs[(size_t)w * 16 + k];
    double all = 0; for (int k = 0; k < 7; ++k) all += tot[k];
    static const char *nm[7] = {"issue loads", "evaluate (+wait u)", "wait idx + issue gather", "q-op (+wait metric)", "integrate", "accumulate", "block boundary"};
    fprintf(stderr, "[bp5 stamps] passes/wg %.1f, cycles/pass %.0f\n", tot[8] / n_wg, all / tot[8]);
    for (int k = 0; k < 7; ++k) fprintf(stderr, "[bp5 stamps]   %-26s %5.1f %%  %8.0f cycles/pass\n", nm[k], 100.0 * tot[k] / all, tot[k] / tot[8]);
  }
  if (ABL & 1023) return BP5_OK; // (1024 and above are real modes) timing-only ablation builds skip the combine pass (1024/2048/8192 are real modes)
  if (call.combine_later) return BP5_OK; // the caller runs launch_combine after its last range
  return launch_combine(mf, call, dp, dst, set);
}

// overwrite == true: dst need not be zeroed by the caller, the launch defines every entry
template <int P, bool COLL, int TW, int LPC, bool PF, int OPT = 0>
inline int launch_team_t(bp5_mf *mf, ApplyCall &call, const double *coef, const double *src, double *dst, uint32_t c0, uint32_t c1, bool overwrite)
{
  constexpr int n = P + 1;
  constexpr int CPT = 64 * TW / LPC;
  using L = LdsLayout<n, LPC>;
  TeamPlan tp{};
  bp5_mf::DevPlan *dp = nullptr;
  BP5_TRY(get_plan(mf, CPT, tp, &dp));
  ApplyArgs a = apply_args(mf, (OPT & BLK_AFFINE) != 0, coef, src, dst);
  a.cell_begin = c0; a.cell_end = c1;
  a.n_teams = (c1 + CPT - 1) / CPT - c0 / CPT;
  a.teams_per_xcd = (a.n_teams + 7) / 8;
  ShapeArg<n> sh;
  fill_shape(sh, mf);
  const size_t lds = (size_t)CPT * L::CS * sizeof(double);
  const dim3 grid(a.teams_per_xcd * 8), block(64 * TW);
  const bool whole = (c0 == 0 && c1 == mf->n_cells);
  snprintf(mf->last_apply_kernel, sizeof(mf->last_apply_kernel), "apply_team_kernel<%d,%s,%d,%d,%s,", P, COLL ? "true" : "false", TW, LPC, PF ? "true" : "false");
  if (!whole || call.atomic_scatter) {
    if (overwrite) BP5_TRY(zero_dst(mf, dst));
    hipLaunchKernelGGL((apply_team_kernel<P, COLL, TW, LPC, PF, SC_ATOMIC, OPT>), grid, block, lds, mf->stream, a, tp, sh);
  } else {
    const bool set = overwrite && dp->covers_all;
    if (overwrite && !set) BP5_TRY(zero_dst(mf, dst));
    if (set) hipLaunchKernelGGL((apply_team_kernel<P, COLL, TW, LPC, PF, SC_OWNER_SET, OPT>), grid, block, lds, mf->stream, a, tp, sh);
    else hipLaunchKernelGGL((apply_team_kernel<P, COLL, TW, LPC, PF, SC_OWNER_ADD, OPT>), grid, block, lds, mf->stream, a, tp, sh);
    KERNEL_CHECK();
    return launch_combine(mf, call, dp, dst, set);
  }
  KERNEL_CHECK();
  return BP5_OK;
}
// The run-time quadrature choice `coll` (collocation: GLL points) as the COLL template argument of a launcher, so that each selection is
// written once: LAUNCH_COLL(launch_block_t, P, (LPC, ABL), coef, src, dst, overwrite).  It takes `mf`, `call` and `coll` from the scope it is
// used in (which is why every launcher has the ApplyCall in its signature, read or not).  BOTH sides are instantiated: a build that exists
// for one quadrature only names its launcher directly
#define BP5_UNPAREN(...) __VA_ARGS__
#define LAUNCH_COLL(FN, P, TARGS, ...)                                                                             \
  (coll ? FN<P, true, BP5_UNPAREN TARGS>(mf, call, __VA_ARGS__) : FN<P, false, BP5_UNPAREN TARGS>(mf, call, __VA_ARGS__))
#define TEAM_CASE(P, V, TW, LPC, PF) BP5_CASE(P, V) return LAUNCH_COLL(launch_team_t, P, (TW, LPC, PF), coef, src, dst, c0, c1, overwrite)

// z-marching kernel (whole cell range only; partial ranges take the plain pencil kernel); atomic scatter: overwrite zeroes dst first
template <int P, bool COLL, int TW, int LPC, bool PF, int ABL = 0>
inline int launch_march_t(bp5_mf *mf, ApplyCall &, const double *coef, const double *src, double *dst, bool overwrite)
{
  constexpr int n = P + 1;
  constexpr int CPT = 64 * TW / LPC;
  using L = LdsLayout<n, LPC>;
  auto it = mf->march_plans.find(CPT);
  if (it == mf->march_plans.end()) {
    MarchPlanHost h;
    BP5_TRY(build_march_plan(mf->h_l2g.data(), mf->n_cells, n, CPT, mf->march_max_steps, h));
    bp5_mf::DevMarch dm;
    BP5_TRY(upload(&dm.team_off, h.team_off.data(), h.team_off.size()));
    BP5_TRY(upload(&dm.entries, h.entries.data(), h.entries.size()));
    dm.n_teams = (uint32_t)h.team_off.size() - 1;
    it = mf->march_plans.emplace(CPT, dm).first;
  }
  MarchPlan mp{};
  mp.team_off = it->second.team_off; mp.entries = it->second.entries; mp.n_teams = it->second.n_teams;
  mp.teams_per_xcd = (mp.n_teams + 7) / 8;
  if (overwrite) BP5_TRY(zero_dst(mf, dst));
  ApplyArgs a = apply_args(mf, (ABL & BLK_AFFINE) != 0, coef, src, dst);
  a.cell_begin = 0; a.cell_end = mf->n_cells; a.n_teams = mp.n_teams; a.teams_per_xcd = mp.teams_per_xcd;
  ShapeArg<n> sh;
  fill_shape(sh, mf);
  const size_t lds = (size_t)CPT * L::CS * sizeof(double);
  snprintf(mf->last_apply_kernel, sizeof(mf->last_apply_kernel), "apply_march_kernel<%d,%s,%d,%d,%s,%d>", P, COLL ? "true" : "false", TW, LPC, PF ? "true" : "false", ABL);
  hipLaunchKernelGGL((apply_march_kernel<P, COLL, TW, LPC, PF, ABL>), dim3(mp.teams_per_xcd * 8), dim3(64 * TW), lds, mf->stream, a, mp, sh);
  KERNEL_CHECK();
  return BP5_OK;
}

// ------------------------------------------------------------------------------------ variant 56: the default block kernel
// The builds of the default block kernel that exist, per degree: a mask each, Gauss-only where marked (the others are compiled for both
// quadratures).  The list IS the inventory: launch_block_default launches nothing else, every entry is instantiated.  Within an operator class
// the builds with more optional features come first.  Every degree: Poisson on double planes, plain or fused, packed or lattice indices; on
// float planes (never fused); Helmholtz, mass and hanging nodes, plain or fused, packed indices only.  p = 4 alone: the face carry (in every lattice
// build; BP5_TUNE_FACE_CARRY switches it per launch), non-temporal metric loads (Gauss only; with lattice blocks, or on hanging-node meshes; never
// on float planes), the affine build, and two older shapes for plans without packed indices (run-length write-out with list loads; list write-out)
template <int M, bool GAUSS_ONLY = false> struct Bld {};
template <typename... B> struct BuildList {};
template <int DEG>
struct DefaultBlockBuilds {
  static constexpr int D = BLK_DEFAULT, F = BLK_FUSE;
  using list = BuildList<Bld<D | BLK_LATT>, Bld<D | F | BLK_LATT>, Bld<D>, Bld<D | F>, Bld<D | BLK_F32M | BLK_LATT>, Bld<D | BLK_F32M>, Bld<D | BLK_HELM>,
                         Bld<D | F | BLK_HELM>, Bld<D | BLK_MASS>, Bld<D | F | BLK_MASS>, Bld<D | BLK_HANG>, Bld<D | F | BLK_HANG>>;
};
template <>
struct DefaultBlockBuilds<4> {
  static constexpr int D = BLK_DEFAULT, F = BLK_FUSE, LATC = BLK_LATT | BLK_CARRY;
  using list = BuildList<Bld<D | F | LATC | BLK_UPD | BLK_NTM>, Bld<D | F | LATC | BLK_UPD>, // + the merged CG's vector update of the brick interiors (both quadratures)
                         Bld<D | LATC | BLK_NTM, true>, Bld<D | F | LATC | BLK_NTM, true>, Bld<D | LATC>, Bld<D | F | LATC>, Bld<D>, Bld<D | F>,
#ifdef BP5_TIMING_BUILDS // variant 63: the rolling metric prefetch (BlockPass::ROLL) -- a measured loss (profiles/r4 d_*)
                         Bld<D | BLK_LATT | BLK_NTM | BLK_ROLL, true>, Bld<D | F | BLK_LATT | BLK_NTM | BLK_ROLL, true>, Bld<D | BLK_LATT | BLK_ROLL, true>,
                         Bld<D | F | BLK_LATT | BLK_ROLL, true>,
#endif
                         Bld<D | BLK_F32M | LATC>, Bld<D | BLK_F32M>, Bld<D | BLK_HELM>, Bld<D | F | BLK_HELM>, Bld<D | BLK_MASS>, Bld<D | F | BLK_MASS>, Bld<D | BLK_HANG | BLK_NTM, true>,
                         Bld<D | F | BLK_HANG | BLK_NTM, true>, Bld<D | BLK_HANG>, Bld<D | F | BLK_HANG>, Bld<D | BLK_AFFINE>,
                         Bld<BLK_SINGLE | BLK_SEQ | BLK_RUNS>, Bld<BLK_SINGLE | BLK_SEQ>>;
};
// Lattice indices, the face carry and non-temporal metric loads are OPTIONAL: they change the speed and no bit of the result.  A build serves a
// request when everything else agrees and it has no optional feature that was not asked for; an optional feature asked for that the operator
// class, the degree or the quadrature has no build with is thereby DROPPED, not refused (non-temporal loads under GLL quadrature, the carry
// outside p = 4, lattice indices for the Helmholtz operator ...).  Everything else (operator class, fused dot products) is served or refused.
constexpr int BLK_OPTIONAL = BLK_LATT | BLK_CARRY | BLK_NTM;
constexpr bool build_serves(int m, bool gauss_only, int want, bool coll)
{
  return (m & ~BLK_OPTIONAL) == (want & ~BLK_OPTIONAL) && (m & BLK_OPTIONAL & ~want) == 0 && !(gauss_only && coll);
}
template <int DEG, int M, bool GAUSS_ONLY>
inline bool launch_if_serves(Bld<M, GAUSS_ONLY>, int want, int *status, bp5_mf *mf, ApplyCall &call, const double *coef, const double *src, double *dst)
{
  const bool coll = mf->quadrature == BP5_QUAD_GLL;
  if (!build_serves(M, GAUSS_ONLY, want, coll)) return false;
  if constexpr (GAUSS_ONLY) *status = launch_block_t<DEG, false, block_lpc(DEG), M>(mf, call, coef, src, dst, call.overwrite);
  else *status = LAUNCH_COLL(launch_block_t, DEG, (block_lpc(DEG), M), coef, src, dst, call.overwrite);
  return true;
}
template <int DEG, typename... B>
inline bool launch_first_that_serves(BuildList<B...>, int want, int *status, bp5_mf *mf, ApplyCall &call, const double *coef, const double *src, double *dst)
{
  return (launch_if_serves<DEG>(B{}, want, status, mf, call, coef, src, dst) || ...);
}
// Variant 56 of every operator class and degree (and three p = 4 siblings that differ in the request only: 48 never asks for lattice indices -- it
// A/Bs the combine pass of the packed shape --, 49 takes the plan as one without packed indices, 63 adds the rolling prefetch): the block range,
// the plan, what the handle and the solver ask for as a mask, then the first build of the degree's list that serves it.
template <int DEG>
inline int launch_block_default(bp5_mf *mf, ApplyCall &call, const double *coef, const double *src, double *dst)
{
  static_assert(block_lpc(DEG) != 0, "no block-kernel shape for this degree");
  const int variant = call.variant % 100;
  if (!block_aligned(mf, call.c0, call.c1, &call.b0, &call.b1)) return fail(BP5_ERR_INVALID, "variant 56 needs a cell range aligned with the cell blocks");
  bp5_mf::DevPlan *dp = nullptr;
  BP5_TRY(get_plan_raw(mf, -(256 / block_lpc(DEG)), &dp));
  const int cls = // operator class (apply_degree_impl has refused the combinations of them, and returned on an empty range)
      mf->f32_metric() ? BLK_F32M : mf->operator_kind == BP5_OP_HELMHOLTZ ? BLK_HELM : mf->operator_kind == BP5_OP_MASS ? BLK_MASS : mf->has_hanging ? BLK_HANG : mf->geometry_mode == BP5_GEOM_AFFINE ? BLK_AFFINE : 0;
  int want;
  if (dp->packed && variant != 49) {
    want = BLK_DEFAULT | cls | (call.fuse ? BLK_FUSE : 0);
    if (dp->lattice && dp->n_lattice_blocks == dp->n_groups && variant != 48) want |= BLK_LATT | BLK_CARRY; // every block a lattice block: closed-form indices, no per-DoF index stream
    // the merged solver asks for its vector update inside the launch (it has checked plan, degree and variant: fused_update_wanted); such a launch
    // reads the metric non-temporally at every size unless told otherwise -- p' and r' are to stay in the memory-side cache until they are read
    const bool upd = call.fuse && call.fuse->upd_mode != 0;
    if (upd) {
      if (DEG != 4 || !(want & BLK_LATT) || cls != 0) return fail(BP5_ERR_INVALID, "the fused vector update needs the p = 4 lattice build of the Poisson operator");
      want |= BLK_UPD;
    }
    if (upd && mf->streaming < 0 ? true : streaming_accesses(mf)) want |= BLK_NTM;
  } else { // more than 128 runs in some block: only the Poisson operator at p = 4 keeps kernels for such plans, none of them fused
    if (DEG != 4 || cls != 0) return fail(BP5_ERR_UNSUPPORTED, "variant " + std::to_string(variant) + " needs packed indices (<= 128 runs per cell block)");
    if (call.fuse) return fail(BP5_ERR_INVALID, "fused dot products need the packed block kernel");
    want = dp->max_runs <= (uint32_t)BLOCK_MAX_RUNS ? BLK_SINGLE | BLK_SEQ | BLK_RUNS : BLK_SINGLE | BLK_SEQ; // write-out without list loads while the runs fit the LDS table
  }
#ifndef BP5_TIMING_BUILDS
  if (variant == 63) return fail(BP5_ERR_INVALID, "variant 63 lives in libbp5_timing.so");
#else
  if (variant == 63) {
    if (!(want & BLK_LATT) || mf->quadrature == BP5_QUAD_GLL) return fail(BP5_ERR_UNSUPPORTED, "variant 63 (rolling metric prefetch) needs lattice blocks and Gauss quadrature");
    want = (want & ~BLK_CARRY) | BLK_ROLL;
  }
#endif
  int status = BP5_OK;
  if (!launch_first_that_serves<DEG>(typename DefaultBlockBuilds<DEG>::list{}, want, &status, mf, call, cls == BLK_AFFINE ? mf->d_scalar_plane : coef, src, dst))
    return fail(BP5_ERR_UNSUPPORTED, "the block kernel has no build for this operator, plan and solver request");
  return status;
}

// ------------------------------------------------------------------------------------ (degree, variant) -> kernel
// pencil variants: (degree, variant) -> (TW, LPC, TPB, PF); variant 0 is DefaultPencil
#define APPLY_CASE(P, V, TW, LPC, TPB, PF) BP5_CASE(P, V) return LAUNCH_COLL(launch_apply_t, P, (TW, LPC, TPB, PF), coef, src, dst, c0, c1, overwrite)

// The affine pencil kernel keeps a shape of its OWN, not DefaultPencil: one four-wave team per workgroup (TW = 4, TPB = 1) at every degree
template <int P>
inline int launch_affine(bp5_mf *mf, ApplyCall &call, const double *src, double *dst, uint32_t c0, uint32_t c1, bool overwrite)
{
  const bool coll = mf->quadrature == BP5_QUAD_GLL;
  return LAUNCH_COLL(launch_apply_t, P, (4, (P + 1) * (P + 1), 1, true, BLK_AFFINE), mf->d_scalar_plane, src, dst, c0, c1, overwrite);
}

// One instantiation per degree: only the cases of DEG are compiled into it.
#define BP5_CASE(P, V) if constexpr (DEG == (P)) if (variant == (V))
#define LAUNCH_DEFAULT_PENCIL(ABL, COEF) LAUNCH_COLL(launch_apply_t, DEG, (DP::TW, DP::LPC, DP::TPB, DP::PF, ABL), COEF, src, dst, c0, c1, overwrite)
template <int DEG>
int apply_degree_impl(bp5_mf *mf, ApplyCall &call, const double *coef, const double *src, double *dst)
{
  using DP = DefaultPencil<DEG>;
  const uint32_t c0 = call.c0, c1 = call.c1;
  const bool overwrite = call.overwrite;
  const bool coll = mf->quadrature == BP5_QUAD_GLL;
  const bool affine = mf->geometry_mode == BP5_GEOM_AFFINE;
  if (c1 <= c0) return overwrite ? zero_dst(mf, dst) : BP5_OK; // the empty range, for every operator and variant
  if (mf->trilinear()) return trilinear_apply(mf, call, src, dst); // the metric from the cells' vertices: kernels of its own, Poisson class, coef is not read
  if (mf->overint()) return overint_apply(mf, call, coef, src, dst); // Gauss(p+2) points: kernels, tables and planes of its own, Poisson and mass class
  if (mf->f32_metric()) {
    // FP32 metric planes (bp5_mf_set_metric_precision): the BLK_F32M builds of what the dispatch picks for an unfused application of the Poisson
    // operator on six planes -- variant 56: the default block kernel, cell ranges and two-part launches included; variant 0: the degree's default
    // pencil kernel
    if (mf->operator_kind != BP5_OP_POISSON || mf->has_hanging || affine)
      return fail(BP5_ERR_UNSUPPORTED, "FP32 metric planes: Poisson operator on a conforming mesh with the six-plane geometry only");
    if (call.fuse) return fail(BP5_ERR_UNSUPPORTED, "FP32 metric planes: no fused dot products");
    if (call.variant == 56) return launch_block_default<DEG>(mf, call, coef, src, dst);
    if (call.variant != 0) return fail(BP5_ERR_UNSUPPORTED, "FP32 metric planes run apply variants 0 (pencil kernel) and 56 (block kernel)");
    return LAUNCH_DEFAULT_PENCIL(BLK_F32M, coef);
  }
  if (mf->operator_kind == BP5_OP_HELMHOLTZ) {
    // step-64's Helmholtz operator (step-64/step-64.cu:154-160,201-219) as a build of the same fused kernels: the degree's default pencil
    // shape (any mesh), or the deterministic block kernel on cell bricks (variant 56; with the CG dot products fused when the solver asks)
    if (mf->has_hanging || affine) return fail(BP5_ERR_UNSUPPORTED, "the Helmholtz operator needs a conforming mesh and the six-plane geometry");
    if (call.variant == 56) return launch_block_default<DEG>(mf, call, coef, src, dst);
#ifdef BP5_TIMING_BUILDS
    // timing-only ablations of the Helmholtz block kernel at p = 3 (wrong results; profiles/r4 j_*): 91 no write-out (and no combine pass), 93 no plane loads, 95 no gather
    if constexpr (DEG == 3) if (call.variant == 91 || call.variant == 93 || call.variant == 95) {
      if (!block_aligned(mf, c0, c1, &call.b0, &call.b1)) return fail(BP5_ERR_INVALID, "needs aligned cell blocks");
      if (call.variant == 91) return launch_block_t<3, false, 16, BLK_DEFAULT | BLK_HELM | 1>(mf, call, coef, src, dst, true);
      if (call.variant == 93) return launch_block_t<3, false, 16, BLK_DEFAULT | BLK_HELM | 2>(mf, call, coef, src, dst, true);
      return launch_block_t<3, false, 16, BLK_DEFAULT | BLK_HELM | 4>(mf, call, coef, src, dst, true);
    }
#endif
    if (call.variant != 0) return fail(BP5_ERR_UNSUPPORTED, "the Helmholtz operator runs apply variants 0 (pencil kernel) and 56 (block kernel)");
    return LAUNCH_DEFAULT_PENCIL(BLK_HELM, coef);
  }
  if (mf->operator_kind == BP5_OP_MASS) {
    // the mass operator (v, rho u) on one plane (CEED BP1, deal.II MatrixFreeOperators::MassOperator): the mass pencil kernel in the degree's default
    // pencil shape (any conforming mesh and cell range), or the BLK_MASS build of the block kernel on cell bricks (variant 56; with the CG dot
    // products fused when the solver asks)
    if (mf->has_hanging || affine) return fail(BP5_ERR_UNSUPPORTED, "the mass operator needs a conforming mesh and the plane geometry (no hanging nodes, no affine mode)");
    if (call.variant == 56) return launch_block_default<DEG>(mf, call, coef, src, dst);
    if (call.fuse) return fail(BP5_ERR_INVALID, "fused dot products need the packed block kernel");
    if (call.variant != 0) return fail(BP5_ERR_UNSUPPORTED, "the mass operator runs apply variants 0 (pencil kernel) and 56 (block kernel)");
    if (coll) return launch_apply_mass_t<DEG, true, DP::TW, DP::LPC, DP::TPB>(mf, coef, src, dst, c0, c1, overwrite);
    return launch_apply_mass_t<DEG, false, DP::TW, DP::LPC, DP::TPB>(mf, coef, src, dst, c0, c1, overwrite);
  }
  if (mf->has_hanging) {
    // 2:1 refined meshes (resolve_hanging_nodes, bp5/fe_evaluation_gl.h:150-151,167-168): the hanging-node fix-up after the gather and its
    // adjoint before the scatter.  Variant 56: the deterministic block kernel (cell blocks, packed indices; the CG dot products fused when
    // the solver asks); variant 90: the degree's default pencil shape with atomics (any mesh; also the affine geometry mode: all cells affine on
    // undeformed 2:1 meshes, per-cell K K^T + one scalar plane)
    if (call.variant == 56 && !affine) return launch_block_default<DEG>(mf, call, coef, src, dst);
    if (call.variant != 90) return fail(BP5_ERR_UNSUPPORTED, "meshes with hanging nodes run apply variants 90 (pencil kernel) and 56 (block kernel)");
    if (affine) return LAUNCH_DEFAULT_PENCIL(BLK_HANG | BLK_AFFINE, mf->d_scalar_plane);
    return LAUNCH_DEFAULT_PENCIL(BLK_HANG, coef);
  }
  if (affine) { // per-cell K K^T + one scalar plane: the affine pencil kernel, whatever the variant; p = 4 also has team and block builds
    const bool whole = c0 == 0 && c1 == mf->n_cells;
    if constexpr (DEG == 4) {
    if (call.variant % 100 == 10) return LAUNCH_COLL(launch_team_t, 4, (4, 25, true, BLK_AFFINE), mf->d_scalar_plane, src, dst, c0, c1, overwrite);
    if (call.variant == 56) return launch_block_default<4>(mf, call, coef, src, dst);
    // 50 / 51: 25 / 32 lanes per cell; 55 / 54: the same with the brick-surface DoFs by atomics (ApplyCall::shared_by_atomics)
    if (whole && (call.variant == 51 || call.variant == 54)) return LAUNCH_COLL(launch_block_t, 4, (32, BLK_AFFINE), mf->d_scalar_plane, src, dst, overwrite);
    if (whole && (call.variant == 50 || call.variant == 55)) return LAUNCH_COLL(launch_block_t, 4, (25, BLK_AFFINE), mf->d_scalar_plane, src, dst, overwrite);
#ifdef BP5_TIMING_BUILDS
    if (call.variant == 85) // timing only: affine, no scatter atomics -> compute/latency floor of the pencil kernel
      return launch_apply_t<4, false, 4, 25, 1, true, 1025>(mf, call, mf->d_scalar_plane, src, dst, c0, c1, false);
#endif
    }
    return launch_affine<DEG>(mf, call, src, dst, c0, c1, overwrite);
  }
  // variants >= 100: the team kernel of (variant - 100) with the global-atomic scatter (A/B tests)
  int variant = call.variant % 100;
  if (variant == 0) {
    // cell-interior DoFs numbered ahead of all others (recognised by bp5_mf_create): the default pencil kernel of p >= 5 stores the entries a cell owns alone
    // plainly -- (p-1)^3 of (p+1)^3 atomics less per cell (47 % at p = 8), and no store ever meets an atomic in one cache line.  A plain store REPLACES
    // what dst held, so the build is taken only where that is known to be zero: the launch zero-fills itself (overwrite), or the caller has
    // (ApplyCall::dst_known_zero).  dst += A src on the caller's own content (bp5_apply with zero_dst = 0, bp5_apply_cells) takes the atomics
    if constexpr (DEG >= 5) if (!call.atomic_scatter && mf->cell_interiors_first && mf->tune[BP5_TUNE_INTERIOR_STORES] && (overwrite || call.dst_known_zero))
      return LAUNCH_DEFAULT_PENCIL(PEN_INTERIOR_STORES, coef);
    return LAUNCH_DEFAULT_PENCIL(0, coef);
  }
  if (variant == 56) return launch_block_default<DEG>(mf, call, coef, src, dst);
  {
    APPLY_CASE(1, 1, 1, 4, 4, true);
    APPLY_CASE(3, 1, 1, 16, 4, true);
    APPLY_CASE(4, 6, 1, 25, 4, true);
    APPLY_CASE(4, 1, 1, 32, 4, true);
    APPLY_CASE(4, 2, 2, 25, 1, true);
    APPLY_CASE(4, 3, 4, 25, 1, true);
    APPLY_CASE(4, 4, 1, 25, 1, true);
    APPLY_CASE(4, 5, 1, 25, 4, false);
    APPLY_CASE(5, 1, 1, 36, 4, true);
    APPLY_CASE(5, 2, 4, 36, 1, false);
    APPLY_CASE(5, 3, 2, 36, 1, true);
    APPLY_CASE(6, 5, 4, 49, 1, false);   // (the defaults for p >= 6 prefetch all planes: the high-degree sweep)
    APPLY_CASE(6, 1, 1, 49, 4, false);
    APPLY_CASE(6, 2, 4, 49, 1, true);
    APPLY_CASE(6, 3, 1, 49, 1, true);
    APPLY_CASE(6, 4, 2, 49, 1, false);
    APPLY_CASE(7, 5, 1, 64, 4, false);
    APPLY_CASE(7, 1, 4, 64, 1, false);
    APPLY_CASE(7, 2, 4, 64, 1, true);
    APPLY_CASE(7, 3, 1, 64, 1, true);
    APPLY_CASE(8, 5, 4, 81, 1, false);
    APPLY_CASE(8, 1, 2, 81, 1, false);
    APPLY_CASE(8, 2, 4, 81, 1, true);
    APPLY_CASE(8, 3, 2, 81, 1, true);
#ifdef BP5_TIMING_BUILDS
    // timing-only ablations of variant 3 (results are wrong by construction): 20 + ABL mask
#define ABL_CASE(M) BP5_CASE(4, 20 + (M)) return launch_apply_t<4, false, 4, 25, 1, true, M>(mf, call, coef, src, dst, c0, c1, false)
#define ABL_CASE_HI(P, L, M) BP5_CASE(P, 20 + (M)) return launch_apply_t<P, false, 4, L, 1, true, M>(mf, call, coef, src, dst, c0, c1, false)
    ABL_CASE_HI(8, 81, 1); ABL_CASE_HI(8, 81, 2); ABL_CASE_HI(8, 81, 4); ABL_CASE_HI(8, 81, 8); ABL_CASE_HI(8, 81, 9); ABL_CASE_HI(8, 81, 11);
    ABL_CASE_HI(6, 49, 1); ABL_CASE_HI(6, 49, 2); ABL_CASE_HI(6, 49, 8); ABL_CASE_HI(6, 49, 9);
    BP5_CASE(4, 7) return LAUNCH_COLL(launch_apply_t, 4, (4, 25, 1, true, 256), coef, src, dst, c0, c1, false);
    BP5_CASE(4, 8) return LAUNCH_COLL(launch_apply_t, 4, (4, 25, 1, true, 512), coef, src, dst, c0, c1, false);
    BP5_CASE(4, 9) return LAUNCH_COLL(launch_apply_t, 4, (2, 25, 1, true, 512), coef, src, dst, c0, c1, false);
    BP5_CASE(4, 82) return launch_apply_t<4, false, 4, 25, 1, true, 257>(mf, call, coef, src, dst, c0, c1, false);
    BP5_CASE(4, 83) return launch_apply_t<4, false, 4, 25, 1, true, 4096>(mf, call, coef, src, dst, c0, c1, false);
    BP5_CASE(4, 84) return launch_apply_t<4, false, 4, 25, 1, true, 8192>(mf, call, coef, src, dst, c0, c1, false);
    BP5_CASE(4, 80) return launch_apply_t<4, false, 4, 25, 1, true, 64>(mf, call, coef, src, dst, c0, c1, false);
    BP5_CASE(4, 81) { // E-vector stores need a big scratch target
      if (!mf->d_evec) HIP_TRY(hipMalloc((void **)&mf->d_evec, (size_t)mf->n_cells * mf->n3 * sizeof(double)));
      return launch_apply_t<4, false, 4, 25, 1, true, 128>(mf, call, coef, src, mf->d_evec, c0, c1, false); }
    BP5_CASE(4, 90) {
      if (!mf->d_evec) HIP_TRY(hipMalloc((void **)&mf->d_evec, ((size_t)mf->n_cells * mf->n3 + 4096 * 5) * sizeof(double) * 2));
      return launch_apply_t<4, false, 4, 25, 1, true, 262144>(mf, call, coef, src, mf->d_evec, c0, c1, false); }
    BP5_CASE(4, 88) {
      if (!mf->d_evec) HIP_TRY(hipMalloc((void **)&mf->d_evec, (size_t)mf->n_cells * mf->n3 * sizeof(double)));
      return launch_apply_t<4, false, 4, 25, 1, true, 128 + 65536>(mf, call, coef, src, mf->d_evec, c0, c1, false); }
    BP5_CASE(4, 89) {
      if (!mf->d_evec) HIP_TRY(hipMalloc((void **)&mf->d_evec, (size_t)mf->n_cells * mf->n3 * sizeof(double)));
      return launch_apply_t<4, false, 4, 25, 1, true, 1 + 131072>(mf, call, coef, src, mf->d_evec, c0, c1, false); }
    BP5_CASE(4, 86) {
      if (!mf->d_evec) HIP_TRY(hipMalloc((void **)&mf->d_evec, (size_t)mf->n_cells * mf->n3 * sizeof(double)));
      return launch_apply_t<4, false, 4, 25, 1, true, 128 + 16384>(mf, call, coef, src, mf->d_evec, c0, c1, false); }
    ABL_CASE(1); ABL_CASE(2); ABL_CASE(3); ABL_CASE(4); ABL_CASE(5); ABL_CASE(7); ABL_CASE(8); ABL_CASE(9); ABL_CASE(15); ABL_CASE(14); ABL_CASE(13); ABL_CASE(11);
#endif
    // z-marching kernel, variants 70+ (a partial cell range takes the pencil kernel of the same shape)
#define MARCH_CASE(P, V, TW, LPC, PF)                                                                              \
  BP5_CASE(P, V) {                                                                                                 \
    if (c0 != 0 || c1 != mf->n_cells)                                                                              \
      return LAUNCH_COLL(launch_apply_t, P, (TW, LPC, 1, PF), coef, src, dst, c0, c1, overwrite);                   \
    return LAUNCH_COLL(launch_march_t, P, (TW, LPC, PF), coef, src, dst, overwrite);                                \
  }
#ifdef BP5_TIMING_BUILDS
    BP5_CASE(4, 73) return launch_march_t<4, false, 4, 25, true, 1>(mf, call, coef, src, dst, false); // timing only: march, no scatter
#endif
    MARCH_CASE(1, 70, 4, 4, true);
    MARCH_CASE(2, 70, 4, 9, true);
    MARCH_CASE(3, 70, 4, 16, true);
    MARCH_CASE(4, 70, 4, 25, true);
    MARCH_CASE(4, 71, 2, 25, true);
    MARCH_CASE(4, 72, 1, 25, true);
    MARCH_CASE(5, 70, 4, 36, true);
    MARCH_CASE(6, 70, 4, 49, true);
    MARCH_CASE(7, 70, 4, 64, true);
    MARCH_CASE(8, 70, 4, 81, true);
    // block-assembled kernel (compact cell blocks, LDS accumulator, no atomics), variants 50+;
    // a partial cell range cannot use the owner scatter and takes the atomic team kernel instead
#define BLOCK_CASE(P, V, LPC, TW_FALLBACK, PF)                                                                     \
  BP5_CASE(P, V) {                                                                                                 \
    if (c0 != 0 || c1 != mf->n_cells)                                                                              \
      return LAUNCH_COLL(launch_team_t, P, (TW_FALLBACK, LPC, PF), coef, src, dst, c0, c1, overwrite);              \
    return LAUNCH_COLL(launch_block_t, P, (LPC), coef, src, dst, overwrite); \
  }
    BLOCK_CASE(1, 50, 4, 4, true);
    BLOCK_CASE(2, 50, 9, 4, true);
    BLOCK_CASE(3, 50, 16, 4, true);
    BLOCK_CASE(4, 50, 25, 4, true);
    BLOCK_CASE(4, 51, 32, 4, true);
    if constexpr (DEG == 4) if (variant == 54 || variant == 55) {
      if (c0 == 0 && c1 == mf->n_cells) // (brick-surface DoFs by atomics: ApplyCall::shared_by_atomics)
        return variant == 54 ? LAUNCH_COLL(launch_block_t, 4, (32), coef, src, dst, overwrite) : LAUNCH_COLL(launch_block_t, 4, (25), coef, src, dst, overwrite);
      return LAUNCH_COLL(launch_team_t, 4, (4, 25, true), coef, src, dst, c0, c1, overwrite);
    }
#ifdef BP5_TIMING_BUILDS
    if constexpr (DEG == 6 || DEG == 8 || DEG == 5) if (variant == 99 || variant == 91 || variant == 93) { // cycle stamps / no write-out / no metric loads
      constexpr int LPCB = block_lpc(DEG);
      if (!block_aligned(mf, c0, c1, &call.b0, &call.b1)) return fail(BP5_ERR_INVALID, "needs aligned cell blocks");
      if (variant == 99) return launch_block_t<DEG, false, LPCB, BLK_DEFAULT | BLK_STAMPS>(mf, call, coef, src, dst, true);
      if (variant == 91) return launch_block_t<DEG, false, LPCB, BLK_DEFAULT | 1>(mf, call, coef, src, dst, true);
      return launch_block_t<DEG, false, LPCB, BLK_DEFAULT | 2>(mf, call, coef, src, dst, true);
    }
#endif
    // p = 4 A/B siblings of 56.  Three differ in the request only and go through launch_block_default:
    // 48 = 56 with the per-DoF CSR combine kernel instead of the run-length one
    // 49 = 56 with run-length write-out but without packed indices
    // 63 = 56 with the rolling metric prefetch (BlockPass::ROLL; lattice blocks only) -- libbp5_timing.so only: a measured loss (profiles/r4 d_*)
    if constexpr (DEG == 4) if (variant == 48 || variant == 49 || variant == 63) return launch_block_default<4>(mf, call, coef, src, dst);
    // ... three are builds of their own on the packed shape:
    // 60 = 56 with the brick's src staged once in LDS (cells gather from LDS)
    // 61 = 56 with non-temporal metric loads on packed indices (A/B: the once-read metric stream then evicts less of a brick's src from L2)
    // 62 = 56 with ds_add_f64 for the accumulation into the LDS vector
    if constexpr (DEG == 4) if (variant == 60 || variant == 61 || variant == 62) {
      if (!block_aligned(mf, c0, c1, &call.b0, &call.b1)) return fail(BP5_ERR_INVALID, "variant 56 needs a cell range aligned with the cell blocks");
      if (variant == 60) return LAUNCH_COLL(launch_block_t, 4, (32, BLK_DEFAULT | BLK_STAGE), coef, src, dst, overwrite);
      if (variant == 61) return LAUNCH_COLL(launch_block_t, 4, (32, BLK_DEFAULT | BLK_NTM), coef, src, dst, overwrite);
      return LAUNCH_COLL(launch_block_t, 4, (32, BLK_DEFAULT | BLK_LDSADD), coef, src, dst, overwrite);
    }
    BP5_CASE(4, 59) { if (c0 == 0 && c1 == mf->n_cells) return LAUNCH_COLL(launch_block_t, 4, (32, BLK_SINGLE | BLK_SEQ), coef, src, dst, overwrite);
      return fail(BP5_ERR_INVALID, "variant 59 needs the whole cell range"); }
    BP5_CASE(4, 57) { if (c0 == 0 && c1 == mf->n_cells) return LAUNCH_COLL(launch_block_t, 4, (32, BLK_SEQ), coef, src, dst, overwrite);
      return fail(BP5_ERR_INVALID, "variant 57 needs the whole cell range"); }
    BP5_CASE(4, 58) { if (c0 == 0 && c1 == mf->n_cells) return LAUNCH_COLL(launch_block_t, 4, (32, BLK_SINGLE | BLK_SEQ | BLK_NTM), coef, src, dst, overwrite);
      return fail(BP5_ERR_INVALID, "variant 58 needs the whole cell range"); }
#ifdef BP5_TIMING_BUILDS
    BP5_CASE(4, 99) return launch_block_t<4, false, 32, BLK_DEFAULT | BLK_STAMPS>(mf, call, coef, src, dst, true);   // stamps of the default shape (sequential tiles, 3 WG/CU, run write-out, packed indices)
#endif
    BP5_CASE(4, 52) { if (c0 == 0 && c1 == mf->n_cells) return LAUNCH_COLL(launch_block_t, 4, (32, BLK_SINGLE), coef, src, dst, overwrite);
      return fail(BP5_ERR_INVALID, "variant 52 needs the whole cell range"); }
    BP5_CASE(4, 53) { if (c0 == 0 && c1 == mf->n_cells) return LAUNCH_COLL(launch_block_t, 4, (25, BLK_SINGLE), coef, src, dst, overwrite);
      return fail(BP5_ERR_INVALID, "variant 53 needs the whole cell range"); }
#ifdef BP5_TIMING_BUILDS
    BP5_CASE(4, 64) return launch_block_t<4, false, 32, BLK_DEFAULT | BLK_LATT>(mf, call, coef, src, dst, true);              // the lattice build (reference point of the two probes below)
    BP5_CASE(4, 65) return launch_block_t<4, false, 32, BLK_DEFAULT | BLK_LATT | 33554432>(mf, call, coef, src, dst, true);   // ... metric as whole aligned lines, 12 instructions
    BP5_CASE(4, 66) return launch_block_t<4, false, 32, BLK_DEFAULT | BLK_LATT | 134217728>(mf, call, coef, src, dst, true);  // ... tails paired, 15 instructions
    BP5_CASE(4, 87) return launch_block_t<4, false, 32, BLK_SINGLE | BLK_SEQ | BLK_RUNS | 65536>(mf, call, coef, src, dst, true);  // variant 56 with plain (not non-temporal) stores
    BP5_CASE(4, 91) return launch_block_t<4, false, 32, BLK_SINGLE | BLK_SEQ | BLK_RUNS | 1>(mf, call, coef, src, dst, true);  // variant 56 without write-out (and combine)
    BP5_CASE(4, 93) return launch_block_t<4, false, 32, BLK_SINGLE | BLK_SEQ | BLK_RUNS | 2>(mf, call, coef, src, dst, true);  // ... without metric loads
    BP5_CASE(4, 95) return launch_block_t<4, false, 32, BLK_SINGLE | BLK_SEQ | BLK_RUNS | 4>(mf, call, coef, src, dst, true);  // ... without gather
    BP5_CASE(4, 97) return launch_block_t<4, false, 32, BLK_STAMPS>(mf, call, coef, src, dst, true);          // stamps, double-buffered
    BP5_CASE(4, 98) return launch_block_t<4, false, 32, BLK_STAMPS | BLK_SINGLE>(mf, call, coef, src, dst, true);   // stamps, single-buffered
    BP5_CASE(4, 92) return launch_block_t<4, false, 32, BLK_SINGLE | 1>(mf, call, coef, src, dst, true);
    BP5_CASE(4, 96) return launch_block_t<4, false, 32, BLK_SINGLE | 5>(mf, call, coef, src, dst, true);
#endif
    BLOCK_CASE(5, 50, 36, 4, true);
    BLOCK_CASE(6, 50, 49, 4, false);
    BLOCK_CASE(7, 50, 64, 4, false);
    BLOCK_CASE(8, 50, 81, 4, false);
#ifdef BP5_TIMING_BUILDS
#define BABL_CASE(M) BP5_CASE(4, 60 + (M)) return launch_block_t<4, false, 25, M>(mf, call, coef, src, dst, true)
    BABL_CASE(16); BABL_CASE(1); BABL_CASE(2); BABL_CASE(3); BABL_CASE(4); BABL_CASE(5); BABL_CASE(7); BABL_CASE(8); BABL_CASE(9); BABL_CASE(15);
    // timing-only ablations of the team kernel (SET mode): 40 + mask (1: no scatter stage, 4: no gather stage)
#define TABL_CASE(M)                                                                                               \
  BP5_CASE(4, 40 + (M)) {                                                                                         \
    TeamPlan tp; bp5_mf::DevPlan *dp = nullptr;                                                                    \
    BP5_TRY(get_plan(mf, 10, tp, &dp));                                                                            \
    ApplyArgs a = apply_args(mf, false, coef, src, dst);                                                           \
    a.cell_begin = c0; a.cell_end = c1; a.n_teams = (c1 + 9) / 10 - c0 / 10; a.teams_per_xcd = (a.n_teams + 7) / 8;  \
    ShapeArg<5> sh; fill_shape(sh, mf);                  \
    hipLaunchKernelGGL((apply_team_kernel<4, false, 4, 25, true, SC_OWNER_SET, M>), dim3(a.teams_per_xcd * 8), dim3(256), \
                       (10 * LdsLayout<5, 25>::CS * sizeof(double)), mf->stream, a, tp, sh);                          \
    KERNEL_CHECK(); return BP5_OK; }
    TABL_CASE(0); TABL_CASE(1); TABL_CASE(4); TABL_CASE(5);
#endif
    // team-assembled kernel (LDS-staged gather + scatter), variants 10+
    TEAM_CASE(1, 10, 4, 4, true);
    TEAM_CASE(2, 10, 4, 9, true);
    TEAM_CASE(3, 10, 4, 16, true);
    TEAM_CASE(4, 10, 4, 25, true);
    TEAM_CASE(4, 11, 8, 25, true);
    TEAM_CASE(4, 12, 4, 25, false);
    TEAM_CASE(4, 13, 2, 25, true);
    BP5_CASE(4, 14) return LAUNCH_COLL(launch_team_t, 4, (4, 25, true, 32), coef, src, dst, c0, c1, overwrite);
    TEAM_CASE(5, 10, 4, 36, true);
    TEAM_CASE(6, 10, 4, 49, false);
    TEAM_CASE(7, 10, 4, 64, false);
    TEAM_CASE(8, 10, 4, 81, false);
  }
  return fail(BP5_ERR_INVALID, "unknown (degree, apply variant)");
}

#define BP5_EXTERN_DEGREE(N) extern template int apply_degree_impl<N>(bp5_mf *, ApplyCall &, const double *, const double *, double *);
BP5_EXTERN_DEGREE(1) BP5_EXTERN_DEGREE(2) BP5_EXTERN_DEGREE(3) BP5_EXTERN_DEGREE(4) BP5_EXTERN_DEGREE(5) BP5_EXTERN_DEGREE(6) BP5_EXTERN_DEGREE(7) BP5_EXTERN_DEGREE(8)

#define BP5_EXTERN_COMPONENTS_DEGREE(N) extern template int apply_components_degree_impl<N>(bp5_mf *, const double *, int, size_t, const double *, double *, uint32_t, uint32_t);
BP5_EXTERN_COMPONENTS_DEGREE(1) BP5_EXTERN_COMPONENTS_DEGREE(2) BP5_EXTERN_COMPONENTS_DEGREE(3) BP5_EXTERN_COMPONENTS_DEGREE(4)
BP5_EXTERN_COMPONENTS_DEGREE(5) BP5_EXTERN_COMPONENTS_DEGREE(6) BP5_EXTERN_COMPONENTS_DEGREE(7) BP5_EXTERN_COMPONENTS_DEGREE(8)
