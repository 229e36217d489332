// C-ABI implementation: MatrixFree handle, operator launches, BLAS-1, CG drivers, RCCL halo.
// Every entry point cites the reference interface it replaces in include/bp5.h.
#include "bp5_device.hpp"


// ------------------------------------------------------------------------------------ device / vectors
extern "C" int bp5_device_count(int *count)
{
  if (!count) return fail(BP5_ERR_INVALID, "null argument");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) { *count = 0; return fail(BP5_ERR_NO_DEVICE, hipGetErrorString(e)); }
  *count = c;
  return BP5_OK;
}
extern "C" int bp5_vec_alloc(size_t n, double **out)
{
  if (!out) return fail(BP5_ERR_INVALID, "null argument");
  HIP_TRY(hipMalloc((void **)out, std::max<size_t>(n, 1) * sizeof(double)));
  HIP_TRY(hipMemset(*out, 0, std::max<size_t>(n, 1) * sizeof(double)));
  HIP_TRY(hipStreamSynchronize(nullptr)); // the fill runs on the null stream; callers use it on (possibly non-blocking) streams
  return BP5_OK;
}
extern "C" int bp5_vec_free(double *v) { HIP_TRY(hipFree(v)); return BP5_OK; }
extern "C" int bp5_copy_h2d(void *dst, const void *src, size_t bytes) { HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return BP5_OK; }
extern "C" int bp5_copy_d2h(void *dst, const void *src, size_t bytes) { HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return BP5_OK; }

// ------------------------------------------------------------------------------------ create / destroy
static void tuning_from_environment(bp5_mf *mf);
static void pack_tab(const Tables &t, std::vector<double> &v)
{
  const int n = t.n, nq = t.nq; // N[nq n], D[nq n], w[nq]
  v.assign(2 * nq * n + nq, 0.0);
  memcpy(v.data(), t.N, nq * n * sizeof(double));
  memcpy(v.data() + nq * n, t.D, nq * n * sizeof(double));
  memcpy(v.data() + 2 * nq * n, t.w, nq * sizeof(double));
}

extern "C" int bp5_mf_create(const bp5_mf_desc *d, bp5_mf **out)
{
  if (!d || !out) return fail(BP5_ERR_INVALID, "null argument");
  if (d->dim != 3) return fail(BP5_ERR_UNSUPPORTED, "only dim == 3");
  if (!d->local_to_global_host || !d->node_coords_host) return fail(BP5_ERR_INVALID, "mesh arrays missing");
  if (d->n_interior_cells > d->n_cells) return fail(BP5_ERR_INVALID, "n_interior_cells > n_cells");
  Tables tab, tabg;
  BP5_TRY(shape_tables(d->degree, d->quadrature, tab));
  BP5_TRY(shape_tables(d->degree, BP5_QUAD_GAUSS, tabg));
  int ndev = 0;
  BP5_TRY(bp5_device_count(&ndev));
  if (ndev <= 0) return fail(BP5_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
  if (d->device < 0 || d->device >= ndev) return fail(BP5_ERR_INVALID, "bad device ordinal");
  HIP_TRY(hipSetDevice(d->device));
  bp5_mf *mf = new bp5_mf;
  struct Guard { // every early return below releases the handle and whatever has been uploaded so far
    bp5_mf *m;
    ~Guard() { if (m) bp5_mf_destroy(m); }
  } guard{mf};
  mf->degree = d->degree; mf->quadrature = d->quadrature; mf->coefficient = d->coefficient;
  mf->n = d->degree + 1; mf->n3 = mf->n * mf->n * mf->n; mf->device = d->device;
  mf->nq = tab.nq; mf->nq3 = tab.nq * tab.nq * tab.nq;
  mf->n_cells = d->n_cells; mf->n_interior = d->n_interior_cells; mf->n_owned = d->n_owned; mf->n_ghost = d->n_ghost;
  mf->n_constrained = d->n_constrained;
  mf->tab = tab; mf->tab_gauss = tabg;
  tuning_from_environment(mf);
  { // metric layout (A/B knob: BP5_COEF_LAYOUT = plane | cell)
    const char *e = getenv("BP5_COEF_LAYOUT");
    const bool cell_major = e && !strcmp(e, "cell") && !mf->overint(); // (an over-integrated handle keeps the plane-major layout)
    mf->coef_plane_stride = cell_major ? (uint64_t)mf->n3 : (uint64_t)mf->n_cells * mf->nq3;
    mf->coef_cell_stride = cell_major ? (uint64_t)6 * mf->n3 : (uint64_t)mf->nq3;
  }
  // validate indices on the host: a bad index would fault on the GPU
  const size_t nl = (size_t)d->n_cells * mf->n3, nloc = mf->n_local();
  for (size_t s = 0; s < nl; ++s)
    if (d->local_to_global_host[s] >= nloc) { return fail(BP5_ERR_INVALID, "local_to_global entry out of range"); }
  for (uint32_t s = 0; s < d->n_constrained; ++s)
    if (d->constrained_host[s] >= nloc) { return fail(BP5_ERR_INVALID, "constrained index out of range"); }
  { // are the DoFs strictly inside a cell numbered ahead of all others, cell after cell, x fastest?  (bp5_mesh_desc.dof_numbering = 2, or any mesh numbered so)
    const int p = d->degree, n = p + 1;
    const uint32_t per = (uint32_t)((p - 1) * (p - 1) * (p - 1));
    bool ok = p >= 2 && d->n_cells > 0 && (uint64_t)d->n_cells * per <= d->n_owned;
    for (uint32_t c = 0; ok && c < d->n_cells; ++c) {
      const uint32_t *l = d->local_to_global_host + (size_t)c * mf->n3;
      uint32_t e = c * per;
      for (int k = 1; ok && k < p; ++k)
        for (int j = 1; j < p; ++j)
          for (int i = 1; i < p; ++i, ++e)
            if (l[i + n * (j + n * k)] != e) ok = false;
    }
    mf->cell_interiors_first = ok;
  }
  mf->stream = (hipStream_t)d->stream; // NULL == the HIP default stream (ordered with the host's other default-stream work)
  BP5_TRY(upload(&mf->d_l2g, d->local_to_global_host, nl));
  mf->h_l2g.assign(d->local_to_global_host, d->local_to_global_host + nl);
  if (d->n_cell_blocks && d->cell_block_offsets_host) {
    const uint32_t *o = d->cell_block_offsets_host;
    bool ok = o[0] == 0 && o[d->n_cell_blocks] == d->n_cells;
    for (uint32_t b = 0; ok && b < d->n_cell_blocks; ++b) ok = o[b] < o[b + 1];
    if (!ok) { return fail(BP5_ERR_INVALID, "cell_block_offsets must ascend from 0 to n_cells"); }
    mf->h_block_off.assign(o, o + d->n_cell_blocks + 1);
  }
  BP5_TRY(upload(&mf->d_coords, d->node_coords_host, nloc * 3));
  BP5_TRY(upload(&mf->d_constrained, d->constrained_host, d->n_constrained));
  mf->h_constrained.assign(nloc, false);
  for (uint32_t s = 0; s < d->n_constrained; ++s) mf->h_constrained[d->constrained_host[s]] = true;
  {
    std::vector<uint32_t> bits((size_t)d->n_owned / 32 + 2, 0u);
    for (uint32_t s = 0; s < d->n_constrained; ++s)
      if (d->constrained_host[s] < d->n_owned) bits[d->constrained_host[s] >> 5] |= 1u << (d->constrained_host[s] & 31);
    BP5_TRY(upload(&mf->d_constrained_bits, bits.data(), bits.size()));
  }
  std::vector<double> tv;
  pack_tab(tab, tv);  BP5_TRY(upload(&mf->d_tab, tv.data(), tv.size()));
  pack_tab(tabg, tv); BP5_TRY(upload(&mf->d_tab_gauss, tv.data(), tv.size()));
  // hanging nodes: validate the masks on the host, upload them and the two 1-D interpolation matrices
  if (d->constraint_mask_host) {
    std::vector<uint32_t> hm(d->constraint_mask_host, d->constraint_mask_host + d->n_cells);
    for (uint32_t m : hm) {
      if (!m) continue;
      if (m >> 12) return fail(BP5_ERR_INVALID, "constraint_mask: unknown bits");
      if (!(m & 0xe07u)) return fail(BP5_ERR_INVALID, "constraint_mask: position bits without a constrained face or edge");
      for (int e = 0; e < 3; ++e) // one position per direction: it locates faces / edges AND selects the half of the coarse entity
        if (((m >> (3 + e)) & 1u) != ((m >> (6 + e)) & 1u)) {
          // planar round-2 masks name only what they use (SIDE of the face's normal, HALF of its two tangential directions)
          const int e1 = e == 0 ? 1 : 0, e2 = e == 2 ? 1 : 2;
          const bool side_used = ((m >> e) & 1u) || ((m >> (9 + e1)) & 1u) || ((m >> (9 + e2)) & 1u);
          const bool half_used = ((m >> e1) & 1u) || ((m >> e2) & 1u) || ((m >> (9 + e)) & 1u);
          if (side_used && half_used) return fail(BP5_ERR_INVALID, "constraint_mask: BP5_HANG_SIDE_d and BP5_HANG_HALF_d disagree");
        }
      mf->has_hanging = true;
    }
    if (mf->has_hanging && mf->overint()) return overint_refuse("meshes with hanging nodes are not supported");
    if (mf->has_hanging) {
      BP5_TRY(upload(&mf->d_hang_mask, hm.data(), hm.size()));
      const int n = mf->n;
      std::vector<double> I(2 * n * n);
      for (int h = 0; h < 2; ++h)
        for (int a = 0; a < n; ++a) {
          const long double x = 0.5L * tab.nodes[a] + 0.5L * h;
          for (int b = 0; b < n; ++b) { // Lagrange polynomial of node b at x
            long double num = 1, den = 1;
            for (int c = 0; c < n; ++c) if (c != b) { num *= x - (long double)tab.nodes[c]; den *= (long double)tab.nodes[b] - (long double)tab.nodes[c]; }
            I[(h * n + a) * n + b] = (double)(num / den);
          }
        }
      BP5_TRY(upload(&mf->d_hang_I, I.data(), I.size()));
    }
  }
  // halo plan
  if (d->n_neighbors > 0) {
    if (!d->neighbor_rank_host || !d->send_offsets_host || !d->recv_offsets_host) { return fail(BP5_ERR_INVALID, "halo plan arrays missing"); }
    mf->neighbors.assign(d->neighbor_rank_host, d->neighbor_rank_host + d->n_neighbors);
    mf->send_off.assign(d->send_offsets_host, d->send_offsets_host + d->n_neighbors + 1);
    mf->recv_off.assign(d->recv_offsets_host, d->recv_offsets_host + d->n_neighbors + 1);
    const uint32_t ns = mf->send_off.back();
    if (mf->recv_off.back() != d->n_ghost) { return fail(BP5_ERR_INVALID, "recv ranges must cover the ghost range"); }
    for (uint32_t s = 0; s < ns; ++s)
      if (d->send_indices_host[s] >= d->n_owned) { return fail(BP5_ERR_INVALID, "send index out of owned range"); }
    BP5_TRY(upload(&mf->d_send_idx, d->send_indices_host, ns));
    std::vector<uint8_t> sd(ns);
    for (uint32_t s = 0; s < ns; ++s) sd[s] = mf->h_constrained[d->send_indices_host[s]] ? 1 : 0;
    BP5_TRY(upload(&mf->d_send_dirichlet, sd.data(), sd.size()));
    HIP_TRY(hipMalloc((void **)&mf->d_sendbuf, std::max<size_t>(ns, 1) * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&mf->d_recvbuf, std::max<size_t>(ns, 1) * sizeof(double)));
  } else if (d->n_ghost) { return fail(BP5_ERR_INVALID, "ghosts without a halo plan"); }
  // solver workspace
  HIP_TRY(hipMalloc((void **)&mf->d_partials, 8 * PARTIAL_STRIDE * sizeof(double)));
  HIP_TRY(hipMalloc((void **)&mf->d_sc, SC_COUNT * sizeof(double)));
  HIP_TRY(hipMalloc((void **)&mf->d_scalar, 8 * sizeof(double)));
  HIP_TRY(hipMalloc((void **)&mf->d_st, ST_COUNT * sizeof(int)));
  HIP_TRY(hipMemset(mf->d_sc, 0, SC_COUNT * sizeof(double)));
  HIP_TRY(hipMemset(mf->d_st, 0, ST_COUNT * sizeof(int)));
  HIP_TRY(hipStreamSynchronize(nullptr)); // null-stream fills must not race with work on a non-blocking handle stream
  HIP_TRY(hipHostMalloc((void **)&mf->h_sc, SC_COUNT * sizeof(double)));
  HIP_TRY(hipHostMalloc((void **)&mf->h_st, ST_COUNT * sizeof(int)));
  HIP_TRY(hipEventCreate(&mf->ev_solve[0]));
  HIP_TRY(hipEventCreate(&mf->ev_solve[1]));
  guard.m = nullptr;
  *out = mf;
  return BP5_OK;
}

extern "C" int bp5_mf_destroy(bp5_mf *mf)
{
  if (!mf) return BP5_OK;
  hipSetDevice(mf->device);
  hipStreamSynchronize(mf->stream);
  void *ptrs[] = {mf->d_constrained_bits, mf->d_l2g, mf->d_constrained, mf->d_send_idx, mf->d_coords, mf->d_tab, mf->d_tab_gauss, mf->d_l2g_padded,
                  mf->d_constraint_mask, mf->d_inv_jac, mf->d_JxW, mf->d_qpoints, mf->d_sendbuf, mf->d_recvbuf, mf->d_partials,
                  mf->d_sc, mf->d_scalar, mf->d_st, mf->ws_base, mf->d_stamps, mf->d_evec, mf->d_scalar_plane, mf->d_gcell, mf->d_vertices, mf->d_hang_mask, mf->d_hang_I, mf->d_send_dirichlet, mf->d_signal, mf->ws_z, mf->wsc_base, mf->wsz_base, mf->wsn_base, mf->hc_base, mf->d_hc_off};
  for (void *p : ptrs) if (p) hipFree(p);
  if (mf->h_sc) hipHostFree(mf->h_sc);
  if (mf->h_st) hipHostFree(mf->h_st);
  for (hipEvent_t e : mf->ev_pool) hipEventDestroy(e);
  for (hipEvent_t e : mf->phase.ev) hipEventDestroy(e);
  for (hipEvent_t e : mf->ev_solve) if (e) hipEventDestroy(e);
  for (hipEvent_t e : mf->ev_halo) if (e) hipEventDestroy(e);
  for (hipEvent_t e : mf->ev_done) if (e) hipEventDestroy(e);
  if (mf->h_done) hipHostFree(mf->h_done);
  if (mf->comm_stream) { hipStreamSynchronize(mf->comm_stream); hipStreamDestroy(mf->comm_stream); }
  for (auto &kv : mf->march_plans) { hipFree(kv.second.team_off); hipFree(kv.second.entries); }
  for (auto &kv : mf->plans) {
    auto &q = kv.second;
    void *pp[] = {q.off, q.dofs, q.sh_dof, q.sh_off, q.sh_slot, q.pos, q.cell_round, q.team_rounds, q.partial, q.cell_off, q.pass_cell, q.pass_off, q.run_off, q.runs, q.gidx, q.packed, q.lattice, q.cell_pos, q.cr_start, q.cr_dof0, q.cr_soff, q.cr_slots, q.cr_tile};
    for (void *x : pp) if (x) hipFree(x);
    if (q.wg_blocks) { for (auto &w : *q.wg_blocks) hipFree(w.second); delete q.wg_blocks; }
    if (q.cr_carry) {
      for (auto &c : *q.cr_carry) { void *cc[] = {c.second.start, c.second.dof0, c.second.soff, c.second.slots, c.second.tile}; for (void *x : cc) if (x) hipFree(x); }
      delete q.cr_carry;
    }
  }
  if (mf->own_stream) hipStreamDestroy(mf->stream);
  delete mf;
  return BP5_OK;
}
extern "C" int bp5_mf_set_stream(bp5_mf *mf, void *s)
{
  if (!mf) return fail(BP5_ERR_INVALID, "null handle");
  if (mf->own_stream) { hipStreamSynchronize(mf->stream); hipStreamDestroy(mf->stream); mf->own_stream = false; }
  mf->stream = (hipStream_t)s;
  return BP5_OK;
}
extern "C" int bp5_mf_sync(bp5_mf *mf)
{
  if (!mf) return fail(BP5_ERR_INVALID, "null handle");
  HIP_TRY(hipStreamSynchronize(mf->stream));
  return BP5_OK;
}
extern "C" int bp5_mf_coef_size(const bp5_mf *mf, size_t *n)
{
  if (!mf || !n) return fail(BP5_ERR_INVALID, "null argument");
  *n = (size_t)mf->n_planes() * mf->n_cells * mf->nq3; // (nq3 == n3 but on a BP5_QUAD_GAUSS_OVER handle: (p+2)^3)
  if (mf->f32_metric()) *n = (*n + 1) / 2; // float entries: the doubles that hold them
  mf->coef_planes_committed = mf->n_planes();
  return BP5_OK;
}
extern "C" int bp5_mf_set_metric_precision(bp5_mf *mf, int precision)
{
  if (!mf) return fail(BP5_ERR_INVALID, "null handle");
  if (precision != BP5_METRIC_F64 && precision != BP5_METRIC_F32) return fail(BP5_ERR_INVALID, "unknown metric precision");
  if (precision == mf->metric_precision) return BP5_OK;
  if (mf->coef_planes_committed)
    return fail(BP5_ERR_INVALID, "the metric array of this handle has been sized or filled in another precision: set the metric precision before bp5_mf_coef_size / bp5_mf_compute_merged_metric");
  if (precision == BP5_METRIC_F32) {
    if (mf->overint()) return overint_refuse("FP32 metric planes are not supported");
    if (mf->has_hanging) return fail(BP5_ERR_UNSUPPORTED, "FP32 metric planes: meshes with hanging nodes keep double planes");
    if (mf->operator_kind == BP5_OP_HELMHOLTZ) return fail(BP5_ERR_UNSUPPORTED, "FP32 metric planes: the Helmholtz operator keeps double planes");
    if (mf->operator_kind == BP5_OP_MASS) return fail(BP5_ERR_UNSUPPORTED, "FP32 metric planes: the mass operator keeps its double plane");
    if (mf->trilinear()) return trilinear_refuse("FP32 metric planes are not supported (the mode reads no plane)");
    if (mf->geometry_mode == BP5_GEOM_AFFINE) return fail(BP5_ERR_UNSUPPORTED, "FP32 metric planes: the affine geometry mode has no six-plane stream to shrink");
    if (mf->apply_variant != 0 && mf->apply_variant != 56) return fail(BP5_ERR_UNSUPPORTED, "FP32 metric planes run apply variants 0 (pencil kernel) and 56 (block kernel)");
  }
  mf->metric_precision = precision;
  mf->auto_block = -1; // (decided per precision: the FP32 block builds need the packed indices at every degree)
  return BP5_OK;
}
extern "C" int bp5_mf_get_metric_precision(const bp5_mf *mf, int *precision)
{
  if (!mf || !precision) return fail(BP5_ERR_INVALID, "null argument");
  *precision = mf->metric_precision;
  return BP5_OK;
}
extern "C" int bp5_mf_set_operator(bp5_mf *mf, int op)
{
  if (!mf || (op != BP5_OP_POISSON && op != BP5_OP_HELMHOLTZ && op != BP5_OP_MASS)) return fail(BP5_ERR_INVALID, "unknown operator");
  if (op == BP5_OP_HELMHOLTZ && mf->trilinear()) return trilinear_refuse("the Helmholtz operator is not supported (Poisson operator only)");
  if (op == BP5_OP_MASS && mf->trilinear()) return trilinear_refuse("the mass operator is not supported (Poisson operator only)");
  if (op == BP5_OP_HELMHOLTZ && mf->overint()) return overint_refuse("the Helmholtz operator is not supported (Poisson and mass operator only)");
  if (op == BP5_OP_HELMHOLTZ && mf->f32_metric()) return fail(BP5_ERR_UNSUPPORTED, "the Helmholtz operator keeps double metric planes (bp5_mf_set_metric_precision)");
  if (op == BP5_OP_HELMHOLTZ && (mf->has_hanging || mf->geometry_mode == BP5_GEOM_AFFINE))
    return fail(BP5_ERR_UNSUPPORTED, "the Helmholtz operator needs a conforming mesh and the six-plane geometry (hanging nodes: the facade's FEEvaluation)");
  if (op == BP5_OP_HELMHOLTZ && mf->apply_variant != 0 && mf->apply_variant != 56) return fail(BP5_ERR_UNSUPPORTED, "the Helmholtz operator runs apply variants 0 and 56");
  if (op == BP5_OP_MASS) {
    if (mf->f32_metric()) return fail(BP5_ERR_UNSUPPORTED, "the mass operator keeps a double metric plane (bp5_mf_set_metric_precision: FP32 planes are not supported)");
    if (mf->has_hanging) return fail(BP5_ERR_UNSUPPORTED, "the mass operator needs a conforming mesh (hanging nodes: the facade's FEEvaluation)");
    if (mf->geometry_mode == BP5_GEOM_AFFINE) return fail(BP5_ERR_UNSUPPORTED, "the mass operator has no build for the affine geometry mode");
    if (mf->apply_variant != 0 && mf->apply_variant != 56) return fail(BP5_ERR_UNSUPPORTED, "the mass operator runs apply variants 0 and 56");
    if (mf->coef_cell_stride != (uint64_t)mf->nq3) return fail(BP5_ERR_UNSUPPORTED, "the mass operator needs the plane-major metric layout");
  }
  if (mf->coef_planes_committed && mf->coef_planes_committed != bp5_mf::planes_of(op))
    return fail(BP5_ERR_INVALID, "the metric array of this handle has been sized or filled for another plane count: set the operator before bp5_mf_coef_size / bp5_mf_compute_merged_metric");
  mf->operator_kind = op;
  mf->auto_block = -1; // (decided per operator: the Helmholtz build of the block kernel runs two workgroups per CU)
  return BP5_OK;
}
// the variants of the product library: every one of them computes the operator (they differ in launch shape, staging and
// scatter strategy).  The timing-only ablation builds (wrong results by construction) exist only in libbp5_timing.so
// (make timing, -DBP5_TIMING_BUILDS; used by tools/bench_apply.py) and are refused here.
static bool product_variant(int degree, int v)
{
  if (v == 0) return true;
  const VariantInfo d = decode_variant(v);
  if (d.atomic_scatter) return v < 200 && d.family == VARIANT_TEAM && product_variant(degree, v - 100); // team kernel, atomic scatter
  if (v == 10 || v == 50 || v == 70) return true;
  if (d.family == VARIANT_BLOCK && block_lpc(degree) != 0) return true;
  switch (degree) {
    case 1: case 3: return v == 1;
    case 4: return (v >= 1 && v <= 6) || (v >= 11 && v <= 14) || (v >= 48 && v <= 62) || v == 71 || v == 72;
    case 5: return v >= 1 && v <= 3;
    case 6: return v >= 1 && v <= 5;
    case 7: case 8: return (v >= 1 && v <= 3) || v == 5;
  }
  return false;
}
extern "C" int bp5_mf_set_apply_variant(bp5_mf *mf, int v)
{
  if (!mf) return fail(BP5_ERR_INVALID, "null handle");
  if (mf->trilinear() && v != 0) return trilinear_refuse("only apply variant 0, the pencil kernel apply_pencil_trilinear_kernel (no block, team or march build)");
  if (mf->overint() && v != 0) return overint_refuse("only apply variant 0, the pencil kernel apply_pencil_q_kernel / apply_pencil_mass_q_kernel (no block, team or march build)");
  if (mf->has_hanging) { // 0: the library decides; 56: block kernel (deterministic; needs cell blocks); 90: pencil kernel with atomics (any mesh)
    if (v != 0 && v != 90 && !(v == 56 && block_lpc(mf->degree) != 0)) return fail(BP5_ERR_UNSUPPORTED, "meshes with hanging nodes run apply variants 90 (pencil kernel) and 56 (block kernel)");
    if (v == 56 && mf->geometry_mode == BP5_GEOM_AFFINE) return fail(BP5_ERR_UNSUPPORTED, "hanging nodes in the affine geometry mode run the pencil kernel: apply variants 0 and 90");
    mf->apply_variant = v;
    return BP5_OK;
  }
  if (v == 90) return fail(BP5_ERR_INVALID, "apply variant 90 is the hanging-node kernel: the mesh has no constraint masks");
  if (mf->f32_metric() && v != 0 && !(v == 56 && block_lpc(mf->degree) != 0)) return fail(BP5_ERR_UNSUPPORTED, "FP32 metric planes run apply variants 0 (pencil kernel) and 56 (block kernel)");
  if (mf->operator_kind == BP5_OP_MASS && v != 0 && !(v == 56 && block_lpc(mf->degree) != 0)) return fail(BP5_ERR_UNSUPPORTED, "the mass operator runs apply variants 0 (pencil kernel) and 56 (block kernel)");
#ifndef BP5_TIMING_BUILDS
  if (mf->operator_kind == BP5_OP_HELMHOLTZ && v != 0 && !(v == 56 && block_lpc(mf->degree) != 0)) return fail(BP5_ERR_UNSUPPORTED, "the Helmholtz operator runs apply variants 0 (pencil kernel) and 56 (block kernel)");
#endif
#ifndef BP5_TIMING_BUILDS
  if (!product_variant(mf->degree, v)) return fail(BP5_ERR_INVALID, "unknown (degree, apply variant): timing-only builds live in libbp5_timing.so");
#endif
  mf->apply_variant = v;
  return BP5_OK;
}

static int effective_variant(bp5_mf *mf, uint32_t c0, uint32_t c1);
extern "C" int bp5_mf_set_cg_fusion(bp5_mf *mf, int on)
{
  if (!mf) return fail(BP5_ERR_INVALID, "null handle");
  mf->cg_fusion = on != 0;
  return BP5_OK;
}
extern "C" int bp5_mf_set_block_workgroups(bp5_mf *mf, int max_workgroups)
{
  if (!mf || max_workgroups < 0) return fail(BP5_ERR_INVALID, "bad argument");
  mf->block_max_wg = max_workgroups;
  return BP5_OK;
}
extern "C" int bp5_mf_set_streaming(bp5_mf *mf, int policy)
{
  if (!mf || policy < -1 || policy > 1) return fail(BP5_ERR_INVALID, "bad argument");
  mf->streaming = policy;
  return BP5_OK;
}
extern "C" int bp5_mf_block_plan_info(bp5_mf *mf, uint32_t *n_blocks, uint32_t *max_runs, int *packed_indices)
{
  if (!mf || !n_blocks || !max_runs || !packed_indices) return fail(BP5_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(mf->device));
  bp5_mf::DevPlan *dp = nullptr;
  BP5_TRY(get_plan_raw(mf, -block_cpt(mf), &dp, 64));
  *n_blocks = dp->n_groups;
  *max_runs = dp->max_runs;
  *packed_indices = dp->packed != nullptr;
  return BP5_OK;
}
extern "C" int bp5_mf_block_plan_lattice(bp5_mf *mf, uint32_t *n_lattice_blocks)
{
  if (!mf || !n_lattice_blocks) return fail(BP5_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(mf->device));
  bp5_mf::DevPlan *dp = nullptr;
  BP5_TRY(get_plan_raw(mf, -block_cpt(mf), &dp, 64));
  *n_lattice_blocks = dp->n_lattice_blocks;
  return BP5_OK;
}
extern "C" int bp5_mf_block_plan_carry(bp5_mf *mf, uint32_t *n_faces, uint32_t *n_shared, uint32_t *n_shared_last_launch)
{
  if (!mf || !n_faces || !n_shared || !n_shared_last_launch) return fail(BP5_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(mf->device));
  bp5_mf::DevPlan *dp = nullptr;
  BP5_TRY(get_plan_raw(mf, -block_cpt(mf), &dp, 64));
  *n_faces = 0;
  for (uint32_t len : dp->h_carry_len) *n_faces += len != 0;
  *n_shared = dp->n_shared;
  *n_shared_last_launch = dp->cr_last_launch ? dp->cr_last_launch->n_shared : dp->n_shared;
  return BP5_OK;
}
extern "C" int bp5_mf_get_apply_variant(bp5_mf *mf, int *effective)
{
  if (!mf || !effective) return fail(BP5_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(mf->device));
  *effective = effective_variant(mf, 0, mf->n_cells);
  return BP5_OK;
}

// ------------------------------------------------------------------------------------ geometry
template <int n>
static int launch_geometry(bp5_mf *mf, GeomOut o)
{
  const uint32_t grid = cell_grid(mf, 65535u * 16);
  o.hang_mask = mf->has_hanging ? mf->d_hang_mask : nullptr;
  o.hang_I = mf->d_hang_I;
  if (o.coef && mf->f32_metric()) // float planes behind o.coef (affine / Data-mirror launches write no planes: the double build)
    hipLaunchKernelGGL((geometry_kernel<n, float>), dim3(grid), dim3(n, n, n), 0, mf->stream, mf->d_l2g, mf->d_coords, mf->d_tab, mf->coefficient,
                       mf->n_cells, o);
  else
    hipLaunchKernelGGL(geometry_kernel<n>, dim3(grid), dim3(n, n, n), 0, mf->stream, mf->d_l2g, mf->d_coords, mf->d_tab, mf->coefficient,
                       mf->n_cells, o);
  KERNEL_CHECK();
  return BP5_OK;
}

// the geometry launch of the handle's degree (the planes, the affine scalars or the Data mirror: whatever o asks for)
static int geometry_dispatch(bp5_mf *mf, GeomOut o)
{
  return for_degree(mf->degree, [&](auto P) { return launch_geometry<P() + 1>(mf, o); });
}
extern "C" int bp5_mf_set_geometry_mode(bp5_mf *mf, int mode)
{
  if (!mf) return fail(BP5_ERR_INVALID, "null handle");
  if (mode != BP5_GEOM_MERGED6 && mode != BP5_GEOM_AFFINE && mode != BP5_GEOM_TRILINEAR) return fail(BP5_ERR_INVALID, "unknown geometry mode");
  HIP_TRY(hipSetDevice(mf->device));
  if (mode == BP5_GEOM_TRILINEAR) {
    if (mf->overint()) return trilinear_refuse("Gauss(p+2) quadrature (BP5_QUAD_GAUSS_OVER) is not supported");
    if (mf->operator_kind == BP5_OP_HELMHOLTZ) return trilinear_refuse("the Helmholtz operator is not supported (Poisson operator only)");
    if (mf->operator_kind == BP5_OP_MASS) return trilinear_refuse("the mass operator is not supported (Poisson operator only)");
    if (mf->has_hanging) return trilinear_refuse("meshes with hanging nodes are not supported");
    if (mf->f32_metric()) return trilinear_refuse("FP32 metric planes are not supported (the mode reads no plane)");
    if (mf->apply_variant != 0) return trilinear_refuse("only apply variant 0, the pencil kernel apply_pencil_trilinear_kernel (no block, team or march build)");
    if (!mf->d_vertices) { // the cells' corners, and the check that every node is the trilinear image of its reference position
      double *vx = nullptr, *dev = nullptr;
      HIP_TRY(hipMalloc((void **)&vx, std::max<size_t>(24 * (size_t)mf->n_cells, 1) * sizeof(double)));
      HIP_TRY(hipMalloc((void **)&dev, std::max<size_t>(mf->n_cells, 1) * sizeof(double)));
      int st = trilinear_setup(mf, vx, dev);
      std::vector<double> h(mf->n_cells);
      if (st == BP5_OK && hipMemcpyAsync(h.data(), dev, mf->n_cells * sizeof(double), hipMemcpyDeviceToHost, mf->stream) != hipSuccess) st = BP5_ERR_HIP;
      if (st == BP5_OK && hipStreamSynchronize(mf->stream) != hipSuccess) st = BP5_ERR_HIP;
      hipFree(dev);
      double worst = 0.0;
      for (double v : h) worst = std::max(worst, v);
      if (st != BP5_OK || !(worst <= 1e-10)) { // (the affine mode's threshold: rounding noise is ~eps |x| / h, real curvature orders larger)
        hipFree(vx);
        if (st != BP5_OK) return fail(st, "trilinear geometry setup failed");
        return fail(BP5_ERR_UNSUPPORTED, "mesh is not trilinear (a node is off the trilinear image of its cell's vertices): use BP5_GEOM_MERGED6");
      }
      mf->d_vertices = vx;
    }
    mf->geometry_mode = mode;
    return BP5_OK;
  }
  if (mode == BP5_GEOM_AFFINE && mf->overint()) return overint_refuse("the affine geometry mode is not supported");
  if (mode == BP5_GEOM_AFFINE && mf->f32_metric()) return fail(BP5_ERR_UNSUPPORTED, "FP32 metric planes need the six-plane geometry (the affine mode has no six-plane stream to shrink)");
  if (mode == BP5_GEOM_AFFINE && mf->operator_kind == BP5_OP_HELMHOLTZ) return fail(BP5_ERR_UNSUPPORTED, "the Helmholtz operator needs the six-plane geometry");
  if (mode == BP5_GEOM_AFFINE && mf->operator_kind == BP5_OP_MASS) return fail(BP5_ERR_UNSUPPORTED, "the mass operator has no build for the affine geometry mode");
  if (mode == BP5_GEOM_AFFINE && mf->has_hanging && mf->apply_variant == 56) return fail(BP5_ERR_UNSUPPORTED, "hanging nodes in the affine geometry mode run the pencil kernel: set apply variant 0 or 90 first");
  if (mode == BP5_GEOM_AFFINE && !mf->d_scalar_plane) {
    double *sp = nullptr, *gc = nullptr, *dev = nullptr;
    const size_t nq = (size_t)mf->n_cells * mf->n3;
    HIP_TRY(hipMalloc((void **)&sp, std::max<size_t>(nq, 1) * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&gc, std::max<size_t>(6 * (size_t)mf->n_cells, 1) * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&dev, std::max<size_t>(mf->n_cells, 1) * sizeof(double)));
    GeomOut o{};
    o.scalar = sp; o.gcell = gc; o.deviation = dev; o.n_cells = mf->n_cells;
    int st = geometry_dispatch(mf, o);
    std::vector<double> h(mf->n_cells);
    if (st == BP5_OK && hipMemcpyAsync(h.data(), dev, mf->n_cells * sizeof(double), hipMemcpyDeviceToHost, mf->stream) != hipSuccess) st = BP5_ERR_HIP;
    if (st == BP5_OK && hipStreamSynchronize(mf->stream) != hipSuccess) st = BP5_ERR_HIP;
    hipFree(dev);
    double worst = 0.0;
    for (double v : h) worst = std::max(worst, v);
    if (st != BP5_OK || !(worst <= 1e-10)) { // rounding noise of the Jacobian is ~eps*|x|/h; real curvature is orders larger
      hipFree(sp); hipFree(gc);
      if (st != BP5_OK) return fail(st, "affine geometry setup failed");
      return fail(BP5_ERR_UNSUPPORTED, "mesh is not affine (K K^T varies inside a cell): use BP5_GEOM_MERGED6");
    }
    mf->d_scalar_plane = sp; mf->d_gcell = gc;
  }
  mf->geometry_mode = mode;
  return BP5_OK;
}

template <int n>
static int launch_mass_plane(bp5_mf *mf, double *coef)
{
  const uint32_t grid = cell_grid(mf, 65535u * 16);
  hipLaunchKernelGGL(mass_plane_kernel<n>, dim3(grid), dim3(n, n, n), 0, mf->stream, mf->d_l2g, mf->d_coords, mf->d_tab, mf->coefficient, mf->n_cells, coef,
                     mf->coef_cell_stride);
  KERNEL_CHECK();
  return BP5_OK;
}
extern "C" int bp5_mf_compute_merged_metric(bp5_mf *mf, double *coef)
{
  if (!mf || !coef) return fail(BP5_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(mf->device));
  if (mf->overint()) { // Q^3 entries per cell and plane, six planes or the mass plane: a kernel of its own
    mf->coef_planes_committed = mf->n_planes();
    return overint_compute_metric(mf, coef);
  }
  if (mf->operator_kind == BP5_OP_MASS) { // one plane rho JxW (plane-major layout, conforming mesh: bp5_mf_set_operator has seen to both)
    mf->coef_planes_committed = mf->n_planes();
    return for_degree(mf->degree, [&](auto P) { return launch_mass_plane<P() + 1>(mf, coef); });
  }
  GeomOut o{};
  o.coef = coef;
  o.plane_stride = mf->coef_plane_stride; o.cell_stride = mf->coef_cell_stride;
  o.helmholtz = mf->operator_kind == BP5_OP_HELMHOLTZ;
  mf->coef_planes_committed = mf->n_planes();
  if (o.helmholtz && mf->coef_cell_stride != (uint64_t)mf->n3) return fail(BP5_ERR_UNSUPPORTED, "the Helmholtz operator needs the plane-major metric layout");
  return geometry_dispatch(mf, o);
}

template <int n>
static int launch_permute(bp5_mf *mf, const double *in, double *out)
{
  const uint64_t total = (uint64_t)mf->n_planes() * mf->n_cells * mf->n3;
  if (mf->f32_metric())
    hipLaunchKernelGGL((metric_permute_kernel<n, float>), dim3(2048), dim3(256), 0, mf->stream, reinterpret_cast<const float *>(in), out, total, (uint64_t)mf->n_cells,
                       mf->coef_plane_stride, mf->coef_cell_stride);
  else
    hipLaunchKernelGGL(metric_permute_kernel<n>, dim3(2048), dim3(256), 0, mf->stream, in, out, total, (uint64_t)mf->n_cells, mf->coef_plane_stride,
                       mf->coef_cell_stride);
  KERNEL_CHECK();
  return BP5_OK;
}
extern "C" int bp5_mf_metric_to_reference_layout(bp5_mf *mf, const double *coef, double *coef_ref)
{
  if (!mf || !coef || !coef_ref) return fail(BP5_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(mf->device));
  if (mf->overint()) return overint_to_reference_layout(mf, coef, coef_ref);
  return for_degree(mf->degree, [&](auto P) { return launch_permute<P() + 1>(mf, coef, coef_ref); });
}

static uint32_t padding_length(int n)
{ // deal.II: 2^ceil(dim*log2(n)) [upstream], SURVEY 8(a3)
  uint32_t p = 1;
  while (p < (uint32_t)(n * n * n)) p <<= 1;
  return p;
}

extern "C" int bp5_mf_get_data(bp5_mf *mf, int color, bp5_mf_data *out)
{
  if (!mf || !out) return fail(BP5_ERR_INVALID, "null argument");
  if (color != 0) return fail(BP5_ERR_INVALID, "this build keeps all cells in one colour");
  if (mf->trilinear()) return trilinear_refuse("bp5_mf_get_data (the unmerged geometry at the quadrature points) is not supported");
  if (mf->overint()) return overint_refuse("bp5_mf_get_data (the unmerged geometry at the quadrature points) is not supported");
  HIP_TRY(hipSetDevice(mf->device));
  if (!mf->d_inv_jac) {
    mf->pad = padding_length(mf->n);
    const size_t gp = (size_t)mf->n_cells * mf->pad;
    HIP_TRY(hipMalloc((void **)&mf->d_inv_jac, std::max<size_t>(9 * gp, 1) * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&mf->d_JxW, std::max<size_t>(gp, 1) * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&mf->d_qpoints, std::max<size_t>(3 * gp, 1) * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&mf->d_l2g_padded, std::max<size_t>(gp, 1) * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void **)&mf->d_constraint_mask, std::max<size_t>(mf->n_cells, 1) * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(mf->d_inv_jac, 0, 9 * gp * sizeof(double), mf->stream));
    HIP_TRY(hipMemsetAsync(mf->d_JxW, 0, gp * sizeof(double), mf->stream));
    HIP_TRY(hipMemsetAsync(mf->d_qpoints, 0, 3 * gp * sizeof(double), mf->stream));
    HIP_TRY(hipMemsetAsync(mf->d_l2g_padded, 0, gp * sizeof(uint32_t), mf->stream));
    if (mf->has_hanging) HIP_TRY(hipMemcpyAsync(mf->d_constraint_mask, mf->d_hang_mask, mf->n_cells * sizeof(uint32_t), hipMemcpyDeviceToDevice, mf->stream));
    else HIP_TRY(hipMemsetAsync(mf->d_constraint_mask, 0, mf->n_cells * sizeof(uint32_t), mf->stream));
    if (mf->n_cells)
      HIP_TRY(hipMemcpy2DAsync(mf->d_l2g_padded, mf->pad * sizeof(uint32_t), mf->d_l2g, mf->n3 * sizeof(uint32_t),
                               mf->n3 * sizeof(uint32_t), mf->n_cells, hipMemcpyDeviceToDevice, mf->stream));
    GeomOut o{};
    o.inv_jac = mf->d_inv_jac; o.JxW = mf->d_JxW; o.q_points = mf->d_qpoints; o.pad = mf->pad; o.geo_plane = gp;
    BP5_TRY(geometry_dispatch(mf, o));
    HIP_TRY(hipStreamSynchronize(mf->stream));
  }
  out->local_to_global = mf->d_l2g_padded; out->inv_jacobian = mf->d_inv_jac; out->JxW = mf->d_JxW; out->q_points = mf->d_qpoints;
  out->constraint_mask = mf->d_constraint_mask; out->n_cells = mf->n_cells; out->padding_length = mf->pad; out->row_start = 0;
  out->use_coloring = 0;
  return BP5_OK;
}

// ------------------------------------------------------------------------------------ operator

// Structured cell blocks ("lattice" blocks).  A block is a lattice block when (1) its cells form a full box of bx x by x bz cells that are
// face neighbours with parallel local axes, and (2) its DoFs are numbered entity by entity: the DoFs of each of the 27 lattice entities of
// the box (interior, 6 faces, 12 edges, 8 corners of its (bx p + 1) x (by p + 1) x (bz p + 1) node lattice) are consecutive, x fastest --
// what a brick-major numbering (bp5_mesh_create_brick: dof_numbering = 1) produces.  The list slot and the DoF of every cell-local entry
// then follow in closed form from the cell's position (cx, cy, cz) and the entry's (i, j, k):  I = cx p + i, ..., entity = class(I) +
// 3 class(J) + 9 class(K) (class: 0 at the low plane, 2 at the high plane, 1 between), offset = interior coordinates in mixed radix --
// the kernels compute both instead of reading 2 bytes per entry (2 r bytes per DoF of HBM traffic).  Recognition is topological (shared
// face corners), the numbering is verified entry by entry; any block that fails keeps the packed stream.
// out `lat`: [n_blocks][BLOCK_LATTICE_WORDS]: slots of the 27 entities, their first DoFs, then bx | by << 8 | bz << 16 | 1 << 31 (0: no lattice).
static uint32_t detect_lattice_blocks(const uint32_t *l2g, int n, const std::vector<uint32_t> &cell_off, const std::vector<uint32_t> &list_off,
                                      const std::vector<uint32_t> &list_dofs, std::vector<uint32_t> &lat, std::vector<uint16_t> &cpos)
{
  const int p = n - 1, n2 = n * n, n3 = n2 * n;
  const size_t n_blocks = cell_off.size() - 1;
  lat.assign(n_blocks * BLOCK_LATTICE_WORDS, 0u);
  cpos.assign(cell_off.back(), 0);
  uint32_t n_ok = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : n_ok)
  for (int64_t g = 0; g < (int64_t)n_blocks; ++g) {
    const uint32_t c0 = cell_off[g], nc = cell_off[g + 1] - c0;
    if (nc == 0 || nc > 4096) continue;
    auto L = [&](uint32_t c, int i, int j, int k) { return l2g[(size_t)(c0 + c) * n3 + i + n * (j + n * k)]; };
    // faces by their four corner DoFs: face f = 2 d + side of cell c
    auto face_key = [&](uint32_t c, int d, int side, uint32_t (&key)[4]) {
      int q = 0;
      for (int b = 0; b < 2; ++b)
        for (int a = 0; a < 2; ++a) {
          int ijk[3];
          ijk[d] = side * p;
          ijk[(d + 1) % 3] = a * p;
          ijk[(d + 2) % 3] = b * p;
          key[q++] = L(c, ijk[0], ijk[1], ijk[2]);
        }
    };
    // neighbours: sort the 6 nc faces by their keys; a +side face of one cell and the -side face of another with the same corners meet
    struct Face { uint32_t k[4]; uint32_t cell; int d, side; };
    std::vector<Face> faces;
    faces.reserve(6 * (size_t)nc);
    for (uint32_t c = 0; c < nc; ++c)
      for (int d = 0; d < 3; ++d)
        for (int side = 0; side < 2; ++side) {
          Face f;
          face_key(c, d, side, f.k);
          f.cell = c; f.d = d; f.side = side;
          faces.push_back(f);
        }
    std::sort(faces.begin(), faces.end(), [](const Face &a, const Face &b) { return std::lexicographical_compare(a.k, a.k + 4, b.k, b.k + 4); });
    std::vector<uint32_t> nbr(6 * (size_t)nc, UINT32_MAX); // [cell][2 d + side]
    for (size_t f = 0; f + 1 < faces.size(); ++f) {
      const Face &a = faces[f], &b = faces[f + 1];
      if (std::equal(a.k, a.k + 4, b.k) && a.d == b.d && a.side != b.side && a.cell != b.cell) {
        nbr[6 * (size_t)a.cell + 2 * a.d + a.side] = b.cell;
        nbr[6 * (size_t)b.cell + 2 * b.d + b.side] = a.cell;
      }
    }
    std::vector<int> pos(3 * (size_t)nc, INT32_MIN);
    std::vector<uint32_t> queue{0};
    pos[0] = pos[1] = pos[2] = 0;
    bool ok = true;
    for (size_t qh = 0; qh < queue.size() && ok; ++qh) { // breadth-first over face neighbours
      const uint32_t c = queue[qh];
      for (int d = 0; d < 3 && ok; ++d)
        for (int side = 0; side < 2 && ok; ++side) {
          const uint32_t o = nbr[6 * (size_t)c + 2 * d + side];
          if (o == UINT32_MAX) continue;
          int want[3] = {pos[3 * c], pos[3 * c + 1], pos[3 * c + 2]};
          want[d] += side ? 1 : -1;
          if (pos[3 * o] == INT32_MIN) {
            pos[3 * o] = want[0]; pos[3 * o + 1] = want[1]; pos[3 * o + 2] = want[2];
            queue.push_back(o);
          } else if (pos[3 * o] != want[0] || pos[3 * o + 1] != want[1] || pos[3 * o + 2] != want[2])
            ok = false;
        }
    }
    if (!ok || queue.size() != nc) continue;
    int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    for (uint32_t c = 0; c < nc; ++c)
      for (int d = 0; d < 3; ++d) { lo[d] = std::min(lo[d], pos[3 * c + d]); hi[d] = std::max(hi[d], pos[3 * c + d]); }
    const int bx = hi[0] - lo[0] + 1, by = hi[1] - lo[1] + 1, bz = hi[2] - lo[2] + 1;
    if ((int64_t)bx * by * bz != (int64_t)nc || bx > 15 || by > 15 || bz > 15) continue;
    std::vector<uint32_t> cell_at((size_t)nc, UINT32_MAX);
    for (uint32_t c = 0; c < nc && ok; ++c) {
      const size_t at = (pos[3 * c] - lo[0]) + (size_t)bx * ((pos[3 * c + 1] - lo[1]) + (size_t)by * (pos[3 * c + 2] - lo[2]));
      if (cell_at[at] != UINT32_MAX) ok = false;
      cell_at[at] = c;
    }
    if (!ok) continue;
    const int N[3] = {bx * p, by * p, bz * p};
    auto cls = [&](int X, int d) { return X == 0 ? 0 : X == N[d] ? 2 : 1; };
    auto dof_at = [&](int I, int J, int K) { // the DoF at a lattice point, through any cell that holds it
      const int cx = std::min(I / p, bx - 1), cy = std::min(J / p, by - 1), cz = std::min(K / p, bz - 1);
      return L(cell_at[cx + (size_t)bx * (cy + (size_t)by * cz)], I - cx * p, J - cy * p, K - cz * p);
    };
    uint32_t ent_dof[27];
    for (int e = 0; e < 27; ++e) {
      const int eI = e % 3, eJ = (e / 3) % 3, eK = e / 9;
      // an entity that does not exist (a direction without interior points: N == 1 has none between the planes) is never referenced
      const int I = eI == 0 ? 0 : eI == 2 ? N[0] : 1, J = eJ == 0 ? 0 : eJ == 2 ? N[1] : 1, K = eK == 0 ? 0 : eK == 2 ? N[2] : 1;
      ent_dof[e] = (I <= N[0] && J <= N[1] && K <= N[2] && !(eI == 1 && N[0] < 2) && !(eJ == 1 && N[1] < 2) && !(eK == 1 && N[2] < 2)) ? dof_at(I, J, K) : 0u;
    }
    for (uint32_t c = 0; c < nc && ok; ++c) { // the numbering, entry by entry
      const int cx = pos[3 * c] - lo[0], cy = pos[3 * c + 1] - lo[1], cz = pos[3 * c + 2] - lo[2];
      for (int k = 0; k < n && ok; ++k)
        for (int j = 0; j < n && ok; ++j)
          for (int i = 0; i < n; ++i) {
            const int I = cx * p + i, J = cy * p + j, K = cz * p + k;
            const int eI = cls(I, 0), eJ = cls(J, 1), eK = cls(K, 2);
            const uint32_t LX = eI == 1 ? N[0] - 1 : 1, LY = eJ == 1 ? N[1] - 1 : 1;
            const uint32_t off = (eI == 1 ? I - 1 : 0) + LX * ((eJ == 1 ? J - 1 : 0) + LY * (eK == 1 ? K - 1 : 0));
            if (L(c, i, j, k) != ent_dof[eI + 3 * eJ + 9 * eK] + off) { ok = false; break; }
          }
    }
    if (!ok) continue;
    uint32_t *row = lat.data() + (size_t)g * BLOCK_LATTICE_WORDS;
    const uint32_t *lb = list_dofs.data() + list_off[g], *le = list_dofs.data() + list_off[g + 1];
    for (int e = 0; e < 27 && ok; ++e) {
      const uint32_t *it = std::lower_bound(lb, le, ent_dof[e], [](uint32_t a, uint32_t b) { return (a & 0x7fffffffu) < b; });
      const int eI = e % 3, eJ = (e / 3) % 3, eK = e / 9;
      const bool exists = !(eI == 1 && N[0] < 2) && !(eJ == 1 && N[1] < 2) && !(eK == 1 && N[2] < 2);
      if (exists && (it == le || (*it & 0x7fffffffu) != ent_dof[e])) ok = false;
      row[e] = exists ? (uint32_t)(it - lb) : 0u;
      row[27 + e] = ent_dof[e];
    }
    if (!ok) { std::fill(row, row + BLOCK_LATTICE_WORDS, 0u); continue; }
    row[54] = (uint32_t)bx | (uint32_t)by << 8 | (uint32_t)bz << 16 | 0x80000000u;
    for (uint32_t c = 0; c < nc; ++c)
      cpos[c0 + c] = (uint16_t)((pos[3 * c] - lo[0]) | (pos[3 * c + 1] - lo[1]) << 4 | (pos[3 * c + 2] - lo[2]) << 8);
    ++n_ok;
  }
  return n_ok;
}

// run-length combine tables (runs of consecutive shared DoFs whose contributions sit in consecutive slab slots): start[r] = first ordinal of run r
// (start[n_runs] = number of shared DoFs), dof0[r] (bit 31: Dirichlet run), slots[soff[r] ...] = the slab slots of the run's first DoF.  Adds the
// tile table (run containing ordinal COMBINE_TILE t) and one entry of slack, uploads.
static int upload_combine_tables(std::vector<uint32_t> start, const std::vector<uint32_t> &dof0, std::vector<uint32_t> soff, const std::vector<uint32_t> &slots,
                                 bp5_mf::DevPlan::CombineTables *ct)
{
  const size_t ns = start.back();
  ct->n_shared = (uint32_t)ns;
  if (!ns) return BP5_OK;
  const size_t n_tiles = (ns + COMBINE_TILE - 1) / COMBINE_TILE;
  std::vector<uint32_t> tile(n_tiles + 1);
  size_t r = 0;
  for (size_t t = 0; t <= n_tiles; ++t) { // run containing ordinal min(COMBINE_TILE t, ns - 1)
    const size_t i = std::min(t * (size_t)COMBINE_TILE, ns - 1);
    while (start[r + 1] <= i) ++r;
    tile[t] = (uint32_t)r;
  }
  start.push_back((uint32_t)ns); // one entry of slack for the staging loop (reads r_hi + 1)
  soff.push_back((uint32_t)slots.size());
  BP5_TRY(upload(&ct->start, start.data(), start.size()));
  BP5_TRY(upload(&ct->dof0, dof0.data(), dof0.size()));
  BP5_TRY(upload(&ct->soff, soff.data(), soff.size()));
  BP5_TRY(upload(&ct->slots, slots.data(), slots.size()));
  BP5_TRY(upload(&ct->tile, tile.data(), tile.size()));
  return BP5_OK;
}

// Face carry (bp5_kernels.hpp: BLOCK_CARRY_MAX).  Block g can hand a face to block g + 1 when the two are lattice blocks that meet in a face whose
// interior DoFs (a) are ONE shared run in both blocks' lists, (b) are owned, unconstrained and (c) have exactly the two contributions of these
// blocks, at the slab slots the lists imply.  Two steps around the construction of the run tables: find_carry_faces (a), (b), (c) without the run
// condition -- the run tables are then CUT at the faces' first and last slots (a run of shared DoFs may span several entities) --, and
// mark_carry_faces, which checks (a) on the finished tables and writes the carry words of the lattice table (lat) and dp.h_carry_*.
struct CarryFace { uint32_t dof, len, s_out, s_in; };
static std::vector<CarryFace> find_carry_faces(const bp5_mf *mf, int p, const TeamPlanHost &h, const std::vector<uint32_t> &lat)
{
  const size_t ng = h.off.size() - 1;
  std::vector<CarryFace> faces(ng, CarryFace{0u, 0u, 0u, 0u});
  static const int E_OUT[3] = {14, 16, 22}, E_IN[3] = {12, 10, 4}; // entity = eI + 3 eJ + 9 eK, e* in {low face, interior, high face}
  for (size_t g = 0; g + 1 < ng; ++g) {
    const uint32_t *ra = lat.data() + g * BLOCK_LATTICE_WORDS, *rb = ra + BLOCK_LATTICE_WORDS;
    if (!(ra[54] >> 31) || !(rb[54] >> 31)) continue;
    const uint32_t da[3] = {ra[54] & 0xffu, (ra[54] >> 8) & 0xffu, (ra[54] >> 16) & 0xffu}, db[3] = {rb[54] & 0xffu, (rb[54] >> 8) & 0xffu, (rb[54] >> 16) & 0xffu};
    for (int d = 0; d < 3; ++d) {
      const int d1 = (d + 1) % 3, d2 = (d + 2) % 3;
      if (da[d1] != db[d1] || da[d2] != db[d2]) continue;
      const uint32_t len = (da[d1] * p - 1) * (da[d2] * p - 1), dof = ra[27 + E_OUT[d]];
      if (len == 0 || len > (uint32_t)BLOCK_CARRY_MAX || dof != rb[27 + E_IN[d]] || (uint64_t)dof + len > mf->n_owned) continue;
      const uint32_t s_out = ra[E_OUT[d]], s_in = rb[E_IN[d]];
      if (s_out > 0xffffu || s_in > 0xffffu) continue;
      const auto it = std::lower_bound(h.sh_dof.begin(), h.sh_dof.end(), dof);
      const size_t o = it - h.sh_dof.begin();
      bool ok = o + len <= h.sh_dof.size();
      for (uint32_t k = 0; ok && k < len; ++k) {
        const uint32_t b = h.sh_off[o + k], want_a = h.off[g] + s_out + k, want_b = h.off[g + 1] + s_in + k;
        ok = h.sh_dof[o + k] == dof + k && h.sh_off[o + k + 1] - b == 2 && !mf->h_constrained[dof + k] &&
             ((h.sh_slot[b] == want_a && h.sh_slot[b + 1] == want_b) || (h.sh_slot[b] == want_b && h.sh_slot[b + 1] == want_a));
      }
      if (!ok) continue;
      faces[g] = CarryFace{dof, len, s_out, s_in};
      break;
    }
  }
  return faces;
}
static size_t mark_carry_faces(const TeamPlanHost &h, const std::vector<CarryFace> &faces, const std::vector<uint32_t> &run_off, const std::vector<uint32_t> &runs,
                               std::vector<uint32_t> &lat, bp5_mf::DevPlan &dp)
{
  const size_t ng = h.off.size() - 1;
  dp.h_carry_dof.assign(ng, 0u);
  dp.h_carry_len.assign(ng, 0u);
  auto one_shared_run = [&](size_t g, uint32_t slot, uint32_t dof, uint32_t len) {
    const uint32_t nr = run_off[g + 1] - run_off[g], m = h.off[g + 1] - h.off[g];
    for (uint32_t r = 0; r < nr; ++r) {
      const uint32_t s0 = runs[2 * (run_off[g] + r)];
      if (s0 != slot) continue;
      const uint32_t s1 = r + 1 < nr ? runs[2 * (run_off[g] + r + 1)] : m;
      return runs[2 * (run_off[g] + r) + 1] == dof && s1 == slot + len; // (no ownership bit, no Dirichlet bit)
    }
    return false;
  };
  size_t n_faces = 0;
  for (size_t g = 0; g + 1 < ng && g < faces.size(); ++g) {
    const CarryFace &f = faces[g];
    if (!f.len || !one_shared_run(g, f.s_out, f.dof, f.len) || !one_shared_run(g + 1, f.s_in, f.dof, f.len)) continue;
    uint32_t *ra = lat.data() + g * BLOCK_LATTICE_WORDS, *rb = ra + BLOCK_LATTICE_WORDS;
    ra[55] = f.len << 16 | f.s_out; // (list slots < 2^16: the packed indices need that already)
    rb[56] = f.len << 16 | f.s_in;
    dp.h_carry_dof[g] = f.dof; dp.h_carry_len[g] = f.len;
    ++n_faces;
  }
  if (!n_faces) { dp.h_carry_dof.clear(); dp.h_carry_len.clear(); }
  return n_faces;
}

int build_carry_tables(bp5_mf *mf, bp5_mf::DevPlan *dp, const std::vector<uint32_t> &wb, uint32_t n_wg, bool two_parts, bp5_mf::DevPlan::CombineTables *out)
{
  // the faces this partition carries: consecutive blocks inside one part of one workgroup's range (the kernel's rule, apply_block_kernel: c_out)
  std::vector<std::pair<uint32_t, uint32_t>> cut; // (first DoF, count)
  for (int part = 0; part < (two_parts ? 2 : 1); ++part) {
    const uint32_t *w = wb.data() + (size_t)part * (n_wg + 1);
    for (uint32_t i = 0; i < n_wg; ++i)
      for (uint32_t g = w[i]; g + 1 < w[i + 1]; ++g)
        if (dp->h_carry_len[g]) cut.emplace_back(dp->h_carry_dof[g], dp->h_carry_len[g]);
  }
  std::sort(cut.begin(), cut.end());
  const std::vector<uint32_t> &st = dp->h_cr_start, &d0 = dp->h_cr_dof0, &so = dp->h_cr_soff, &sl = dp->h_cr_slots;
  const size_t nr = d0.size();
  std::vector<uint32_t> start, dof0, soff, slots;
  uint32_t ord = 0, owned = 0;
  size_t ci = 0;
  auto emit = [&](size_t r, uint32_t first, uint32_t count) { // DoFs [first, first + count) of run r stay
    if (!count) return;
    const uint32_t base = d0[r] & 0x7fffffffu;
    start.push_back(ord);
    dof0.push_back(first | (d0[r] & 0x80000000u));
    soff.push_back((uint32_t)slots.size());
    for (uint32_t q = so[r]; q < so[r + 1]; ++q) slots.push_back(sl[q] + (first - base));
    ord += count;
    if (first < mf->n_owned) owned += std::min(count, mf->n_owned - first);
  };
  for (size_t r = 0; r < nr; ++r) {
    uint32_t first = d0[r] & 0x7fffffffu;
    const uint32_t end = first + (st[r + 1] - st[r]);
    while (ci < cut.size() && cut[ci].first + cut[ci].second <= first) ++ci;
    size_t c = ci;
    while (c < cut.size() && cut[c].first < end) { // (faces are disjoint; each lies inside one run of shared DoFs)
      const uint32_t c0 = std::max(cut[c].first, first), c1 = std::min(cut[c].first + cut[c].second, end);
      emit(r, first, c0 - first);
      first = c1;
      ++c;
    }
    emit(r, first, end - first);
  }
  start.push_back(ord);
  soff.push_back((uint32_t)slots.size());
  BP5_TRY(upload_combine_tables(start, dof0, soff, slots, out));
  out->n_shared_owned = owned;
  return BP5_OK;
}

// Fused vector update (BLK_UPD, BP5_TUNE_FUSED_UPDATE): the block kernel may apply the merged solver's update to the interior run of every brick
// (lattice entity (1,1,1)) when those runs are disjoint, together cover exactly the DoFs [0, n_int), every one of their DoFs is touched by its
// block alone, owned and unconstrained -- what bp5_mesh_create_brick's block-major numbering produces (interior class first; the planes of the
// domain boundary are brick planes).  Returns n_int, or 0 for a plan (a mesh numbered by someone else) without that property.
static uint32_t interior_runs_cover(const bp5_mf *mf, int p, const TeamPlanHost &h, const std::vector<uint32_t> &lat)
{
  const size_t ng = h.off.size() - 1;
  std::vector<std::pair<uint32_t, uint32_t>> runs(ng);
  bool ok = true;
#pragma omp parallel for schedule(dynamic, 16) reduction(&& : ok)
  for (int64_t g = 0; g < (int64_t)ng; ++g) {
    const uint32_t *row = lat.data() + (size_t)g * BLOCK_LATTICE_WORDS;
    const uint32_t hdr = row[54];
    if (!(hdr >> 31)) { ok = false; continue; }
    const uint32_t len = ((hdr & 255u) * p - 1u) * (((hdr >> 8) & 255u) * p - 1u) * (((hdr >> 16) & 255u) * p - 1u), dof = row[27 + 13], slot = row[13];
    runs[g] = {dof, len};
    if (!len || (uint64_t)h.off[g] + slot + len > h.off[g + 1]) { ok = false; continue; }
    const uint32_t *l = h.dofs.data() + h.off[g] + slot;
    for (uint32_t k = 0; k < len; ++k)
      if (l[k] != ((dof + k) | 0x80000000u)) { ok = false; break; } // consecutive, and bit 31: no other block touches it
  }
  if (!ok) return 0;
  std::sort(runs.begin(), runs.end());
  uint64_t end = 0;
  for (const auto &r : runs) {
    if (r.first != end) return 0;
    end += r.second;
  }
  if (end == 0 || end > mf->n_owned) return 0;
  for (uint64_t i = 0; i < end; ++i) if (mf->h_constrained[i]) return 0;
  return (uint32_t)end;
}

// key > 0: uniform teams of `key` cells (team kernel); key < 0: cell blocks walked in passes of
// -key cells (block kernel) -- the caller's blocks if given, else groups of `default_block` cells
int get_plan_raw(bp5_mf *mf, int key, bp5_mf::DevPlan **dpo, int default_block)
{
  auto it = mf->plans.find(key);
  if (it == mf->plans.end()) {
    TeamPlanHost h;
    if (key < 0 && mf->n_local() >= (1ull << 30)) return fail(BP5_ERR_UNSUPPORTED, "block plan needs fewer than 2^30 local DoFs");
    if (key > 0) BP5_TRY(build_team_plan(mf->h_l2g.data(), mf->n_cells, mf->n3, mf->n_local(), key, h));
    else if (!mf->h_block_off.empty())
      BP5_TRY(build_team_plan(mf->h_l2g.data(), mf->n_cells, mf->n3, mf->n_local(), 0, h, mf->h_block_off.data(),
                              (uint32_t)mf->h_block_off.size() - 1, -key));
    else BP5_TRY(build_team_plan(mf->h_l2g.data(), mf->n_cells, mf->n3, mf->n_local(), default_block, h, nullptr, 0, -key));
    bp5_mf::DevPlan dp;
    BP5_TRY(upload(&dp.off, h.off.data(), h.off.size()));
    BP5_TRY(upload(&dp.dofs, h.dofs.data(), h.dofs.size()));
    std::vector<uint32_t> run_off, runs;
    if (key < 0) {
      // lattice blocks: recognised and VERIFIED entry by entry here; everything else keeps the packed stream
      std::vector<uint32_t> lat;
      std::vector<uint16_t> cpos;
      const bool lattice_enabled = mf->tune[BP5_TUNE_LATTICE_INDICES] != 0; // (A/B knob, fixed once the plan is built)
      dp.n_lattice_blocks = detect_lattice_blocks(mf->h_l2g.data(), mf->degree + 1, h.group_cell_off, h.off, h.dofs, lat, cpos);
      // ... and the faces consecutive blocks could hand on in LDS (face carry): the run tables are cut at their ends
      std::vector<CarryFace> faces;
      if (dp.n_lattice_blocks && dp.n_lattice_blocks == (uint32_t)(h.off.size() - 1)) faces = find_carry_faces(mf, mf->degree, h, lat);
      auto face_edge = [&](size_t g, uint32_t slot) { // slot = first slot of a carried face of block g, or the first slot behind one
        if (faces.empty()) return false;
        if (faces[g].len && (slot == faces[g].s_out || slot == faces[g].s_out + faces[g].len)) return true;
        return g > 0 && faces[g - 1].len && (slot == faces[g - 1].s_in || slot == faces[g - 1].s_in + faces[g - 1].len);
      };
      // run-length form of the sorted block lists: consecutive DoFs with equal ownership flag, cut at 512 entries (and where the Dirichlet flag changes) so
      // that (run, offset) packs into 7 + 9 bits
      run_off.assign(h.off.size(), 0);
      for (size_t g = 0; g + 1 < h.off.size(); ++g) {
        uint32_t start = h.off[g];
        for (uint32_t i = h.off[g]; i < h.off[g + 1]; ++i) {
          const bool con = mf->h_constrained[h.dofs[i] & 0x7fffffffu];
          if (i == h.off[g] || h.dofs[i] != h.dofs[i - 1] + 1 || i - start == (1u << BLOCK_PACK_OFF_BITS) ||
              con != (bool)mf->h_constrained[h.dofs[i - 1] & 0x7fffffffu] || face_edge(g, i - h.off[g])) {
            start = i;
            runs.push_back(i - h.off[g]);
            runs.push_back(h.dofs[i] | (con ? BLOCK_DOF_CONSTRAINED : 0u)); // bit 31 exclusive (from dofs), bit 30 Dirichlet
          }
        }
        run_off[g + 1] = (uint32_t)(runs.size() / 2);
        dp.max_runs = std::max(dp.max_runs, run_off[g + 1] - run_off[g]);
      }
      // block kernel: per-cell index arrays in the pair layout of the z-pencils (two entries per load, see coef_off)
      const int n = mf->degree + 1, n2 = n * n;
      auto off = [&](int k, int ab) { return k < 2 * (n / 2) ? (k / 2) * (2 * n2) + 2 * ab + (k & 1) : (n / 2) * (2 * n2) + ab; };
      std::vector<uint16_t> pos2(h.pos.size()), packed(dp.max_runs <= (uint32_t)BLOCK_PACK_MAX_RUNS ? h.pos.size() : 0);
      std::vector<uint32_t> gidx(h.pos.size());
#pragma omp parallel
      {
        std::vector<uint16_t> run_of_slot;
#pragma omp for schedule(dynamic, 16)
        for (int64_t g = 0; g < (int64_t)h.group_cell_off.size() - 1; ++g) {
          const uint32_t nr = run_off[g + 1] - run_off[g], m = h.off[g + 1] - h.off[g];
          if (!packed.empty()) {
            run_of_slot.assign(m, 0);
            for (uint32_t r = 0; r < nr; ++r) {
              const uint32_t s0 = runs[2 * (run_off[g] + r)], s1 = r + 1 < nr ? runs[2 * (run_off[g] + r + 1)] : m;
              for (uint32_t sl = s0; sl < s1; ++sl) run_of_slot[sl] = (uint16_t)r;
            }
          }
          for (size_t c = h.group_cell_off[g]; c < h.group_cell_off[g + 1]; ++c)
            for (int k = 0; k < n; ++k)
              for (int ab = 0; ab < n2; ++ab) {
                const size_t from = c * mf->n3 + (size_t)k * n2 + ab, to = c * mf->n3 + off(k, ab);
                pos2[to] = h.pos[from];
                gidx[to] = mf->h_l2g[from];
                if (!packed.empty()) {
                  const uint32_t sl = h.pos[from], r = run_of_slot[sl];
                  packed[to] = (uint16_t)(r << BLOCK_PACK_OFF_BITS | (sl - runs[2 * (run_off[g] + r)]));
                }
              }
        }
      }
      BP5_TRY(upload(&dp.pos, pos2.data(), pos2.size()));
      BP5_TRY(upload(&dp.gidx, gidx.data(), gidx.size()));
      if (!packed.empty()) BP5_TRY(upload(&dp.packed, packed.data(), packed.size()));
      if (!packed.empty() && dp.n_lattice_blocks && lattice_enabled) { // (knob off: the same run tables, cuts included -- the two builds give the same bits)
        if (!faces.empty()) mark_carry_faces(h, faces, run_off, runs, lat, dp);
        BP5_TRY(upload(&dp.lattice, lat.data(), lat.size()));
        BP5_TRY(upload(&dp.cell_pos, cpos.data(), cpos.size()));
        if (dp.n_lattice_blocks == (uint32_t)(h.off.size() - 1)) dp.upd_n_int = interior_runs_cover(mf, mf->degree, h, lat);
      } else
        dp.n_lattice_blocks = 0;
    } else
      BP5_TRY(upload(&dp.pos, h.pos.data(), h.pos.size()));
    BP5_TRY(upload(&dp.cell_round, h.cell_round.data(), h.cell_round.size()));
    BP5_TRY(upload(&dp.team_rounds, h.team_rounds.data(), h.team_rounds.size()));
    BP5_TRY(upload(&dp.sh_dof, h.sh_dof.data(), h.sh_dof.size()));
    BP5_TRY(upload(&dp.sh_off, h.sh_off.data(), h.sh_off.size()));
    BP5_TRY(upload(&dp.sh_slot, h.sh_slot.data(), h.sh_slot.size()));
    HIP_TRY(hipMalloc((void **)&dp.partial, std::max<size_t>(h.dofs.size(), 1) * sizeof(double)));
    HIP_TRY(hipMemsetAsync(dp.partial, 0, std::max<size_t>(h.dofs.size(), 1) * sizeof(double), mf->stream)); // on the handle's stream (bp5.h:14)
    BP5_TRY(upload(&dp.cell_off, h.group_cell_off.data(), h.group_cell_off.size()));
    if (key < 0) {
      BP5_TRY(upload(&dp.pass_cell, h.pass_cell.data(), h.pass_cell.size()));
      BP5_TRY(upload(&dp.pass_off, h.pass_off.data(), h.pass_off.size()));
      // cost model of a block in units of one pass, calibrated on the slab mesh of a rank > 0 (profiles/r1 k_*: thin
      // boundary bricks next to full ones): every accumulation round after the first +0.18, the write-out 1.5 per 4913
      // list slots, ONE pass-equivalent fixed per block (barrier, block switch, table hand-over)
      dp.h_cost.assign(h.pass_off.size(), 0.0);
      for (size_t g = 0; g + 1 < h.pass_off.size(); ++g) {
        const double passes = h.pass_off[g + 1] - h.pass_off[g], rounds = h.team_rounds[g], m = h.off[g + 1] - h.off[g];
        dp.h_cost[g + 1] = dp.h_cost[g] + passes * (1.0 + 0.18 * (rounds - 1.0)) + 1.5 * m / 4913.0 + 1.0;
      }
      runs.push_back(0); runs.push_back(0);
      BP5_TRY(upload(&dp.run_off, run_off.data(), run_off.size()));
      BP5_TRY(upload(&dp.runs, runs.data(), runs.size()));
    }
    dp.n_shared = (uint32_t)h.sh_dof.size();
    dp.n_shared_owned = (uint32_t)(std::lower_bound(h.sh_dof.begin(), h.sh_dof.end(), mf->n_owned) - h.sh_dof.begin());
    if (dp.n_shared) { // run-length form of the shared-DoF CSR for combine_runs_kernel
      std::vector<uint32_t> start, dof0, soff, slots, tile;
      const size_t ns = h.sh_dof.size();
      for (size_t i = 0; i < ns; ++i) {
        const uint32_t b = h.sh_off[i], e = h.sh_off[i + 1];
        bool cont = i > 0 && h.sh_dof[i] == h.sh_dof[i - 1] + 1 && (e - b) == (h.sh_off[i] - h.sh_off[i - 1]) &&
                    mf->h_constrained[h.sh_dof[i]] == mf->h_constrained[h.sh_dof[i - 1]];
        for (uint32_t q = 0; cont && q < e - b; ++q) cont = h.sh_slot[b + q] == h.sh_slot[h.sh_off[i - 1] + q] + 1;
        if (!cont) {
          start.push_back((uint32_t)i);
          dof0.push_back(h.sh_dof[i] | (mf->h_constrained[h.sh_dof[i]] ? 0x80000000u : 0u)); // bit 31: Dirichlet run
          soff.push_back((uint32_t)slots.size());
          slots.insert(slots.end(), h.sh_slot.begin() + b, h.sh_slot.begin() + e);
        }
      }
      start.push_back((uint32_t)ns);
      soff.push_back((uint32_t)slots.size());
      bp5_mf::DevPlan::CombineTables ct;
      BP5_TRY(upload_combine_tables(start, dof0, soff, slots, &ct));
      dp.cr_start = ct.start; dp.cr_dof0 = ct.dof0; dp.cr_soff = ct.soff; dp.cr_slots = ct.slots; dp.cr_tile = ct.tile;
      if (!dp.h_carry_len.empty()) { dp.h_cr_start = start; dp.h_cr_dof0 = dof0; dp.h_cr_soff = soff; dp.h_cr_slots = slots; } // (the partitions' tables are cut from these)
    }
    dp.covers_all = h.covers_all;
    dp.n_groups = (uint32_t)h.group_cell_off.size() - 1;
    for (uint32_t g = 0; g < dp.n_groups; ++g) dp.max_list = std::max(dp.max_list, h.off[g + 1] - h.off[g]);
    it = mf->plans.emplace(key, dp).first;
  }
  *dpo = &it->second;
  return BP5_OK;
}
int get_plan(bp5_mf *mf, int cpt, TeamPlan &tp, bp5_mf::DevPlan **dpo)
{
  bp5_mf::DevPlan *q = nullptr;
  BP5_TRY(get_plan_raw(mf, cpt, &q));
  tp.off = q->off; tp.dofs = q->dofs; tp.pos = q->pos; tp.cell_round = q->cell_round; tp.team_rounds = q->team_rounds; tp.partial = q->partial;
  if (dpo) *dpo = q;
  return BP5_OK;
}

// fixed grid of the fused solver's combine pass: k workgroups per CU (BP5_TUNE_COMBINE_WG_PER_CU, default 16: profiles/r4 h_*; each
// workgroup walks its tiles two at a time), never more than tiles or free dot-product columns
int device_cus(bp5_mf *mf)
{
  if (!mf->n_cus) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, mf->device) == hipSuccess) mf->n_cus = prop.multiProcessorCount;
  }
  return mf->n_cus;
}
static uint32_t combine_grid(bp5_mf *mf, uint32_t tiles, uint32_t cols_used)
{
  const uint32_t cols = (uint32_t)PARTIAL_STRIDE - cols_used - 1024u;
  uint32_t grid = std::min<uint32_t>(tiles, cols);
  const int k = mf->tune[BP5_TUNE_COMBINE_WG_PER_CU];
  if (k > 0) grid = std::min<uint32_t>(grid, (uint32_t)k * (uint32_t)std::max(device_cus(mf), 1));
  return std::max<uint32_t>(grid, 1u);
}
int launch_combine(bp5_mf *mf, ApplyCall &call, bp5_mf::DevPlan *dp, double *dst, bool set, int window, bool on_comm_stream)
{
  if (!dp->n_shared) return BP5_OK;
  const hipStream_t stream = on_comm_stream ? mf->comm_stream : mf->stream;
  FuseState *const fuse = call.fuse;
  const bool runs = dp->cr_tile && !call.csr_combine; // the run-length form of the pass (else: the per-DoF CSR kernel)
  // the tables of the block launch this pass follows: the plan's own, or (face carry) its partition's without the carried faces
  bp5_mf::DevPlan::CombineTables own;
  own.start = dp->cr_start; own.dof0 = dp->cr_dof0; own.soff = dp->cr_soff; own.slots = dp->cr_slots; own.tile = dp->cr_tile;
  own.n_shared = dp->n_shared; own.n_shared_owned = dp->n_shared_owned;
  const bp5_mf::DevPlan::CombineTables &ct = (call.combine_tables && runs) ? *call.combine_tables : own;
  if (!ct.n_shared) return BP5_OK;
  if (fuse && !(set && runs)) return fail(BP5_ERR_INVALID, "fused dot products need the run-length combine pass in overwrite mode");
  if (window != COMBINE_ALL && !runs) return fail(BP5_ERR_INVALID, "combine windows need the run-length combine pass");
  if (call.mark_event && !call.mark_recorded && window != COMBINE_GHOST) { HIP_TRY(hipEventRecord(call.mark_event, stream)); call.mark_recorded = true; }
  const dim3 cg((dp->n_shared + 255) / 256); // CSR kernel
  if (runs) {
    CombineRuns cr{};
    cr.start = ct.start; cr.dof0 = ct.dof0; cr.soff = ct.soff; cr.slots = ct.slots; cr.tile_run = ct.tile;
    cr.n_shared = ct.n_shared;
    // tiles of the window: the shared DoFs are listed in ascending order, owned ones first
    const uint32_t all_tiles = (ct.n_shared + COMBINE_TILE - 1) / COMBINE_TILE;
    cr.tile0 = window == COMBINE_GHOST ? ct.n_shared_owned / COMBINE_TILE : 0u;
    const uint32_t tile1 = window == COMBINE_OWNED ? (ct.n_shared_owned + COMBINE_TILE - 1) / COMBINE_TILE : all_tiles;
    cr.dof_lo = window == COMBINE_GHOST ? mf->n_owned : 0u;
    cr.dof_hi = window == COMBINE_OWNED ? mf->n_owned : 0xffffffffu;
    if (window == COMBINE_GHOST_THEN_OWNED) {
      // owned rows exactly as COMBINE_OWNED (tiles, columns), preceded in the SAME launch by one workgroup per ghost tile that signals
      if (!(fuse && set && mf->d_signal)) return fail(BP5_ERR_INVALID, "ghost-rows-first combine launch: fused overwrite launches with a signal word only");
      cr.tile0 = 0u;
      cr.dof_lo = 0u; cr.dof_hi = mf->n_owned;
      cr.ghost_tile0 = ct.n_shared_owned / COMBINE_TILE;
      cr.ghost_blocks = all_tiles - cr.ghost_tile0;
      cr.signal = mf->d_signal;
      const uint32_t owned_tiles = (ct.n_shared_owned + COMBINE_TILE - 1) / COMBINE_TILE;
      cr.cg_p = fuse->p; cr.cg_r = fuse->r; cr.dot_partials = mf->d_partials; cr.dot_col0 = fuse->n_cols;
      cr.n_owned = mf->n_owned; cr.n_tiles = owned_tiles; cr.cg_state = mf->d_st;
      if (fuse->n_cols + 1024u + 8u > (uint32_t)PARTIAL_STRIDE) return fail(BP5_ERR_UNSUPPORTED, "no partial-sum columns left for the combine pass");
      const uint32_t grid = combine_grid(mf, owned_tiles, fuse->n_cols);
      if (ct.n_shared >= (8u << 20)) hipLaunchKernelGGL((combine_runs_kernel<false, true, true>), dim3(grid + cr.ghost_blocks), dim3(256), 0, stream, cr, dp->partial, dst);
      else hipLaunchKernelGGL((combine_runs_kernel<false, true, false>), dim3(grid + cr.ghost_blocks), dim3(256), 0, stream, cr, dp->partial, dst);
      KERNEL_CHECK();
      fuse->n_cols += grid;
      mf->signal_target += cr.ghost_blocks; // every ghost workgroup counts itself in once
      return BP5_OK;
    }
    if (tile1 <= cr.tile0) return BP5_OK; // no row in the window
    const dim3 cgt(tile1 - cr.tile0);
    if (fuse && window != COMBINE_GHOST) { // fused CG dot products over the brick-surface DoFs; columns behind the block kernel's workgroups
      // (ghost rows never enter the dot products: their window takes the plain kernel below)
      cr.cg_p = fuse->p; cr.cg_r = fuse->r; cr.dot_partials = mf->d_partials; cr.dot_col0 = fuse->n_cols;
      cr.n_owned = mf->n_owned; cr.n_tiles = cgt.x; cr.cg_state = mf->d_st;
      if (fuse->n_cols + 1024u + 8u > (uint32_t)PARTIAL_STRIDE) return fail(BP5_ERR_UNSUPPORTED, "no partial-sum columns left for the combine pass");
      const uint32_t grid = combine_grid(mf, cgt.x, fuse->n_cols); // (1024 columns stay free for the exchange)
      // pairs of consecutive ordinals pay on long passes; short ones (config 2, the strong-scaling ranks) are latency-bound
      if (ct.n_shared >= (8u << 20)) hipLaunchKernelGGL((combine_runs_kernel<false, true, true>), dim3(grid), dim3(256), 0, stream, cr, dp->partial, dst);
      else hipLaunchKernelGGL((combine_runs_kernel<false, true, false>), dim3(grid), dim3(256), 0, stream, cr, dp->partial, dst);
      KERNEL_CHECK();
      fuse->n_cols += grid;
      return BP5_OK;
    }
    const bool pairs = ct.n_shared >= (8u << 20) && window != COMBINE_GHOST;
    if (set && pairs) hipLaunchKernelGGL((combine_runs_kernel<false, false, true>), cgt, dim3(256), 0, stream, cr, dp->partial, dst);
    else if (set) hipLaunchKernelGGL((combine_runs_kernel<false, false, false>), cgt, dim3(256), 0, stream, cr, dp->partial, dst);
    else if (pairs) hipLaunchKernelGGL((combine_runs_kernel<true, false, true>), cgt, dim3(256), 0, stream, cr, dp->partial, dst);
    else hipLaunchKernelGGL((combine_runs_kernel<true, false, false>), cgt, dim3(256), 0, stream, cr, dp->partial, dst);
    KERNEL_CHECK();
    return BP5_OK;
  }
  if (set) hipLaunchKernelGGL(combine_kernel<false>, cg, dim3(256), 0, stream, dp->sh_dof, dp->sh_off, dp->sh_slot, dp->partial, dst, dp->n_shared);
  else hipLaunchKernelGGL(combine_kernel<true>, cg, dim3(256), 0, stream, dp->sh_dof, dp->sh_off, dp->sh_slot, dp->partial, dst, dp->n_shared);
  KERNEL_CHECK();
  return BP5_OK;
}

// [c0,c1) == union of whole cell blocks [b0,b1) of the caller's blocking?
bool block_aligned(const bp5_mf *mf, uint32_t c0, uint32_t c1, uint32_t *b0, uint32_t *b1)
{
  const auto &o = mf->h_block_off;
  if (o.empty() || c1 <= c0) return false;
  const auto i0 = std::lower_bound(o.begin(), o.end(), c0), i1 = std::lower_bound(o.begin(), o.end(), c1);
  if (i0 == o.end() || i1 == o.end() || *i0 != c0 || *i1 != c1) return false;
  *b0 = (uint32_t)(i0 - o.begin());
  *b1 = (uint32_t)(i1 - o.begin());
  return true;
}
// The block kernel for the cells [c0, c1) = the blocks [b0, b1) of the caller's blocking?  Decided once per handle (auto_block): the LDS of the
// default shape fits `wg_per_cu` workgroups per CU, the plan has packed indices where the build at hand needs them, and there are bricks
// enough for the persistent workgroups to balance.  Round 1 measured 3.6 bricks per workgroup (54^3 cells) 4 % behind the pencil kernel
// as a bare operator; with the CG dot products fused into the write-out the block kernel is ahead there too (profiles/r2: 0.439 vs
// 0.446 ms per iteration), so the bar dropped to 3 bricks per workgroup -- and, measured down the reference's mesh family at p = 4
// (profiles/r2 "small meshes"), the fused iteration wins from 2 bricks per CU on (1.1e6 DoFs: +15 %; 5.4e5 DoFs: par; below: the pencil
// kernel; p = 3: +34 %, p = 6: +14 %, p = 7: +8 %, p = 1: +4 % at 2-7 bricks per CU).
// Sub-ranges: worth it only while the range still feeds the persistent grid (else the pencil kernel)
static bool block_kernel_pays(bp5_mf *mf, uint32_t c0, uint32_t c1, uint32_t b0, uint32_t b1, int wg_per_cu, bool need_packed)
{
  if (mf->auto_block < 0) {
    bp5_mf::DevPlan *dp = nullptr;
    mf->auto_block = 0;
    if (get_plan_raw(mf, -block_cpt(mf), &dp, 64) == BP5_OK && (dp->packed || !need_packed)) {
      const size_t lds = block_default_lds_bytes(mf->degree, dp->max_list); // (the launcher's own formula)
      mf->auto_block = lds * wg_per_cu <= 160 * 1024 && dp->n_groups >= 2u * (uint32_t)std::max(device_cus(mf), 1);
    }
  }
  if (!mf->auto_block) return false;
  return (c0 == 0 && c1 == mf->n_cells) || (b1 - b0) >= 30u * (uint32_t)std::max(mf->n_cus, 1);
}
// Variant 0 = library default.  The measured choices (profiles/r1): p = 1, 3 x-row team kernel; p = 4 on a mesh
// handed over in cell blocks that fit three workgroups per CU: block-assembled kernel (no atomics, no zero-fill,
// bitwise reproducible), whole cell range only; p = 4 affine geometry: team kernel; everything else: pencil kernel.
static int effective_variant(bp5_mf *mf, uint32_t c0, uint32_t c1)
{
  const int v = mf->apply_variant;
  if (v != 0) return v;
  if (mf->trilinear()) return 0; // the trilinear pencil kernel whatever the mesh, brick-ordered ones included: no block, team or march build computes the metric
  if (mf->overint()) return 0; // the pencil kernel whatever the mesh: no block, team or march build reads Q^3 points (so no fused dot products either)
  if (mf->has_hanging && mf->geometry_mode == BP5_GEOM_AFFINE) return 90;
  uint32_t b0, b1;
  if (mf->f32_metric() || mf->operator_kind == BP5_OP_MASS) {
    // FP32 planes, the mass operator: the degree's (mass) pencil kernel, or the block kernel where it pays, with packed indices at every degree and
    // the workgroups per CU of the build: FP32 planes three up to p = 4 and two beyond, the mass build what block_wg_per_cu launches it with
    if (!block_lpc(mf->degree) || mf->h_block_off.empty() || !block_aligned(mf, c0, c1, &b0, &b1)) return 0;
    const int wg = mf->f32_metric() ? (mf->degree <= 4 ? 3 : 2) : mass_block_wg_per_cu(mf->degree);
    return block_kernel_pays(mf, c0, c1, b0, b1, wg, true) ? 56 : 0;
  }
  if (mf->operator_kind == BP5_OP_HELMHOLTZ || mf->has_hanging) { // pencil kernel, or the block kernel (two workgroups per CU, packed indices)
    const int pencil = mf->has_hanging ? 90 : 0;
    if (!block_lpc(mf->degree) || mf->h_block_off.empty() || !block_aligned(mf, c0, c1, &b0, &b1)) return pencil;
    return block_kernel_pays(mf, c0, c1, b0, b1, 2, true) ? 56 : pencil;
  }
  if ((mf->degree == 1 || mf->degree == 3) && mf->h_block_off.empty()) {
    if (mf->geometry_mode == BP5_GEOM_AFFINE) return 0;
    if (mf->auto_team < 0) { // an irregular cell order can exhaust the team plan's rounds: then the atomic pencil kernel
      bp5_mf::DevPlan *dp = nullptr;
      mf->auto_team = get_plan_raw(mf, mf->degree == 1 ? 64 : 16, &dp) == BP5_OK;
    }
    return mf->auto_team ? 10 : 0;
  }
  if (!block_lpc(mf->degree)) return 0;
  const int fallback = (mf->degree == 4 && mf->geometry_mode == BP5_GEOM_AFFINE) ? 10 : (mf->degree == 3 || mf->degree == 1) ? 10 : 0; // else the pencil kernel
  if (mf->degree != 4 && mf->geometry_mode == BP5_GEOM_AFFINE) return 0; // the affine block build exists at p = 4 only
  if (mf->h_block_off.empty() || !block_aligned(mf, c0, c1, &b0, &b1)) return fallback;
  // LDS of the default shape: one transpose tile per cell slot + the brick's accumulator + two run tables; p <= 4 must fit
  // three workgroups per CU, p >= 5 (more registers per lane: two workgroups per CU anyway) two
  if (!block_kernel_pays(mf, c0, c1, b0, b1, mf->degree <= 4 ? 3 : 2, mf->degree != 4)) return fallback;
  if (mf->geometry_mode == BP5_GEOM_AFFINE) { // the affine build needs the packed indices
    bp5_mf::DevPlan *dp = nullptr;
    if (get_plan_raw(mf, -block_cpt(mf), &dp, 64) != BP5_OK || !dp->packed) return fallback;
  }
  return 56;
}
// the block kernel through launch_block_default: variant 56 at every degree that has one, at p = 4 also 63 (its sibling of the timing library)
static bool is_default_block(const bp5_mf *mf, int ev) { return block_lpc(mf->degree) != 0 && (ev == 56 || (mf->degree == 4 && ev == 63)); }
// kernels that define every entry of dst themselves (owner stores + combine pass) need no zero-fill
static bool variant_overwrites(const bp5_mf *mf, int ev)
{
  return decode_variant(ev).overwrites && !(mf->geometry_mode == BP5_GEOM_AFFINE && mf->degree != 4); // (affine: the pencil kernel but at p = 4)
}

// One operator application: resolves the variant for the call's range (unless the caller fixed it) and dispatches on the degree
static int launch_apply(bp5_mf *mf, ApplyCall &call, const double *coef, const double *src, double *dst)
{
  if (!call.keep_variant) call.set_variant(effective_variant(mf, call.c0, call.c1));
  return for_degree(mf->degree, [&](auto P) { return apply_degree_impl<P()>(mf, call, coef, src, dst); });
}
// ... with nothing asked for but a cell range and the overwrite mode
static int launch_apply(bp5_mf *mf, const double *coef, const double *src, double *dst, uint32_t c0, uint32_t c1, bool overwrite = false)
{
  ApplyCall call;
  call.c0 = c0; call.c1 = c1; call.overwrite = overwrite;
  return launch_apply(mf, call, coef, src, dst);
}

extern "C" int bp5_apply_cells(bp5_mf *mf, const double *coef, const double *src, double *dst, uint32_t c0, uint32_t c1)
{
  if (!mf || (!coef && mf->geometry_mode == BP5_GEOM_MERGED6) || !src || !dst) return fail(BP5_ERR_INVALID, "null argument");
  if (c1 > mf->n_cells || c0 > c1) return fail(BP5_ERR_INVALID, "cell range out of bounds");
  if (src == dst) return fail(BP5_ERR_INVALID, "src and dst must differ");
  HIP_TRY(hipSetDevice(mf->device));
  return launch_apply(mf, coef, src, dst, c0, c1);
}
extern "C" int bp5_copy_constrained(bp5_mf *mf, const double *src, double *dst)
{
  if (!mf || !src || !dst) return fail(BP5_ERR_INVALID, "null argument");
  if (!mf->n_constrained) return BP5_OK;
  hipLaunchKernelGGL(copy_constrained_kernel, dim3((mf->n_constrained + 255) / 256), dim3(256), 0, mf->stream, mf->d_constrained,
                     mf->n_constrained, src, dst);
  KERNEL_CHECK();
  return BP5_OK;
}
extern "C" int bp5_set_constrained(bp5_mf *mf, double value, double *dst)
{
  if (!mf || !dst) return fail(BP5_ERR_INVALID, "null argument");
  if (!mf->n_constrained) return BP5_OK;
  hipLaunchKernelGGL(set_constrained_kernel, dim3((mf->n_constrained + 255) / 256), dim3(256), 0, mf->stream, mf->d_constrained,
                     mf->n_constrained, value, dst);
  KERNEL_CHECK();
  return BP5_OK;
}
extern "C" int bp5_apply(bp5_mf *mf, const double *coef, const double *src, double *dst, int zero_dst)
{
  if (!mf || (!coef && mf->geometry_mode == BP5_GEOM_MERGED6) || !src || !dst) return fail(BP5_ERR_INVALID, "null argument");
  if (src == dst) return fail(BP5_ERR_INVALID, "src and dst must differ");
  HIP_TRY(hipSetDevice(mf->device));
  BP5_TRY(launch_apply(mf, coef, src, dst, 0, mf->n_cells, zero_dst != 0));
  return bp5_copy_constrained(mf, src, dst);
}

// ------------------------------------------------------------------------------------ block vectors (n_components)
// every refusal of bp5_apply_components / bp5_cg_solve_components and of their *_distributed twins, decided before any launch.  What needs no
// handle comes first, so that a bad layout is named as such whatever the handle is.
static inline bool aligned16(const void *p);
// ... the part that needs no handle (all that the bp5_halo_*_components entries, which take ONE block vector, check besides the handle: v == w)
static int components_layout_check(int n_components, size_t ld, const double *v, const double *w)
{
  if (!v || !w) return fail(BP5_ERR_INVALID, "null argument");
  if (n_components < 1 || n_components > BP5_MAX_COMPONENTS) return fail(BP5_ERR_INVALID, "n_components must be 1 .. BP5_MAX_COMPONENTS");
  if (ld & 1) return fail(BP5_ERR_INVALID, "block vectors: ld must be even (every block 16-byte aligned)");
  if (!aligned16(v) || !aligned16(w)) return fail(BP5_ERR_INVALID, "block vectors must be 16-byte aligned");
  return BP5_OK;
}
// with_exchange: the *_distributed entries, which bring the halo exchange a handle with a communicator and neighbours needs
static int components_check(const bp5_mf *mf, const double *coef, int n_components, size_t ld, const double *src, double *dst, bool with_exchange = false)
{
  BP5_TRY(components_layout_check(n_components, ld, src, dst));
  if (src == dst) return fail(BP5_ERR_INVALID, "src and dst overlap");
  if (!mf) return fail(BP5_ERR_INVALID, "null handle");
  if (ld < mf->n_local()) return fail(BP5_ERR_INVALID, "block vectors: ld < n_owned + n_ghost");
  const size_t extent = (size_t)(n_components - 1) * ld + mf->n_local();
  if (src < dst + extent && dst < src + extent) return fail(BP5_ERR_INVALID, "src and dst overlap");
  if (mf->overint()) return overint_refuse("block vectors (CEED BP2 / BP4) are not supported");
  if (mf->f32_metric()) return fail(BP5_ERR_UNSUPPORTED, "block vectors: FP32 metric planes are not supported");
  if (mf->operator_kind == BP5_OP_MASS) return fail(BP5_ERR_UNSUPPORTED, "block vectors: the mass operator is not supported");
  if (mf->operator_kind != BP5_OP_POISSON) return fail(BP5_ERR_UNSUPPORTED, "block vectors: the Helmholtz operator is not supported");
  if (mf->has_hanging) return fail(BP5_ERR_UNSUPPORTED, "block vectors: meshes with hanging nodes are not supported");
  if (mf->trilinear()) return trilinear_refuse("block vectors are not supported");
  if (mf->geometry_mode != BP5_GEOM_MERGED6) return fail(BP5_ERR_UNSUPPORTED, "block vectors: the affine geometry mode is not supported");
  if (!with_exchange && mf->has_neighbors()) return fail(BP5_ERR_UNSUPPORTED, "block vectors: no halo exchange (a handle with a communicator and neighbours)");
  if (!coef) return fail(BP5_ERR_INVALID, "null argument");
  return BP5_OK;
}
// zero-fill of the blocks, padding untouched: one 1-D fill per block (hipMemset2DAsync takes a slow path whenever ld != n_local: a three-component
// application at 1e8 DoFs took 24.2 ms with it against 8.2 ms with these fills, profiles/components a_* / b_*)
static int components_zero(bp5_mf *mf, int n_components, size_t ld, double *dst)
{
  for (int c = 0; c < n_components; ++c) HIP_TRY(hipMemsetAsync(dst + (size_t)c * ld, 0, mf->n_local() * sizeof(double), mf->stream));
  return BP5_OK;
}
// [dst = 0] ; dst_c += A src_c on validated arguments (the Dirichlet copy is the caller's next launch)
static int components_apply_cells(bp5_mf *mf, const double *coef, int n_components, size_t ld, const double *src, double *dst, uint32_t c0, uint32_t c1);
static int components_apply(bp5_mf *mf, const double *coef, int n_components, size_t ld, const double *src, double *dst, bool zero)
{
  if (zero) BP5_TRY(components_zero(mf, n_components, ld, dst));
  return components_apply_cells(mf, coef, n_components, ld, src, dst, 0, mf->n_cells);
}
// dst_c += A src_c over the cells [c0, c1) (empty: nothing is launched)
static int components_apply_cells(bp5_mf *mf, const double *coef, int n_components, size_t ld, const double *src, double *dst, uint32_t c0, uint32_t c1)
{
  switch (mf->degree) {
    case 1: BP5_TRY(apply_components_degree_impl<1>(mf, coef, n_components, ld, src, dst, c0, c1)); break;
    case 2: BP5_TRY(apply_components_degree_impl<2>(mf, coef, n_components, ld, src, dst, c0, c1)); break;
    case 3: BP5_TRY(apply_components_degree_impl<3>(mf, coef, n_components, ld, src, dst, c0, c1)); break;
    case 4: BP5_TRY(apply_components_degree_impl<4>(mf, coef, n_components, ld, src, dst, c0, c1)); break;
    case 5: BP5_TRY(apply_components_degree_impl<5>(mf, coef, n_components, ld, src, dst, c0, c1)); break;
    case 6: BP5_TRY(apply_components_degree_impl<6>(mf, coef, n_components, ld, src, dst, c0, c1)); break;
    case 7: BP5_TRY(apply_components_degree_impl<7>(mf, coef, n_components, ld, src, dst, c0, c1)); break;
    case 8: BP5_TRY(apply_components_degree_impl<8>(mf, coef, n_components, ld, src, dst, c0, c1)); break;
    default: return fail(BP5_ERR_INVALID, "unsupported degree");
  }
  return BP5_OK;
}
static int components_copy_constrained(bp5_mf *mf, int n_components, size_t ld, const double *src, double *dst)
{
  if (!mf->n_constrained) return BP5_OK;
  hipLaunchKernelGGL(copy_constrained_components_kernel, dim3((mf->n_constrained + 255) / 256, n_components), dim3(256), 0, mf->stream, mf->d_constrained,
                     mf->n_constrained, src, dst, ld);
  KERNEL_CHECK();
  return BP5_OK;
}
extern "C" int bp5_apply_components(bp5_mf *mf, const double *coef, int n_components, size_t ld, const double *src, double *dst, int zero_dst)
{
  BP5_TRY(components_check(mf, coef, n_components, ld, src, dst));
  HIP_TRY(hipSetDevice(mf->device));
  BP5_TRY(components_apply(mf, coef, n_components, ld, src, dst, zero_dst != 0));
  return components_copy_constrained(mf, n_components, ld, src, dst);
}

// ------------------------------------------------------------------------------------ linear elasticity (three coupled components)
// every refusal of the bp5_elasticity_* entries and of bp5_cg_solve_elasticity, decided before any launch, each naming "elasticity".  What needs
// no handle comes first (layout, then the parameters), so that a bad layout is named as such whatever the handle is.
static int elasticity_refuse(int status, const char *what) { return fail(status, std::string("elasticity: ") + what); }
static int elasticity_parameter_check(double lambda, double mu)
{
  if (!std::isfinite(lambda) || !std::isfinite(mu)) return elasticity_refuse(BP5_ERR_INVALID, "lambda and mu must be finite");
  if (!(mu > 0.0)) return elasticity_refuse(BP5_ERR_INVALID, "mu must be positive");
  if (!(lambda + 2.0 / 3.0 * mu > 0.0)) return elasticity_refuse(BP5_ERR_INVALID, "the bulk modulus lambda + 2/3 mu must be positive");
  return BP5_OK;
}
// the handle can serve the operator at all (the ten planes, the kernels): what bp5_elasticity_coef_size / _compute_metric check
static int elasticity_handle_check(const bp5_mf *mf)
{
  if (!mf) return elasticity_refuse(BP5_ERR_INVALID, "null handle");
  if (mf->overint()) return elasticity_refuse(BP5_ERR_UNSUPPORTED, "Gauss(p+2) quadrature (BP5_QUAD_GAUSS_OVER) is not supported");
  if (mf->operator_kind != BP5_OP_POISSON) return elasticity_refuse(BP5_ERR_UNSUPPORTED, "a handle of the Helmholtz or mass operator class is not supported (Poisson class only)");
  if (mf->has_hanging) return elasticity_refuse(BP5_ERR_UNSUPPORTED, "meshes with hanging nodes are not supported");
  if (mf->trilinear()) return elasticity_refuse(BP5_ERR_UNSUPPORTED, "the trilinear geometry mode (BP5_GEOM_TRILINEAR) is not supported");
  if (mf->geometry_mode != BP5_GEOM_MERGED6) return elasticity_refuse(BP5_ERR_UNSUPPORTED, "the affine geometry mode is not supported");
  if (mf->f32_metric()) return elasticity_refuse(BP5_ERR_UNSUPPORTED, "FP32 metric planes are not supported");
  if (mf->has_neighbors()) return elasticity_refuse(BP5_ERR_UNSUPPORTED, "no halo exchange (a handle with a communicator and neighbours)");
  return BP5_OK;
}
// v, w: the block vectors of the call (w == NULL: one vector); distinct: they must not overlap
static int elasticity_check(const bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, const double *v, const double *w, bool distinct)
{
  if (!v || (distinct && !w) || !coef) return elasticity_refuse(BP5_ERR_INVALID, "null argument");
  if (ld & 1) return elasticity_refuse(BP5_ERR_INVALID, "ld must be even (every block 16-byte aligned)");
  if (!aligned16(v) || (w && !aligned16(w))) return elasticity_refuse(BP5_ERR_INVALID, "block vectors must be 16-byte aligned");
  if (distinct && v == w) return elasticity_refuse(BP5_ERR_INVALID, "src and dst overlap");
  BP5_TRY(elasticity_parameter_check(lambda, mu));
  if (!mf) return elasticity_refuse(BP5_ERR_INVALID, "null handle");
  if (ld < mf->n_local()) return elasticity_refuse(BP5_ERR_INVALID, "ld < n_owned + n_ghost");
  const size_t extent = 2 * ld + mf->n_local();
  if (distinct && v < w + extent && w < v + extent) return elasticity_refuse(BP5_ERR_INVALID, "src and dst overlap");
  return elasticity_handle_check(mf);
}
// ... of a call that brings no vector of its own (bp5_elasticity_chebyshev_create with inv_diag == NULL): the metric array, the stride, the
// parameters, the handle -- in elasticity_check's order
static int elasticity_check_no_vector(const bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld)
{
  if (!coef) return elasticity_refuse(BP5_ERR_INVALID, "null argument");
  if (ld & 1) return elasticity_refuse(BP5_ERR_INVALID, "ld must be even (every block 16-byte aligned)");
  if (!aligned16(coef)) return elasticity_refuse(BP5_ERR_INVALID, "the metric array must be 16-byte aligned");
  BP5_TRY(elasticity_parameter_check(lambda, mu));
  if (!mf) return elasticity_refuse(BP5_ERR_INVALID, "null handle");
  if (ld < mf->n_local()) return elasticity_refuse(BP5_ERR_INVALID, "ld < n_owned + n_ghost");
  return elasticity_handle_check(mf);
}
extern "C" int bp5_elasticity_coef_size(const bp5_mf *mf, size_t *n_doubles)
{
  if (!n_doubles) return elasticity_refuse(BP5_ERR_INVALID, "null argument");
  BP5_TRY(elasticity_handle_check(mf));
  *n_doubles = 10 * (size_t)mf->n_cells * mf->n3; // (the handle's own plane count stays uncommitted: this array is not the one bp5_apply reads)
  return BP5_OK;
}
extern "C" int bp5_elasticity_compute_metric(bp5_mf *mf, double *coef)
{
  if (!coef) return elasticity_refuse(BP5_ERR_INVALID, "null argument");
  BP5_TRY(elasticity_handle_check(mf));
  HIP_TRY(hipSetDevice(mf->device));
  return elasticity_compute_metric(mf, coef);
}
extern "C" int bp5_elasticity_apply(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, const double *src, double *dst, int zero_dst)
{
  BP5_TRY(elasticity_check(mf, coef, lambda, mu, ld, src, dst, true));
  HIP_TRY(hipSetDevice(mf->device));
  if (zero_dst) BP5_TRY(components_zero(mf, 3, ld, dst));
  BP5_TRY(elasticity_apply_cells(mf, coef, lambda, mu, ld, src, dst, 0, mf->n_cells));
  return components_copy_constrained(mf, 3, ld, src, dst);
}
extern "C" int bp5_elasticity_apply_cells(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, const double *src, double *dst, uint32_t cell_begin,
                                          uint32_t cell_end)
{
  BP5_TRY(elasticity_check(mf, coef, lambda, mu, ld, src, dst, true));
  if (cell_begin > cell_end || cell_end > mf->n_cells) return elasticity_refuse(BP5_ERR_INVALID, "cell range outside [0, n_cells]");
  HIP_TRY(hipSetDevice(mf->device));
  return elasticity_apply_cells(mf, coef, lambda, mu, ld, src, dst, cell_begin, cell_end);
}
extern "C" int bp5_elasticity_compute_diagonal(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, double *diag, int invert)
{
  BP5_TRY(elasticity_check(mf, coef, lambda, mu, ld, diag, nullptr, false));
  HIP_TRY(hipSetDevice(mf->device));
  BP5_TRY(components_zero(mf, 3, ld, diag));
  BP5_TRY(elasticity_diagonal(mf, coef, lambda, mu, ld, diag));
  for (int c = 0; c < 3; ++c) { // bp5_compute_diagonal's convention, block by block: A_eff = P A P + (I - P)
    BP5_TRY(bp5_set_constrained(mf, 1.0, diag + (size_t)c * ld));
    if (invert && mf->n_owned) {
      hipLaunchKernelGGL(reciprocal_kernel, dim3((mf->n_owned + 255) / 256), dim3(256), 0, mf->stream, diag + (size_t)c * ld, (size_t)mf->n_owned);
      KERNEL_CHECK();
    }
  }
  return BP5_OK;
}

// ------------------------------------------------------------------------------------ rhs / norms
template <int n>
static int launch_rhs(bp5_mf *mf, double *b)
{
  const uint32_t grid = cell_grid(mf, 65535u * 16);
  hipLaunchKernelGGL(rhs_kernel<n>, dim3(grid), dim3(n, n, n), 0, mf->stream, mf->d_l2g, mf->d_coords, mf->d_tab_gauss, mf->n_cells, b,
                     mf->has_hanging ? (const uint32_t *)mf->d_hang_mask : (const uint32_t *)nullptr, (const double *)mf->d_hang_I);
  KERNEL_CHECK();
  return BP5_OK;
}
extern "C" int bp5_assemble_rhs(bp5_mf *mf, double *b)
{
  if (!mf || !b) return fail(BP5_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(mf->device));
  HIP_TRY(hipMemsetAsync(b, 0, mf->n_local() * sizeof(double), mf->stream));
  BP5_TRY(for_degree(mf->degree, [&](auto P) { return launch_rhs<P() + 1>(mf, b); }));
  if (mf->has_neighbors()) BP5_TRY(bp5_halo_scatter_add(mf, b));
  return bp5_set_constrained(mf, 0.0, b);
}
template <int n>
static int launch_diagonal(bp5_mf *mf, const double *coef, double *diag)
{
  const uint32_t grid = cell_grid(mf, 65536u);
  const bool affine = mf->geometry_mode == BP5_GEOM_AFFINE;
  if (mf->operator_kind == BP5_OP_MASS) { // (conforming, one double plane: bp5_mf_set_operator refuses everything else)
    hipLaunchKernelGGL(mass_diagonal_kernel<n>, dim3(grid), dim3(n, n, n), 0, mf->stream, mf->d_l2g, coef, mf->coef_cell_stride, mf->d_tab, mf->n_cells, diag);
    KERNEL_CHECK();
    return BP5_OK;
  }
  if (mf->f32_metric()) // (conforming, six planes: bp5_mf_set_metric_precision refuses everything else)
    hipLaunchKernelGGL((diagonal_kernel<n, float>), dim3(grid), dim3(n, n, n), 0, mf->stream, mf->d_l2g, reinterpret_cast<const float *>(coef), mf->coef_plane_stride,
                       mf->coef_cell_stride, (const double *)nullptr, mf->d_tab, mf->n_cells, diag, (const uint32_t *)nullptr, mf->n_planes());
  else
  hipLaunchKernelGGL(diagonal_kernel<n>, dim3(grid), dim3(n, n, n), 0, mf->stream, mf->d_l2g, affine ? mf->d_scalar_plane : coef,
                     affine ? (uint64_t)mf->n_cells * mf->n3 : mf->coef_plane_stride, mf->coef_cell_stride, affine ? mf->d_gcell : (const double *)nullptr, mf->d_tab, mf->n_cells, diag,
                     mf->has_hanging ? (const uint32_t *)mf->d_hang_mask : (const uint32_t *)nullptr, mf->n_planes());
  KERNEL_CHECK();
  if (mf->has_hanging) { // the coarse DoFs named on constrained faces / edges: one cell-operator application per such entry
    hipLaunchKernelGGL(diagonal_hanging_kernel<n>, dim3(grid), dim3(n, n, n), 0, mf->stream, mf->d_l2g, affine ? mf->d_scalar_plane : coef,
                       affine ? (uint64_t)mf->n_cells * mf->n3 : mf->coef_plane_stride, affine ? (uint64_t)mf->n3 : mf->coef_cell_stride, affine ? mf->d_gcell : (const double *)nullptr,
                       mf->d_tab, mf->n_cells, diag, (const uint32_t *)mf->d_hang_mask, (const double *)mf->d_hang_I);
    KERNEL_CHECK();
  }
  return BP5_OK;
}
static int diagonal_dispatch(bp5_mf *mf, const double *coef, double *diag)
{
  return for_degree(mf->degree, [&](auto P) { return launch_diagonal<P() + 1>(mf, coef, diag); });
}
extern "C" int bp5_compute_diagonal(bp5_mf *mf, const double *coef, double *diag, int invert)
{
  if (!mf || (!coef && mf->geometry_mode == BP5_GEOM_MERGED6) || !diag) return fail(BP5_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(mf->device));
  HIP_TRY(hipMemsetAsync(diag, 0, mf->n_local() * sizeof(double), mf->stream));
  if (mf->n_cells) BP5_TRY(mf->trilinear() ? trilinear_diagonal(mf, diag) : mf->overint() ? overint_diagonal(mf, coef, diag) : diagonal_dispatch(mf, coef, diag));
  if (mf->has_neighbors()) { // ghost contributions to their owners
    BP5_TRY(bp5_halo_scatter_add(mf, diag));
    BP5_TRY(bp5_halo_zero_ghosts(mf, diag));
  }
  BP5_TRY(bp5_set_constrained(mf, 1.0, diag));                                     // A_eff = P A P + (I - P)
  if (invert && mf->n_owned) {
    hipLaunchKernelGGL(reciprocal_kernel, dim3((mf->n_owned + 255) / 256), dim3(256), 0, mf->stream, diag, (size_t)mf->n_owned);
    KERNEL_CHECK();
  }
  return BP5_OK;
}
template <int n>
static int launch_l2(bp5_mf *mf, const double *u, double *out)
{
  const uint32_t grid = cell_grid(mf, 4096u);
  hipLaunchKernelGGL(l2norm_kernel<n>, dim3(grid), dim3(n, n, n), 0, mf->stream, mf->d_l2g, mf->d_coords, mf->d_tab_gauss, mf->n_cells, u,
                     out, mf->has_hanging ? (const uint32_t *)mf->d_hang_mask : (const uint32_t *)nullptr, (const double *)mf->d_hang_I);
  KERNEL_CHECK();
  return BP5_OK;
}
static int l2_dispatch(bp5_mf *mf, const double *u, double *out)
{
  return for_degree(mf->degree, [&](auto P) { return launch_l2<P() + 1>(mf, u, out); });
}
extern "C" int bp5_l2_norm_solution(bp5_mf *mf, const double *u, double *result)
{
  if (!mf || !u || !result) return fail(BP5_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(mf->device));
  // the cell integrals read ghost DoFs through local_to_global: refresh them first, as the reference does on its ghosted copy
  // (ghost_solution_host, bp5/step-64.cu:602-616; deal.II's update_ghost_values() is const as well), and leave them zeroed
  const bool ghosts = mf->has_neighbors();
  if (ghosts) BP5_TRY(bp5_halo_gather(mf, const_cast<double *>(u)));
  HIP_TRY(hipMemsetAsync(mf->d_scalar, 0, sizeof(double), mf->stream));
  BP5_TRY(l2_dispatch(mf, u, mf->d_scalar));
  if (ghosts) BP5_TRY(bp5_halo_zero_ghosts(mf, const_cast<double *>(u)));
  if (mf->comm) BP5_TRY(bp5_comm_allreduce_sum(mf, mf->d_scalar, 1));
  double s = 0.0;
  HIP_TRY(hipMemcpyAsync(&s, mf->d_scalar, sizeof(double), hipMemcpyDeviceToHost, mf->stream));
  HIP_TRY(hipStreamSynchronize(mf->stream));
  *result = std::sqrt(s);
  return BP5_OK;
}

// ------------------------------------------------------------------------------------ BLAS-1
static inline int stream_grid(size_t n, int per_thread)
{
  size_t b = (n + (size_t)VB * per_thread - 1) / ((size_t)VB * per_thread);
  return (int)std::min<size_t>(std::max<size_t>(b, 1), MAXBLK);
}
// Streaming kernels WITHOUT a reduction: one trip per workgroup ("flat" launch).  profiles/r4 hbm_sweep: on a capped grid-stride grid the
// workgroups drift apart and the write stream loses its locality -- fill 4.3 against 6.7 TB/s, the update kernels 4.8-4.9 against 5.6-5.9
static inline int stream_grid_flat(const bp5_mf *mf, size_t n, int per_thread)
{
  if (!mf->tune[BP5_TUNE_UPDATE_FLAT]) return stream_grid(n, per_thread);
  const size_t b = (n + (size_t)VB * per_thread - 1) / ((size_t)VB * per_thread);
  return (int)std::min<size_t>(std::max<size_t>(b, 1), (size_t)1 << 30);
}
static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

extern "C" int bp5_vec_fill(bp5_mf *mf, double *v, double value, size_t n)
{
  if (!mf || !v) return fail(BP5_ERR_INVALID, "null argument");
  if (!aligned16(v)) return fail(BP5_ERR_INVALID, "vectors must be 16-byte aligned");
  hipLaunchKernelGGL(vec_kernel<0>, dim3(stream_grid_flat(mf, n, 2)), dim3(VB), 0, mf->stream, v, (const double *)nullptr, value, 0.0, n);
  KERNEL_CHECK();
  return BP5_OK;
}
extern "C" int bp5_vec_axpy(bp5_mf *mf, double *y, double a, const double *x, size_t n)
{
  if (!mf || !y || !x) return fail(BP5_ERR_INVALID, "null argument");
  if (!aligned16(y) || !aligned16(x)) return fail(BP5_ERR_INVALID, "vectors must be 16-byte aligned");
  hipLaunchKernelGGL(vec_kernel<1>, dim3(stream_grid_flat(mf, n, 2)), dim3(VB), 0, mf->stream, y, x, 0.0, a, n);
  KERNEL_CHECK();
  return BP5_OK;
}
extern "C" int bp5_vec_equ(bp5_mf *mf, double *y, double a, const double *x, size_t n)
{
  if (!mf || !y || !x) return fail(BP5_ERR_INVALID, "null argument");
  if (!aligned16(y) || !aligned16(x)) return fail(BP5_ERR_INVALID, "vectors must be 16-byte aligned");
  hipLaunchKernelGGL(vec_kernel<2>, dim3(stream_grid_flat(mf, n, 2)), dim3(VB), 0, mf->stream, y, x, 0.0, a, n);
  KERNEL_CHECK();
  return BP5_OK;
}
extern "C" int bp5_vec_sadd(bp5_mf *mf, double *y, double s, double a, const double *x, size_t n)
{
  if (!mf || !y || !x) return fail(BP5_ERR_INVALID, "null argument");
  if (!aligned16(y) || !aligned16(x)) return fail(BP5_ERR_INVALID, "vectors must be 16-byte aligned");
  hipLaunchKernelGGL(vec_kernel<3>, dim3(stream_grid_flat(mf, n, 2)), dim3(VB), 0, mf->stream, y, x, s, a, n);
  KERNEL_CHECK();
  return BP5_OK;
}
extern "C" int bp5_vec_dot(bp5_mf *mf, const double *x, const double *y, size_t n, double *result)
{
  if (!mf || !y || !x || !result) return fail(BP5_ERR_INVALID, "null argument");
  if (!aligned16(y) || !aligned16(x)) return fail(BP5_ERR_INVALID, "vectors must be 16-byte aligned");
  const int g = stream_grid(n, 2);
  hipLaunchKernelGGL(dot_kernel, dim3(g), dim3(VB), 0, mf->stream, x, y, n, mf->d_partials);
  hipLaunchKernelGGL(finalize_kernel<1>, dim3(1), dim3(VB), 0, mf->stream, mf->d_partials, g, mf->d_scalar, (const int *)nullptr);
  KERNEL_CHECK();
  HIP_TRY(hipMemcpyAsync(result, mf->d_scalar, sizeof(double), hipMemcpyDeviceToHost, mf->stream));
  HIP_TRY(hipStreamSynchronize(mf->stream));
  return BP5_OK;
}

// global reductions of the distributed vector (owned entries of every rank): one on-stream all-reduce when a
// communicator is attached
static int reduce_to_host(bp5_mf *mf, int grid, double *result)
{
  hipLaunchKernelGGL(finalize_kernel<1>, dim3(1), dim3(VB), 0, mf->stream, mf->d_partials, grid, mf->d_scalar, (const int *)nullptr);
  KERNEL_CHECK();
  if (mf->comm) NCCL_TRY(ncclAllReduce(mf->d_scalar, mf->d_scalar, 1, ncclDouble, ncclSum, mf->comm->comm, mf->stream));
  HIP_TRY(hipMemcpyAsync(result, mf->d_scalar, sizeof(double), hipMemcpyDeviceToHost, mf->stream));
  HIP_TRY(hipStreamSynchronize(mf->stream));
  return BP5_OK;
}
extern "C" int bp5_vec_l2_norm(bp5_mf *mf, const double *x, size_t n, double *result)
{
  if (!mf || !x || !result) return fail(BP5_ERR_INVALID, "null argument");
  if (!aligned16(x)) return fail(BP5_ERR_INVALID, "vectors must be 16-byte aligned");
  HIP_TRY(hipSetDevice(mf->device));
  const int g = stream_grid(n, 2);
  hipLaunchKernelGGL(dot_kernel, dim3(g), dim3(VB), 0, mf->stream, x, x, n, mf->d_partials);
  double s = 0.0;
  BP5_TRY(reduce_to_host(mf, g, &s));
  *result = sqrt(s);
  return BP5_OK;
}
extern "C" int bp5_vec_all_zero(bp5_mf *mf, const double *x, size_t n, int *result)
{
  if (!mf || !x || !result) return fail(BP5_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(mf->device));
  const int g = stream_grid(n, 1);
  hipLaunchKernelGGL(count_nonzero_kernel, dim3(g), dim3(VB), 0, mf->stream, x, n, mf->d_partials);
  double s = 0.0;
  BP5_TRY(reduce_to_host(mf, g, &s));
  *result = s == 0.0;
  return BP5_OK;
}

// ------------------------------------------------------------------------------------ RCCL
extern "C" int bp5_comm_unique_id(char *id)
{
  if (!id) return fail(BP5_ERR_INVALID, "null argument");
  static_assert(sizeof(ncclUniqueId) <= BP5_UNIQUE_ID_BYTES, "unique id size");
  ncclUniqueId uid;
  NCCL_TRY(ncclGetUniqueId(&uid));
  memset(id, 0, BP5_UNIQUE_ID_BYTES);
  memcpy(id, &uid, sizeof(uid));
  return BP5_OK;
}
extern "C" int bp5_comm_create(const char *id, int rank, int n_ranks, bp5_comm **out)
{
  if (!id || !out || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(BP5_ERR_INVALID, "bad argument");
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof(uid));
  bp5_comm *c = new bp5_comm;
  c->rank = rank; c->n_ranks = n_ranks;
  ncclResult_t r = ncclCommInitRank(&c->comm, n_ranks, uid, rank);
  if (r != ncclSuccess) { delete c; return fail(BP5_ERR_RCCL, std::string("ncclCommInitRank: ") + ncclGetErrorString(r)); }
  *out = c;
  return BP5_OK;
}
extern "C" int bp5_comm_destroy(bp5_comm *c)
{
  if (!c) return BP5_OK;
  if (c->comm) ncclCommDestroy(c->comm);
  delete c;
  return BP5_OK;
}
extern "C" int bp5_mf_set_comm(bp5_mf *mf, bp5_comm *comm)
{
  if (!mf) return fail(BP5_ERR_INVALID, "null handle");
  mf->comm = comm;
  return BP5_OK;
}
extern "C" int bp5_comm_allreduce_sum(bp5_mf *mf, double *buf, size_t n)
{
  if (!mf || !buf) return fail(BP5_ERR_INVALID, "null argument");
  if (!mf->comm) return BP5_OK; // (a one-rank communicator still goes through RCCL: the single-GPU tests exercise the call)
  NCCL_TRY(ncclAllReduce(buf, buf, n, ncclDouble, ncclSum, mf->comm->comm, mf->stream));
  return BP5_OK;
}
// Halo exchange.  The RCCL traffic runs on the handle's own communication stream, ordered against the compute stream by
// events, so that cell work enqueued between a *_start and its *_finish overlaps the transfer (the reference:
// update_ghost_values_start/finish, compress_start/finish inside cell_loop with overlap_communication_computation,
// bp5/step-64.cu:241,274).  With overlap switched off (bp5_mf_set_overlap) everything stays on the compute stream.
static int halo_streams(bp5_mf *mf)
{
  if (mf->comm_stream) return BP5_OK;
  // highest priority: the stream then gets a hardware queue of its own (a plain second stream was seen to share the
  // compute stream's queue -- in-order, no overlap at all: profiles/r2 c_*), and the short RCCL kernels are not queued
  // behind the cell kernel's workgroups
  int prio_lo = 0, prio_hi = 0;
  HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
  HIP_TRY(hipStreamCreateWithPriority(&mf->comm_stream, hipStreamNonBlocking, prio_hi));
  for (hipEvent_t &e : mf->ev_halo) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); // (hipEventReleaseToDevice was tried: +20 us per iteration, profiles/r4 z_*)
  // boundary-first schedule inside ONE launch: the communication stream waits for a counter the block kernel's workgroups bump once
  // their ghost-touching bricks are written out (hipStreamWaitValue64).  The counter is plain device memory: there the runtime implements
  // the wait by POLLING (profiles/r3/a_wait_value_probe.txt: same timing as a spin kernel; on signal memory the wait released only after
  // the producer kernel had ended), i.e. a mid-kernel release rests on runtime behaviour the API does not promise.  So the capability bit
  // alone is not trusted: a one-off producer / consumer pair checks that the waiting stream really is released while the producing kernel
  // is still running (bounded: the producer gives up after 2 ms); if not, the ghost-touching bricks get a launch of their own
  // (BP5_TUNE_BOUNDARY_FIRST = 0 selects that form by hand).
  int can = 0;
  if (hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, mf->device) != hipSuccess) can = 0;
  if (can && !mf->d_signal) {
    HIP_TRY(hipMalloc((void **)&mf->d_signal, 4 * sizeof(unsigned long long))); // [0] the counter, [1] consumer-ran flag, [2] self-check result
    HIP_TRY(hipMemset(mf->d_signal, 0, 4 * sizeof(unsigned long long)));
    HIP_TRY(hipStreamSynchronize(nullptr));
    mf->signal_target = 0;
  }
  if (can) {
    mf->signal_target += 1;
    hipLaunchKernelGGL(wait_value_probe_producer, dim3(1), dim3(64), 0, mf->stream, mf->d_signal, mf->d_signal + 1, mf->d_signal + 2, 200000LL /* 2 ms of the 100 MHz clock */);
    KERNEL_CHECK();
    const bool waited = hipStreamWaitValue64(mf->comm_stream, mf->d_signal, mf->signal_target, hipStreamWaitValueGte, ~0ull) == hipSuccess;
    if (waited) { hipLaunchKernelGGL(wait_value_probe_consumer, dim3(1), dim3(64), 0, mf->comm_stream, mf->d_signal + 1); KERNEL_CHECK(); }
    else (void)hipGetLastError();
    HIP_TRY(hipStreamSynchronize(mf->stream));
    HIP_TRY(hipStreamSynchronize(mf->comm_stream));
    unsigned long long released_mid_kernel = 0;
    HIP_TRY(hipMemcpy(&released_mid_kernel, mf->d_signal + 2, sizeof(released_mid_kernel), hipMemcpyDeviceToHost));
    if (!waited || !released_mid_kernel) can = 0;
  }
  mf->wait_value_ok = can;
  mf->can_wait_value = can && mf->tune[BP5_TUNE_BOUNDARY_FIRST] != 0;
  return BP5_OK;
}
extern "C" int bp5_mf_wait_value_available(bp5_mf *mf, int *available)
{
  if (!mf || !available) return fail(BP5_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(mf->device));
  BP5_TRY(halo_streams(mf));
  *available = mf->wait_value_ok == 1;
  return BP5_OK;
}
static int env_int(const char *name, int fallback)
{
  const char *e = getenv(name);
  return (e && *e) ? atoi(e) : fallback;
}
// initial values of the handle's knobs: the environment is read here, once per handle, and nowhere else (bp5.h: BP5_TUNE_*)
static void tuning_from_environment(bp5_mf *mf)
{
  mf->tune[BP5_TUNE_LATTICE_INDICES] = env_int("BP5_LATTICE_INDICES", 1) != 0;
  mf->tune[BP5_TUNE_EARLY_GATHER] = env_int("BP5_EARLY_GATHER", 1) != 0;
  mf->tune[BP5_TUNE_COMBINE_SIGNAL] = env_int("BP5_COMBINE_SIGNAL", 0) == 1;
  { const char *e = getenv("BP5_BOUNDARY_FIRST"); mf->tune[BP5_TUNE_BOUNDARY_FIRST] = !(e && !strcmp(e, "launches")); }
  mf->tune[BP5_TUNE_FOLD_SMALL] = env_int("BP5_FOLD_SMALL", 1) != 0;
  { const int u = env_int("BP5_UPDATE_UNROLL", 1); mf->tune[BP5_TUNE_UPDATE_UNROLL] = (u == 2 || u == 4) ? u : 1; }
  mf->tune[BP5_TUNE_UPDATE_FLAT] = env_int("BP5_UPDATE_FLAT", 1) != 0;
  { const int v = env_int("BP5_UPDATE_NT", -1); mf->tune[BP5_TUNE_UPDATE_NT] = v < 0 ? -1 : v != 0; }
  { const int v = env_int("BP5_COMBINE_WG_PER_CU", 16); mf->tune[BP5_TUNE_COMBINE_WG_PER_CU] = (v >= 0 && v <= 32) ? v : 16; }
  mf->tune[BP5_TUNE_INTERIOR_STORES] = env_int("BP5_INTERIOR_STORES", 1) != 0;
  mf->tune[BP5_TUNE_GHOST_COMBINE_ON_COMM] = env_int("BP5_GHOST_COMBINE_ON_COMM", 0) != 0;
  mf->tune[BP5_TUNE_FACE_CARRY] = env_int("BP5_FACE_CARRY", 1) != 0;
  { const int v = env_int("BP5_FUSED_UPDATE", -1); mf->tune[BP5_TUNE_FUSED_UPDATE] = (v >= -1 && v <= 1) ? v : -1; }
}
extern "C" int bp5_mf_set_tuning(bp5_mf *mf, int knob, int value)
{
  if (!mf || knob < 0 || knob >= BP5_TUNE_COUNT) return fail(BP5_ERR_INVALID, "unknown tuning knob");
  switch (knob) {
    case BP5_TUNE_UPDATE_UNROLL:
      if (value != 1 && value != 2 && value != 4) return fail(BP5_ERR_INVALID, "BP5_TUNE_UPDATE_UNROLL: 1, 2 or 4");
      break;
    case BP5_TUNE_UPDATE_NT:
      if (value < -1 || value > 1) return fail(BP5_ERR_INVALID, "BP5_TUNE_UPDATE_NT: -1, 0 or 1");
      break;
    case BP5_TUNE_FUSED_UPDATE:
      if (value < -1 || value > 1) return fail(BP5_ERR_INVALID, "BP5_TUNE_FUSED_UPDATE: -1, 0 or 1");
      break;
    case BP5_TUNE_COMBINE_WG_PER_CU:
      if (value < 0 || value > 32) return fail(BP5_ERR_INVALID, "BP5_TUNE_COMBINE_WG_PER_CU: 0 ... 32");
      break;
    case BP5_TUNE_LATTICE_INDICES:
      if (value != 0 && value != 1) return fail(BP5_ERR_INVALID, "switch: 0 or 1");
      if (value != mf->tune[knob] && mf->plans.count(-block_cpt(mf))) return fail(BP5_ERR_INVALID, "BP5_TUNE_LATTICE_INDICES: the block plan of this handle is already built");
      break;
    default:
      if (value != 0 && value != 1) return fail(BP5_ERR_INVALID, "switch: 0 or 1");
  }
  mf->tune[knob] = value;
  if (knob == BP5_TUNE_BOUNDARY_FIRST && mf->wait_value_ok >= 0) mf->can_wait_value = mf->wait_value_ok == 1 && value != 0;
  return BP5_OK;
}
extern "C" int bp5_mf_get_tuning(const bp5_mf *mf, int knob, int *value)
{
  if (!mf || !value || knob < 0 || knob >= BP5_TUNE_COUNT) return fail(BP5_ERR_INVALID, "unknown tuning knob");
  *value = mf->tune[knob];
  return BP5_OK;
}
extern "C" int bp5_mf_set_overlap(bp5_mf *mf, int mode)
{
  if (!mf || mode < 0 || mode > 2) return fail(BP5_ERR_INVALID, "bad argument");
  mf->overlap = mode;
  return BP5_OK;
}
// auto: the split into interior / boundary / interior launches and its four cross-stream dependencies cost 50-80 us per
// application on one GPU (profiles/r2 p_*), the exchange it hides is one DoF plane each way: worth it on large slabs only
static bool overlap_wanted(const bp5_mf *mf) { return mf->overlap == 1 || (mf->overlap == 2 && mf->n_interior >= 1000000u); }
// ghost gather: owners send their interface values (packed through send_indices), ghosts are
// received straight into the vector's ghost range (contiguous per neighbour)
static int gather_exchange(bp5_mf *mf, double *v, bool on_comm_stream);
// pack + exchange; the caller says which stream the exchange takes (the public call: the handle's overlap setting; the fused solves: their schedule)
static int gather_start(bp5_mf *mf, double *v, bool on_comm_stream)
{
  HIP_TRY(hipSetDevice(mf->device));
  BP5_TRY(halo_streams(mf));
  const uint32_t ns = mf->send_off.back();
  if (ns) {
    hipLaunchKernelGGL(pack_kernel, dim3((ns + 255) / 256), dim3(256), 0, mf->stream, mf->d_send_idx, ns, v, mf->d_sendbuf);
    KERNEL_CHECK();
  }
  return gather_exchange(mf, v, on_comm_stream);
}
extern "C" int bp5_halo_gather_start(bp5_mf *mf, double *v)
{
  if (!mf || !v) return fail(BP5_ERR_INVALID, "null argument");
  if (mf->neighbors.empty()) return BP5_OK;
  if (!mf->comm) return fail(BP5_ERR_INVALID, "halo exchange needs bp5_mf_set_comm");
  return gather_start(mf, v, overlap_wanted(mf));
}
// the RCCL part of the ghost gather: d_sendbuf is packed (on the compute stream); ghosts arrive in v's ghost range
static int gather_exchange(bp5_mf *mf, double *v, bool on_comm_stream)
{
  mf->overlap_now = on_comm_stream;
  hipStream_t cs = mf->overlap_now ? mf->comm_stream : mf->stream;
  if (mf->overlap_now) { // the exchange starts once the values are packed (and everything before them on the compute stream is done)
    HIP_TRY(hipEventRecord(mf->ev_halo[0], mf->stream));
    HIP_TRY(hipStreamWaitEvent(cs, mf->ev_halo[0], 0));
  }
  NCCL_TRY(ncclGroupStart());
  for (size_t k = 0; k < mf->neighbors.size(); ++k) {
    const uint32_t sc = mf->send_off[k + 1] - mf->send_off[k], rc = mf->recv_off[k + 1] - mf->recv_off[k];
    if (sc) NCCL_TRY(ncclSend(mf->d_sendbuf + mf->send_off[k], sc, ncclDouble, mf->neighbors[k], mf->comm->comm, cs));
    if (rc) NCCL_TRY(ncclRecv(v + mf->n_owned + mf->recv_off[k], rc, ncclDouble, mf->neighbors[k], mf->comm->comm, cs));
  }
  NCCL_TRY(ncclGroupEnd());
  if (mf->overlap_now) HIP_TRY(hipEventRecord(mf->ev_halo[1], cs));
  return BP5_OK;
}
extern "C" int bp5_halo_gather_finish(bp5_mf *mf, double *v)
{
  if (!mf || !v) return fail(BP5_ERR_INVALID, "null argument");
  if (mf->neighbors.empty()) return BP5_OK;
  if (!mf->comm || !mf->comm_stream) return fail(BP5_ERR_INVALID, "bp5_halo_gather_finish without bp5_halo_gather_start");
  if (mf->overlap_now) HIP_TRY(hipStreamWaitEvent(mf->stream, mf->ev_halo[1], 0)); // later compute work sees the ghosts
  return BP5_OK;
}
extern "C" int bp5_halo_gather(bp5_mf *mf, double *v)
{
  BP5_TRY(bp5_halo_gather_start(mf, v));
  return bp5_halo_gather_finish(mf, v);
}
// compress(add): ghost contributions travel back to the owners and are added; ghosts zeroed
static int scatter_exchange(bp5_mf *mf, double *v, bool on_comm_stream, bool ordered_by_caller = false)
{
  mf->overlap_now = on_comm_stream;
  hipStream_t cs = mf->overlap_now ? mf->comm_stream : mf->stream;
  if (mf->overlap_now && !ordered_by_caller) { // the ghost entries are complete at this point of the compute stream
    HIP_TRY(hipEventRecord(mf->ev_halo[2], mf->stream));
    HIP_TRY(hipStreamWaitEvent(cs, mf->ev_halo[2], 0));
  }
  NCCL_TRY(ncclGroupStart());
  for (size_t k = 0; k < mf->neighbors.size(); ++k) {
    const uint32_t sc = mf->send_off[k + 1] - mf->send_off[k], rc = mf->recv_off[k + 1] - mf->recv_off[k];
    if (rc) NCCL_TRY(ncclSend(v + mf->n_owned + mf->recv_off[k], rc, ncclDouble, mf->neighbors[k], mf->comm->comm, cs));
    if (sc) NCCL_TRY(ncclRecv(mf->d_recvbuf + mf->send_off[k], sc, ncclDouble, mf->neighbors[k], mf->comm->comm, cs));
  }
  NCCL_TRY(ncclGroupEnd());
  if (mf->overlap_now) HIP_TRY(hipEventRecord(mf->ev_halo[3], cs));
  return BP5_OK;
}
extern "C" int bp5_halo_scatter_add_start(bp5_mf *mf, double *v)
{
  if (!mf || !v) return fail(BP5_ERR_INVALID, "null argument");
  if (mf->neighbors.empty()) return BP5_OK;
  if (!mf->comm) return fail(BP5_ERR_INVALID, "halo exchange needs bp5_mf_set_comm");
  HIP_TRY(hipSetDevice(mf->device));
  BP5_TRY(halo_streams(mf));
  return scatter_exchange(mf, v, overlap_wanted(mf));
}
// fuse != NULL: the unpack kernels also correct the fused dot products and zero the ghost ranges of v and p
static int scatter_add_finish(bp5_mf *mf, double *v, FuseState *fuse)
{
  if (mf->overlap_now) HIP_TRY(hipStreamWaitEvent(mf->stream, mf->ev_halo[3], 0));
  for (size_t k = 0; k < mf->neighbors.size(); ++k) { // per neighbour: indices distinct -> race-free, fixed order
    const uint32_t sc = mf->send_off[k + 1] - mf->send_off[k];
    if (!sc) continue;
    if (fuse) { // fused CG dot products: correct the sums the write-out formed with the local part of these DoFs
      const uint32_t grid = std::min<uint32_t>((sc + 255) / 256, 1024u / (uint32_t)mf->neighbors.size());
      const uint32_t ng = fuse->ghosts_zeroed ? 0u : mf->n_ghost; // the first of these launches also zeroes both ghost ranges
      hipLaunchKernelGGL(unpack_add_dots_kernel, dim3(grid), dim3(256), 0, mf->stream, mf->d_send_idx + mf->send_off[k],
                         mf->d_send_dirichlet + mf->send_off[k], sc, mf->d_recvbuf + mf->send_off[k], v, fuse->r, mf->d_partials,
                         fuse->n_cols, mf->d_st, v + mf->n_owned, const_cast<double *>(fuse->p) + mf->n_owned, ng);
      fuse->n_cols += grid;
      fuse->ghosts_zeroed = true;
    } else
      hipLaunchKernelGGL(unpack_add_kernel, dim3((sc + 255) / 256), dim3(256), 0, mf->stream, mf->d_send_idx + mf->send_off[k], sc,
                         mf->d_recvbuf + mf->send_off[k], v);
    KERNEL_CHECK();
  }
  if (fuse && fuse->ghosts_zeroed) return BP5_OK;
  return bp5_halo_zero_ghosts(mf, v);
}
extern "C" int bp5_halo_scatter_add_finish(bp5_mf *mf, double *v)
{
  if (!mf || !v) return fail(BP5_ERR_INVALID, "null argument");
  if (mf->neighbors.empty()) return BP5_OK;
  if (!mf->comm || !mf->comm_stream) return fail(BP5_ERR_INVALID, "bp5_halo_scatter_add_finish without bp5_halo_scatter_add_start");
  return scatter_add_finish(mf, v, nullptr);
}
extern "C" int bp5_halo_scatter_add(bp5_mf *mf, double *v)
{
  BP5_TRY(bp5_halo_scatter_add_start(mf, v));
  return bp5_halo_scatter_add_finish(mf, v);
}
extern "C" int bp5_halo_zero_ghosts(bp5_mf *mf, double *v)
{
  if (!mf || !v) return fail(BP5_ERR_INVALID, "null argument");
  if (mf->n_ghost) HIP_TRY(hipMemsetAsync(v + mf->n_owned, 0, (size_t)mf->n_ghost * sizeof(double), mf->stream));
  return BP5_OK;
}

// The operator application in phases (MatrixFree::cell_loop with overlap_communication_computation, bp5/step-64.cu:241,274;
// SURVEY 3.2 / Appendix C3): ghost gather in flight under the first part of the interior cells, then the cells that touch
// ghosts, then the ghost contributions travel to their owners under the rest of the interior cells.  ONE kernel family is
// chosen for the whole application; the block kernel runs its brick ranges with owner stores + partial slab and a single
// combine pass at the end, so the result is bitwise the one of the unsplit launch.
struct ApplyPhases {
  bool block = false, set = false;
  bp5_mf::DevPlan *dp = nullptr;
};
// overwrite: what the whole application is asked for; call: filled in with what every range launch is asked for
static int phases_begin(bp5_mf *mf, double *dst, bool overwrite, ApplyCall &call, ApplyPhases &ph)
{
  const int ev = effective_variant(mf, 0, mf->n_cells);
  ph.block = is_default_block(mf, ev) || (mf->degree == 4 && (ev == 48 || ev == 49 || (ev >= 60 && ev <= 62))); // (p = 4, which has a block kernel -- block_lpc(4) != 0 as is_default_block asks --: and the A/B siblings that run brick ranges)
  call.overwrite = false;
  if (ph.block) {
    BP5_TRY(get_plan_raw(mf, -block_cpt(mf), &ph.dp));
    ph.set = overwrite && ph.dp->covers_all;
    call.overwrite = ph.set;
    if (overwrite && !ph.set) HIP_TRY(hipMemsetAsync(dst, 0, mf->n_local() * sizeof(double), mf->stream));
    call.combine_later = true;
    call.set_variant(ev); // every range takes the block kernel, however few bricks it holds (and the combine passes the form the variant implies)
    call.keep_variant = true;
  } else if (overwrite) { // atomic kernels accumulate: one zero-fill, then every range adds
    HIP_TRY(hipMemsetAsync(dst, 0, mf->n_local() * sizeof(double), mf->stream));
    // Known zero for EVERY range, not the first alone: the only launches that rely on it store the entries strictly inside a cell (interior stores
    // of the pencil kernel).  Such an entry belongs to one cell, every cell is in exactly one range, and neither the other ranges' atomics nor the
    // halo exchange (interface and ghost DoFs: on cell surfaces) ever touch it -- it still holds the zero of this fill when its one store arrives
    call.dst_known_zero = true;
  }
  return BP5_OK;
}
static int phases_range(bp5_mf *mf, ApplyCall &call, const double *coef, const double *src, double *dst, uint32_t c0, uint32_t c1)
{
  if (c1 <= c0) return BP5_OK;
  call.c0 = c0; call.c1 = c1;
  return launch_apply(mf, call, coef, src, dst);
}
static int phases_end(bp5_mf *mf, ApplyCall &call, double *dst, ApplyPhases &ph, int window = COMBINE_ALL)
{
  return ph.block ? launch_combine(mf, call, ph.dp, dst, ph.set, window) : BP5_OK;
}
// interior cells [0, split) run under the ghost gather, [split, n_interior) under the scatter-add; split on a brick boundary
static uint32_t interior_split(const bp5_mf *mf)
{
  const uint32_t half = mf->n_interior / 2;
  if (mf->h_block_off.empty()) return half;
  const auto it = std::lower_bound(mf->h_block_off.begin(), mf->h_block_off.end(), half);
  return it == mf->h_block_off.end() || *it > mf->n_interior ? mf->n_interior : *it;
}
// overwrite: of the whole application.  call: the caller's, for its profiling mark; range, overwrite mode and variant of the range launches are set here
static int apply_overlapped(bp5_mf *mf, ApplyCall &call, const double *coef, double *src, double *dst, bool overwrite)
{
  // block-kernel ranges must be unions of whole bricks: the generator emits interior and ghost-touching bricks separately;
  // a mesh whose n_interior_cells cuts through a brick runs unsplit (the exchange is then not overlapped)
  uint32_t b0, b1;
  const bool aligned = mf->h_block_off.empty() || mf->n_interior == 0 || mf->n_interior == mf->n_cells ||
                       block_aligned(mf, 0, mf->n_interior, &b0, &b1);
  ApplyPhases ph;
  BP5_TRY(bp5_halo_gather_start(mf, src));
  BP5_TRY(phases_begin(mf, dst, overwrite, call, ph));
  if (!aligned || !overlap_wanted(mf)) {
    BP5_TRY(bp5_halo_gather_finish(mf, src));
    BP5_TRY(phases_range(mf, call, coef, src, dst, 0, mf->n_cells));
    BP5_TRY(phases_end(mf, call, dst, ph));
    return bp5_halo_scatter_add(mf, dst);
  }
  const uint32_t split = interior_split(mf);
  BP5_TRY(phases_range(mf, call, coef, src, dst, 0, split));                      // under the gather
  BP5_TRY(bp5_halo_gather_finish(mf, src));
  BP5_TRY(phases_range(mf, call, coef, src, dst, mf->n_interior, mf->n_cells));   // cells that touch ghosts
  // The atomic kernels have completed the ghost entries of dst once the ghost-touching cells are done; the block kernel needs the
  // ghost ROWS of its combine pass on top (ghost DoFs on brick faces go through the partial slab): one small launch over the ghost
  // window.  Either way the ghost contributions travel to their owners under the second part of the interior cells, and the block
  // kernel's owned rows are combined after the last range -- every row once, in the order of the unsplit pass.
  const bool ghost_rows = ph.block && ph.dp->n_shared && mf->n_ghost;                  // ghost rows (may) pass through the partial slab
  if (ghost_rows && !(ph.dp->cr_tile && !call.csr_combine)) { // (per-DoF CSR combine pass: no windows -- the ghost rows are final after the last range only)
    BP5_TRY(phases_range(mf, call, coef, src, dst, split, mf->n_interior));
    BP5_TRY(phases_end(mf, call, dst, ph));
    return bp5_halo_scatter_add(mf, dst);
  }
  if (ghost_rows) BP5_TRY(launch_combine(mf, call, ph.dp, dst, ph.set, COMBINE_GHOST));
  BP5_TRY(bp5_halo_scatter_add_start(mf, dst));
  BP5_TRY(phases_range(mf, call, coef, src, dst, split, mf->n_interior));
  BP5_TRY(phases_end(mf, call, dst, ph, ghost_rows ? COMBINE_OWNED : COMBINE_ALL));
  return bp5_halo_scatter_add_finish(mf, dst);
}
extern "C" int bp5_apply_distributed(bp5_mf *mf, const double *coef, double *src, double *dst, int zero_dst)
{
  if (!mf || (!coef && mf->geometry_mode == BP5_GEOM_MERGED6) || !src || !dst) return fail(BP5_ERR_INVALID, "null argument");
  if (src == dst) return fail(BP5_ERR_INVALID, "src and dst must differ");
  HIP_TRY(hipSetDevice(mf->device));
  if (mf->has_neighbors()) {
    ApplyCall call;
    BP5_TRY(apply_overlapped(mf, call, coef, src, dst, zero_dst != 0));
  } else BP5_TRY(launch_apply(mf, coef, src, dst, 0, mf->n_cells, zero_dst != 0));
  BP5_TRY(bp5_halo_zero_ghosts(mf, src));
  return bp5_copy_constrained(mf, src, dst);
}

// ------------------------------------------------------------------------------------ halo exchange of block vectors
// The ghost ranges of a block vector are n_components strided pieces: they can neither be received in place nor sent from one buffer, and an
// exchange per component would multiply the RCCL groups (the expensive part: profiles/r4 z_*).  So every exchange goes through staging buffers
// in which a neighbour's message is contiguous and holds all components (bp5_kernels.hpp: halo_message_pos): ONE send and ONE receive per
// neighbour and direction, launches and RCCL calls independent of n_components.  Streams, events and the one-in-flight rule are the scalar path's.
struct HaloStaging { double *gather_send, *gather_recv, *scatter_send, *scatter_recv; const uint32_t *send_off, *recv_off; };
static int halo_components_staging(bp5_mf *mf, int n_components, HaloStaging &st)
{
  const size_t ns = mf->send_off.back(), ng = mf->n_ghost, nb = mf->neighbors.size();
  const size_t need = 2 * (size_t)n_components * (ns + ng);
  if (!mf->d_hc_off) {
    std::vector<uint32_t> off(mf->send_off);
    off.insert(off.end(), mf->recv_off.begin(), mf->recv_off.end());
    BP5_TRY(upload(&mf->d_hc_off, off.data(), off.size()));
  }
  if (mf->hc_cap < need) {
    if (mf->hc_base) { // (send and receive staging are distinct: a rank may be its own neighbour)
      HIP_TRY(hipStreamSynchronize(mf->stream));
      if (mf->comm_stream) HIP_TRY(hipStreamSynchronize(mf->comm_stream));
      HIP_TRY(hipFree(mf->hc_base));
      mf->hc_base = nullptr; mf->hc_cap = 0;
    }
    HIP_TRY(hipMalloc((void **)&mf->hc_base, std::max<size_t>(need, 1) * sizeof(double)));
    mf->hc_cap = need;
  }
  st.gather_send = mf->hc_base;
  st.gather_recv = st.gather_send + (size_t)n_components * ns;
  st.scatter_send = st.gather_recv + (size_t)n_components * ng;
  st.scatter_recv = st.scatter_send + (size_t)n_components * ng;
  st.send_off = mf->d_hc_off;
  st.recv_off = mf->d_hc_off + nb + 1;
  return BP5_OK;
}
// the RCCL group of one exchange: `out` travels to the neighbours in pieces out_off, `in` arrives in pieces in_off (offsets of ONE component)
static int halo_components_group(bp5_mf *mf, int n_components, const double *out, const std::vector<uint32_t> &out_off, double *in,
                                 const std::vector<uint32_t> &in_off, hipStream_t cs)
{
  const size_t nc = (size_t)n_components;
  NCCL_TRY(ncclGroupStart());
  for (size_t k = 0; k < mf->neighbors.size(); ++k) {
    const size_t oc = out_off[k + 1] - out_off[k], ic = in_off[k + 1] - in_off[k];
    if (oc) NCCL_TRY(ncclSend(out + nc * out_off[k], nc * oc, ncclDouble, mf->neighbors[k], mf->comm->comm, cs));
    if (ic) NCCL_TRY(ncclRecv(in + nc * in_off[k], nc * ic, ncclDouble, mf->neighbors[k], mf->comm->comm, cs));
  }
  NCCL_TRY(ncclGroupEnd());
  return BP5_OK;
}
static inline dim3 halo_components_grid(uint32_t n, int n_components) { return dim3((n + 255) / 256, n_components); }
// update_ghost_values_start: pack on the compute stream, the group on the communication stream (on_comm_stream) or behind the pack
static int gather_components_start(bp5_mf *mf, int n_components, size_t ld, double *v, bool on_comm_stream)
{
  BP5_TRY(halo_streams(mf));
  HaloStaging st;
  BP5_TRY(halo_components_staging(mf, n_components, st));
  const uint32_t ns = mf->send_off.back(), nb = (uint32_t)mf->neighbors.size();
  if (ns) {
    hipLaunchKernelGGL(pack_components_kernel, halo_components_grid(ns, n_components), dim3(256), 0, mf->stream, mf->d_send_idx, st.send_off, nb, ns, v, ld,
                       st.gather_send);
    KERNEL_CHECK();
  }
  mf->overlap_now = on_comm_stream;
  hipStream_t cs = on_comm_stream ? mf->comm_stream : mf->stream;
  if (on_comm_stream) {
    HIP_TRY(hipEventRecord(mf->ev_halo[0], mf->stream));
    HIP_TRY(hipStreamWaitEvent(cs, mf->ev_halo[0], 0));
  }
  BP5_TRY(halo_components_group(mf, n_components, st.gather_send, mf->send_off, st.gather_recv, mf->recv_off, cs));
  if (on_comm_stream) HIP_TRY(hipEventRecord(mf->ev_halo[1], cs));
  return BP5_OK;
}
// update_ghost_values_finish: the compute stream waits for the transfer and unpacks the messages into the ghost ranges
static int gather_components_finish(bp5_mf *mf, int n_components, size_t ld, double *v)
{
  if (mf->overlap_now) HIP_TRY(hipStreamWaitEvent(mf->stream, mf->ev_halo[1], 0));
  if (!mf->n_ghost) return BP5_OK;
  HaloStaging st;
  BP5_TRY(halo_components_staging(mf, n_components, st));
  hipLaunchKernelGGL(unpack_ghosts_components_kernel, halo_components_grid(mf->n_ghost, n_components), dim3(256), 0, mf->stream, st.recv_off,
                     (uint32_t)mf->neighbors.size(), mf->n_ghost, st.gather_recv, v + mf->n_owned, ld);
  KERNEL_CHECK();
  return BP5_OK;
}
// compress_start(add): the ghost ranges are packed (and zeroed: nothing reads them before the exchange is finished) on the compute stream
static int scatter_components_start(bp5_mf *mf, int n_components, size_t ld, double *v, bool on_comm_stream)
{
  BP5_TRY(halo_streams(mf));
  HaloStaging st;
  BP5_TRY(halo_components_staging(mf, n_components, st));
  if (mf->n_ghost) {
    hipLaunchKernelGGL(pack_ghosts_components_kernel, halo_components_grid(mf->n_ghost, n_components), dim3(256), 0, mf->stream, st.recv_off,
                       (uint32_t)mf->neighbors.size(), mf->n_ghost, v + mf->n_owned, ld, st.scatter_send);
    KERNEL_CHECK();
  }
  mf->overlap_now = on_comm_stream;
  hipStream_t cs = on_comm_stream ? mf->comm_stream : mf->stream;
  if (on_comm_stream) {
    HIP_TRY(hipEventRecord(mf->ev_halo[2], mf->stream));
    HIP_TRY(hipStreamWaitEvent(cs, mf->ev_halo[2], 0));
  }
  BP5_TRY(halo_components_group(mf, n_components, st.scatter_send, mf->recv_off, st.scatter_recv, mf->send_off, cs));
  if (on_comm_stream) HIP_TRY(hipEventRecord(mf->ev_halo[3], cs));
  return BP5_OK;
}
// compress_finish(add): neighbour after neighbour on the compute stream (indices of one neighbour are distinct; the fixed order makes the
// exchange bitwise reproducible)
static int scatter_components_finish(bp5_mf *mf, int n_components, size_t ld, double *v)
{
  if (mf->overlap_now) HIP_TRY(hipStreamWaitEvent(mf->stream, mf->ev_halo[3], 0));
  HaloStaging st;
  BP5_TRY(halo_components_staging(mf, n_components, st));
  for (size_t k = 0; k < mf->neighbors.size(); ++k) {
    const uint32_t sc = mf->send_off[k + 1] - mf->send_off[k];
    if (!sc) continue;
    hipLaunchKernelGGL(unpack_add_components_kernel, halo_components_grid(sc, n_components), dim3(256), 0, mf->stream, mf->d_send_idx + mf->send_off[k], sc,
                       st.scatter_recv + (size_t)n_components * mf->send_off[k], v, ld);
    KERNEL_CHECK();
  }
  return BP5_OK;
}
static int zero_ghosts_components(bp5_mf *mf, int n_components, size_t ld, double *v)
{
  if (!mf->n_ghost) return BP5_OK;
  hipLaunchKernelGGL(zero_ghosts_components_kernel, halo_components_grid(mf->n_ghost, n_components), dim3(256), 0, mf->stream, v + mf->n_owned, mf->n_ghost, ld);
  KERNEL_CHECK();
  return BP5_OK;
}
// what the three public exchanges check: the layout of one block vector, then the handle
static int halo_components_check(const bp5_mf *mf, int n_components, size_t ld, const double *v)
{
  BP5_TRY(components_layout_check(n_components, ld, v, v));
  if (!mf) return fail(BP5_ERR_INVALID, "null handle");
  if (ld < mf->n_local()) return fail(BP5_ERR_INVALID, "block vectors: ld < n_owned + n_ghost");
  if (!mf->neighbors.empty() && !mf->comm) return fail(BP5_ERR_INVALID, "halo exchange needs bp5_mf_set_comm");
  return BP5_OK;
}
extern "C" int bp5_halo_gather_components(bp5_mf *mf, int n_components, size_t ld, double *v)
{
  BP5_TRY(halo_components_check(mf, n_components, ld, v));
  if (mf->neighbors.empty()) return BP5_OK;
  HIP_TRY(hipSetDevice(mf->device));
  BP5_TRY(gather_components_start(mf, n_components, ld, v, overlap_wanted(mf)));
  return gather_components_finish(mf, n_components, ld, v);
}
extern "C" int bp5_halo_scatter_add_components(bp5_mf *mf, int n_components, size_t ld, double *v)
{
  BP5_TRY(halo_components_check(mf, n_components, ld, v));
  HIP_TRY(hipSetDevice(mf->device));
  if (mf->neighbors.empty()) return zero_ghosts_components(mf, n_components, ld, v); // (as the scalar call: ghosts zeroed either way)
  BP5_TRY(scatter_components_start(mf, n_components, ld, v, overlap_wanted(mf)));
  return scatter_components_finish(mf, n_components, ld, v);
}
extern "C" int bp5_halo_zero_ghosts_components(bp5_mf *mf, int n_components, size_t ld, double *v)
{
  BP5_TRY(components_layout_check(n_components, ld, v, v));
  if (!mf) return fail(BP5_ERR_INVALID, "null handle");
  if (ld < mf->n_local()) return fail(BP5_ERR_INVALID, "block vectors: ld < n_owned + n_ghost");
  HIP_TRY(hipSetDevice(mf->device));
  return zero_ghosts_components(mf, n_components, ld, v);
}

// dst_c += A src_c with the exchange (dst zeroed first where asked), on a handle with a communicator and neighbours: the schedules of
// apply_overlapped for an atomic kernel.  Unsplit (overlap off, or auto below the threshold of overlap_wanted): gather, all cells, scatter-add
// on the handle's stream.  Three-phase: gather in flight under the cells [0, split), the ghost-touching cells, the ghost contributions on their
// way under the cells [split, n_interior).  Ghosts of src are zeroed again; the Dirichlet copy is the caller's next launch.
static int components_apply_exchanged(bp5_mf *mf, const double *coef, int n_components, size_t ld, double *src, double *dst, bool zero)
{
  const bool split = overlap_wanted(mf);
  BP5_TRY(gather_components_start(mf, n_components, ld, src, split));
  if (zero) BP5_TRY(components_zero(mf, n_components, ld, dst));
  if (!split) {
    BP5_TRY(gather_components_finish(mf, n_components, ld, src));
    BP5_TRY(components_apply_cells(mf, coef, n_components, ld, src, dst, 0, mf->n_cells));
    BP5_TRY(scatter_components_start(mf, n_components, ld, dst, false));
  } else {
    const uint32_t half = interior_split(mf);
    BP5_TRY(components_apply_cells(mf, coef, n_components, ld, src, dst, 0, half));                       // under the gather
    BP5_TRY(gather_components_finish(mf, n_components, ld, src));
    BP5_TRY(components_apply_cells(mf, coef, n_components, ld, src, dst, mf->n_interior, mf->n_cells));   // cells that touch ghosts
    BP5_TRY(scatter_components_start(mf, n_components, ld, dst, true));
    BP5_TRY(components_apply_cells(mf, coef, n_components, ld, src, dst, half, mf->n_interior));          // under the scatter-add
  }
  BP5_TRY(scatter_components_finish(mf, n_components, ld, dst));
  return zero_ghosts_components(mf, n_components, ld, src);
}
extern "C" int bp5_apply_components_distributed(bp5_mf *mf, const double *coef, int n_components, size_t ld, double *src, double *dst, int zero_dst)
{
  BP5_TRY(components_check(mf, coef, n_components, ld, src, dst, true));
  HIP_TRY(hipSetDevice(mf->device));
  if (mf->has_neighbors()) BP5_TRY(components_apply_exchanged(mf, coef, n_components, ld, src, dst, zero_dst != 0));
  else BP5_TRY(components_apply(mf, coef, n_components, ld, src, dst, zero_dst != 0));
  return components_copy_constrained(mf, n_components, ld, src, dst);
}

// ------------------------------------------------------------------------------------ events
extern "C" int bp5_event_create(bp5_event **out)
{
  if (!out) return fail(BP5_ERR_INVALID, "null argument");
  bp5_event *e = new bp5_event;
  hipError_t r = hipEventCreate(&e->ev);
  if (r != hipSuccess) { delete e; return fail(BP5_ERR_HIP, hipGetErrorString(r)); }
  *out = e;
  return BP5_OK;
}
extern "C" int bp5_event_record(bp5_mf *mf, bp5_event *ev)
{
  if (!mf || !ev) return fail(BP5_ERR_INVALID, "null argument");
  HIP_TRY(hipEventRecord(ev->ev, mf->stream));
  return BP5_OK;
}
extern "C" int bp5_event_elapsed_ms(bp5_event *a, bp5_event *b, double *ms)
{
  if (!a || !b || !ms) return fail(BP5_ERR_INVALID, "null argument");
  HIP_TRY(hipEventSynchronize(b->ev));
  float f = 0.f;
  HIP_TRY(hipEventElapsedTime(&f, a->ev, b->ev));
  *ms = f;
  return BP5_OK;
}
extern "C" int bp5_event_destroy(bp5_event *e)
{
  if (!e) return BP5_OK;
  hipEventDestroy(e->ev);
  delete e;
  return BP5_OK;
}

// ------------------------------------------------------------------------------------ CG
static int ensure_ws(bp5_mf *mf)
{
  if (mf->ws_g) return BP5_OK;
  // one allocation for the three work vectors (staggering their bases by 256 B ... 1 MiB was measured
  // to make no difference to the BLAS-1 kernels: profiles/r1/README.md)
  const size_t stagger = 0;
  const size_t nb = (std::max<size_t>(mf->n_local(), 2) * sizeof(double) + 4095) / 4096 * 4096;
  char *base = nullptr;
  HIP_TRY(hipMalloc((void **)&base, 3 * nb + 2 * stagger + 4096));
  HIP_TRY(hipMemsetAsync(base, 0, 3 * nb + 2 * stagger + 4096, mf->stream)); // ordered with the solver kernels that follow on this stream
  mf->ws_base = base;
  mf->ws_g = (double *)base;
  mf->ws_d = (double *)(base + nb + stagger);
  mf->ws_h = (double *)(base + 2 * nb + 2 * stagger);
  return BP5_OK;
}

// four events per profiled application: [0] before the zero-fill, [1] before the cell kernel, [2] after the cell kernel
// (before the combine pass of the owner-scatter kernels), [3] after everything launch_apply enqueued
struct ApplyProfile {
  bp5_mf *mf;
  bool on;
  int used = 0;
  static constexpr int MAX_PROFILED = 512; // applications bracketed per solve; later ones run unbracketed (bounded pool)
  int mark(int k)
  {
    if (!on) return BP5_OK;
    if (used >= 4 * MAX_PROFILED) { on = false; return BP5_OK; }
    while ((size_t)used + 4 > mf->ev_pool.size()) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); mf->ev_pool.push_back(e); }
    HIP_TRY(hipEventRecord(mf->ev_pool[used + k], mf->stream));
    return BP5_OK;
  }
};

// What one solve decided once and every operator application inside it follows; it lives on the solver's stack
struct SolveState {
  ApplyProfile prof;
  // fused dot products across ranks: where the exchange is enqueued (ApplyCall::exchange) and whether whole-range launches walk the
  // ghost-touching bricks first (ApplyCall::two_parts)
  int exchange = EXCHANGE_NONE;
  bool two_parts = false;
  bool gather_in_flight = false; // the solver started the ghost gather of p under its update kernel
  // one rank, separate dot-product kernel: dst arrives zeroed (the update kernel stored the zeros) / the Dirichlet copy follows in the dots kernel
  bool dst_prezeroed = false, copies_dirichlet = false;
  // merged solve with the vector update of the brick interiors inside the block kernel (OperatorPlan::fused_update): what the next operator
  // application is to apply (FuseState::upd_*; 0: nothing -- the first iteration)
  int upd_mode = 0;
  double *upd_x = nullptr;
  const double *upd_diag = nullptr;
  // profile == 2: stamps of the iteration `phase_it` (0-based; stamps beyond MAX_ITERS are dropped); bit k of phase_recorded[it]: mark k recorded
  bool phase_on = false;
  int phase_it = 0;
  uint8_t phase_recorded[bp5_mf::PhaseProfile::MAX_ITERS] = {};
};

// profile == 2: stamp k of the iteration being profiled (bp5_cg_result.phase_ms)
static int phase_mark(bp5_mf *mf, SolveState &ss, int k)
{
  if (!ss.phase_on || ss.phase_it >= bp5_mf::PhaseProfile::MAX_ITERS) return BP5_OK;
  HIP_TRY(hipEventRecord(mf->phase.ev[(size_t)ss.phase_it * bp5_mf::PhaseProfile::MARKS + k], mf->stream));
  ss.phase_recorded[ss.phase_it] |= (uint8_t)(1u << k);
  return BP5_OK;
}

// The three exchange schedules of an operator application with fused dot products across ranks (fused_vmult_distributed).  All of them
// run the same kernels with the same per-brick sums and the same combine order: v is bitwise the same (the dot products are summed over a
// different column layout).
// Unsplit (bp5_mf_set_overlap 0): one launch with its combine pass, then the exchange on the compute stream.
static int fused_unsplit(bp5_mf *mf, SolveState &ss, ApplyCall &call, const double *coef, const double *src, double *dst)
{
  ApplyProfile &prof = ss.prof;
  if (prof.on) call.mark_event = mf->ev_pool[prof.used + 2];
  BP5_TRY(launch_apply(mf, call, coef, src, dst));
  if (!call.mark_recorded) BP5_TRY(prof.mark(2));
  BP5_TRY(prof.mark(3));
  if (prof.on) prof.used += 4;
  BP5_TRY(phase_mark(mf, ss, 3));
  BP5_TRY(halo_streams(mf));
  BP5_TRY(scatter_exchange(mf, dst, false));
  return scatter_add_finish(mf, dst, call.fuse); // (dot-product corrections + ghost zeroing inside)
}
// Ghost-rows-first (the automatic choice): all bricks in one launch; then the GHOST rows of the combine pass (a small launch), the exchange on
// the communication stream, and the owned rows combined underneath it: nothing runs beside the bandwidth-bound brick kernel (a co-running
// RCCL kernel crawls there -- 300 us for one DoF plane -- and slows it: profiles/r3), the exchange hides behind the owned-row combine
static int fused_ghost_rows_first(bp5_mf *mf, SolveState &ss, ApplyCall &call, const double *coef, const double *src, double *dst)
{
  ApplyProfile &prof = ss.prof;
  bp5_mf::DevPlan *dp = nullptr;
  BP5_TRY(get_plan_raw(mf, -block_cpt(mf), &dp));
  BP5_TRY(halo_streams(mf));
  call.combine_later = true;
  BP5_TRY(launch_apply(mf, call, coef, src, dst));
  BP5_TRY(prof.mark(2));
  // BP5_TUNE_COMBINE_SIGNAL (A/B knob of the handle): the two combine launches as ONE -- its first workgroups
  // complete the ghost rows and count themselves in, the communication stream waits for the count (stream wait-value) and starts the
  // exchange while the same launch walks the owned rows; same tiles and columns as the two launches: same bits.  One launch, one gap and
  // one cross-stream event less -- and on ONE GPU 16 us per iteration SLOWER than the two launches (0.547 against 0.531 ms on the slab of
  // rank 3 of 8, profiles/r3 z_*: the RCCL kernel then runs beside the bandwidth-bound combine pass from its first microsecond and both
  // crawl), hence not the default; whether a longer xGMI transfer pays for the earlier start is for a multi-GPU run to say
  const bool combine_signal = mf->tune[BP5_TUNE_COMBINE_SIGNAL] != 0;
  const bool one_combine = combine_signal && mf->can_wait_value == 1 && mf->n_ghost && mf->d_signal && dp->n_shared > dp->n_shared_owned && dp->cr_tile && !call.csr_combine; // (ghost rows among the shared ones: at least one workgroup signals)
  if (one_combine) {
    BP5_TRY(launch_combine(mf, call, dp, dst, true, COMBINE_GHOST_THEN_OWNED));
    HIP_TRY(hipStreamWaitValue64(mf->comm_stream, mf->d_signal, mf->signal_target, hipStreamWaitValueGte, ~0ull));
    BP5_TRY(scatter_exchange(mf, dst, true, true));
  } else if (mf->tune[BP5_TUNE_GHOST_COMBINE_ON_COMM] && mf->n_ghost) {
    // the ghost rows of the combine pass on the COMMUNICATION stream (behind an event that says the brick kernel is done, in front of the send): the
    // owned rows start right behind the brick kernel on the compute stream -- one small launch and its gap off the critical path (same kernels, same bits)
    HIP_TRY(hipEventRecord(mf->ev_halo[2], mf->stream));
    HIP_TRY(hipStreamWaitEvent(mf->comm_stream, mf->ev_halo[2], 0));
    BP5_TRY(launch_combine(mf, call, dp, dst, true, COMBINE_GHOST, true));
    BP5_TRY(scatter_exchange(mf, dst, true, true));
    BP5_TRY(launch_combine(mf, call, dp, dst, true, COMBINE_OWNED));
  } else {
    if (mf->n_ghost) BP5_TRY(launch_combine(mf, call, dp, dst, true, COMBINE_GHOST));
    BP5_TRY(scatter_exchange(mf, dst, true));
    BP5_TRY(launch_combine(mf, call, dp, dst, true, mf->n_ghost ? COMBINE_OWNED : COMBINE_ALL));
  }
  BP5_TRY(prof.mark(3));
  if (prof.on) prof.used += 4;
  BP5_TRY(phase_mark(mf, ss, 3));
  return scatter_add_finish(mf, dst, call.fuse);
}
// Boundary-first (bp5_mf_set_overlap 1, the twin of overlap_communication_computation, bp5/step-64.cu:241,274): the bricks that touch ghost
// DoFs run FIRST, one small combine pass completes the ghost rows, the exchange starts on the communication stream and the interior bricks
// run underneath it; the owned rows are combined after the last brick.
static int fused_boundary_first(bp5_mf *mf, SolveState &ss, ApplyCall &call, const double *coef, const double *src, double *dst)
{
  ApplyProfile &prof = ss.prof;
  bp5_mf::DevPlan *dp = nullptr;
  BP5_TRY(get_plan_raw(mf, -block_cpt(mf), &dp));
  BP5_TRY(halo_streams(mf));
  call.set_variant(56);      // every range takes the block kernel, however few bricks it holds
  call.keep_variant = true;
  call.combine_later = true; // one combine pass per window, launched here
  const bool has_boundary = mf->n_interior < mf->n_cells, in_one_launch = mf->can_wait_value == 1 && has_boundary && mf->n_interior > 0 && ss.two_parts;
  if (in_one_launch) {
    // ONE launch: every workgroup walks its share of the ghost-touching bricks first and counts itself in; the communication
    // stream waits for the count, combines the ghost rows and sends them while the same launch works through the interior bricks
    call.signal = true;
    BP5_TRY(launch_apply(mf, call, coef, src, dst));
    HIP_TRY(hipStreamWaitValue64(mf->comm_stream, mf->d_signal, mf->signal_target, hipStreamWaitValueGte, ~0ull));
    if (mf->n_ghost) BP5_TRY(launch_combine(mf, call, dp, dst, true, COMBINE_GHOST, true)); // on the communication stream, between the wait and the send
    BP5_TRY(scatter_exchange(mf, dst, true, true));
  } else if (has_boundary) {
    call.two_parts = false; // (range launches)
    call.c0 = mf->n_interior; call.c1 = mf->n_cells; // bricks that touch ghosts
    BP5_TRY(launch_apply(mf, call, coef, src, dst));
    if (mf->n_ghost) BP5_TRY(launch_combine(mf, call, dp, dst, true, COMBINE_GHOST));
    BP5_TRY(scatter_exchange(mf, dst, true)); // send the ghost rows / post the receives: under the interior bricks
    call.c0 = 0; call.c1 = mf->n_interior;
    if (mf->n_interior) BP5_TRY(launch_apply(mf, call, coef, src, dst));
  } else { // (a rank without ghost-touching cells only receives: post the receives, then all bricks)
    BP5_TRY(scatter_exchange(mf, dst, true));
    BP5_TRY(launch_apply(mf, call, coef, src, dst));
  }
  BP5_TRY(prof.mark(2)); // (the profile brackets the brick launch(es))
  BP5_TRY(launch_combine(mf, call, dp, dst, true, mf->n_ghost ? COMBINE_OWNED : COMBINE_ALL));
  BP5_TRY(prof.mark(3));
  if (prof.on) prof.used += 4;
  BP5_TRY(phase_mark(mf, ss, 3));
  return scatter_add_finish(mf, dst, call.fuse);
}
// Fused dot products across ranks: gather, fused launch(es) over all cells (p.v is a sum over cells, so it needs no owner
// bookkeeping; v.v, r.v, r.r run over owned DoFs), then the ghost contributions travel to their owners, whose unpack kernel
// corrects v.v and r.v for what it adds.  The fused exchanges choose their streams themselves, whatever the handle's overlap setting.
static int fused_vmult_distributed(bp5_mf *mf, SolveState &ss, const double *coef, double *src, double *dst, const double *fuse_r, uint32_t *n_cols)
{
  if (ss.gather_in_flight) { ss.gather_in_flight = false; BP5_TRY(bp5_halo_gather_finish(mf, src)); } // started under the update kernel
  else {
    BP5_TRY(gather_start(mf, src, false));
    BP5_TRY(bp5_halo_gather_finish(mf, src));
  }
  BP5_TRY(phase_mark(mf, ss, 2));
  BP5_TRY(ss.prof.mark(0));
  BP5_TRY(ss.prof.mark(1));
  FuseState fuse;
  fuse.p = src; fuse.r = fuse_r;
  ApplyCall call;
  call.c0 = 0; call.c1 = mf->n_cells; call.overwrite = true;
  call.fuse = &fuse;
  call.exchange = ss.exchange;
  call.two_parts = ss.two_parts;
  if (ss.exchange == EXCHANGE_BOUNDARY_FIRST) BP5_TRY(fused_boundary_first(mf, ss, call, coef, src, dst));
  else if (ss.exchange == EXCHANGE_GHOST_ROWS_FIRST) BP5_TRY(fused_ghost_rows_first(mf, ss, call, coef, src, dst));
  else BP5_TRY(fused_unsplit(mf, ss, call, coef, src, dst));
  *n_cols = fuse.n_cols;
  if (!fuse.ghosts_zeroed) BP5_TRY(bp5_halo_zero_ghosts(mf, src)); // (a rank that owns no interface DoFs launched no unpack kernel; dst: scatter_add_finish)
  // no Dirichlet copy: the write-out stored v = p on this rank's Dirichlet rows and the unpack kernel leaves them alone
  return BP5_OK;
}

// A.vmult(h, d) inside the solvers: dst already zero on entry when zeroed == true
// n_cols != nullptr (CG on the packed block kernel, one rank's worth of cells): the operator's write-out and
// combine pass also form the v-dependent dot products of update_b (bp5/solver.h:142-311) and apply the Dirichlet copy; the
// partial sums land in d_partials, *n_cols columns of them.  fuse_r: the residual vector of the merged solver (D == 1), or NULL when
// only p.v is wanted (standard CG: rows 2-6 of the sums are then meaningless and r is never read)
static int solver_vmult(bp5_mf *mf, SolveState &ss, const double *coef, double *src, double *dst, bool zero, const double *fuse_r = nullptr,
                        uint32_t *n_cols = nullptr)
{
  ApplyProfile &prof = ss.prof;
  const bool dist = mf->has_neighbors(); // halo exchange: whenever there are neighbours (tests: a self neighbour)
  const bool fusing = n_cols != nullptr;
  if (dist && fusing) return fused_vmult_distributed(mf, ss, coef, src, dst, fuse_r, n_cols);
  ApplyCall call;
  call.c0 = 0; call.c1 = mf->n_cells;
  if (dist) { // phased application: the exchange overlaps the interior cells (apply_overlapped)
    BP5_TRY(prof.mark(0));
    BP5_TRY(prof.mark(1));
    if (prof.on) call.mark_event = mf->ev_pool[prof.used + 2];
    BP5_TRY(apply_overlapped(mf, call, coef, src, dst, zero));
    if (!call.mark_recorded) BP5_TRY(prof.mark(2));
    BP5_TRY(prof.mark(3));
    if (prof.on) prof.used += 4;
    BP5_TRY(bp5_halo_zero_ghosts(mf, src));
    return bp5_copy_constrained(mf, src, dst);
  }
  // kernels that accumulate with atomics need a zeroed target (owner-scatter kernels define every entry themselves)
  const bool owner_scatter = variant_overwrites(mf, effective_variant(mf, 0, mf->n_cells));
  BP5_TRY(prof.mark(0));
  if (zero && !owner_scatter) {
    if (!ss.dst_prezeroed) HIP_TRY(hipMemsetAsync(dst, 0, mf->n_local() * sizeof(double), mf->stream)); // (else: the update kernel stored the zeros)
    zero = false;
    call.dst_known_zero = true;
  }
  BP5_TRY(prof.mark(1));
  if (prof.on) call.mark_event = mf->ev_pool[prof.used + 2];
  FuseState fuse;
  if (fusing) { fuse.p = src; fuse.r = fuse_r; fuse.upd_mode = ss.upd_mode; fuse.upd_x = ss.upd_x; fuse.upd_diag = ss.upd_diag; call.fuse = &fuse; }
  call.overwrite = zero;
  BP5_TRY(launch_apply(mf, call, coef, src, dst));
  if (fusing) *n_cols = fuse.n_cols;
  if (!call.mark_recorded) BP5_TRY(prof.mark(2));
  BP5_TRY(prof.mark(3));
  if (prof.on) prof.used += 4;
  if (fusing) return BP5_OK; // Dirichlet DoFs were written by the fused write-out
  if (ss.copies_dirichlet) return BP5_OK; // ... or will be by the solver's dot-product kernel, which reads src and dst anyway
  return bp5_copy_constrained(mf, src, dst);
}

static int poll_state(bp5_mf *mf)
{
  HIP_TRY(hipMemcpyAsync(mf->h_st, mf->d_st, ST_COUNT * sizeof(int), hipMemcpyDeviceToHost, mf->stream));
  HIP_TRY(hipMemcpyAsync(mf->h_sc, mf->d_sc, SC_COUNT * sizeof(double), hipMemcpyDeviceToHost, mf->stream));
  HIP_TRY(hipStreamSynchronize(mf->stream));
  return BP5_OK;
}

// ---- what every solver shares: begin and finish (the refusals stay with the entry points: their order is part of each one's contract)
// tolerance + iteration cap to the device, the bracketing events of a profiled solve, the start event
static int solve_begin(bp5_mf *mf, const bp5_cg_params *prm, const ApplyProfile &prof)
{
  hipStream_t s = mf->stream;
  if (prof.on) { // create the bracketing events before the timed region starts
    const size_t want = 4 * (size_t)std::min(prm->max_iter, ApplyProfile::MAX_PROFILED);
    while (mf->ev_pool.size() < want) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); mf->ev_pool.push_back(e); }
  }
  mf->h_sc[SC_TOL] = prm->abs_tol;
  HIP_TRY(hipMemcpyAsync(mf->d_sc + SC_TOL, mf->h_sc + SC_TOL, sizeof(double), hipMemcpyHostToDevice, s));
  mf->h_st[ST_MAXIT] = prm->max_iter;
  HIP_TRY(hipMemcpyAsync(mf->d_st + ST_MAXIT, mf->h_st + ST_MAXIT, sizeof(int), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s)); // pinned staging words are reused below
  HIP_TRY(hipEventRecord(mf->ev_solve[0], s));
  return BP5_OK;
}
// end event, the device's state to the host, the result (phase_ms: zero, the merged solver fills it in); returns the breakdown status
static int solve_finish(bp5_mf *mf, const ApplyProfile &prof, bool fused_dots, int exchange_schedule, bool own_operator, bp5_cg_result *res)
{
  HIP_TRY(hipEventRecord(mf->ev_solve[1], mf->stream));
  BP5_TRY(poll_state(mf));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, mf->ev_solve[0], mf->ev_solve[1]));
  memset(res, 0, sizeof(*res));
  res->iterations = mf->h_st[ST_ITER];
  res->residual = mf->h_sc[SC_RES];
  res->initial_residual = mf->h_sc[SC_RES0];
  res->solve_ms = ms;
  res->apply_launches = prof.used / 4;
  res->dot_products_fused = fused_dots ? 1 : 0;
  res->exchange_schedule = exchange_schedule;
  if (prof.on && prof.used) {
    double tot = 0.0, tot_op = 0.0;
    for (int k = 0; k < prof.used; k += 4) {
      float t = 0.f;
      HIP_TRY(hipEventElapsedTime(&t, mf->ev_pool[k + 1], mf->ev_pool[k + 2]));
      tot += t;
      HIP_TRY(hipEventElapsedTime(&t, mf->ev_pool[k], mf->ev_pool[k + 3]));
      tot_op += t;
    }
    res->apply_ms_avg = tot / (prof.used / 4);
    res->operator_ms_avg = tot_op / (prof.used / 4);
  }
  if (own_operator) strncpy(res->apply_kernel, mf->last_apply_kernel, sizeof(res->apply_kernel) - 1);
  if (mf->h_st[ST_BREAKDOWN]) return fail(BP5_ERR_BREAKDOWN, "CG breakdown: p.Ap is zero or NaN");
  return BP5_OK;
}

// dst = A src through the caller's callback, bracketed like an operator launch
static int user_vmult(ApplyProfile &prof, bp5_vmult_fn user, void *user_ctx, double *src, double *dst)
{
  BP5_TRY(prof.mark(0));
  BP5_TRY(prof.mark(1));
  const int st = user(user_ctx, dst, src);
  if (st != BP5_OK) return fail(st, "the operator's vmult callback reported a failure");
  BP5_TRY(prof.mark(2));
  BP5_TRY(prof.mark(3));
  if (prof.on) prof.used += 4;
  return BP5_OK;
}

// What a solve on scalar vectors decides once about its operator applications (the defaults: what a solve takes that asks for none of it)
struct OperatorPlan {
  bool dist = false;       // halo exchange inside every application
  bool fused_dots = false; // the operator kernels form the dot products with its result
  bool fold_small = false; // the dot-product kernel applies the Dirichlet copy ...
  bool prezero = false;    // ... and the update kernel stores the zeros an atomic scatter needs
  uint32_t fused_update = 0; // merged solver: the block kernel updates the DoFs [0, fused_update & ~1) itself (brick interiors); 0: the update kernel all of them
  int schedule = 0;        // bp5_cg_result.exchange_schedule
};
// own_operator: the library's operator, not a callback.  fusable: no preconditioner enters the dot products the kernel would form
static int plan_operator(bp5_mf *mf, bool own_operator, bool fusable, SolveState &ss, OperatorPlan &op)
{
  // fused dot products: whenever the operator resolves to the packed block kernel on all cells of one rank (merged solver: and D == 1;
  // the plain solver takes only d.h = the quadrature-point energy from the kernel, which no preconditioner enters).
  // Across ranks the fused iteration keeps its dot products in every exchange schedule (fused_vmult_distributed): unsplit (bp5_mf_set_overlap 0:
  // gather, one launch, combine, scatter-add on the compute stream), boundary-first (1, the reference's setting: the ghost-touching
  // bricks come first, their rows travel to the owners on the communication stream under the interior bricks), and the automatic
  // choice (2): one launch, ghost rows combined first, the exchange under the owned-row combine.
  op.dist = mf->has_neighbors();
  bool split = false, split_possible = false, late = false;
  if (own_operator && mf->cg_fusion && !mf->f32_metric() /* no fused build reads float planes */ && fusable && mf->geometry_mode == BP5_GEOM_MERGED6 &&
      is_default_block(mf, effective_variant(mf, 0, mf->n_cells))) {
    bp5_mf::DevPlan *dp = nullptr;
    BP5_TRY(get_plan_raw(mf, -block_cpt(mf), &dp));
    op.fused_dots = dp->packed && dp->covers_all && (dp->n_shared == 0 || dp->cr_tile);
    if (op.fused_dots && op.dist) {
      uint32_t b0_, b1_;
      split_possible = !mf->h_block_off.empty() && (mf->n_interior == 0 || mf->n_interior == mf->n_cells || block_aligned(mf, 0, mf->n_interior, &b0_, &b1_));
      split = split_possible && mf->overlap == 1;
      if (mf->overlap == 1 && !split) op.fused_dots = false; // explicit overlap on a mesh that cannot run boundary-first: 3-phase schedule, separate dot products
      // automatic: one launch, ghost rows combined first, exchange under the owned-row combine (needs the run-length combine windows)
      late = op.fused_dots && mf->overlap == 2 && (dp->n_shared == 0 || dp->cr_tile); // (variant 56 / 63: the run-length pass wherever its tables exist)
    }
  }
  // BP5_TUNE_FUSED_UPDATE: the vector update of the brick interiors inside the block kernel -- one-rank solves with fused dot products on the p = 4
  // lattice build of variant 56, on a plan whose interior runs cover a leading range of the DoFs (interior_runs_cover); -1: where the vectors do
  // not fit the memory-side cache anyway.  Everything else takes the separate update launch over all DoFs
  if (op.fused_dots && !op.dist && !mf->comm && mf->n_ghost == 0 && mf->degree == 4 && mf->tune[BP5_TUNE_FUSED_UPDATE] != 0 &&
      mf->operator_kind == BP5_OP_POISSON && !mf->has_hanging && !mf->overint() && effective_variant(mf, 0, mf->n_cells) == 56) {
    bp5_mf::DevPlan *dp = nullptr;
    BP5_TRY(get_plan_raw(mf, -block_cpt(mf), &dp));
    const bool by_size = mf->tune[BP5_TUNE_FUSED_UPDATE] < 0;
    if (dp->lattice && dp->n_lattice_blocks == dp->n_groups && dp->upd_n_int >= 2 && (!by_size || mf->n_local() > STREAMING_MAX_DOFS)) op.fused_update = dp->upd_n_int;
  }
  ss.exchange = split ? EXCHANGE_BOUNDARY_FIRST : late ? EXCHANGE_GHOST_ROWS_FIRST : EXCHANGE_NONE;
  // whole-range launches of a distributed fused solve walk the ghost-touching bricks first in EITHER exchange schedule: same workgroup
  // ranges, same dot-product columns -- the two schedules then differ only in where the exchange is enqueued and give the same bits
  ss.two_parts = op.fused_dots && op.dist && split_possible;
  // one rank, separate dot-product kernel: the two small launches around an operator that scatters with atomics fold into their
  // neighbours -- the update kernel stores the zeros the operator needs in h / v (it holds the values in registers for the last time),
  // the dot-product kernel applies the Dirichlet copy while it reads both vectors (bitmap of the Dirichlet DoFs)
  const bool fold_enabled = mf->tune[BP5_TUNE_FOLD_SMALL] != 0; // A/B knob of the handle
  op.fold_small = fold_enabled && !op.fused_dots && own_operator && !op.dist;
  op.prezero = op.fold_small && mf->n_ghost == 0 && !variant_overwrites(mf, effective_variant(mf, 0, mf->n_cells)); // (the update kernels cover owned entries)
  // (the operator then sits between a zero-storing update and a copying dot-product kernel; neither holds for a fused application)
  ss.dst_prezeroed = op.prezero;
  ss.copies_dirichlet = op.fold_small;
  op.schedule = !op.dist ? 0 : split ? 2 : late ? 4 : op.fused_dots ? 1 : overlap_wanted(mf) ? 3 : 1;
  return BP5_OK;
}

// ---- which operator a solve or a preconditioner applies, and on what vector shape: the ONE description that PlainCG, bp5_chebyshev and bp5_mg hold.
// Its makers (the entry points) have checked the arguments
struct LinearOp {
  // NATIVE: the handle's scalar operator on coef (Poisson, Helmholtz, mass); CALLBACK: the caller's vmult (scalar vectors only); BLOCK_POISSON: the
  // scalar operator block by block; ELASTICITY: the coupled three-component operator (coef: its ten planes); HYPERELASTIC_TANGENT: the neo-Hookean
  // tangent at `state` (the ten state planes of bp5_hyperelasticity_residual)
  enum Kind { NATIVE, CALLBACK, BLOCK_POISSON, ELASTICITY, HYPERELASTIC_TANGENT } kind = NATIVE;
  const double *coef = nullptr;
  bp5_vmult_fn user = nullptr;
  void *user_ctx = nullptr;
  // vectors: n_components blocks ld apart; a scalar vector: 1 and 0
  int n_components = 1;
  size_t ld = 0;
  bool exchange = false; // BLOCK_POISSON: every application carries the halo exchange
  double lambda = 0.0, mu = 0.0;
  const double *state = nullptr;
  bool block() const { return kind >= BLOCK_POISSON; }
};
static LinearOp scalar_op(const double *coef, bp5_vmult_fn user, void *user_ctx) { return {user ? LinearOp::CALLBACK : LinearOp::NATIVE, coef, user, user_ctx}; }
static LinearOp elasticity_op(const double *coef, double lambda, double mu, size_t ld, const double *state = nullptr)
{
  return {state ? LinearOp::HYPERELASTIC_TANGENT : LinearOp::ELASTICITY, coef, nullptr, nullptr, 3, ld, false, lambda, mu, state};
}
// dst = A src for a block operator on validated arguments, Dirichlet rows included: the zero-fill, the cell loop, the Dirichlet copy, with the four
// marks of a profiled application around them
static int block_op_apply(bp5_mf *mf, const LinearOp &A, double *src, double *dst, ApplyProfile &prof)
{
  const int nc = A.n_components;
  BP5_TRY(prof.mark(0));
  BP5_TRY(components_zero(mf, nc, A.ld, dst));
  BP5_TRY(prof.mark(1));
  switch (A.kind) {
    case LinearOp::HYPERELASTIC_TANGENT: BP5_TRY(hyperelasticity_apply_cells(mf, A.coef, A.state, A.lambda, A.mu, A.ld, src, dst, 0, mf->n_cells)); break;
    case LinearOp::ELASTICITY: BP5_TRY(elasticity_apply_cells(mf, A.coef, A.lambda, A.mu, A.ld, src, dst, 0, mf->n_cells)); break;
    default:
      if (A.exchange) BP5_TRY(components_apply_exchanged(mf, A.coef, nc, A.ld, src, dst, false));
      else BP5_TRY(components_apply(mf, A.coef, nc, A.ld, src, dst, false));
  }
  BP5_TRY(prof.mark(2));
  BP5_TRY(components_copy_constrained(mf, nc, A.ld, src, dst));
  BP5_TRY(prof.mark(3));
  if (prof.on) prof.used += 4;
  return BP5_OK;
}

// ---- the plain recurrence (deal.II SolverCG): ONE driver for scalar vectors, block vectors and any preconditioner.  Its entry points have
// checked their arguments and made the work vectors; they describe the solve by this struct
struct PlainCG {
  LinearOp op;                                     // the operator and the shape of every vector of the solve
  double *g = nullptr, *d = nullptr, *h = nullptr; // the workspace triple
  // preconditioner: an inverse diagonal (NULL == 1), or a callback that writes z = P g -- on scalar vectors (bp5_cg_solve_preconditioned) or on
  // block vectors of the solve's n_components and ld (bp5_cg_solve_elasticity_preconditioned); z is laid out like g (scalar: ws_z; block:
  // wsz_base, block_cg_workspace).  diag_ld: doubles between the diagonals of two components -- 0: ONE scalar diagonal applied to every block;
  // ld: a block inverse diagonal
  const double *diag = nullptr;
  size_t diag_ld = 0;
  bp5_vmult_fn precond = nullptr;
  void *precond_ctx = nullptr;
  double *z = nullptr;
  bool allreduce = true; // d.h, g.g and g.z summed over the ranks (block vectors without exchange: no)
  // alpha / beta of iteration k into history[2k], history[2k + 1] on the device, k < history_cap (Chebyshev estimate)
  double *history = nullptr;
  int history_cap = 0;
};
// Per iteration: h = A d, d.h, x += alpha d, g += alpha h, [z = P g,] g.g and g.Dg (g.z) in ONE all-reduce, the scalar step, d = beta d - D g (z).
// Every kernel is gated on the device-side stop flag.  A callback preconditioner is not (the host does not know the flag before it looks), it
// writes only z and its own work vectors, and z is not read once the solve has stopped: the same bits for every check_every.
static int cg_solve_plain(bp5_mf *mf, const PlainCG &cg, const double *b, double *x, const bp5_cg_params *prm, bp5_cg_result *res)
{
  hipStream_t s = mf->stream;
  const LinearOp &A = cg.op;
  const size_t n = mf->n_owned, ld = A.ld;
  const int nc = A.n_components;
  double *g = cg.g, *d = cg.d, *h = cg.h, *z = cg.z;
  const double *diag = cg.diag;
  const size_t dld = cg.diag_ld;
  // launch geometry: the component is the second grid dimension and owns PARTIAL_STRIDE / n_components columns of a partial-sum row (a scalar
  // vector: all of them, stream_grid never asks for more).  Scalar vectors launch the direction kernel, which reduces nothing, flat
  const int cols = PARTIAL_STRIDE / nc;
  const dim3 grid1(std::min(stream_grid(n, 1), cols), nc), grid2(std::min(stream_grid(n, 2), cols), nc), block(VB);
  const dim3 gridd = A.block() ? grid2 : dim3(stream_grid_flat(mf, n, 2));
  const int nblk1 = (int)grid1.x * nc, nblk2 = (int)grid2.x * nc;
  const int *no_flag = nullptr; // (the stop flag is the last solve's until the control step of the initialisation)
  SolveState ss{ApplyProfile{mf, prm->profile != 0 && !cg.precond}}; // (a callback preconditioner: the applications are not bracketed)
  ApplyProfile &prof = ss.prof;
  BP5_TRY(solve_begin(mf, prm, prof)); // (the plan below may build the block kernel's tables on a handle's first solve: inside solve_ms)
  OperatorPlan op;
  if (!A.block() && !cg.precond) BP5_TRY(plan_operator(mf, !A.user, true, ss, op));
  else op.schedule = A.user || !mf->has_neighbors() ? 0 : overlap_wanted(mf) ? 3 : 1;
  std::string operator_kernel; // block vectors with a callback preconditioner: the name of the solve's OWN operator kernel, for the result
  // h = A d, Dirichlet rows included (unless the dot-product kernel copies them).  Fused dot products: d.h lies in *n_cols columns of d_partials
  auto apply_A = [&](uint32_t *n_cols) -> int {
    if (A.user) return user_vmult(prof, A.user, A.user_ctx, d, h);
    if (!A.block()) return solver_vmult(mf, ss, A.coef, d, h, true, nullptr, op.fused_dots ? n_cols : nullptr); // (no residual vector: the write-out does not read g)
    BP5_TRY(block_op_apply(mf, A, d, h, prof));
    if (cg.precond) operator_kernel = mf->last_apply_kernel; // (a preconditioner on the same handle launches operator kernels of its own)
    return BP5_OK;
  };
  auto apply_P = [&]() -> int {
    const int st = cg.precond(cg.precond_ctx, z, g);
    return st == BP5_OK ? BP5_OK : fail(st, "the preconditioner's vmult callback reported a failure");
  };
  // g = -b, d = -D g, x = 0   (x0 = 0 short-circuit, bp5/solver.h:375-381); a callback: z = P g and d = -z behind the control step
  if (cg.precond) {
    hipLaunchKernelGGL(cg_init_kernel<false>, grid1, block, 0, s, b, diag, x, g, d, n, ld, mf->d_partials, dld);
    hipLaunchKernelGGL(finalize_kernel<1>, dim3(1), block, 0, s, mf->d_partials, nblk1, mf->d_sc + SC_GG, no_flag);
    KERNEL_CHECK();
    BP5_TRY(apply_P());
    if (A.block()) BP5_TRY(blockvec_dot(s, grid2, g, z, n, ld, mf->d_partials)); // g.z over the owned entries of all blocks
    else hipLaunchKernelGGL(dot_kernel, grid2, block, 0, s, g, z, n, mf->d_partials);
    hipLaunchKernelGGL(finalize_kernel<1>, dim3(1), block, 0, s, mf->d_partials, nblk2, mf->d_sc + SC_GDG, no_flag);
  } else {
    hipLaunchKernelGGL(cg_init_kernel<true>, grid1, block, 0, s, b, diag, x, g, d, n, ld, mf->d_partials, dld);
    hipLaunchKernelGGL(finalize_kernel<2>, dim3(2), block, 0, s, mf->d_partials, nblk1, mf->d_sc + SC_GG, no_flag);
  }
  KERNEL_CHECK();
  if (cg.allreduce) BP5_TRY(bp5_comm_allreduce_sum(mf, mf->d_sc + SC_GG, 2));
  hipLaunchKernelGGL(cg_init_control_kernel, dim3(1), dim3(1), 0, s, mf->d_sc, mf->d_st); // res0, gh = g.Dg (g.z), stop test
  if (cg.precond) hipLaunchKernelGGL((cg_direction_kernel<true, true>), gridd, block, 0, s, d, z, diag, n, ld, mf->d_sc, mf->d_st, dld);
  KERNEL_CHECK();
  if (op.prezero) HIP_TRY(hipMemsetAsync(h, 0, mf->n_local() * sizeof(double), s)); // once: every later zero-fill is stored by cg_update_kernel
  const int check = prm->check_every;
  // check_every = 0 with a callback preconditioner: the operator and the preconditioner are not gated on the stop flag (a preconditioner is any
  // callback), so the host looks at the flag itself -- with a lag of DONE_LAG iterations (the copy of iteration k's flag is waited for after iteration
  // k + DONE_LAG has been enqueued): the queue never drains, and at most DONE_LAG iterations run on a stopped solve, whose kernels leave x, g, d alone
  constexpr int DONE_LAG = 2;
  const bool lagged_look = cg.precond && check <= 0;
  if (lagged_look) {
    if (!mf->h_done) HIP_TRY(hipHostMalloc((void **)&mf->h_done, (DONE_LAG + 1) * sizeof(int)));
    for (hipEvent_t &e : mf->ev_done) if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  for (int it = 1; it <= prm->max_iter; ++it) {
    uint32_t n_cols = 0;
    BP5_TRY(apply_A(&n_cols));
    if (op.fused_dots) // d.h = sum over the cells of the quadrature-point energy (+ d^2 on Dirichlet rows, where h = d): row 0 of the fused sums
      hipLaunchKernelGGL(finalize_kernel<1>, dim3(1), block, 0, s, mf->d_partials, (int)n_cols, mf->d_sc + SC_DH, mf->d_st);
    else {
      if (op.fold_small) hipLaunchKernelGGL(cg_dh_kernel<true>, grid2, block, 0, s, d, h, n, ld, mf->d_partials, mf->d_st, (const uint32_t *)mf->d_constrained_bits);
      else hipLaunchKernelGGL(cg_dh_kernel<false>, grid2, block, 0, s, d, h, n, ld, mf->d_partials, mf->d_st, (const uint32_t *)nullptr);
      hipLaunchKernelGGL(finalize_kernel<1>, dim3(1), block, 0, s, mf->d_partials, nblk2, mf->d_sc + SC_DH, mf->d_st);
    }
    if (cg.allreduce) { KERNEL_CHECK(); BP5_TRY(bp5_comm_allreduce_sum(mf, mf->d_sc + SC_DH, 1)); }
    if (cg.precond) {
      hipLaunchKernelGGL(cg_update_kernel<false>, grid2, block, 0, s, x, g, d, h, diag, n, ld, mf->d_sc, mf->d_st, mf->d_partials, false, dld);
      hipLaunchKernelGGL(finalize_kernel<1>, dim3(1), block, 0, s, mf->d_partials, nblk2, mf->d_sc + SC_GG, mf->d_st);
      KERNEL_CHECK();
      BP5_TRY(apply_P()); // (the sum g.g is in SC_GG already: the preconditioner may run reductions of its own)
      hipLaunchKernelGGL(cg_dh_kernel<false>, grid2, block, 0, s, g, z, n, ld, mf->d_partials, mf->d_st, (const uint32_t *)nullptr);
      hipLaunchKernelGGL(finalize_kernel<1>, dim3(1), block, 0, s, mf->d_partials, nblk2, mf->d_sc + SC_GDG, mf->d_st);
    } else {
      hipLaunchKernelGGL(cg_update_kernel<true>, grid2, block, 0, s, x, g, d, h, diag, n, ld, mf->d_sc, mf->d_st, mf->d_partials, op.prezero, dld);
      hipLaunchKernelGGL(finalize_kernel<2>, dim3(2), block, 0, s, mf->d_partials, nblk2, mf->d_sc + SC_GG, mf->d_st);
    }
    if (cg.allreduce) { KERNEL_CHECK(); BP5_TRY(bp5_comm_allreduce_sum(mf, mf->d_sc + SC_GG, 2)); } // g.g, g.Dg (g.z)
    hipLaunchKernelGGL(cg_control_kernel, dim3(1), dim3(1), 0, s, mf->d_sc, mf->d_st); // res, ++it, stop test, beta
    if (cg.history) hipLaunchKernelGGL(cg_record_kernel, dim3(1), dim3(1), 0, s, mf->d_sc, mf->d_st, cg.history, cg.history_cap);
    if (cg.precond) hipLaunchKernelGGL((cg_direction_kernel<true, false>), gridd, block, 0, s, d, z, diag, n, ld, mf->d_sc, mf->d_st, dld);
    else hipLaunchKernelGGL((cg_direction_kernel<false, false>), gridd, block, 0, s, d, g, diag, n, ld, mf->d_sc, mf->d_st, dld);
    KERNEL_CHECK();
    if (check > 0 && it % check == 0 && it < prm->max_iter) {
      BP5_TRY(poll_state(mf));
      if (mf->h_st[ST_DONE]) break;
    } else if (lagged_look && it < prm->max_iter) {
      const int slot = it % (DONE_LAG + 1);
      HIP_TRY(hipMemcpyAsync(mf->h_done + slot, mf->d_st + ST_DONE, sizeof(int), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipEventRecord(mf->ev_done[slot], s));
      if (it > DONE_LAG) {
        const int seen = (it - DONE_LAG) % (DONE_LAG + 1);
        HIP_TRY(hipEventSynchronize(mf->ev_done[seen]));
        if (mf->h_done[seen]) break;
      }
    }
  }
  if (!operator_kernel.empty()) snprintf(mf->last_apply_kernel, sizeof(mf->last_apply_kernel), "%s", operator_kernel.c_str());
  return solve_finish(mf, prof, op.fused_dots, op.schedule, !A.user, res);
}

// ---- SolverCGFullMerge on scalar vectors (bp5/solver.h:343-542): g == r, d == p, h == v
static int cg_solve_merged(bp5_mf *mf, const double *coef, bp5_vmult_fn user, void *user_ctx, const double *diag, const double *b, double *x,
                           const bp5_cg_params *prm, bp5_cg_result *res)
{
  const size_t n = mf->n_owned;
  const int grid2 = stream_grid(n, 2), grid1 = stream_grid(n, 1);
  hipStream_t s = mf->stream;
  double *g = mf->ws_g, *d = mf->ws_d, *h = mf->ws_h;
  SolveState ss{ApplyProfile{mf, prm->profile != 0}};
  ss.phase_on = prm->profile == 2;
  if (ss.phase_on) {
    const size_t want = (size_t)bp5_mf::PhaseProfile::MAX_ITERS * bp5_mf::PhaseProfile::MARKS;
    while (mf->phase.ev.size() < want) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); mf->phase.ev.push_back(e); }
  }
  BP5_TRY(solve_begin(mf, prm, ss.prof)); // (the plan below may build the block kernel's tables on a handle's first solve: inside solve_ms)
  OperatorPlan op;
  BP5_TRY(plan_operator(mf, !user, !diag, ss, op));
  const bool fused = op.fused_dots, dist_solve = op.dist, fold_small = op.fold_small, prezero = op.prezero;
  // h = A d.  dst is fully defined by the call (the reference zeroes it in update_a* for its atomic scatter)
  auto vmult = [&](double *src, double *dst, const double *fuse_r, uint32_t *n_cols) -> int {
    if (!user) return solver_vmult(mf, ss, coef, src, dst, true, fuse_r, n_cols);
    return user_vmult(ss.prof, user, user_ctx, src, dst);
  };
  const int check = prm->check_every;
  // (v: the fused block kernel of a one-rank solve overwrites every entry before anything reads it; every other path keeps the zero-fill)
  hipLaunchKernelGGL(cgm_init_kernel, dim3(grid1), dim3(VB), 0, s, b, x, g, d, h, diag, n, mf->d_partials, !(fused && !dist_solve));
  hipLaunchKernelGGL(finalize_kernel<2>, dim3(2), dim3(VB), 0, s, mf->d_partials, grid1, mf->d_sc + SC_GG, (const int *)nullptr);
  KERNEL_CHECK();
  BP5_TRY(bp5_comm_allreduce_sum(mf, mf->d_sc + SC_GG, 2));
  // Fused update (op.fused_update, plan_operator): in the iterations after the first the block kernel updates the brick interiors [0, n_first)
  // itself and the update launch shrinks to the rest.  A stopped solve: the block kernel is a no-op, so the in-loop rest launch is one too, and the x
  // epilogue stays pending (ST_HOLD) for the whole-range launch behind the loop, whatever number of stopped iterations check_every lets through
  const size_t n_first = fused && !user ? (size_t)(op.fused_update & ~1u) : 0; // (even: the rest launch starts on a 16-byte boundary)
  hipLaunchKernelGGL(cgm_init_control_kernel, dim3(1), dim3(1), 0, s, mf->d_sc, mf->d_st, n_first ? 1 : 0);
  KERNEL_CHECK();
  // update kernels: U chunks of 256 pairs per workgroup (flat launch: one trip per workgroup), all loads ahead of the first store.
  // profiles/r4 hbm_sweep: U = 1 flat 5.5-5.9 TB/s, the capped grid-stride grid of rounds 1-3 (U = 4, 2048 workgroups) 4.8-4.9
  const int unroll = mf->tune[BP5_TUNE_UPDATE_UNROLL];
  const int gridu = stream_grid_flat(mf, n, 2 * unroll);
  // v and x non-temporally: at every size since round 4 (-1 = on; profiles/r4 ab_update_*: 3.741 -> 3.707 ms per iteration at 1e8 DoFs with the flat
  // launch, 0.4075 -> 0.4025 at 1e7; rounds 1-3 followed the streaming policy of the metric loads, which is off at 1e8 DoFs)
  const bool streaming = mf->tune[BP5_TUNE_UPDATE_NT] != 0;
  auto launch_update = [&](int mode) {
#define BP5_UPD(M, U, ZV, NT) hipLaunchKernelGGL((cgm_update_kernel<M, U, ZV, NT>), dim3(gridu), dim3(VB), 0, s, d, g, h, x, diag, n, mf->d_sc, mf->d_st)
#define BP5_UPD_U(M, ZV, NT) do { if (unroll == 1) BP5_UPD(M, 1, ZV, NT); else if (unroll == 2) BP5_UPD(M, 2, ZV, NT); else BP5_UPD(M, 4, ZV, NT); } while (0)
    if (mode == 0) { BP5_UPD_U(0, false, false); return; }
    if (prezero) { if (mode == 1) BP5_UPD_U(1, true, false); else BP5_UPD_U(2, true, false); return; }
    if (streaming) { if (mode == 1) BP5_UPD_U(1, false, true); else BP5_UPD_U(2, false, true); return; }
    if (mode == 1) BP5_UPD_U(1, false, false); else BP5_UPD_U(2, false, false);
#undef BP5_UPD_U
#undef BP5_UPD
  };
  const int gridr = n > n_first ? stream_grid_flat(mf, n - n_first, 2 * unroll) : 0;
  auto launch_update_rest = [&](int mode) {
    if (!gridr) return;
#define BP5_UPR(M, U, NT) hipLaunchKernelGGL((cgm_update_rest_kernel<M, U, NT>), dim3(gridr), dim3(VB), 0, s, d, g, h, x, diag, n_first, n - n_first, mf->d_sc, mf->d_st)
#define BP5_UPR_U(M, NT) do { if (unroll == 1) BP5_UPR(M, 1, NT); else if (unroll == 2) BP5_UPR(M, 2, NT); else BP5_UPR(M, 4, NT); } while (0)
    if (streaming) { if (mode == 1) BP5_UPR_U(1, true); else BP5_UPR_U(2, true); return; }
    if (mode == 1) BP5_UPR_U(1, false); else BP5_UPR_U(2, false);
#undef BP5_UPR_U
#undef BP5_UPR
  };
  // fused iteration across ranks: the values of the NEW p at the DoFs this rank sends are computed into the send buffer first, so the
  // ghost gather of p runs on the communication stream underneath the update kernel (which touches owned entries only); the operator
  // then just waits for the event
  const bool early_gather_enabled = mf->tune[BP5_TUNE_EARLY_GATHER] != 0; // A/B knob of the handle
  const bool early_gather = fused && dist_solve && early_gather_enabled;
  auto gather_under_update = [&](int mode) -> int {
    BP5_TRY(halo_streams(mf));
    const uint32_t ns = mf->send_off.back();
    if (ns) {
      const dim3 gr((ns + 255) / 256), bl(256);
      if (mode == 0) hipLaunchKernelGGL(cgm_pack_updated_kernel<0>, gr, bl, 0, s, mf->d_send_idx, ns, d, g, h, diag, mf->d_sc, mf->d_st, mf->d_sendbuf);
      else hipLaunchKernelGGL(cgm_pack_updated_kernel<1>, gr, bl, 0, s, mf->d_send_idx, ns, d, g, h, diag, mf->d_sc, mf->d_st, mf->d_sendbuf);
      KERNEL_CHECK();
    }
    return gather_exchange(mf, d, true);
  };
  int it = 1;
  for (; it <= prm->max_iter; ++it) {
    const int mode = it == 1 ? 0 : it % 2 == 0 ? 1 : 2;
    BP5_TRY(phase_mark(mf, ss, 0));
    if (early_gather) { BP5_TRY(gather_under_update(mode)); ss.gather_in_flight = true; }
    if (mode != 0) { // (mode 0, p = -D r: written by cgm_init_kernel already)
      if (n_first) launch_update_rest(mode); else launch_update(mode);
    }
    ss.upd_mode = n_first ? mode : 0; ss.upd_x = x; ss.upd_diag = diag;
    KERNEL_CHECK();
    BP5_TRY(phase_mark(mf, ss, 1));
    const bool one_launch = fused && !mf->comm; // no all-reduce between the local sums and the scalar step
    if (fused) {
      uint32_t n_cols = 0;
      BP5_TRY(vmult(d, h, g, &n_cols));
      BP5_TRY(phase_mark(mf, ss, 4));
      if (one_launch) hipLaunchKernelGGL(cgm_finalize4_kernel<true>, dim3(1), dim3(FIN4_THREADS), 0, s, mf->d_partials, (int)n_cols, mf->d_sc, mf->d_st);
      else hipLaunchKernelGGL(cgm_finalize4_kernel<false>, dim3(1), dim3(FIN4_THREADS), 0, s, mf->d_partials, (int)n_cols, mf->d_sc, mf->d_st);
    } else {
      BP5_TRY(vmult(d, h, nullptr, nullptr)); // (h: zeroed by cgm_init_kernel before the first, by the update kernel before every later application)
      BP5_TRY(phase_mark(mf, ss, 4));
      hipLaunchKernelGGL(cgm_dots_kernel, dim3(grid2), dim3(VB), 0, s, d, g, h, diag, n, mf->d_st, mf->d_partials,
                         fold_small ? (const uint32_t *)mf->d_constrained_bits : (const uint32_t *)nullptr);
      hipLaunchKernelGGL(finalize_kernel<7>, dim3(7), dim3(VB), 0, s, mf->d_partials, grid2, mf->d_sc + SC_R0, mf->d_st);
    }
    KERNEL_CHECK();
    BP5_TRY(phase_mark(mf, ss, 5));
    if (!one_launch) {
      BP5_TRY(bp5_comm_allreduce_sum(mf, mf->d_sc + SC_R0, 7));
      BP5_TRY(phase_mark(mf, ss, 6));
      hipLaunchKernelGGL(cgm_control_kernel, dim3(1), dim3(1), 0, s, mf->d_sc, mf->d_st);
      KERNEL_CHECK();
    } else
      BP5_TRY(phase_mark(mf, ss, 6));
    BP5_TRY(phase_mark(mf, ss, 7));
    if (ss.phase_on) ++ss.phase_it;
    if (check > 0 && it % check == 0 && it < prm->max_iter) {
      BP5_TRY(poll_state(mf));
      if (mf->h_st[ST_DONE]) break;
    }
  }
  // epilogue x update (solver.h:510-526) runs inside the next update kernel; with max_iter == 0 no
  // iteration has been done and nothing is pending
  if (prm->max_iter > 0) {
    launch_update(1);
    if (n_first) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(mf->d_st + ST_HOLD), 0, 1, s)); // the epilogue is applied: the control step may clear the flag
    hipLaunchKernelGGL(cgm_control_kernel, dim3(1), dim3(1), 0, s, mf->d_sc, mf->d_st);
    KERNEL_CHECK();
  }
  const int status = solve_finish(mf, ss.prof, fused, op.schedule, !user, res);
  if (!ss.phase_on || (status != BP5_OK && status != BP5_ERR_BREAKDOWN)) return status;
  // averages over the stamped iterations after the first (whose update kernel is the cheap update_a0)
  using PP = bp5_mf::PhaseProfile;
  const int n_it = std::min(ss.phase_it, (int)PP::MAX_ITERS);
  int counted = 0;
  for (int i = n_it > 1 ? 1 : 0; i < n_it; ++i) {
    const uint8_t rec = ss.phase_recorded[i];
    const uint8_t need = (1u << 0) | (1u << 1) | (1u << 4) | (1u << 5) | (1u << 6) | (1u << 7);
    if ((rec & need) != need) continue;
    auto ms = [&](int a, int b, double &out) -> int {
      float t = 0.f;
      HIP_TRY(hipEventElapsedTime(&t, mf->phase.ev[(size_t)i * PP::MARKS + a], mf->phase.ev[(size_t)i * PP::MARKS + b]));
      out += t;
      return BP5_OK;
    };
    const bool g = rec & (1u << 2), x = rec & (1u << 3);
    BP5_TRY(ms(0, 1, res->phase_ms[BP5_PHASE_UPDATE]));
    if (g) BP5_TRY(ms(1, 2, res->phase_ms[BP5_PHASE_GATHER_WAIT]));
    BP5_TRY(ms(g ? 2 : 1, x ? 3 : 4, res->phase_ms[BP5_PHASE_OPERATOR]));
    if (x) BP5_TRY(ms(3, 4, res->phase_ms[BP5_PHASE_EXCHANGE]));
    BP5_TRY(ms(4, 5, res->phase_ms[BP5_PHASE_REDUCE]));
    BP5_TRY(ms(5, 6, res->phase_ms[BP5_PHASE_ALLREDUCE]));
    BP5_TRY(ms(6, 7, res->phase_ms[BP5_PHASE_CONTROL]));
    BP5_TRY(ms(0, 7, res->phase_ms[BP5_PHASE_ITERATION]));
    ++counted;
  }
  if (counted) for (double &v : res->phase_ms) v /= counted;
  return status;
}

// cg.solve(A, x, b, preconditioner) on scalar vectors with a diagonal: the solvers need nothing of A but vmult (bp5/solver.h:25-30,377,475).
// user == nullptr: the built-in Poisson operator (coef); otherwise the caller's operator through its callback.
// history != NULL (plain solve): the Lanczos coefficients for the Chebyshev estimate (PlainCG::history)
static int cg_solve_impl(bp5_mf *mf, const double *coef, bp5_vmult_fn user, void *user_ctx, const double *diag, const double *b, double *x,
                         const bp5_cg_params *prm, bp5_cg_result *res, double *history = nullptr, int history_cap = 0)
{
  if (!mf || (!user && !coef && mf->geometry_mode == BP5_GEOM_MERGED6) || !b || !x || !prm || !res) return fail(BP5_ERR_INVALID, "null argument");
  if (prm->max_iter < 0) return fail(BP5_ERR_INVALID, "max_iter < 0");
  if (prm->variant != BP5_CG_PLAIN && prm->variant != BP5_CG_MERGED) return fail(BP5_ERR_INVALID, "unknown CG variant");
  if (!aligned16(b) || !aligned16(x) || (diag && !aligned16(diag))) return fail(BP5_ERR_INVALID, "vectors must be 16-byte aligned");
  HIP_TRY(hipSetDevice(mf->device));
  BP5_TRY(ensure_ws(mf));
  if (prm->variant == BP5_CG_MERGED) return cg_solve_merged(mf, coef, user, user_ctx, diag, b, x, prm, res);
  PlainCG cg;
  cg.g = mf->ws_g; cg.d = mf->ws_d; cg.h = mf->ws_h;
  cg.op = scalar_op(coef, user, user_ctx);
  cg.diag = diag;
  cg.history = history; cg.history_cap = history_cap;
  return cg_solve_plain(mf, cg, b, x, prm, res);
}

extern "C" int bp5_cg_solve(bp5_mf *mf, const double *coef, const double *diag, const double *b, double *x, const bp5_cg_params *prm,
                            bp5_cg_result *res)
{
  return cg_solve_impl(mf, coef, nullptr, nullptr, diag, b, x, prm, res);
}
extern "C" int bp5_cg_solve_operator(bp5_mf *mf, bp5_vmult_fn vmult, void *ctx, const double *diag, const double *b, double *x,
                                     const bp5_cg_params *prm, bp5_cg_result *res)
{
  if (!vmult) return fail(BP5_ERR_INVALID, "null vmult callback");
  return cg_solve_impl(mf, nullptr, vmult, ctx, diag, b, x, prm, res);
}

// a work array of the handle (base, cap) of `need` doubles: grown on demand -- freed only to grow, behind a synchronisation of the stream -- and
// zero-filled on every call
static int grown_workspace(double *&base, size_t &cap, size_t need, hipStream_t stream)
{
  if (cap < need) {
    if (base) { HIP_TRY(hipStreamSynchronize(stream)); HIP_TRY(hipFree(base)); base = nullptr; cap = 0; }
    HIP_TRY(hipMalloc((void **)&base, need * sizeof(double)));
    cap = need;
  }
  HIP_TRY(hipMemsetAsync(base, 0, need * sizeof(double), stream));
  return BP5_OK;
}
// the work vectors g, d, h of a plain solve on the block vectors of cg.op: 3 n_components ld doubles (the ghost entries of d are read by the
// operator: defined, zero); with_z: and z = P g of a solve with a callback preconditioner, a vector of its own (the padding of z is the callback's)
static int block_cg_workspace(bp5_mf *mf, PlainCG &cg, bool with_z)
{
  const size_t block = (size_t)cg.op.n_components * cg.op.ld;
  BP5_TRY(grown_workspace(mf->wsc_base, mf->wsc_cap, 3 * block, mf->stream));
  cg.g = mf->wsc_base; cg.d = cg.g + block; cg.h = cg.d + block;
  if (with_z) {
    BP5_TRY(grown_workspace(mf->wsz_base, mf->wsz_cap, block, mf->stream));
    cg.z = mf->wsz_base;
  }
  return BP5_OK;
}
// what every CG entry point checks first, in the words of its refusing function: prm and res, the variant (plain_only: the refusal of everything
// but BP5_CG_PLAIN, in these words), max_iter, and the 16-byte alignment of v0 and v1 (NULL: not there)
typedef int (*Refuse)(int status, const char *what);
static int plainly_refuse(int status, const char *what) { return fail(status, what); }
static int cg_preamble(Refuse refuse, const bp5_cg_params *prm, const void *res, const double *v0, const double *v1, const char *misaligned,
                       const char *plain_only = nullptr)
{
  if (!prm || !res) return refuse(BP5_ERR_INVALID, "null argument");
  if (plain_only ? prm->variant != BP5_CG_PLAIN : prm->variant != BP5_CG_PLAIN && prm->variant != BP5_CG_MERGED)
    return refuse(BP5_ERR_INVALID, plain_only ? plain_only : "unknown CG variant");
  if (prm->max_iter < 0) return refuse(BP5_ERR_INVALID, "max_iter < 0");
  if ((v0 && !aligned16(v0)) || (v1 && !aligned16(v1))) return refuse(BP5_ERR_INVALID, misaligned);
  return BP5_OK;
}
// cg.solve(A, x, b, DiagonalMatrix) on a block vector: the plain recurrence on the stacked system, one launch per BLAS-1 step
// with_exchange (bp5_cg_solve_components_distributed): a handle with a communicator and neighbours is taken, every operator application carries
// the halo exchange (components_apply_exchanged) and d.h, g.g and g.z are all-reduced where the scalar plain solver all-reduces them
static int cg_solve_components_impl(bp5_mf *mf, const double *coef, int n_components, size_t ld, const double *diag, const double *b, double *x,
                                    const bp5_cg_params *prm, bp5_cg_result *res, bool with_exchange)
{
  if (!b || !x) return fail(BP5_ERR_INVALID, "null argument");
  BP5_TRY(cg_preamble(plainly_refuse, prm, res, diag, nullptr, "vectors must be 16-byte aligned"));
  BP5_TRY(components_check(mf, coef, n_components, ld, b, x, with_exchange));
  if (prm->variant == BP5_CG_MERGED) return fail(BP5_ERR_UNSUPPORTED, "block vectors: SolverCGFullMerge (BP5_CG_MERGED) is not offered, use BP5_CG_PLAIN");
  HIP_TRY(hipSetDevice(mf->device));
  PlainCG cg;
  cg.op = {LinearOp::BLOCK_POISSON, coef, nullptr, nullptr, n_components, ld, with_exchange && mf->has_neighbors()};
  BP5_TRY(block_cg_workspace(mf, cg, false));
  cg.diag = diag;
  cg.allreduce = with_exchange;
  return cg_solve_plain(mf, cg, b, x, prm, res);
}
extern "C" int bp5_cg_solve_components(bp5_mf *mf, const double *coef, int n_components, size_t ld, const double *diag, const double *b, double *x,
                                       const bp5_cg_params *prm, bp5_cg_result *res)
{
  return cg_solve_components_impl(mf, coef, n_components, ld, diag, b, x, prm, res, false);
}
extern "C" int bp5_cg_solve_components_distributed(bp5_mf *mf, const double *coef, int n_components, size_t ld, const double *diag, const double *b,
                                                   double *x, const bp5_cg_params *prm, bp5_cg_result *res)
{
  return cg_solve_components_impl(mf, coef, n_components, ld, diag, b, x, prm, res, true);
}

// cg.solve(A, x, b, DiagonalMatrix) for the elasticity operator: the plain recurrence on the stacked three-component system, the operator step the
// coupled application and the preconditioner a BLOCK inverse diagonal (three blocks ld apart, as bp5_elasticity_compute_diagonal returns them)
// precond != NULL (bp5_cg_solve_elasticity_preconditioned): z = P g from the callback in place of the diagonal; history != NULL: the Lanczos
// coefficients of the solve (PlainCG::history: the estimate of bp5_elasticity_chebyshev_create)
static int cg_solve_elasticity_impl(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, const double *inv_diag, bp5_vmult_fn precond,
                                    void *precond_ctx, const double *b, double *x, const bp5_cg_params *prm, bp5_cg_result *res, double *history = nullptr,
                                    int history_cap = 0)
{
  BP5_TRY(cg_preamble(elasticity_refuse, prm, res, inv_diag, nullptr, "block vectors must be 16-byte aligned"));
  BP5_TRY(elasticity_check(mf, coef, lambda, mu, ld, b, x, true));
  if (inv_diag) { // the update kernels read it while they write x
    const size_t extent = 2 * ld + mf->n_local();
    if (inv_diag < x + extent && x < inv_diag + extent) return elasticity_refuse(BP5_ERR_INVALID, "inv_diag and x overlap");
  }
  if (prm->variant == BP5_CG_MERGED) return elasticity_refuse(BP5_ERR_UNSUPPORTED, "SolverCGFullMerge (BP5_CG_MERGED) is not offered, use BP5_CG_PLAIN");
  HIP_TRY(hipSetDevice(mf->device));
  PlainCG cg;
  cg.op = elasticity_op(coef, lambda, mu, ld);
  BP5_TRY(block_cg_workspace(mf, cg, precond != nullptr));
  cg.diag = inv_diag; cg.diag_ld = ld;
  cg.allreduce = false;
  cg.precond = precond; cg.precond_ctx = precond_ctx;
  cg.history = history; cg.history_cap = history_cap;
  return cg_solve_plain(mf, cg, b, x, prm, res);
}
extern "C" int bp5_cg_solve_elasticity(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, const double *inv_diag, const double *b, double *x,
                                       const bp5_cg_params *prm, bp5_cg_result *res)
{
  return cg_solve_elasticity_impl(mf, coef, lambda, mu, ld, inv_diag, nullptr, nullptr, b, x, prm, res);
}
// cg.solve(A, x, b, P) for the elasticity operator and a P given by its vmult on three-block vectors of the same ld: the plain recurrence with
// z = P g in place of D g (cg_solve_plain's callback path on block vectors)
extern "C" int bp5_cg_solve_elasticity_preconditioned(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, bp5_vmult_fn precond, void *precond_ctx,
                                                      const double *b, double *x, const bp5_cg_params *prm, bp5_cg_result *res)
{
  if (!precond) return elasticity_refuse(BP5_ERR_INVALID, "null argument (the preconditioner's vmult callback)");
  return cg_solve_elasticity_impl(mf, coef, lambda, mu, ld, nullptr, precond, precond_ctx, b, x, prm, res);
}

// ------------------------------------------------------------------------------------ neo-Hookean hyperelasticity (residual, tangent, Newton)
// The vectors, the handle and the geometry planes are the elasticity operator's, and so is every refusal: its checks run as they are and their
// reason ("elasticity: ...") is handed on under this operator's name
static int hyperelasticity_refuse(int status, const char *what) { return fail(status, std::string("hyperelasticity: ") + what); }
static int as_hyperelasticity(int status) { return status == BP5_OK ? BP5_OK : fail(status, std::string("hyper") + bp5_last_error()); }
static int hyperelasticity_check(const bp5_mf *mf, const double *coef, const double *state, double lambda, double mu, size_t ld, const double *src, const double *dst)
{
  if (!state) return hyperelasticity_refuse(BP5_ERR_INVALID, "null argument (the state array)");
  if (!aligned16(state)) return hyperelasticity_refuse(BP5_ERR_INVALID, "the state array must be 16-byte aligned");
  return as_hyperelasticity(elasticity_check(mf, coef, lambda, mu, ld, src, dst, true));
}
extern "C" int bp5_hyperelasticity_state_size(const bp5_mf *mf, size_t *n_doubles)
{
  if (!n_doubles) return hyperelasticity_refuse(BP5_ERR_INVALID, "null argument");
  BP5_TRY(as_hyperelasticity(elasticity_handle_check(mf)));
  *n_doubles = 10 * (size_t)mf->n_cells * mf->n3;
  return BP5_OK;
}
// r = [0 +] F_int(u) with zeros on the Dirichlet rows of every block; validated arguments
static int hyperelasticity_residual(bp5_mf *mf, const double *coef, double *state, double lambda, double mu, size_t ld, const double *u, double *r, bool zero)
{
  if (zero) BP5_TRY(components_zero(mf, 3, ld, r));
  BP5_TRY(hyperelasticity_residual_cells(mf, coef, state, lambda, mu, ld, u, r, 0, mf->n_cells));
  for (int c = 0; c < 3; ++c) BP5_TRY(bp5_set_constrained(mf, 0.0, r + (size_t)c * ld));
  return BP5_OK;
}
extern "C" int bp5_hyperelasticity_residual(bp5_mf *mf, const double *coef, double *state, double lambda, double mu, size_t ld, const double *u, double *r, int zero_dst)
{
  BP5_TRY(hyperelasticity_check(mf, coef, state, lambda, mu, ld, u, r));
  HIP_TRY(hipSetDevice(mf->device));
  return hyperelasticity_residual(mf, coef, state, lambda, mu, ld, u, r, zero_dst != 0);
}
extern "C" int bp5_hyperelasticity_apply(bp5_mf *mf, const double *coef, const double *state, double lambda, double mu, size_t ld, const double *src, double *dst,
                                         int zero_dst)
{
  BP5_TRY(hyperelasticity_check(mf, coef, state, lambda, mu, ld, src, dst));
  HIP_TRY(hipSetDevice(mf->device));
  if (zero_dst) BP5_TRY(components_zero(mf, 3, ld, dst));
  BP5_TRY(hyperelasticity_apply_cells(mf, coef, state, lambda, mu, ld, src, dst, 0, mf->n_cells));
  return components_copy_constrained(mf, 3, ld, src, dst);
}
extern "C" int bp5_hyperelasticity_apply_cells(bp5_mf *mf, const double *coef, const double *state, double lambda, double mu, size_t ld, const double *src, double *dst,
                                               uint32_t cell_begin, uint32_t cell_end)
{
  BP5_TRY(hyperelasticity_check(mf, coef, state, lambda, mu, ld, src, dst));
  if (cell_begin > cell_end || cell_end > mf->n_cells) return hyperelasticity_refuse(BP5_ERR_INVALID, "cell range outside [0, n_cells]");
  HIP_TRY(hipSetDevice(mf->device));
  return hyperelasticity_apply_cells(mf, coef, state, lambda, mu, ld, src, dst, cell_begin, cell_end);
}
// every refusal of the tangent solve, before any launch
static int cg_solve_hyperelasticity_check(const bp5_mf *mf, const double *coef, const double *state, double lambda, double mu, size_t ld, const double *b, const double *x,
                                          const bp5_cg_params *prm, const void *res)
{
  BP5_TRY(cg_preamble(hyperelasticity_refuse, prm, res, nullptr, nullptr, ""));
  BP5_TRY(hyperelasticity_check(mf, coef, state, lambda, mu, ld, b, x));
  if (prm->variant == BP5_CG_MERGED) return hyperelasticity_refuse(BP5_ERR_UNSUPPORTED, "SolverCGFullMerge (BP5_CG_MERGED) is not offered, use BP5_CG_PLAIN");
  return BP5_OK;
}
// the tangent solve on validated arguments: cg_solve_plain's block-vector path, the preconditioner a callback or the identity
static int cg_solve_hyperelasticity(bp5_mf *mf, const double *coef, const double *state, double lambda, double mu, size_t ld, bp5_vmult_fn precond, void *precond_ctx,
                                    const double *b, double *x, const bp5_cg_params *prm, bp5_cg_result *res)
{
  PlainCG cg;
  cg.op = elasticity_op(coef, lambda, mu, ld, state);
  BP5_TRY(block_cg_workspace(mf, cg, precond != nullptr));
  cg.allreduce = false;
  cg.precond = precond; cg.precond_ctx = precond_ctx;
  return cg_solve_plain(mf, cg, b, x, prm, res);
}
extern "C" int bp5_cg_solve_hyperelasticity(bp5_mf *mf, const double *coef, const double *state, double lambda, double mu, size_t ld, bp5_vmult_fn precond,
                                            void *precond_ctx, const double *b, double *x, const bp5_cg_params *prm, bp5_cg_result *res)
{
  BP5_TRY(cg_solve_hyperelasticity_check(mf, coef, state, lambda, mu, ld, b, x, prm, res));
  HIP_TRY(hipSetDevice(mf->device));
  return cg_solve_hyperelasticity(mf, coef, state, lambda, mu, ld, precond, precond_ctx, b, x, prm, res);
}

// Newton's method with backtracking (bp5.h).  Every vector step is an existing kernel, block by block; one norm per residual
extern "C" int bp5_hyperelasticity_newton(bp5_mf *mf, const double *coef, double *state, double lambda, double mu, size_t ld, bp5_vmult_fn precond, void *precond_ctx,
                                          const double *f_ext, double *u, const bp5_newton_params *prm, bp5_newton_result *res)
{
  if (!prm || !res) return hyperelasticity_refuse(BP5_ERR_INVALID, "null argument");
  if (prm->max_newton < 0 || prm->max_backtracks < 0) return hyperelasticity_refuse(BP5_ERR_INVALID, "max_newton < 0 or max_backtracks < 0");
  if (!(prm->abs_tol >= 0.0) || !(prm->rel_tol >= 0.0) || !(prm->cg_rel_tol >= 0.0) || !std::isfinite(prm->abs_tol + prm->rel_tol + prm->cg_rel_tol))
    return hyperelasticity_refuse(BP5_ERR_INVALID, "tolerances must be finite and >= 0");
  bp5_cg_result cr;
  BP5_TRY(cg_solve_hyperelasticity_check(mf, coef, state, lambda, mu, ld, f_ext, u, &prm->cg, &cr));
  HIP_TRY(hipSetDevice(mf->device));
  const size_t nl = mf->n_local();
  BP5_TRY(grown_workspace(mf->wsn_base, mf->wsn_cap, 9 * ld, mf->stream)); // (zero-filled: the padding of the three work vectors)
  double *delta = mf->wsn_base, *trial = delta + 3 * ld, *r = trial + 3 * ld;
  // r = f_ext - F_int(v) with zeros on the Dirichlet rows, and its stacked l2 norm over the owned entries
  auto residual = [&](const double *v, double *norm) -> int {
    BP5_TRY(hyperelasticity_residual(mf, coef, state, lambda, mu, ld, v, r, true));
    for (int c = 0; c < 3; ++c) BP5_TRY(bp5_vec_sadd(mf, r + (size_t)c * ld, -1.0, 1.0, f_ext + (size_t)c * ld, nl));
    for (int c = 0; c < 3; ++c) BP5_TRY(bp5_set_constrained(mf, 0.0, r + (size_t)c * ld));
    const dim3 grid(std::min(stream_grid(mf->n_owned, 2), PARTIAL_STRIDE / 3), 3);
    BP5_TRY(blockvec_dot(mf->stream, grid, r, r, mf->n_owned, ld, mf->d_partials));
    double s = 0.0;
    BP5_TRY(reduce_to_host(mf, (int)grid.x * 3, &s));
    *norm = sqrt(s);
    return BP5_OK;
  };
  auto copy_blocks = [&](double *dst, const double *src) -> int { // (block by block: the padding of u is neither read nor written)
    for (int c = 0; c < 3; ++c) HIP_TRY(hipMemcpyAsync(dst + (size_t)c * ld, src + (size_t)c * ld, nl * sizeof(double), hipMemcpyDeviceToDevice, mf->stream));
    return BP5_OK;
  };
  memset(res, 0, sizeof(*res));
  auto finish = [&](int status) { res->status = status; return status; };
  auto record = [&](double norm) { if (res->newton_iterations < 32) res->residual_history[res->newton_iterations] = norm; };
  double rn = 0.0;
  BP5_TRY(residual(u, &rn));
  record(rn);
  if (!std::isfinite(rn)) return finish(hyperelasticity_refuse(BP5_ERR_BREAKDOWN, "Newton: the residual of the start vector is not finite (J <= 0 at a quadrature point?)"));
  const double tol = std::max(prm->abs_tol, prm->rel_tol * rn);
  for (int k = 0; k < prm->max_newton; ++k) {
    if (rn <= tol) return finish(BP5_OK);
    bp5_cg_params cp = prm->cg;
    cp.abs_tol = prm->cg_rel_tol * rn;
    const int st = cg_solve_hyperelasticity(mf, coef, state, lambda, mu, ld, precond, precond_ctx, r, delta, &cp, &cr);
    res->total_cg_iterations += cr.iterations;
    if (st != BP5_OK) return finish(st);
    double alpha = 1.0, rt = 0.0;
    for (int bt = 0;; ++bt) {
      BP5_TRY(copy_blocks(trial, u));
      for (int c = 0; c < 3; ++c) BP5_TRY(bp5_vec_axpy(mf, trial + (size_t)c * ld, alpha, delta + (size_t)c * ld, nl));
      BP5_TRY(residual(trial, &rt));
      if (std::isfinite(rt) && rt < rn) break;
      if (bt == prm->max_backtracks) {
        BP5_TRY(residual(u, &rt)); // the state of the last accepted iterate
        return finish(hyperelasticity_refuse(BP5_ERR_BREAKDOWN, "Newton: backtracking exhausted, the residual norm does not decrease"));
      }
      alpha *= 0.5;
      ++res->backtracks;
    }
    BP5_TRY(copy_blocks(u, trial));
    rn = rt;
    ++res->newton_iterations;
    record(rn);
  }
  HIP_TRY(hipStreamSynchronize(mf->stream));
  if (rn <= tol) return finish(BP5_OK);
  return finish(hyperelasticity_refuse(BP5_ERR_NO_CONVERGENCE, "Newton: max_newton steps without reaching the tolerance"));
}

// cg.solve(A, x, b, P) for a P given by its vmult (deal.II SolverCG, bp5/step-64.cu:446-453): the plain recurrence with z = P g in place of D g
extern "C" int bp5_cg_solve_preconditioned(bp5_mf *mf, const double *coef, bp5_vmult_fn vmult, void *ctx, bp5_vmult_fn precond, void *precond_ctx,
                                           const double *b, double *x, const bp5_cg_params *prm, bp5_cg_result *res)
{
  if (!mf || (!vmult && !coef && mf->geometry_mode == BP5_GEOM_MERGED6) || !precond || !b || !x) return fail(BP5_ERR_INVALID, "null argument");
  BP5_TRY(cg_preamble(plainly_refuse, prm, res, b, x, "vectors must be 16-byte aligned",
                      "a general preconditioner needs BP5_CG_PLAIN (SolverCGFullMerge takes a diagonal only)"));
  HIP_TRY(hipSetDevice(mf->device));
  BP5_TRY(ensure_ws(mf));
  if (!mf->ws_z) {
    HIP_TRY(hipMalloc((void **)&mf->ws_z, std::max<size_t>(mf->n_local(), 2) * sizeof(double)));
    HIP_TRY(hipMemsetAsync(mf->ws_z, 0, std::max<size_t>(mf->n_local(), 2) * sizeof(double), mf->stream));
  }
  PlainCG cg;
  cg.g = mf->ws_g; cg.d = mf->ws_d; cg.h = mf->ws_h;
  cg.op = scalar_op(coef, vmult, ctx);
  cg.precond = precond; cg.precond_ctx = precond_ctx; cg.z = mf->ws_z;
  return cg_solve_plain(mf, cg, b, x, prm, res);
}

// ------------------------------------------------------------------------------------ PreconditionChebyshev
struct bp5_chebyshev {
  bp5_mf *mf = nullptr;
  // the operator: native, a callback, or (bp5_elasticity_chebyshev_create) the coupled elasticity one -- then every vector is three blocks op.ld
  // apart, w and t too, and inv_diag a BLOCK inverse diagonal (blocks op.ld apart)
  LinearOp op;
  const double *inv_diag = nullptr;
  int degree = 1;
  double min_est = 0.0, max_est = 0.0, min_used = 0.0, max_used = 0.0, theta = 1.0, delta = 0.0;
  int cg_its = 0;
  std::vector<double> f1, f2; // step k = 1 .. degree-1
  double *w = nullptr, *t = nullptr; // the other iterate and t = A x_k: owned + ghost each (one allocation)
};

// t = A x in overwrite mode (zero_dst = 1 and the Dirichlet copy); the distributed apply when there are neighbours
static int cheb_apply(bp5_chebyshev *c, double *x, double *t)
{
  bp5_mf *mf = c->mf;
  const LinearOp &A = c->op;
  if (A.block()) { // (the arguments were checked when the handle was made)
    ApplyProfile none{mf, false};
    HIP_TRY(hipSetDevice(mf->device));
    return block_op_apply(mf, A, x, t, none);
  }
  if (A.user) {
    const int st = A.user(A.user_ctx, t, x);
    return st == BP5_OK ? BP5_OK : fail(st, "the operator's vmult callback reported a failure");
  }
  if (mf->has_neighbors()) return bp5_apply_distributed(mf, A.coef, x, t, 1);
  return bp5_apply(mf, A.coef, x, t, 1);
}

// one Chebyshev step kernel (blockvec/bp5_blockvec.hip): FORM as chebyshev_step_kernel, the streaming policy (BP5_TUNE_UPDATE_NT) and the flat launch
// shape from the handle.  Elasticity: the three blocks, and those of the block inverse diagonal, ld apart in one launch
template <int FORM>
static int cheb_step_launch(bp5_chebyshev *c, double *x_new, const double *x, const double *x_old, const double *src, double f1, double f2)
{
  bp5_mf *mf = c->mf;
  const size_t n = mf->n_owned;
  if (!n) return BP5_OK;
  const unsigned grid_x = stream_grid_flat(mf, n, 2);
  return blockvec_chebyshev_step(mf->stream, FORM, grid_x, c->op.n_components, mf->tune[BP5_TUNE_UPDATE_NT] != 0, x_new, x, x_old, src, c->t, c->inv_diag, n, c->op.ld,
                                 c->op.ld, f1, f2);
}

// op: a scalar operator, or the elasticity one (bp5_elasticity_chebyshev_create, which has checked handle, layout and parameters) on three-block
// vectors op.ld apart, inv_diag then a block inverse diagonal
static int chebyshev_create_impl(bp5_mf *mf, const LinearOp &op, const double *inv_diag, const bp5_chebyshev_params *prm, bp5_chebyshev **out)
{
  const size_t el_ld = op.ld;
  if (!mf || !prm || !out || (!op.user && !op.coef && mf->geometry_mode == BP5_GEOM_MERGED6)) return fail(BP5_ERR_INVALID, "null argument");
  *out = nullptr;
  if (prm->degree < 1) return fail(BP5_ERR_INVALID, "Chebyshev degree < 1");
  const bool given = prm->max_eigenvalue > 0.0 && prm->min_eigenvalue > 0.0;
  if (given && !(prm->min_eigenvalue < prm->max_eigenvalue)) return fail(BP5_ERR_INVALID, "Chebyshev bounds: need 0 < min_eigenvalue < max_eigenvalue");
  if (!given && prm->eig_cg_n_iterations < 1) return fail(BP5_ERR_INVALID, "eig_cg_n_iterations < 1 and no bounds given");
  if (inv_diag && !aligned16(inv_diag)) return fail(BP5_ERR_INVALID, "vectors must be 16-byte aligned");
  HIP_TRY(hipSetDevice(mf->device));
  std::unique_ptr<bp5_chebyshev> c(new bp5_chebyshev);
  c->mf = mf; c->op = op; c->inv_diag = inv_diag; c->degree = prm->degree;
  const size_t nb = (std::max<size_t>(el_ld ? 3 * el_ld : mf->n_local(), 2) * sizeof(double) + 4095) / 4096 * 4096;
  char *base = nullptr;
  HIP_TRY(hipMalloc((void **)&base, 2 * nb));
  c->w = (double *)base;
  c->t = (double *)(base + nb);
  struct Free { bp5_chebyshev *c; bool keep = false; ~Free() { if (!keep && c->w) hipFree(c->w); } } guard{c.get()};
  HIP_TRY(hipMemsetAsync(base, 0, 2 * nb, mf->stream));
  if (given) {
    c->min_used = prm->min_eigenvalue;
    c->max_used = prm->max_eigenvalue;
  } else {
    // Jacobi-PCG on A x = v (x_0 = 0) with the alpha / beta history on the device; one copy to the host at the end
    const int m = prm->eig_cg_n_iterations;
    const int n_blocks = op.n_components;
    std::vector<double> v(std::max<size_t>(mf->n_owned, 1) * n_blocks, 0.0);
    for (int cb = 0; cb < n_blocks; ++cb)
      for (uint32_t i = 0; i < mf->n_owned; ++i) {
        const uint64_t id = prm->start_ids_host ? prm->start_ids_host[i] : i;
        // block vectors: v_c[i] = ((3 id + c) mod 11) - 5, the scalar start vector of the stacked numbering 3 id + c
        v[(size_t)cb * mf->n_owned + i] = (double)(int)((el_ld ? 3u * (id % 11u) + (unsigned)cb : id) % 11u) - 5.0;
      }
    double *vb = c->w, *xs = c->t, *hist = nullptr;
    double vnorm = 0.0;
    for (int cb = 0; cb < n_blocks; ++cb) {
      double *vbc = vb + (size_t)cb * el_ld;
      HIP_TRY(hipMemcpyAsync(vbc, v.data() + (size_t)cb * mf->n_owned, mf->n_owned * sizeof(double), hipMemcpyHostToDevice, mf->stream));
      BP5_TRY(bp5_set_constrained(mf, 0.0, vbc));
      double nb_ = 0.0;
      BP5_TRY(bp5_vec_l2_norm(mf, vbc, mf->n_owned, &nb_));
      vnorm = n_blocks == 1 ? nb_ : std::sqrt(vnorm * vnorm + nb_ * nb_); // (the stacked norm; one block: the value as it is)
    }
    HIP_TRY(hipMalloc((void **)&hist, 2 * (size_t)m * sizeof(double)));
    struct FreeHist { double *h; ~FreeHist() { hipFree(h); } } hguard{hist};
    HIP_TRY(hipMemsetAsync(hist, 0, 2 * (size_t)m * sizeof(double), mf->stream));
    bp5_cg_params cp{};
    cp.variant = BP5_CG_PLAIN; cp.max_iter = m; cp.abs_tol = 1e-5 * vnorm; cp.check_every = 0; cp.profile = 0;
    bp5_cg_result cr{};
    if (op.block()) BP5_TRY(cg_solve_elasticity_impl(mf, op.coef, op.lambda, op.mu, el_ld, inv_diag, nullptr, nullptr, vb, xs, &cp, &cr, hist, m));
    else BP5_TRY(cg_solve_impl(mf, op.coef, op.user, op.user_ctx, inv_diag, vb, xs, &cp, &cr, hist, m));
    std::vector<double> h(2 * (size_t)m);
    HIP_TRY(hipMemcpy(h.data(), hist, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    const int k = cr.iterations;
    if (k < 1) return fail(BP5_ERR_INVALID, "Chebyshev estimate: the start vector is zero (no unconstrained DoF)");
    std::vector<double> T(k), E(std::max(k - 1, 1)), eig(k);
    for (int j = 0; j < k; ++j) {
      T[j] = 1.0 / h[2 * j] + (j > 0 ? h[2 * j - 1] / h[2 * j - 2] : 0.0);
      if (j + 1 < k) E[j] = std::sqrt(h[2 * j + 1]) / h[2 * j];
    }
    BP5_TRY(bp5_tridiagonal_eigenvalues(k, T.data(), E.data(), eig.data()));
    c->cg_its = k;
    c->min_est = eig.front();
    c->max_est = eig.back();
    c->max_used = 1.2 * c->max_est;
    c->min_used = prm->smoothing_range > 1.0 ? c->max_used / prm->smoothing_range : std::min(0.9 * c->max_used, c->min_est);
  }
  if (!(c->max_used > c->min_used) || !(c->min_used > 0.0)) return fail(BP5_ERR_BREAKDOWN, "Chebyshev: degenerate eigenvalue bounds");
  c->theta = 0.5 * (c->max_used + c->min_used);
  c->delta = 0.5 * (c->max_used - c->min_used);
  double rho = c->delta / c->theta;
  for (int k = 1; k < c->degree; ++k) {
    const double rho_new = 1.0 / (2.0 * c->theta / c->delta - rho);
    c->f1.push_back(rho_new * rho);
    c->f2.push_back(2.0 * rho_new / c->delta);
    rho = rho_new;
  }
  HIP_TRY(hipStreamSynchronize(mf->stream));
  guard.keep = true;
  *out = c.release();
  return BP5_OK;
}
extern "C" int bp5_chebyshev_create(bp5_mf *mf, const double *coef, bp5_vmult_fn vmult, void *ctx, const double *inv_diag,
                                    const bp5_chebyshev_params *prm, bp5_chebyshev **out)
{
  return chebyshev_create_impl(mf, scalar_op(coef, vmult, ctx), inv_diag, prm, out);
}
// PreconditionChebyshev for the elasticity operator: the same handle type, every vector three blocks ld apart, the estimate Jacobi-PCG on the
// stacked system (one Krylov space) with the block inverse diagonal
extern "C" int bp5_elasticity_chebyshev_create(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, const double *inv_diag,
                                               const bp5_chebyshev_params *prm, bp5_chebyshev **out)
{
  if (!prm || !out) return elasticity_refuse(BP5_ERR_INVALID, "null argument");
  *out = nullptr;
  if (inv_diag && !aligned16(inv_diag)) return elasticity_refuse(BP5_ERR_INVALID, "block vectors must be 16-byte aligned");
  if (inv_diag) BP5_TRY(elasticity_check(mf, coef, lambda, mu, ld, inv_diag, nullptr, false));
  else BP5_TRY(elasticity_check_no_vector(mf, coef, lambda, mu, ld));
  return chebyshev_create_impl(mf, elasticity_op(coef, lambda, mu, ld), inv_diag, prm, out);
}

extern "C" int bp5_chebyshev_eigenvalues(const bp5_chebyshev *c, double *min_est, double *max_est, double *min_used, double *max_used, int *cg_its)
{
  if (!c) return fail(BP5_ERR_INVALID, "null argument");
  if (min_est) *min_est = c->min_est;
  if (max_est) *max_est = c->max_est;
  if (min_used) *min_used = c->min_used;
  if (max_used) *max_used = c->max_used;
  if (cg_its) *cg_its = c->cg_its;
  return BP5_OK;
}

// dst = P src: x_1 = D^-1 src / theta, then degree-1 times t = A x_k and one step kernel.  x_{k+1} lands in x_{k-1}'s buffer: the odd
// iterates live in one buffer, the even ones in the other, chosen so that x_degree is dst
extern "C" int bp5_chebyshev_vmult(void *cv, double *dst, double *src)
{
  bp5_chebyshev *c = static_cast<bp5_chebyshev *>(cv);
  if (!c || !dst || !src) return fail(BP5_ERR_INVALID, "null argument");
  if (!aligned16(dst) || !aligned16(src)) return fail(BP5_ERR_INVALID, "vectors must be 16-byte aligned");
  if (dst == src) return fail(BP5_ERR_INVALID, "Chebyshev vmult: dst and src must differ");
  double *odd = (c->degree & 1) ? dst : c->w, *even = (c->degree & 1) ? c->w : dst;
  BP5_TRY(cheb_step_launch<0>(c, odd, nullptr, nullptr, src, 0.0, 1.0 / c->theta));
  for (int k = 1; k < c->degree; ++k) {
    double *xk = (k & 1) ? odd : even, *xo = (k & 1) ? even : odd; // x_k, and x_{k-1} (== x_0 = 0 for k = 1), which receives x_{k+1}
    BP5_TRY(cheb_apply(c, xk, c->t));
    if (k == 1) BP5_TRY(cheb_step_launch<2>(c, xo, xk, nullptr, src, c->f1[0], c->f2[0]));
    else BP5_TRY(cheb_step_launch<1>(c, xo, xk, xo, src, c->f1[k - 1], c->f2[k - 1]));
  }
  return BP5_OK;
}

// smoother: x_0 = dst; x_1 = x_0 + D^-1 (src - A x_0) / theta; then the recurrence (degree operator applications).  Even degree: x_0 stays
// in dst and x_degree lands there; odd degree: x_0 is copied to the work vector first
extern "C" int bp5_chebyshev_step(bp5_chebyshev *c, double *dst, double *src)
{
  if (!c || !dst || !src) return fail(BP5_ERR_INVALID, "null argument");
  if (!aligned16(dst) || !aligned16(src)) return fail(BP5_ERR_INVALID, "vectors must be 16-byte aligned");
  if (dst == src) return fail(BP5_ERR_INVALID, "Chebyshev step: dst and src must differ");
  bp5_mf *mf = c->mf;
  double *a = dst, *b = c->w; // a: x_0, x_2, ...   b: x_1, x_3, ...
  if (c->degree & 1) {
    for (int cb = 0; cb < c->op.n_components; ++cb) // (block by block: the padding of dst is not read)
      HIP_TRY(hipMemcpyAsync(c->w + (size_t)cb * c->op.ld, dst + (size_t)cb * c->op.ld, mf->n_owned * sizeof(double), hipMemcpyDeviceToDevice, mf->stream));
    a = c->w; b = dst;
  }
  BP5_TRY(cheb_apply(c, a, c->t));
  BP5_TRY(cheb_step_launch<3>(c, b, a, nullptr, src, 0.0, 1.0 / c->theta));
  for (int k = 1; k < c->degree; ++k) {
    double *xk = (k & 1) ? b : a, *xo = (k & 1) ? a : b;
    BP5_TRY(cheb_apply(c, xk, c->t));
    BP5_TRY(cheb_step_launch<1>(c, xo, xk, xo, src, c->f1[k - 1], c->f2[k - 1]));
  }
  return BP5_OK;
}

extern "C" int bp5_chebyshev_destroy(bp5_chebyshev *c)
{
  if (!c) return BP5_OK;
  hipSetDevice(c->mf->device);
  hipStreamSynchronize(c->mf->stream);
  if (c->w) hipFree(c->w);
  delete c;
  return BP5_OK;
}

// ------------------------------------------------------------------------------------ p-multigrid transfer (MGTwoLevelTransfer)
struct bp5_mg_transfer {
  bp5_mf *fine = nullptr, *coarse = nullptr;
  int pf = 0, pc = 0;
  bool geometric = false;                                      // h-transfer (pf == pc): parent cells, M_0 and M_1
  double *d_M = nullptr, *d_w = nullptr, *d_slots = nullptr;   // M [(pf+1)(pc+1)] (geometric: [2][(p+1)^2]), fine weights [n_local fine], slots [fine n_cells (pc+1)^3]
  uint32_t *d_cidx = nullptr, *d_wmask = nullptr;             // coarse indices per cell (MG_NO_DOF: Dirichlet; geometric: per COARSE cell), writer masks per fine cell
  uint32_t *d_coff = nullptr, *d_cslot = nullptr;             // per coarse local DoF: its slots, ascending
  uint32_t *d_pcode = nullptr;                                 // geometric: per fine cell parent << 3 | child
  // block vectors (bp5_mg_transfer_*_components): slots [component][cell][(pc+1)^3] for slots_components > 1 components, an array of its own that
  // bp5_elasticity_mg_create reserves at setup (the entry points grow it when a call brings more components than any before)
  double *d_slots_c = nullptr;
  int slots_components = 0;
  size_t slot_stride() const { return (size_t)fine->n_cells * coarse->n3; }
  std::vector<void *> device_arrays() const { return {d_M, d_w, d_slots, d_cidx, d_wmask, d_coff, d_cslot, d_pcode, d_slots_c}; }
};

// the CSR of each coarse local DoF's slots, ascending (= cell order): slot_dof[s] the coarse DoF slot s adds to (MG_NO_DOF: none)
static int mg_upload_slot_csr(bp5_mg_transfer *t, const std::vector<uint32_t> &slot_dof)
{
  const size_t nlc = t->coarse->n_local();
  std::vector<uint32_t> coff(nlc + 1, 0u);
  for (uint32_t g : slot_dof)
    if (g != MG_NO_DOF) ++coff[g + 1];
  for (size_t g = 0; g < nlc; ++g) coff[g + 1] += coff[g];
  std::vector<uint32_t> cslot(coff[nlc]), fill(coff.begin(), coff.end() - 1);
  for (size_t s = 0; s < slot_dof.size(); ++s)
    if (slot_dof[s] != MG_NO_DOF) cslot[fill[slot_dof[s]]++] = (uint32_t)s;
  BP5_TRY(upload(&t->d_coff, coff.data(), coff.size()));
  BP5_TRY(upload(&t->d_cslot, cslot.data(), cslot.size()));
  return BP5_OK;
}

// fine side of either transfer: writer masks (the first cell in handle order that holds an owned fine DoF writes it), the weights w = 1 /
// (cells that hold the DoF, all ranks), the slot array; synchronises the stream
static int mg_setup_fine_side(bp5_mg_transfer *t)
{
  bp5_mf *fine = t->fine;
  const int f3 = fine->n3, c3 = t->coarse->n3;
  const uint32_t ncell = fine->n_cells;
  const size_t nlf = fine->n_local();
  const int words = (f3 + 31) / 32;
  std::vector<uint32_t> wmask((size_t)ncell * words, 0u);
  std::vector<uint8_t> written(fine->n_owned, 0);
  std::vector<double> count(std::max<size_t>(nlf, 1), 0.0);
  for (uint32_t c = 0; c < ncell; ++c)
    for (int r = 0; r < f3; ++r) {
      const uint32_t g = fine->h_l2g[(size_t)c * f3 + r];
      count[g] += 1.0;
      if (g < fine->n_owned && !written[g]) {
        written[g] = 1;
        wmask[(size_t)c * words + r / 32] |= 1u << (r & 31);
      }
    }
  for (uint32_t g = 0; g < fine->n_owned; ++g)
    if (!written[g]) return fail(BP5_ERR_INVALID, "multigrid transfer: an owned fine DoF lies in none of the rank's cells");
  BP5_TRY(upload(&t->d_wmask, wmask.data(), wmask.size()));
  BP5_TRY(upload(&t->d_w, count.data(), count.size()));
  if (fine->has_neighbors()) { // the counts of all ranks: ghost counts to their owners, the totals back to the ghosts
    BP5_TRY(bp5_halo_scatter_add(fine, t->d_w));
    BP5_TRY(bp5_halo_gather(fine, t->d_w));
  }
  if (nlf) {
    hipLaunchKernelGGL(reciprocal_kernel, dim3((nlf + 255) / 256), dim3(256), 0, fine->stream, t->d_w, nlf);
    KERNEL_CHECK();
  }
  HIP_TRY(hipMalloc((void **)&t->d_slots, std::max<size_t>((size_t)ncell * c3, 1) * sizeof(double)));
  HIP_TRY(hipStreamSynchronize(fine->stream));
  return BP5_OK;
}

// frees the device arrays of a transfer that was not handed out
struct MgTransferGuard {
  bp5_mg_transfer *t;
  bool keep = false;
  ~MgTransferGuard() { if (!keep) for (void *p : t->device_arrays()) if (p) hipFree(p); }
};

extern "C" int bp5_mg_transfer_create(bp5_mf *fine, bp5_mf *coarse, bp5_mg_transfer **out)
{
  if (!fine || !coarse || !out) return fail(BP5_ERR_INVALID, "null argument");
  *out = nullptr;
  if (fine->degree < 2 || coarse->degree != std::max(1, fine->degree / 2))
    return fail(BP5_ERR_INVALID, "multigrid transfer: need fine degree >= 2 and coarse degree max(1, fine degree / 2)");
  if (fine->d_hang_mask || coarse->d_hang_mask || fine->has_hanging || coarse->has_hanging)
    return fail(BP5_ERR_INVALID, "multigrid transfer: hanging-node meshes (constraint_mask) are not supported");
  if (fine->n_cells != coarse->n_cells) return fail(BP5_ERR_INVALID, "multigrid transfer: the handles have different cells");
  if (fine->comm != coarse->comm) return fail(BP5_ERR_INVALID, "multigrid transfer: the handles have different communicators");
  if (fine->stream != coarse->stream || fine->device != coarse->device) return fail(BP5_ERR_INVALID, "multigrid transfer: the handles have different streams");
  const int nf = fine->n, nc = coarse->n, f3 = fine->n3, c3 = coarse->n3;
  const uint32_t ncell = fine->n_cells;
  const size_t nlf = fine->n_local(), nlc = coarse->n_local();
  // same cells: the corner DoFs of the cells correspond one to one
  {
    std::vector<uint32_t> f2c(nlf, MG_NO_DOF), c2f(nlc, MG_NO_DOF);
    for (uint32_t c = 0; c < ncell; ++c)
      for (int k = 0; k < 2; ++k)
        for (int j = 0; j < 2; ++j)
          for (int i = 0; i < 2; ++i) {
            const uint32_t gf = fine->h_l2g[(size_t)c * f3 + i * (nf - 1) + nf * (j * (nf - 1) + nf * k * (nf - 1))];
            const uint32_t gc = coarse->h_l2g[(size_t)c * c3 + i * (nc - 1) + nc * (j * (nc - 1) + nc * k * (nc - 1))];
            if ((f2c[gf] != MG_NO_DOF && f2c[gf] != gc) || (c2f[gc] != MG_NO_DOF && c2f[gc] != gf))
              return fail(BP5_ERR_INVALID, "multigrid transfer: the handles do not have the same cells (corner DoFs differ)");
            f2c[gf] = gc;
            c2f[gc] = gf;
          }
  }
  HIP_TRY(hipSetDevice(fine->device));
  // ... in the same local frame: a consistent pairing does not say so (a column of cells turned about its axis in one handle pairs up too), the
  // geometry does -- corner (i, j, k) of every cell has the same coordinates in both handles (to 1e-12 of the cell's size)
  {
    std::vector<double> xf(nlf * 3), xc(nlc * 3);
    HIP_TRY(hipStreamSynchronize(fine->stream));
    if (!xf.empty()) HIP_TRY(hipMemcpy(xf.data(), fine->d_coords, xf.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (!xc.empty()) HIP_TRY(hipMemcpy(xc.data(), coarse->d_coords, xc.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (uint32_t c = 0; c < ncell; ++c) {
      const uint32_t *lf = &fine->h_l2g[(size_t)c * f3], *lc = &coarse->h_l2g[(size_t)c * c3];
      const double *a = &xc[3 * (size_t)lc[0]], *z = &xc[3 * (size_t)lc[c3 - 1]];
      const double size = std::sqrt((z[0] - a[0]) * (z[0] - a[0]) + (z[1] - a[1]) * (z[1] - a[1]) + (z[2] - a[2]) * (z[2] - a[2]));
      for (int q = 0; q < 8; ++q) {
        const int i = q & 1, j = (q >> 1) & 1, k = q >> 2;
        const double *Xf = &xf[3 * (size_t)lf[i * (nf - 1) + nf * (j * (nf - 1) + nf * k * (nf - 1))]];
        const double *Xc = &xc[3 * (size_t)lc[i * (nc - 1) + nc * (j * (nc - 1) + nc * k * (nc - 1))]];
        for (int e = 0; e < 3; ++e)
          if (!(std::fabs(Xf[e] - Xc[e]) <= 1e-12 * size))
            return fail(BP5_ERR_INVALID, "multigrid transfer: cell " + std::to_string(c) + " does not sit in the same local frame in the two handles (the coordinates of its corners differ)");
      }
    }
  }
  std::unique_ptr<bp5_mg_transfer> t(new bp5_mg_transfer);
  MgTransferGuard guard{t.get()};
  t->fine = fine; t->coarse = coarse; t->pf = fine->degree; t->pc = coarse->degree;
  // M from the product formula on the FE_Q nodes; end rows exact unit vectors
  std::vector<double> xf(nf), xc(nc), M((size_t)nf * nc);
  BP5_TRY(bp5_shape_tables(t->pf, BP5_QUAD_GAUSS, xf.data(), nullptr, nullptr, nullptr, nullptr));
  BP5_TRY(bp5_shape_tables(t->pc, BP5_QUAD_GAUSS, xc.data(), nullptr, nullptr, nullptr, nullptr));
  for (int a = 0; a < nf; ++a)
    for (int b = 0; b < nc; ++b) {
      double v = 1.0;
      for (int m = 0; m < nc; ++m)
        if (m != b) v *= (xf[a] - xc[m]) / (xc[b] - xc[m]);
      M[(size_t)a * nc + b] = v;
    }
  for (int b = 0; b < nc; ++b) {
    M[b] = b == 0 ? 1.0 : 0.0;
    M[(size_t)(nf - 1) * nc + b] = b == nc - 1 ? 1.0 : 0.0;
  }
  BP5_TRY(upload(&t->d_M, M.data(), M.size()));
  // coarse indices (Dirichlet DoFs: MG_NO_DOF) and the CSR of each coarse DoF's slots, in cell order
  std::vector<uint32_t> cidx(coarse->h_l2g);
  for (size_t s = 0; s < cidx.size(); ++s)
    if (coarse->h_constrained[cidx[s]]) cidx[s] = MG_NO_DOF;
  if ((uint64_t)ncell * c3 >= MG_NO_DOF) return fail(BP5_ERR_INVALID, "multigrid transfer: too many coarse cell entries for 32-bit slots");
  BP5_TRY(upload(&t->d_cidx, cidx.data(), cidx.size()));
  BP5_TRY(mg_upload_slot_csr(t.get(), cidx));
  BP5_TRY(mg_setup_fine_side(t.get()));
  guard.keep = true;
  *out = t.release();
  return BP5_OK;
}

extern "C" int bp5_mg_transfer_create_geometric(bp5_mf *fine, bp5_mf *coarse, const uint32_t *parent, const uint8_t *child, bp5_mg_transfer **out)
{
  if (!fine || !coarse || !out || (fine->n_cells && (!parent || !child))) return fail(BP5_ERR_INVALID, "null argument");
  *out = nullptr;
  if (fine->degree != coarse->degree || fine->degree < 1 || fine->degree > 4)
    return fail(BP5_ERR_INVALID, "geometric multigrid transfer: need equal degrees in 1..4");
  if (fine->d_hang_mask || coarse->d_hang_mask || fine->has_hanging || coarse->has_hanging)
    return fail(BP5_ERR_INVALID, "geometric multigrid transfer: hanging-node meshes (constraint_mask) are not supported");
  if (fine->comm != coarse->comm) return fail(BP5_ERR_INVALID, "geometric multigrid transfer: the handles have different communicators");
  if (fine->stream != coarse->stream || fine->device != coarse->device)
    return fail(BP5_ERR_INVALID, "geometric multigrid transfer: the handles have different streams");
  const int n = fine->n, p = fine->degree, n3 = fine->n3;
  const uint32_t nf = fine->n_cells, nc = coarse->n_cells;
  if ((uint64_t)nf != 8ull * nc) return fail(BP5_ERR_INVALID, "geometric multigrid transfer: the fine handle must have 8 cells per coarse cell");
  if (nc >= (1u << 29)) return fail(BP5_ERR_INVALID, "geometric multigrid transfer: too many coarse cells for 29-bit parent indices");
  if ((uint64_t)nf * n3 >= MG_NO_DOF) return fail(BP5_ERR_INVALID, "geometric multigrid transfer: too many fine cell entries for 32-bit slots");
  // every coarse cell: 8 children with distinct child codes
  std::vector<uint8_t> seen(nc, 0);
  for (uint32_t k = 0; k < nf; ++k) {
    if (parent[k] >= nc) return fail(BP5_ERR_INVALID, "geometric multigrid transfer: a parent index is not a local coarse cell");
    if (child[k] > 7) return fail(BP5_ERR_INVALID, "geometric multigrid transfer: a child code is not in 0..7");
    if (seen[parent[k]] & (1u << child[k])) return fail(BP5_ERR_INVALID, "geometric multigrid transfer: a coarse cell has two children with one child code");
    seen[parent[k]] |= (uint8_t)(1u << child[k]);
  }
  for (uint32_t c = 0; c < nc; ++c)
    if (seen[c] != 0xff) return fail(BP5_ERR_INVALID, "geometric multigrid transfer: a coarse cell does not have 8 children");
  // the map against the geometry: the corner a child shares with its parent has the parent's coordinates (to 1e-12 of the parent's size)
  {
    std::vector<double> xf(fine->n_local() * 3), xc(coarse->n_local() * 3);
    HIP_TRY(hipSetDevice(fine->device));
    HIP_TRY(hipStreamSynchronize(fine->stream));
    if (!xf.empty()) HIP_TRY(hipMemcpy(xf.data(), fine->d_coords, xf.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (!xc.empty()) HIP_TRY(hipMemcpy(xc.data(), coarse->d_coords, xc.size() * sizeof(double), hipMemcpyDeviceToHost));
    auto corner = [&](int ch) { return (ch & 1) * p + n * (((ch >> 1) & 1) * p + n * ((ch >> 2) & 1) * p); };
    for (uint32_t k = 0; k < nf; ++k) {
      const uint32_t *lc = &coarse->h_l2g[(size_t)parent[k] * n3];
      const double *a = &xc[3 * (size_t)lc[0]], *z = &xc[3 * (size_t)lc[n3 - 1]];
      const double size = std::sqrt((z[0] - a[0]) * (z[0] - a[0]) + (z[1] - a[1]) * (z[1] - a[1]) + (z[2] - a[2]) * (z[2] - a[2]));
      const double *Xf = &xf[3 * (size_t)fine->h_l2g[(size_t)k * n3 + corner(child[k])]], *Xc = &xc[3 * (size_t)lc[corner(child[k])]];
      for (int e = 0; e < 3; ++e)
        if (!(std::fabs(Xf[e] - Xc[e]) <= 1e-12 * size))
          return fail(BP5_ERR_INVALID, "geometric multigrid transfer: a fine cell's corner does not lie on its parent's corner (wrong parent map)");
    }
  }
  std::unique_ptr<bp5_mg_transfer> t(new bp5_mg_transfer);
  MgTransferGuard guard{t.get()};
  t->fine = fine; t->coarse = coarse; t->pf = t->pc = p; t->geometric = true;
  // M_s[a][b] = phi_b(xi_a / 2 + s / 2) from the product formula; rows on a coarse node exact unit rows
  std::vector<double> x(n), M(2 * (size_t)n * n);
  BP5_TRY(bp5_shape_tables(p, BP5_QUAD_GAUSS, x.data(), nullptr, nullptr, nullptr, nullptr));
  for (int sh = 0; sh < 2; ++sh)
    for (int a = 0; a < n; ++a) {
      const double xa = 0.5 * x[a] + 0.5 * sh;
      double *row = &M[((size_t)sh * n + a) * n];
      int hit = -1;
      for (int b = 0; b < n; ++b)
        if (std::fabs(xa - x[b]) < 1e-12) hit = b;
      for (int b = 0; b < n; ++b) {
        double v = 1.0;
        for (int m = 0; m < n; ++m)
          if (m != b) v *= (xa - x[m]) / (x[b] - x[m]);
        row[b] = hit < 0 ? v : (b == hit ? 1.0 : 0.0);
      }
    }
  BP5_TRY(upload(&t->d_M, M.data(), M.size()));
  // per coarse cell its Dirichlet-masked coarse indices; per fine cell parent << 3 | child; the slots of fine cell k add to its parent's DoFs
  std::vector<uint32_t> pidx(coarse->h_l2g), pcode(nf), slot_dof((size_t)nf * n3);
  for (uint32_t &g : pidx)
    if (coarse->h_constrained[g]) g = MG_NO_DOF;
  for (uint32_t k = 0; k < nf; ++k) {
    pcode[k] = parent[k] << 3 | child[k];
    std::copy(pidx.begin() + (size_t)parent[k] * n3, pidx.begin() + (size_t)(parent[k] + 1) * n3, slot_dof.begin() + (size_t)k * n3);
  }
  BP5_TRY(upload(&t->d_cidx, pidx.data(), pidx.size()));
  BP5_TRY(upload(&t->d_pcode, pcode.data(), pcode.size()));
  BP5_TRY(mg_upload_slot_csr(t.get(), slot_dof));
  BP5_TRY(mg_setup_fine_side(t.get()));
  guard.keep = true;
  *out = t.release();
  return BP5_OK;
}

// ---- the transfers on validated arguments, scalar vectors as n_components = 1 (blockvec/bp5_blockvec.hip): the lists are per scalar DoF and shared by
// all components.  The halo gather / scatter-add of handles with neighbours is reachable from the scalar entries only: mg_components_check refuses
// neighbours on the block entries
static MgComponentsArgs mg_components_args(const bp5_mg_transfer *t)
{
  MgComponentsArgs a;
  a.pf = t->pf; a.geometric = t->geometric;
  a.M = t->d_M; a.w = t->d_w; a.cidx = t->d_cidx; a.pcode = t->d_pcode; a.fidx = t->fine->d_l2g; a.wmask = t->d_wmask; a.coff = t->d_coff; a.cslot = t->d_cslot;
  a.n_cells = t->fine->n_cells; a.stream = t->fine->stream;
  return a;
}
// slots for n_components blocks: one component uses the scalar array
static int mg_reserve_slots(bp5_mg_transfer *t, int n_components, double **slots)
{
  if (n_components == 1) { *slots = t->d_slots; return BP5_OK; }
  if (t->slots_components < n_components) {
    HIP_TRY(hipSetDevice(t->fine->device));
    if (t->d_slots_c) { HIP_TRY(hipStreamSynchronize(t->fine->stream)); HIP_TRY(hipFree(t->d_slots_c)); t->d_slots_c = nullptr; t->slots_components = 0; }
    HIP_TRY(hipMalloc((void **)&t->d_slots_c, std::max<size_t>((size_t)n_components * t->slot_stride(), 1) * sizeof(double)));
    t->slots_components = n_components;
  }
  *slots = t->d_slots_c;
  return BP5_OK;
}
static int mg_components_check(const bp5_mg_transfer *t, int n_components, size_t ld_f, const double *vf, size_t ld_c, const double *vc)
{
  if (!t) return fail(BP5_ERR_INVALID, "null argument");
  BP5_TRY(components_layout_check(n_components, ld_f, vf, vc));
  if (ld_c & 1) return fail(BP5_ERR_INVALID, "block vectors: ld must be even (every block 16-byte aligned)");
  if (ld_f < t->fine->n_local() || ld_c < t->coarse->n_local()) return fail(BP5_ERR_INVALID, "block vectors: ld < n_owned + n_ghost");
  if (t->fine->has_neighbors() || t->coarse->has_neighbors())
    return fail(BP5_ERR_UNSUPPORTED, "multigrid transfer on block vectors: no halo exchange (handles with a communicator and neighbours)");
  return BP5_OK;
}
// dst_f += P src_c; with neighbours the coarse ghosts of src are gathered first
static int mg_prolongate(bp5_mg_transfer *t, int n_components, size_t ld_f, double *dst, size_t ld_c, double *src)
{
  HIP_TRY(hipSetDevice(t->fine->device));
  if (t->coarse->has_neighbors()) BP5_TRY(bp5_halo_gather(t->coarse, src));
  return blockvec_mg_prolongate(mg_components_args(t), n_components, ld_c, src, ld_f, dst);
}
// dst_c (+)= P^T (w (.) (b - tv)), tv == NULL: P^T (w (.) b); with neighbours the fine ghosts of b (and tv) are gathered first and the
// coarse ghost rows are sent to their owners
static int mg_restrict(bp5_mg_transfer *t, int n_components, size_t ld_c, double *dst, size_t ld_f, double *b, double *tv, bool add)
{
  HIP_TRY(hipSetDevice(t->fine->device));
  if (t->fine->has_neighbors()) {
    BP5_TRY(bp5_halo_gather(t->fine, b));
    if (tv) BP5_TRY(bp5_halo_gather(t->fine, tv));
  }
  double *slots = nullptr;
  BP5_TRY(mg_reserve_slots(t, n_components, &slots));
  const MgComponentsArgs a = mg_components_args(t);
  BP5_TRY(blockvec_mg_restrict(a, n_components, ld_f, b, tv, t->slot_stride(), slots));
  BP5_TRY(blockvec_mg_combine(a, n_components, slots, t->slot_stride(), t->coarse->n_owned, (uint32_t)t->coarse->n_local(), ld_c, dst, add));
  if (t->coarse->has_neighbors()) BP5_TRY(bp5_halo_scatter_add(t->coarse, dst));
  return BP5_OK;
}

extern "C" int bp5_mg_transfer_prolongate_add(bp5_mg_transfer *t, double *dst, double *src)
{
  if (!t || !dst || !src) return fail(BP5_ERR_INVALID, "null argument");
  return mg_prolongate(t, 1, 0, dst, 0, src);
}
extern "C" int bp5_mg_transfer_restrict_add(bp5_mg_transfer *t, double *dst, double *src)
{
  if (!t || !dst || !src) return fail(BP5_ERR_INVALID, "null argument");
  return mg_restrict(t, 1, 0, dst, 0, src, nullptr, true);
}
extern "C" int bp5_mg_transfer_prolongate_add_components(bp5_mg_transfer *t, int n_components, size_t ld_fine, double *dst_fine, size_t ld_coarse, double *src_coarse)
{
  BP5_TRY(mg_components_check(t, n_components, ld_fine, dst_fine, ld_coarse, src_coarse));
  return mg_prolongate(t, n_components, ld_fine, dst_fine, ld_coarse, src_coarse);
}
extern "C" int bp5_mg_transfer_restrict_add_components(bp5_mg_transfer *t, int n_components, size_t ld_coarse, double *dst_coarse, size_t ld_fine, double *src_fine)
{
  BP5_TRY(mg_components_check(t, n_components, ld_fine, src_fine, ld_coarse, dst_coarse));
  return mg_restrict(t, n_components, ld_coarse, dst_coarse, ld_fine, src_fine, nullptr, true);
}

extern "C" int bp5_mg_transfer_destroy(bp5_mg_transfer *t)
{
  if (!t) return BP5_OK;
  hipSetDevice(t->fine->device);
  hipStreamSynchronize(t->fine->stream);
  for (void *p : t->device_arrays())
    if (p) hipFree(p);
  delete t;
  return BP5_OK;
}

// ------------------------------------------------------------------------------------ PreconditionMG (V-cycle)
struct bp5_mg {
  int n_levels = 0;
  std::vector<bp5_mf *> mf;
  // per level: its operator on its own metric.  bp5_elasticity_mg_create: the elasticity one with (lambda, mu), every vector three blocks op[l].ld
  // apart (op[0].ld: the caller's; below: the level's n_local rounded up to even); scalar levels: ld = 0
  std::vector<LinearOp> op;
  std::vector<bp5_mg_transfer *> tr;
  std::vector<bp5_chebyshev *> cheb;          // [l]: the smoother; [n_levels - 1]: the coarse solver
  std::vector<double *> inv_diag, x, b, t;    // per level; x, b of levels >= 1 (level 0: the caller's dst, src); t of levels < n_levels - 1
  std::vector<void *> allocs;
};

extern "C" void bp5_mg_params_default(bp5_mg_params *p)
{
  if (!p) return;
  p->smoother_degree = 4;
  p->smoothing_range = 20.0;
  p->eig_cg_n_iterations = 10;
  p->coarse_degree = 60;
  p->coarse_range = 1000.0;
  p->coarse_eig_cg_n_iterations = 30;
  p->start_ids_host = nullptr;
}

extern "C" int bp5_mg_destroy(bp5_mg *mg)
{
  if (!mg) return BP5_OK;
  if (!mg->mf.empty()) {
    hipSetDevice(mg->mf[0]->device);
    hipStreamSynchronize(mg->mf[0]->stream);
  }
  for (bp5_chebyshev *c : mg->cheb) bp5_chebyshev_destroy(c);
  for (void *p : mg->allocs) hipFree(p);
  delete mg;
  return BP5_OK;
}

// what both constructors check first (null arguments -- in the words `null_words` --, *out = NULL, the Chebyshev degrees) ...
static int mg_arguments_check(Refuse refuse, const char *null_words, int n_levels, bp5_mf *const *mfs, const double *const *coefs,
                              bp5_mg_transfer *const *transfers, const bp5_mg_params *prm, bp5_mg **out)
{
  if (n_levels < 1 || !mfs || !coefs || !prm || !out || (n_levels > 1 && !transfers)) return refuse(BP5_ERR_INVALID, null_words);
  *out = nullptr;
  if (prm->smoother_degree < 1 || prm->coarse_degree < 1) return refuse(BP5_ERR_INVALID, "multigrid: Chebyshev degrees must be >= 1");
  return BP5_OK;
}
// ... and last
static int mg_transfers_check(Refuse refuse, int n_levels, bp5_mf *const *mfs, bp5_mg_transfer *const *transfers)
{
  for (int l = 0; l + 1 < n_levels; ++l)
    if (!transfers[l] || transfers[l]->fine != mfs[l] || transfers[l]->coarse != mfs[l + 1])
      return refuse(BP5_ERR_INVALID, "multigrid: transfers[l] must connect mfs[l] (fine) and mfs[l + 1] (coarse)");
  return BP5_OK;
}
// the V-cycle handle of checked arguments: per level the inverse diagonal, the work vectors (op[l].n_components blocks op[l].ld apart; scalar
// levels: n_local doubles), the transfer's slots and the Chebyshev smoother (the last level: the coarse solver) of the level's operator
static int mg_create_impl(int n_levels, bp5_mf *const *mfs, const std::vector<LinearOp> &ops, bp5_mg_transfer *const *transfers, const bp5_mg_params *prm,
                          bp5_mg **out)
{
  HIP_TRY(hipSetDevice(mfs[0]->device));
  std::unique_ptr<bp5_mg, int (*)(bp5_mg *)> mg(new bp5_mg, bp5_mg_destroy);
  mg->n_levels = n_levels;
  mg->mf.assign(mfs, mfs + n_levels);
  mg->op = ops;
  mg->tr.assign(transfers, transfers + (n_levels - 1));
  mg->inv_diag.assign(n_levels, nullptr);
  mg->x.assign(n_levels, nullptr);
  mg->b.assign(n_levels, nullptr);
  mg->t.assign(n_levels, nullptr);
  auto alloc = [&](double **p, size_t n) -> int {
    HIP_TRY(hipMalloc((void **)p, std::max<size_t>(n, 2) * sizeof(double)));
    mg->allocs.push_back(*p);
    HIP_TRY(hipMemsetAsync(*p, 0, std::max<size_t>(n, 2) * sizeof(double), mfs[0]->stream));
    return BP5_OK;
  };
  for (int l = 0; l < n_levels; ++l) {
    bp5_mf *m = mfs[l];
    const LinearOp &A = ops[l];
    const size_t len = A.block() ? A.n_components * A.ld : m->n_local();
    BP5_TRY(alloc(&mg->inv_diag[l], len));
    if (l > 0) { BP5_TRY(alloc(&mg->x[l], len)); BP5_TRY(alloc(&mg->b[l], len)); }
    if (l + 1 < n_levels) {
      BP5_TRY(alloc(&mg->t[l], len));
      double *slots = nullptr;
      BP5_TRY(mg_reserve_slots(mg->tr[l], A.n_components, &slots)); // at setup: nothing allocates inside vmult (one component: the transfer's own)
    }
    if (A.block()) BP5_TRY(bp5_elasticity_compute_diagonal(m, A.coef, A.lambda, A.mu, A.ld, mg->inv_diag[l], 1));
    else BP5_TRY(bp5_compute_diagonal(m, A.coef, mg->inv_diag[l], 1));
    const bool coarsest = l + 1 == n_levels;
    bp5_chebyshev_params cp{};
    cp.degree = coarsest ? prm->coarse_degree : prm->smoother_degree;
    cp.smoothing_range = coarsest ? prm->coarse_range : prm->smoothing_range;
    cp.eig_cg_n_iterations = coarsest ? prm->coarse_eig_cg_n_iterations : prm->eig_cg_n_iterations;
    cp.start_ids_host = prm->start_ids_host ? prm->start_ids_host[l] : nullptr;
    bp5_chebyshev *c = nullptr;
    BP5_TRY(chebyshev_create_impl(m, A, mg->inv_diag[l], &cp, &c));
    mg->cheb.push_back(c);
  }
  HIP_TRY(hipStreamSynchronize(mfs[0]->stream));
  *out = mg.release();
  return BP5_OK;
}

extern "C" int bp5_mg_create(int n_levels, bp5_mf *const *mfs, const double *const *coefs, bp5_mg_transfer *const *transfers, const bp5_mg_params *prm,
                             bp5_mg **out)
{
  BP5_TRY(mg_arguments_check(plainly_refuse, "null argument or n_levels < 1", n_levels, mfs, coefs, transfers, prm, out));
  for (int l = 0; l < n_levels; ++l) {
    if (!mfs[l] || (!coefs[l] && mfs[l]->geometry_mode == BP5_GEOM_MERGED6)) return fail(BP5_ERR_INVALID, "multigrid: null level handle or metric");
    if (mfs[l]->stream != mfs[0]->stream) return fail(BP5_ERR_INVALID, "multigrid: the levels must share one stream");
    if (mfs[l]->overint()) return overint_refuse("multigrid levels are not supported");
  }
  BP5_TRY(mg_transfers_check(plainly_refuse, n_levels, mfs, transfers));
  std::vector<LinearOp> ops;
  for (int l = 0; l < n_levels; ++l) ops.push_back(scalar_op(coefs[l], nullptr, nullptr));
  return mg_create_impl(n_levels, mfs, ops, transfers, prm, out);
}

// The elasticity V-cycle: mg_level on three-block vectors
extern "C" int bp5_elasticity_mg_create(int n_levels, bp5_mf *const *mfs, const double *const *coefs, double lambda, double mu, size_t ld,
                                        bp5_mg_transfer *const *transfers, const bp5_mg_params *prm, bp5_mg **out)
{
  BP5_TRY(mg_arguments_check(elasticity_refuse, "multigrid: null argument or n_levels < 1", n_levels, mfs, coefs, transfers, prm, out));
  if (ld & 1) return elasticity_refuse(BP5_ERR_INVALID, "ld must be even (every block 16-byte aligned)");
  BP5_TRY(elasticity_parameter_check(lambda, mu));
  for (int l = 0; l < n_levels; ++l) {
    if (!mfs[l] || !coefs[l]) return elasticity_refuse(BP5_ERR_INVALID, "multigrid: null level handle or metric");
    if (!aligned16(coefs[l])) return elasticity_refuse(BP5_ERR_INVALID, "multigrid: the metric arrays must be 16-byte aligned");
  }
  if (ld < mfs[0]->n_local()) return elasticity_refuse(BP5_ERR_INVALID, "ld < n_owned + n_ghost");
  for (int l = 0; l < n_levels; ++l) {
    BP5_TRY(elasticity_handle_check(mfs[l]));
    if (mfs[l]->stream != mfs[0]->stream || mfs[l]->device != mfs[0]->device) return elasticity_refuse(BP5_ERR_INVALID, "multigrid: the levels must share one stream");
    // the coarse polynomial is no solver for a singular level (the rigid-body modes), and a smoother's estimate has no meaning on one
    if (!mfs[l]->n_constrained) return elasticity_refuse(BP5_ERR_UNSUPPORTED, "multigrid: a level without Dirichlet DoFs is singular (rigid-body modes)");
  }
  BP5_TRY(mg_transfers_check(elasticity_refuse, n_levels, mfs, transfers));
  std::vector<LinearOp> ops;
  for (int l = 0; l < n_levels; ++l)
    ops.push_back(elasticity_op(coefs[l], lambda, mu, l == 0 ? ld : std::max<size_t>((mfs[l]->n_local() + 1) & ~(size_t)1, 2)));
  return mg_create_impl(n_levels, mfs, ops, transfers, prm, out);
}
// one level of the V-cycle.  The scalar and the elasticity cycle are the same steps: the level's Chebyshev handle knows its operator (elasticity,
// distributed or plain apply on the level's own metric), and the vectors are the op[l].n_components blocks, op[l].ld apart, of its descriptor
static int mg_level(bp5_mg *mg, int l, double *x, double *b)
{
  if (l + 1 == mg->n_levels) return bp5_chebyshev_vmult(mg->cheb[l], x, b);
  const int nc = mg->op[l].n_components;
  const size_t ld = mg->op[l].ld, ldc = mg->op[l + 1].ld;
  BP5_TRY(bp5_chebyshev_vmult(mg->cheb[l], x, b));                                   // pre-smoothing from zero
  BP5_TRY(cheb_apply(mg->cheb[l], x, mg->t[l]));                                     // t = A x
  BP5_TRY(mg_restrict(mg->tr[l], nc, ldc, mg->b[l + 1], ld, b, mg->t[l], false));    // b_c = P^T (w (.) (b - t)), Dirichlet rows 0
  BP5_TRY(mg_level(mg, l + 1, mg->x[l + 1], mg->b[l + 1]));
  BP5_TRY(mg_prolongate(mg->tr[l], nc, ld, x, ldc, mg->x[l + 1]));                   // x += P x_c
  return bp5_chebyshev_step(mg->cheb[l], x, b);                                      // post-smoothing
}

extern "C" int bp5_mg_vmult(void *mgv, double *dst, double *src)
{
  bp5_mg *mg = static_cast<bp5_mg *>(mgv);
  if (!mg || !dst || !src) return fail(BP5_ERR_INVALID, "null argument");
  if (dst == src) return fail(BP5_ERR_INVALID, "multigrid vmult: dst and src must differ");
  HIP_TRY(hipSetDevice(mg->mf[0]->device));
  return mg_level(mg, 0, dst, src);
}

extern "C" int bp5_mg_level_info(const bp5_mg *mg, int level, bp5_mg_level *o)
{
  if (!mg || !o) return fail(BP5_ERR_INVALID, "null argument");
  if (level < 0 || level >= mg->n_levels) return fail(BP5_ERR_INVALID, "multigrid: level out of range");
  memset(o, 0, sizeof(*o));
  o->n_levels = mg->n_levels;
  o->degree = mg->mf[level]->degree;
  o->n_owned = mg->mf[level]->n_owned;
  const bp5_chebyshev *c = mg->cheb[level];
  o->chebyshev_degree = c->degree;
  return bp5_chebyshev_eigenvalues(c, &o->min_est, &o->max_est, &o->min_used, &o->max_used, &o->cg_its);
}
