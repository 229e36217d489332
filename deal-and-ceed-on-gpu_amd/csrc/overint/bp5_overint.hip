// Gauss(p+2) quadrature (BP5_QUAD_GAUSS_OVER; CEED BP1 and BP3): every kernel instantiation and launch of the over-integrated handle, all degrees,
// in ONE translation unit of its own -- the per-degree units (bp5_apply_p4 is the critical path of the build) do not grow.  It sits in a directory of
// its own so that its ISA (--save-temps) lands beside it: tests/test_isa_overint.py reads it there.
#include "../bp5_device.hpp"

namespace {

template <int n, int Q>
void fill_shape_q(ShapeArgQ<n, Q> &sh, const bp5_mf *mf) // the half of each rectangular table the kernels read (mv_rect)
{
  memcpy(sh.N, mf->tab.N, sizeof(sh.N));
  memcpy(sh.D, mf->tab.D, sizeof(sh.D));
}

// cells [c0, c1) through the degree's pencil kernel of the handle's operator class (atomic scatter: an overwriting launch zero-fills dst first)
template <int P>
int launch_apply_q(bp5_mf *mf, const double *coef, const double *src, double *dst, uint32_t c0, uint32_t c1, bool overwrite)
{
  using SH = OverintShape<P>;
  constexpr int n = P + 1, Q = P + 2, TW = SH::TW, LPC = SH::LPC, TPB = SH::TPB, CPT = SH::CPT;
  using L = LdsLayout<Q, LPC>;
  if (overwrite) BP5_TRY(zero_dst(mf, dst));
  ApplyArgs a = apply_args(mf, false, coef, src, dst);
  a.cell_begin = c0; a.cell_end = c1;
  a.n_teams = (c1 - c0 + CPT - 1) / CPT;
  const uint32_t nblk = (a.n_teams + TPB - 1) / TPB;
  a.teams_per_xcd = (nblk + 7) / 8;
  ShapeArgQ<n, Q> sh;
  fill_shape_q(sh, mf);
  if (mf->operator_kind == BP5_OP_MASS) {
    const size_t lds = (size_t)TPB * CPT * mass_tile_stride<Q, LPC>() * sizeof(double); // one field per cell slot
    snprintf(mf->last_apply_kernel, sizeof(mf->last_apply_kernel), "apply_pencil_mass_q_kernel<%d,%d,%d,%d>", P, TW, LPC, TPB);
    hipLaunchKernelGGL((apply_pencil_mass_q_kernel<P, TW, LPC, TPB>), dim3(a.teams_per_xcd * 8), dim3(64 * TW * TPB), lds, mf->stream, a, sh);
  } else {
    const size_t lds = (size_t)TPB * CPT * L::CS * sizeof(double);
    snprintf(mf->last_apply_kernel, sizeof(mf->last_apply_kernel), "apply_pencil_q_kernel<%d,%d,%d,%d,%s>", P, TW, LPC, TPB, SH::PF ? "true" : "false");
    hipLaunchKernelGGL((apply_pencil_q_kernel<P, TW, LPC, TPB, SH::PF>), dim3(a.teams_per_xcd * 8), dim3(64 * TW * TPB), lds, mf->stream, a, sh);
  }
  KERNEL_CHECK();
  return BP5_OK;
}

template <int n>
int launch_metric_q(bp5_mf *mf, double *coef)
{
  constexpr int Q = n + 1;
  const uint32_t grid = std::min<uint32_t>(std::max<uint32_t>(mf->n_cells, 1), 65535u * 16);
  hipLaunchKernelGGL(overint_metric_kernel<n>, dim3(grid), dim3(Q * Q * Q), 0, mf->stream, mf->d_l2g, mf->d_coords, mf->d_tab, mf->coefficient, mf->n_cells,
                     mf->n_planes(), coef, mf->coef_plane_stride, mf->coef_cell_stride);
  KERNEL_CHECK();
  return BP5_OK;
}

template <int n>
int launch_diagonal_q(bp5_mf *mf, const double *coef, double *diag)
{
  constexpr int Q = n + 1;
  const uint32_t grid = std::min<uint32_t>(std::max<uint32_t>(mf->n_cells, 1), 65536u);
  hipLaunchKernelGGL(overint_diagonal_kernel<n>, dim3(grid), dim3(Q * Q * Q), 0, mf->stream, mf->d_l2g, coef, mf->coef_plane_stride, mf->coef_cell_stride, mf->d_tab,
                     mf->n_cells, mf->n_planes(), diag);
  KERNEL_CHECK();
  return BP5_OK;
}

template <int n>
int launch_permute_q(bp5_mf *mf, const double *in, double *out)
{
  const uint64_t total = (uint64_t)mf->n_planes() * mf->n_cells * mf->nq3;
  hipLaunchKernelGGL(metric_permute_kernel<n + 1>, dim3(2048), dim3(256), 0, mf->stream, in, out, total, (uint64_t)mf->n_cells, mf->coef_plane_stride, mf->coef_cell_stride);
  KERNEL_CHECK();
  return BP5_OK;
}

#define OVERINT_DISPATCH_N(fn, ...)                                                                                \
  switch (mf->n) {                                                                                                 \
    case 2: return fn<2>(__VA_ARGS__);                                                                             \
    case 3: return fn<3>(__VA_ARGS__);                                                                             \
    case 4: return fn<4>(__VA_ARGS__);                                                                             \
    case 5: return fn<5>(__VA_ARGS__);                                                                             \
    case 6: return fn<6>(__VA_ARGS__);                                                                             \
    case 7: return fn<7>(__VA_ARGS__);                                                                             \
    case 8: return fn<8>(__VA_ARGS__);                                                                             \
    case 9: return fn<9>(__VA_ARGS__);                                                                             \
  }                                                                                                                \
  return fail(BP5_ERR_INVALID, "unsupported degree")

} // namespace

int overint_apply(bp5_mf *mf, ApplyCall &call, const double *coef, const double *src, double *dst)
{
  // what the setters refuse one by one (in either call order), once more in front of the launch
  if (mf->operator_kind != BP5_OP_POISSON && mf->operator_kind != BP5_OP_MASS) return overint_refuse("Poisson and mass operator only");
  if (mf->has_hanging || mf->geometry_mode != BP5_GEOM_MERGED6 || mf->f32_metric())
    return overint_refuse("conforming meshes, the plane geometry and double planes only (no hanging nodes, no affine mode, no FP32 planes)");
  if (call.variant != 0) return overint_refuse("only apply variant 0, the pencil kernel (no block, team or march build)");
  if (call.fuse) return fail(BP5_ERR_INVALID, "fused dot products need the packed block kernel");
  const uint32_t c0 = call.c0, c1 = call.c1;
  switch (mf->degree) {
    case 1: return launch_apply_q<1>(mf, coef, src, dst, c0, c1, call.overwrite);
    case 2: return launch_apply_q<2>(mf, coef, src, dst, c0, c1, call.overwrite);
    case 3: return launch_apply_q<3>(mf, coef, src, dst, c0, c1, call.overwrite);
    case 4: return launch_apply_q<4>(mf, coef, src, dst, c0, c1, call.overwrite);
    case 5: return launch_apply_q<5>(mf, coef, src, dst, c0, c1, call.overwrite);
    case 6: return launch_apply_q<6>(mf, coef, src, dst, c0, c1, call.overwrite);
    case 7: return launch_apply_q<7>(mf, coef, src, dst, c0, c1, call.overwrite);
    case 8: return launch_apply_q<8>(mf, coef, src, dst, c0, c1, call.overwrite);
  }
  return fail(BP5_ERR_INVALID, "unsupported degree");
}
int overint_compute_metric(bp5_mf *mf, double *coef) { OVERINT_DISPATCH_N(launch_metric_q, mf, coef); }
int overint_diagonal(bp5_mf *mf, const double *coef, double *diag) { OVERINT_DISPATCH_N(launch_diagonal_q, mf, coef, diag); }
int overint_to_reference_layout(bp5_mf *mf, const double *coef, double *coef_ref) { OVERINT_DISPATCH_N(launch_permute_q, mf, coef, coef_ref); }
