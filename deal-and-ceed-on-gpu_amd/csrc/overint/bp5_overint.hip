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
  const PencilLaunch pl = pencil_launch<CPT, TW, TPB>(a, c0, c1);
  ShapeArgQ<n, Q> sh;
  fill_shape_q(sh, mf);
  if (mf->operator_kind == BP5_OP_MASS) {
    const size_t lds = (size_t)TPB * CPT * mass_tile_stride<Q, LPC>() * sizeof(double); // one field per cell slot
    snprintf(mf->last_apply_kernel, sizeof(mf->last_apply_kernel), "apply_pencil_mass_q_kernel<%d,%d,%d,%d>", P, TW, LPC, TPB);
    hipLaunchKernelGGL((apply_pencil_mass_q_kernel<P, TW, LPC, TPB>), pl.grid, pl.block, lds, mf->stream, a, sh);
  } else {
    const size_t lds = (size_t)TPB * CPT * L::CS * sizeof(double);
    snprintf(mf->last_apply_kernel, sizeof(mf->last_apply_kernel), "apply_pencil_q_kernel<%d,%d,%d,%d,%s>", P, TW, LPC, TPB, SH::PF ? "true" : "false");
    hipLaunchKernelGGL((apply_pencil_q_kernel<P, TW, LPC, TPB, SH::PF>), pl.grid, pl.block, lds, mf->stream, a, sh);
  }
  KERNEL_CHECK();
  return BP5_OK;
}

template <int n>
int launch_metric_q(bp5_mf *mf, double *coef)
{
  constexpr int Q = n + 1;
  const uint32_t grid = cell_grid(mf, 65535u * 16);
  hipLaunchKernelGGL(overint_metric_kernel<n>, dim3(grid), dim3(Q * Q * Q), 0, mf->stream, mf->d_l2g, mf->d_coords, mf->d_tab, mf->coefficient, mf->n_cells,
                     mf->n_planes(), coef, mf->coef_plane_stride, mf->coef_cell_stride);
  KERNEL_CHECK();
  return BP5_OK;
}

template <int n>
int launch_diagonal_q(bp5_mf *mf, const double *coef, double *diag)
{
  constexpr int Q = n + 1;
  const uint32_t grid = cell_grid(mf, 65536u);
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

} // namespace

int overint_apply(bp5_mf *mf, ApplyCall &call, const double *coef, const double *src, double *dst)
{
  // what the setters refuse one by one (in either call order), once more in front of the launch
  if (mf->operator_kind != BP5_OP_POISSON && mf->operator_kind != BP5_OP_MASS) return overint_refuse("Poisson and mass operator only");
  if (mf->has_hanging || mf->geometry_mode != BP5_GEOM_MERGED6 || mf->f32_metric())
    return overint_refuse("conforming meshes, the plane geometry and double planes only (no hanging nodes, no affine mode, no FP32 planes)");
  if (call.variant != 0) return overint_refuse("only apply variant 0, the pencil kernel (no block, team or march build)");
  if (call.fuse) return fail(BP5_ERR_INVALID, "fused dot products need the packed block kernel");
  return for_degree(mf->degree, [&](auto P) { return launch_apply_q<P()>(mf, coef, src, dst, call.c0, call.c1, call.overwrite); });
}
int overint_compute_metric(bp5_mf *mf, double *coef)
{
  return for_degree(mf->degree, [&](auto P) { return launch_metric_q<P() + 1>(mf, coef); });
}
int overint_diagonal(bp5_mf *mf, const double *coef, double *diag)
{
  return for_degree(mf->degree, [&](auto P) { return launch_diagonal_q<P() + 1>(mf, coef, diag); });
}
int overint_to_reference_layout(bp5_mf *mf, const double *coef, double *coef_ref)
{
  return for_degree(mf->degree, [&](auto P) { return launch_permute_q<P() + 1>(mf, coef, coef_ref); });
}
