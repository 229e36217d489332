// Linear elasticity (bp5_elasticity_*; deal.II step-8 / step-18, the CEED "solids" mini-app): every kernel instantiation and launch of the coupled
// three-component operator, all degrees and both quadratures, in ONE translation unit of its own -- the per-degree units (bp5_apply_p4 is the
// critical path of the build) do not grow.  It sits in a directory of its own so that its ISA (--save-temps) lands beside it:
// tests/test_isa_elasticity.py reads it there.
#include "../bp5_device.hpp"

namespace {

// cells [c0, c1) (non-empty) through the degree's default pencil shape: ONE launch for the three components
template <int P, bool COLL>
int launch_elasticity_t(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, const double *src, double *dst, uint32_t c0, uint32_t c1)
{
  using DP = DefaultPencil<P>;
  constexpr int n = P + 1, TW = DP::TW, LPC = DP::LPC, TPB = DP::TPB;
  constexpr int CPT = 64 * TW / LPC;
  using L = LdsLayout<n, LPC>;
  ApplyArgs a = apply_args(mf, false, coef, src, dst);
  a.plane_stride = (uint64_t)mf->n_cells * mf->n3; a.cell_stride = (uint64_t)mf->n3; // ten planes, plane-major
  const PencilLaunch pl = pencil_launch<CPT, TW, TPB>(a, c0, c1);
  ElasticityArgs ea{lambda, mu, (uint64_t)ld};
  ShapeArg<n> sh;
  fill_shape(sh, mf);
  const size_t lds = (size_t)TPB * CPT * L::CS * sizeof(double);
  snprintf(mf->last_apply_kernel, sizeof(mf->last_apply_kernel), "apply_pencil_elasticity_kernel<%d,%s,%d,%d,%d>", P, COLL ? "true" : "false", TW, LPC, TPB);
  hipLaunchKernelGGL((apply_pencil_elasticity_kernel<P, COLL, TW, LPC, TPB>), pl.grid, pl.block, lds, mf->stream, a, ea, sh);
  KERNEL_CHECK();
  return BP5_OK;
}
template <int P>
int launch_elasticity(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, const double *src, double *dst, uint32_t c0, uint32_t c1)
{
  if (mf->quadrature == BP5_QUAD_GLL) return launch_elasticity_t<P, true>(mf, coef, lambda, mu, ld, src, dst, c0, c1);
  return launch_elasticity_t<P, false>(mf, coef, lambda, mu, ld, src, dst, c0, c1);
}

template <int n>
int launch_metric(bp5_mf *mf, double *coef)
{
  const uint32_t grid = cell_grid(mf, 65535u * 16);
  hipLaunchKernelGGL(elasticity_metric_kernel<n>, dim3(grid), dim3(n, n, n), 0, mf->stream, mf->d_l2g, mf->d_coords, mf->d_tab, mf->coefficient, mf->n_cells, coef,
                     (uint64_t)mf->n_cells * mf->n3);
  KERNEL_CHECK();
  return BP5_OK;
}

template <int n>
int launch_diagonal(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, double *diag)
{
  const uint32_t grid = cell_grid(mf, 65536u);
  hipLaunchKernelGGL(elasticity_diagonal_kernel<n>, dim3(grid), dim3(n, n, n), 0, mf->stream, mf->d_l2g, coef, (uint64_t)mf->n_cells * mf->n3, mf->d_tab, mf->n_cells,
                     lambda, mu, (uint64_t)ld, diag);
  KERNEL_CHECK();
  return BP5_OK;
}

const char *const UNSUPPORTED_DEGREE = "elasticity: unsupported degree";

} // namespace

int elasticity_compute_metric(bp5_mf *mf, double *coef)
{
  if (!mf->n_cells) return BP5_OK;
  return for_degree(mf->degree, [&](auto P) { return launch_metric<P() + 1>(mf, coef); }, UNSUPPORTED_DEGREE);
}
int elasticity_diagonal(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, double *diag)
{
  if (!mf->n_cells) return BP5_OK;
  return for_degree(mf->degree, [&](auto P) { return launch_diagonal<P() + 1>(mf, coef, lambda, mu, ld, diag); }, UNSUPPORTED_DEGREE);
}
int elasticity_apply_cells(bp5_mf *mf, const double *coef, double lambda, double mu, size_t ld, const double *src, double *dst, uint32_t c0, uint32_t c1)
{
  if (c1 <= c0) return BP5_OK;
  return for_degree(mf->degree, [&](auto P) { return launch_elasticity<P()>(mf, coef, lambda, mu, ld, src, dst, c0, c1); }, UNSUPPORTED_DEGREE);
}
