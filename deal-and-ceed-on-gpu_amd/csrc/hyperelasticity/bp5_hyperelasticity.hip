// Finite-strain neo-Hookean hyperelasticity (bp5_hyperelasticity_*; the CEED "solids" mini-app's ElasFSInitialNH1F / dF, deal.II step-44's
// assemble_system_rhs / tangent): every kernel instantiation and launch of the residual and tangent operators, all degrees and both quadratures, in
// ONE translation unit of its own, in a directory of its own so that its ISA (--save-temps) lands beside it: tests/test_isa_hyperelasticity.py
// reads it there.
#include "../bp5_device.hpp"

namespace {

// cells [c0, c1) (non-empty) through the degree's default pencil shape: ONE launch for the three components
template <int P, bool COLL, int MODE>
int launch_hyperelasticity_t(bp5_mf *mf, const double *coef, double *state, double lambda, double mu, size_t ld, const double *src, double *dst, uint32_t c0,
                             uint32_t c1)
{
  using DP = DefaultPencil<P>;
  constexpr int n = P + 1, TW = DP::TW, LPC = DP::LPC, TPB = DP::TPB;
  constexpr int CPT = 64 * TW / LPC;
  using L = LdsLayout<n, LPC>;
  ApplyArgs a = apply_args(mf, false, coef, src, dst);
  a.plane_stride = (uint64_t)mf->n_cells * mf->n3; a.cell_stride = (uint64_t)mf->n3; // ten planes, plane-major (geometry and state alike)
  const PencilLaunch pl = pencil_launch<CPT, TW, TPB>(a, c0, c1);
  HyperelasticityArgs ea{lambda, mu, (uint64_t)ld, state};
  ShapeArg<n> sh;
  fill_shape(sh, mf);
  const size_t lds = (size_t)TPB * CPT * L::CS * sizeof(double);
  snprintf(mf->last_apply_kernel, sizeof(mf->last_apply_kernel), "apply_pencil_hyperelasticity_kernel<%d,%s,%d,%d,%d,%s>", P, COLL ? "true" : "false", TW, LPC, TPB,
           MODE == HYPER_RESIDUAL ? "residual" : "tangent");
  hipLaunchKernelGGL((apply_pencil_hyperelasticity_kernel<P, COLL, TW, LPC, TPB, MODE>), pl.grid, pl.block, lds, mf->stream, a, ea, sh);
  KERNEL_CHECK();
  return BP5_OK;
}
template <int P, int MODE>
int launch_hyperelasticity(bp5_mf *mf, const double *coef, double *state, double lambda, double mu, size_t ld, const double *src, double *dst, uint32_t c0, uint32_t c1)
{
  if (mf->quadrature == BP5_QUAD_GLL) return launch_hyperelasticity_t<P, true, MODE>(mf, coef, state, lambda, mu, ld, src, dst, c0, c1);
  return launch_hyperelasticity_t<P, false, MODE>(mf, coef, state, lambda, mu, ld, src, dst, c0, c1);
}

const char *const UNSUPPORTED_DEGREE = "hyperelasticity: unsupported degree";

} // namespace

int hyperelasticity_residual_cells(bp5_mf *mf, const double *coef, double *state, double lambda, double mu, size_t ld, const double *u, double *r, uint32_t c0,
                                   uint32_t c1)
{
  if (c1 <= c0) return BP5_OK;
  return for_degree(mf->degree, [&](auto P) { return launch_hyperelasticity<P(), HYPER_RESIDUAL>(mf, coef, state, lambda, mu, ld, u, r, c0, c1); }, UNSUPPORTED_DEGREE);
}
int hyperelasticity_apply_cells(bp5_mf *mf, const double *coef, const double *state, double lambda, double mu, size_t ld, const double *src, double *dst, uint32_t c0,
                                uint32_t c1)
{
  if (c1 <= c0) return BP5_OK;
  return for_degree(mf->degree,
                    [&](auto P) { return launch_hyperelasticity<P(), HYPER_TANGENT>(mf, coef, const_cast<double *>(state), lambda, mu, ld, src, dst, c0, c1); },
                    UNSUPPORTED_DEGREE);
}
