// Block-vector forms of the pointwise and transfer kernels (the preconditioners of the elasticity operator: bp5_elasticity_chebyshev_create,
// bp5_elasticity_mg_create, bp5_cg_solve_elasticity_preconditioned, bp5_mg_transfer_*_components): every instantiation and launch in ONE translation
// unit of its own, so that the device unit and the per-degree units do not grow and their code objects stay what they were.  Its ISA
// (--save-temps) lands beside it.  The callers (bp5_device.hip) have validated handles and layouts.
#include "../bp5_device.hpp"

namespace {

template <int FORM>
int cheb_launch(hipStream_t s, dim3 grid, bool nt, double *x_new, const double *x, const double *x_old, const double *src, const double *t, const double *dg,
                size_t n, size_t ld, size_t dld, double f1, double f2)
{
  const dim3 block(VB);
  if (dg) {
    if (nt) hipLaunchKernelGGL((chebyshev_step_components_kernel<FORM, true, true>), grid, block, 0, s, x_new, x, x_old, src, t, dg, n, ld, dld, f1, f2);
    else hipLaunchKernelGGL((chebyshev_step_components_kernel<FORM, true, false>), grid, block, 0, s, x_new, x, x_old, src, t, dg, n, ld, dld, f1, f2);
  } else {
    if (nt) hipLaunchKernelGGL((chebyshev_step_components_kernel<FORM, false, true>), grid, block, 0, s, x_new, x, x_old, src, t, dg, n, ld, dld, f1, f2);
    else hipLaunchKernelGGL((chebyshev_step_components_kernel<FORM, false, false>), grid, block, 0, s, x_new, x, x_old, src, t, dg, n, ld, dld, f1, f2);
  }
  KERNEL_CHECK();
  return BP5_OK;
}

template <int NF, int NC>
int prolongate_launch(const MgComponentsArgs &a, int nc, size_t ld_c, const double *src, size_t ld_f, double *dst)
{
  using S = MgShape<NF, NC>;
  const uint32_t grid = (a.n_cells + S::CPB - 1) / S::CPB;
  if (grid) hipLaunchKernelGGL((mg_prolongate_components_kernel<NF, NC>), dim3(grid), dim3(256), 0, a.stream, a.M, a.cidx, a.fidx, a.wmask, a.n_cells, nc, ld_c, src,
                              ld_f, dst);
  KERNEL_CHECK();
  return BP5_OK;
}
template <int NF, int NC>
int restrict_launch(const MgComponentsArgs &a, int nc, size_t ld_f, const double *b, const double *tv, size_t slot_stride, double *slots)
{
  using S = MgShape<NF, NC>;
  const uint32_t grid = (a.n_cells + S::CPB - 1) / S::CPB;
  if (!grid) return BP5_OK;
  if (tv) hipLaunchKernelGGL((mg_restrict_components_kernel<NF, NC, true>), dim3(grid), dim3(256), 0, a.stream, a.M, a.fidx, a.n_cells, a.w, nc, ld_f, b, tv, slot_stride,
                             slots);
  else hipLaunchKernelGGL((mg_restrict_components_kernel<NF, NC, false>), dim3(grid), dim3(256), 0, a.stream, a.M, a.fidx, a.n_cells, a.w, nc, ld_f, b, tv, slot_stride,
                          slots);
  KERNEL_CHECK();
  return BP5_OK;
}
template <int N>
int geo_prolongate_launch(const MgComponentsArgs &a, int nc, size_t ld_c, const double *src, size_t ld_f, double *dst)
{
  using S = MgShape<N, N>;
  const uint32_t grid = (a.n_cells + S::CPB - 1) / S::CPB;
  if (grid) hipLaunchKernelGGL((mg_geo_prolongate_components_kernel<N>), dim3(grid), dim3(256), 0, a.stream, a.M, a.cidx, a.pcode, a.fidx, a.wmask, a.n_cells, nc, ld_c,
                              src, ld_f, dst);
  KERNEL_CHECK();
  return BP5_OK;
}
template <int N>
int geo_restrict_launch(const MgComponentsArgs &a, int nc, size_t ld_f, const double *b, const double *tv, size_t slot_stride, double *slots)
{
  using S = MgShape<N, N>;
  const uint32_t grid = (a.n_cells + S::CPB - 1) / S::CPB;
  if (!grid) return BP5_OK;
  if (tv) hipLaunchKernelGGL((mg_geo_restrict_components_kernel<N, true>), dim3(grid), dim3(256), 0, a.stream, a.M, a.pcode, a.fidx, a.n_cells, a.w, nc, ld_f, b, tv,
                             slot_stride, slots);
  else hipLaunchKernelGGL((mg_geo_restrict_components_kernel<N, false>), dim3(grid), dim3(256), 0, a.stream, a.M, a.pcode, a.fidx, a.n_cells, a.w, nc, ld_f, b, tv,
                          slot_stride, slots);
  KERNEL_CHECK();
  return BP5_OK;
}

// the instantiated degree pairs of the p-transfer (pf -> max(1, pf / 2)) and the degrees of the geometric one (1..4), as in bp5_device.hip
#define BLOCKVEC_MG_DISPATCH(fn, geo_fn, a, ...)                                                                   \
  if (a.geometric) switch (a.pf) {                                                                                 \
    case 1: return geo_fn<2>(a, __VA_ARGS__);                                                                      \
    case 2: return geo_fn<3>(a, __VA_ARGS__);                                                                      \
    case 3: return geo_fn<4>(a, __VA_ARGS__);                                                                      \
    case 4: return geo_fn<5>(a, __VA_ARGS__);                                                                      \
    default: return fail(BP5_ERR_INVALID, "geometric multigrid transfer: degree must be 1..4");                    \
  }                                                                                                                \
  switch (a.pf) {                                                                                                  \
    case 2: return fn<3, 2>(a, __VA_ARGS__);                                                                       \
    case 3: return fn<4, 2>(a, __VA_ARGS__);                                                                       \
    case 4: return fn<5, 3>(a, __VA_ARGS__);                                                                       \
    case 5: return fn<6, 3>(a, __VA_ARGS__);                                                                       \
    case 6: return fn<7, 4>(a, __VA_ARGS__);                                                                       \
    case 7: return fn<8, 4>(a, __VA_ARGS__);                                                                       \
    case 8: return fn<9, 5>(a, __VA_ARGS__);                                                                       \
    default: return fail(BP5_ERR_INVALID, "multigrid transfer: fine degree must be 2..8");                         \
  }

} // namespace

int blockvec_dot(hipStream_t s, dim3 grid, const double *x, const double *y, size_t n, size_t ld, double *partials)
{
  hipLaunchKernelGGL(dot_components_kernel<BlockvecUnit>, grid, dim3(VB), 0, s, x, y, n, ld, partials);
  KERNEL_CHECK();
  return BP5_OK;
}

int blockvec_chebyshev_step(hipStream_t s, int form, unsigned grid_x, int n_components, bool nt, double *x_new, const double *x, const double *x_old, const double *src,
                            const double *t, const double *diag, size_t n, size_t ld, size_t diag_ld, double f1, double f2)
{
  if (!n) return BP5_OK;
  const dim3 grid(grid_x, n_components);
  switch (form) {
    case 0: return cheb_launch<0>(s, grid, nt, x_new, x, x_old, src, t, diag, n, ld, diag_ld, f1, f2);
    case 1: return cheb_launch<1>(s, grid, nt, x_new, x, x_old, src, t, diag, n, ld, diag_ld, f1, f2);
    case 2: return cheb_launch<2>(s, grid, nt, x_new, x, x_old, src, t, diag, n, ld, diag_ld, f1, f2);
    case 3: return cheb_launch<3>(s, grid, nt, x_new, x, x_old, src, t, diag, n, ld, diag_ld, f1, f2);
  }
  return fail(BP5_ERR_INVALID, "Chebyshev step: unknown form");
}

int blockvec_mg_prolongate(const MgComponentsArgs &a, int n_components, size_t ld_c, const double *src, size_t ld_f, double *dst)
{
  BLOCKVEC_MG_DISPATCH(prolongate_launch, geo_prolongate_launch, a, n_components, ld_c, src, ld_f, dst)
}

int blockvec_mg_restrict(const MgComponentsArgs &a, int n_components, size_t ld_f, const double *b, const double *tv, size_t slot_stride, double *slots)
{
  BLOCKVEC_MG_DISPATCH(restrict_launch, geo_restrict_launch, a, n_components, ld_f, b, tv, slot_stride, slots)
}

int blockvec_mg_combine(const MgComponentsArgs &a, int n_components, const double *slots, size_t slot_stride, uint32_t n_owned, uint32_t n, size_t ld, double *dst, bool add)
{
  if (!n) return BP5_OK;
  const uint32_t grid = std::min<uint32_t>((n + 255) / 256, 65536u);
  if (add) hipLaunchKernelGGL(mg_combine_components_kernel<true>, dim3(grid), dim3(256), 0, a.stream, a.coff, a.cslot, slots, slot_stride, n_components, n_owned, n, ld, dst);
  else hipLaunchKernelGGL(mg_combine_components_kernel<false>, dim3(grid), dim3(256), 0, a.stream, a.coff, a.cslot, slots, slot_stride, n_components, n_owned, n, ld, dst);
  KERNEL_CHECK();
  return BP5_OK;
}
