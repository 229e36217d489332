// The pointwise and transfer kernels of every vector shape -- the Chebyshev step and the multigrid prolongate / restrict / combine of scalar vectors
// (n_components = 1) and of block vectors alike, and the dot product of block vectors: every instantiation and launch in ONE translation unit of
// its own, so that the device unit and the per-degree units carry none of them.  Its ISA (--save-temps) lands beside it.  The callers
// (bp5_device.hip) have validated handles and layouts.
#include "../bp5_device.hpp"

namespace {

template <int FORM>
int cheb_launch(hipStream_t s, dim3 grid, bool nt, double *x_new, const double *x, const double *x_old, const double *src, const double *t, const double *dg,
                size_t n, size_t ld, size_t dld, double f1, double f2)
{
  const dim3 block(VB);
  if (dg) {
    if (nt) hipLaunchKernelGGL((chebyshev_step_kernel<FORM, true, true>), grid, block, 0, s, x_new, x, x_old, src, t, dg, n, ld, dld, f1, f2);
    else hipLaunchKernelGGL((chebyshev_step_kernel<FORM, true, false>), grid, block, 0, s, x_new, x, x_old, src, t, dg, n, ld, dld, f1, f2);
  } else {
    if (nt) hipLaunchKernelGGL((chebyshev_step_kernel<FORM, false, true>), grid, block, 0, s, x_new, x, x_old, src, t, dg, n, ld, dld, f1, f2);
    else hipLaunchKernelGGL((chebyshev_step_kernel<FORM, false, false>), grid, block, 0, s, x_new, x, x_old, src, t, dg, n, ld, dld, f1, f2);
  }
  KERNEL_CHECK();
  return BP5_OK;
}

// One transfer kernel shape: the p-transfer pf -> max(1, pf / 2) (NF = pf + 1 fine, NC coarse nodes per direction) or the geometric one (NF = NC)
template <int NF, int NC, bool GEO>
struct MgBuild {
  static uint32_t grid(const MgComponentsArgs &a) { return (a.n_cells + MgShape<NF, NC>::CPB - 1) / MgShape<NF, NC>::CPB; }
};
// ... resolved in ONE place from the transfer's kind and fine degree: f(MgBuild<...>{}) for the degrees that are instantiated (p-transfer 2..8,
// geometric 1..4), a refusal for the others
template <class F>
int mg_dispatch(const MgComponentsArgs &a, F &&f)
{
  const bool geo = a.geometric;
  const char *refusal = geo ? "geometric multigrid transfer: degree must be 1..4" : "multigrid transfer: fine degree must be 2..8";
  return for_degree((geo ? a.pf <= 4 : a.pf >= 2) ? a.pf : 0, [&](auto P) {
    constexpr int p = P();
    if constexpr (p <= 4) if (geo) return f(MgBuild<p + 1, p + 1, true>{});
    if constexpr (p >= 2) if (!geo) return f(MgBuild<p + 1, p / 2 + 1, false>{});
    return fail(BP5_ERR_INVALID, refusal);
  }, refusal);
}

template <int NF, int NC, bool GEO>
int prolongate_launch(MgBuild<NF, NC, GEO> B, const MgComponentsArgs &a, int nc, size_t ld_c, const double *src, size_t ld_f, double *dst)
{
  const dim3 grid(B.grid(a)), block(256);
  if (!grid.x) return BP5_OK;
  if constexpr (GEO) hipLaunchKernelGGL((mg_geo_prolongate_kernel<NF>), grid, block, 0, a.stream, a.M, a.cidx, a.pcode, a.fidx, a.wmask, a.n_cells, nc, ld_c, src, ld_f, dst);
  else hipLaunchKernelGGL((mg_prolongate_kernel<NF, NC>), grid, block, 0, a.stream, a.M, a.cidx, a.fidx, a.wmask, a.n_cells, nc, ld_c, src, ld_f, dst);
  KERNEL_CHECK();
  return BP5_OK;
}
template <bool RESIDUAL, int NF, int NC, bool GEO>
int restrict_launch(MgBuild<NF, NC, GEO> B, const MgComponentsArgs &a, int nc, size_t ld_f, const double *b, const double *tv, size_t slot_stride, double *slots)
{
  const dim3 grid(B.grid(a)), block(256);
  if (!grid.x) return BP5_OK;
  if constexpr (GEO) hipLaunchKernelGGL((mg_geo_restrict_kernel<NF, RESIDUAL>), grid, block, 0, a.stream, a.M, a.pcode, a.fidx, a.n_cells, a.w, nc, ld_f, b, tv, slot_stride, slots);
  else if (nc == 1) hipLaunchKernelGGL((mg_restrict_kernel<NF, NC, RESIDUAL>), grid, block, 0, a.stream, a.M, a.fidx, a.n_cells, a.w, b, tv, slots); // (its own body: bp5_kernels.hpp)
  else hipLaunchKernelGGL((mg_restrict_components_kernel<NF, NC, RESIDUAL>), grid, block, 0, a.stream, a.M, a.fidx, a.n_cells, a.w, nc, ld_f, b, tv, slot_stride, slots);
  KERNEL_CHECK();
  return BP5_OK;
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
  return mg_dispatch(a, [&](auto B) { return prolongate_launch(B, a, n_components, ld_c, src, ld_f, dst); });
}

int blockvec_mg_restrict(const MgComponentsArgs &a, int n_components, size_t ld_f, const double *b, const double *tv, size_t slot_stride, double *slots)
{
  return mg_dispatch(a, [&](auto B) {
    return tv ? restrict_launch<true>(B, a, n_components, ld_f, b, tv, slot_stride, slots) : restrict_launch<false>(B, a, n_components, ld_f, b, tv, slot_stride, slots);
  });
}

int blockvec_mg_combine(const MgComponentsArgs &a, int n_components, const double *slots, size_t slot_stride, uint32_t n_owned, uint32_t n, size_t ld, double *dst, bool add)
{
  if (!n) return BP5_OK;
  const uint32_t grid = std::min<uint32_t>((n + 255) / 256, 65536u);
  if (add) hipLaunchKernelGGL(mg_combine_kernel<true>, dim3(grid), dim3(256), 0, a.stream, a.coff, a.cslot, slots, slot_stride, n_components, n_owned, n, ld, dst);
  else hipLaunchKernelGGL(mg_combine_kernel<false>, dim3(grid), dim3(256), 0, a.stream, a.coff, a.cslot, slots, slot_stride, n_components, n_owned, n, ld, dst);
  KERNEL_CHECK();
  return BP5_OK;
}
