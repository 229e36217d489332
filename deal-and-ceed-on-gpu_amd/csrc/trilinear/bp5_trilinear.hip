// Trilinear geometry (BP5_GEOM_TRILINEAR; deal.II MappingQ1): every kernel instantiation and launch of a handle that computes its metric from the
// cells' vertices, all degrees and both quadratures, in ONE translation unit of its own -- the per-degree units (bp5_apply_p4 is the critical path
// of the build) do not grow.  It sits in a directory of its own so that its ISA (--save-temps) lands beside it: tests/test_isa_trilinear.py reads it there.
#include "../bp5_device.hpp"

namespace {

template <int n>
TrilinearRule<n> rule_of(const double *x, const double *w, int kappa_mode)
{
  TrilinearRule<n> r;
  memcpy(r.x, x, sizeof(r.x));
  memcpy(r.w, w, sizeof(r.w));
  r.kappa_mode = kappa_mode;
  return r;
}

// cells [c0, c1) through the degree's trilinear pencil kernel (atomic scatter: an overwriting launch zero-fills dst first)
template <int P, bool COLL>
int launch_apply_trilinear(bp5_mf *mf, const double *src, double *dst, uint32_t c0, uint32_t c1, bool overwrite)
{
  using DP = DefaultPencil<P>;
  constexpr int n = P + 1, TW = DP::TW, LPC = DP::LPC, TPB = DP::TPB, CPT = 64 * TW / LPC;
  using L = LdsLayout<n, LPC>;
  if (overwrite) BP5_TRY(zero_dst(mf, dst));
  ApplyArgs a = apply_args(mf, false, mf->d_vertices, src, dst);
  a.cell_stride = 24;
  const PencilLaunch pl = pencil_launch<CPT, TW, TPB>(a, c0, c1);
  ShapeArg<n> tables;
  fill_shape(tables, mf);
  TrilinearArg<n> sh;
  memcpy(sh.N, tables.N, sizeof(sh.N));
  memcpy(sh.D, tables.D, sizeof(sh.D));
  sh.rule = rule_of<n>(mf->tab.pts, mf->tab.w, mf->coefficient);
  const size_t lds = (size_t)TPB * CPT * L::CS * sizeof(double);
  snprintf(mf->last_apply_kernel, sizeof(mf->last_apply_kernel), "apply_pencil_trilinear_kernel<%d,%s,%d,%d,%d>", P, COLL ? "true" : "false", TW, LPC, TPB);
  hipLaunchKernelGGL((apply_pencil_trilinear_kernel<P, COLL, TW, LPC, TPB>), pl.grid, pl.block, lds, mf->stream, a, sh);
  KERNEL_CHECK();
  return BP5_OK;
}

template <int n>
int launch_setup_trilinear(bp5_mf *mf, double *vertices, double *deviation)
{
  const uint32_t grid = cell_grid(mf, 65535u * 16);
  hipLaunchKernelGGL(trilinear_setup_kernel<n>, dim3(grid), dim3(n, n, n), 0, mf->stream, mf->d_l2g, mf->d_coords, rule_of<n>(mf->tab.nodes, mf->tab.w, 0), mf->n_cells,
                     vertices, deviation);
  KERNEL_CHECK();
  return BP5_OK;
}

template <int n>
int launch_diagonal_trilinear(bp5_mf *mf, double *diag)
{
  const uint32_t grid = cell_grid(mf, 65536u);
  hipLaunchKernelGGL(trilinear_diagonal_kernel<n>, dim3(grid), dim3(n, n, n), 0, mf->stream, mf->d_l2g, mf->d_vertices, rule_of<n>(mf->tab.pts, mf->tab.w, mf->coefficient),
                     mf->d_tab, mf->n_cells, diag);
  KERNEL_CHECK();
  return BP5_OK;
}

} // namespace

int trilinear_apply(bp5_mf *mf, ApplyCall &call, const double *src, double *dst)
{
  // what the setters refuse one by one (in either call order), once more in front of the launch
  if (mf->operator_kind != BP5_OP_POISSON || mf->overint() || mf->has_hanging || mf->f32_metric())
    return trilinear_refuse("Poisson operator, Gauss(p+1) or GLL points, conforming meshes only (no Helmholtz or mass operator, no Gauss(p+2) points, no hanging nodes, no FP32 planes)");
  if (call.variant != 0) return trilinear_refuse("only apply variant 0, the pencil kernel apply_pencil_trilinear_kernel (no block, team or march build)");
  if (call.fuse) return fail(BP5_ERR_INVALID, "fused dot products need the packed block kernel");
  const bool coll = mf->quadrature == BP5_QUAD_GLL;
  return for_degree(mf->degree, [&](auto P) {
    return coll ? launch_apply_trilinear<P(), true>(mf, src, dst, call.c0, call.c1, call.overwrite) : launch_apply_trilinear<P(), false>(mf, src, dst, call.c0, call.c1, call.overwrite);
  });
}
int trilinear_setup(bp5_mf *mf, double *vertices, double *deviation)
{
  return for_degree(mf->degree, [&](auto P) { return launch_setup_trilinear<P() + 1>(mf, vertices, deviation); });
}
int trilinear_diagonal(bp5_mf *mf, double *diag)
{
  return for_degree(mf->degree, [&](auto P) { return launch_diagonal_trilinear<P() + 1>(mf, diag); });
}
