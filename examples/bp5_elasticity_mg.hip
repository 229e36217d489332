// Linear elasticity with the multigrid preconditioner on the C ABI directly (include/bp5.h: bp5_elasticity_mg_create, bp5_mg_vmult,
// bp5_cg_solve_elasticity_preconditioned; deal.II step-8's operator under step-37's PreconditionMG): the problem of examples/bp5_elasticity -- a brick
// of nx x ny x nz cells of side 1 at degree p, sine-deformed, clamped on its whole boundary, stiffness scaled by the step-64 coefficient, body force
// (0, 0, -1) -- solved by CG with one V-cycle per iteration over the levels p, p / 2, ..., 1 on the same cells (scalar p-transfers on all three
// components).  Prints the iteration count, the residual, every level's degree, size and Chebyshev bounds, and the solution norm.
//
//   bp5_elasticity_mg <p> <nx> <ny> <nz> <deform_amp> <lambda> <mu> <rel_tol>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bp5.h"

#define CHECK(expr)                                                                                                \
  do {                                                                                                             \
    const int s_ = (expr);                                                                                         \
    if (s_ != BP5_OK) {                                                                                            \
      fprintf(stderr, "error: %s: %s: %s\n", #expr, bp5_strerror(s_), bp5_last_error());                           \
      return 1;                                                                                                    \
    }                                                                                                              \
  } while (0)

int main(int argc, char **argv)
{
  if (argc < 9) {
    fprintf(stderr, "usage: %s p nx ny nz deform_amp lambda mu rel_tol\n", argv[0]);
    return 2;
  }
  const double lambda = atof(argv[6]), mu = atof(argv[7]), rel_tol = atof(argv[8]);
  std::vector<int> degrees{atoi(argv[1])};
  while (degrees.back() > 1) degrees.push_back(degrees.back() / 2 > 1 ? degrees.back() / 2 : 1);
  const int n_levels = (int)degrees.size();
  std::vector<bp5_mesh *> meshes(n_levels);
  std::vector<bp5_mesh_view> views(n_levels);
  std::vector<bp5_mf *> mfs(n_levels);
  std::vector<double *> coefs(n_levels);
  std::vector<const uint64_t *> ids(n_levels);
  for (int l = 0; l < n_levels; ++l) {
    bp5_mesh_desc md{};
    md.degree = degrees[l];
    for (int d = 0; d < 3; ++d) md.cells[d] = (uint32_t)atoi(argv[2 + d]);
    md.h = 1.0; md.deform_amp = atof(argv[5]); md.n_ranks = 1;
    CHECK(bp5_mesh_create_brick(&md, &meshes[l]));
    bp5_mesh_view &mv = views[l];
    CHECK(bp5_mesh_view_get(meshes[l], &mv));
    bp5_mf_desc d{};
    d.dim = 3; d.degree = mv.degree; d.quadrature = BP5_QUAD_GAUSS; d.coefficient = BP5_COEF_STEP64;
    d.n_cells = mv.n_cells; d.n_interior_cells = mv.n_interior_cells; d.n_owned = mv.n_owned; d.n_ghost = mv.n_ghost;
    d.local_to_global_host = mv.local_to_global_host; d.node_coords_host = mv.node_coords_host;
    d.constrained_host = mv.constrained_host; d.n_constrained = mv.n_constrained;
    d.n_cell_blocks = mv.n_cell_blocks; d.cell_block_offsets_host = mv.cell_block_offsets_host;
    CHECK(bp5_mf_create(&d, &mfs[l]));
    size_t n_coef;
    CHECK(bp5_elasticity_coef_size(mfs[l], &n_coef));
    CHECK(bp5_vec_alloc(n_coef, &coefs[l]));
    CHECK(bp5_elasticity_compute_metric(mfs[l], coefs[l]));
    ids[l] = mv.global_ids_host;
  }
  std::vector<bp5_mg_transfer *> transfers(n_levels > 1 ? n_levels - 1 : 1, nullptr);
  for (int l = 0; l + 1 < n_levels; ++l) CHECK(bp5_mg_transfer_create(mfs[l], mfs[l + 1], &transfers[l]));

  bp5_mf *mf = mfs[0];
  const bp5_mesh_view &mv = views[0];
  const size_t n_local = (size_t)mv.n_owned + mv.n_ghost, ld = n_local + (n_local & 1);
  bp5_mg_params mp;
  bp5_mg_params_default(&mp);
  mp.start_ids_host = ids.data();
  bp5_mg *mg;
  CHECK(bp5_elasticity_mg_create(n_levels, mfs.data(), coefs.data(), lambda, mu, ld, transfers.data(), &mp, &mg));

  // body force (0, 0, -1): b_2 = -int phi_i, zero on the clamped DoFs
  double *b, *x;
  CHECK(bp5_vec_alloc(3 * ld, &b));
  CHECK(bp5_vec_alloc(3 * ld, &x));
  CHECK(bp5_assemble_rhs(mf, x));                       // (x as scratch: the solver zeroes its owned entries)
  CHECK(bp5_vec_axpy(mf, b + 2 * ld, -1.0, x, n_local));
  double nb;
  CHECK(bp5_vec_l2_norm(mf, b + 2 * ld, mv.n_owned, &nb));

  bp5_cg_params prm{};
  prm.variant = BP5_CG_PLAIN; prm.max_iter = 500; prm.abs_tol = rel_tol * nb; prm.check_every = 0;
  bp5_cg_result res{};
  CHECK(bp5_cg_solve_elasticity_preconditioned(mf, coefs[0], lambda, mu, ld, bp5_mg_vmult, mg, b, x, &prm, &res));
  double xx = 0.0;
  for (int c = 0; c < 3; ++c) {
    double nc;
    CHECK(bp5_vec_l2_norm(mf, x + c * ld, mv.n_owned, &nc));
    xx += nc * nc;
  }
  printf("dofs %llu\niterations %d\nresidual %.6e\n", 3ull * (unsigned long long)mv.n_global_dofs, res.iterations, res.residual);
  for (int l = 0; l < n_levels; ++l) {
    bp5_mg_level o;
    CHECK(bp5_mg_level_info(mg, l, &o));
    printf("level%d %d %u %.12e %.12e\n", l, o.degree, o.n_owned, o.min_used, o.max_used);
  }
  printf("solution_norm %.15e\nsolve_ms %.3f\n", std::sqrt(xx), res.solve_ms);

  bp5_mg_destroy(mg);
  for (int l = 0; l + 1 < n_levels; ++l) bp5_mg_transfer_destroy(transfers[l]);
  bp5_vec_free(b); bp5_vec_free(x);
  for (int l = 0; l < n_levels; ++l) { bp5_vec_free(coefs[l]); bp5_mf_destroy(mfs[l]); bp5_mesh_destroy(meshes[l]); }
  return 0;
}
