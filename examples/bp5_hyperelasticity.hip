// Finite-strain neo-Hookean hyperelasticity on the C ABI directly (include/bp5.h: bp5_hyperelasticity_newton; the CEED "solids" mini-app's
// ElasFSInitialNH1F, deal.II step-44): a brick of nx x ny x nz cells of side 1 at degree p, sine-deformed, clamped on its whole boundary, energy scaled by
// the step-64 coefficient, under the body force (0, 0, -load).  Newton's method with backtracking from u = 0; every tangent system is solved by CG with
// the V-cycle of the LINEAR elasticity operator (levels p, p / 2, ..., 1 on the same cells) as preconditioner.  Prints the residual history.
//
//   bp5_hyperelasticity <p> <nx> <ny> <nz> <deform_amp> <lambda> <mu> <load>
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
    fprintf(stderr, "usage: %s p nx ny nz deform_amp lambda mu load\n", argv[0]);
    return 2;
  }
  const double lambda = atof(argv[6]), mu = atof(argv[7]), load = atof(argv[8]);
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

  // the state array and the body force (0, 0, -load): f_2 = -load int phi_i, zero on the clamped DoFs
  size_t n_state;
  double *state, *f, *u;
  CHECK(bp5_hyperelasticity_state_size(mf, &n_state));
  CHECK(bp5_vec_alloc(n_state, &state));
  CHECK(bp5_vec_alloc(3 * ld, &f));
  CHECK(bp5_vec_alloc(3 * ld, &u));
  CHECK(bp5_assemble_rhs(mf, u));                       // (u as scratch, zeroed again below)
  CHECK(bp5_vec_axpy(mf, f + 2 * ld, -load, u, n_local));
  CHECK(bp5_vec_fill(mf, u, 0.0, n_local));

  bp5_newton_params prm{};
  prm.max_newton = 20; prm.abs_tol = 0.0; prm.rel_tol = 1e-10; prm.cg_rel_tol = 1e-12; prm.max_backtracks = 8;
  prm.cg.variant = BP5_CG_PLAIN; prm.cg.max_iter = 2000; prm.cg.check_every = 0;
  bp5_newton_result res{};
  const int status = bp5_hyperelasticity_newton(mf, coefs[0], state, lambda, mu, ld, bp5_mg_vmult, mg, f, u, &prm, &res);
  printf("dofs %llu\n", 3ull * (unsigned long long)mv.n_global_dofs);
  for (int k = 0; k <= res.newton_iterations && k < 32; ++k) printf("newton_step %d %.12e\n", k, res.residual_history[k]);
  printf("newton_iterations %d\ncg_iterations %d\nbacktracks %d\nstatus %d\n", res.newton_iterations, res.total_cg_iterations, res.backtracks, status);
  if (status != BP5_OK) fprintf(stderr, "newton: %s: %s\n", bp5_strerror(status), bp5_last_error());
  double uu = 0.0;
  for (int c = 0; c < 3; ++c) {
    double nc;
    CHECK(bp5_vec_l2_norm(mf, u + c * ld, mv.n_owned, &nc));
    uu += nc * nc;
  }
  printf("solution_norm %.15e\n", std::sqrt(uu));

  bp5_mg_destroy(mg);
  for (int l = 0; l + 1 < n_levels; ++l) bp5_mg_transfer_destroy(transfers[l]);
  bp5_vec_free(f); bp5_vec_free(u); bp5_vec_free(state);
  for (int l = 0; l < n_levels; ++l) { bp5_vec_free(coefs[l]); bp5_mf_destroy(mfs[l]); bp5_mesh_destroy(meshes[l]); }
  return status == BP5_OK ? 0 : 1;
}
