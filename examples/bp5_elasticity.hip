// Linear elasticity on the C ABI directly (include/bp5.h: bp5_elasticity_*, bp5_cg_solve_elasticity; deal.II step-8, the CEED "solids" mini-app):
// a brick of nx x ny x nz cells of side 1 at degree p, sine-deformed, clamped on its whole boundary, stiffness scaled by the step-64 coefficient,
// under the body force (0, 0, -1) -- b_2 = -bp5_assemble_rhs, b_0 = b_1 = 0.  Jacobi-PCG (the block inverse diagonal) to a relative tolerance.
// Prints the iteration count, the residual and the L2 norm of each displacement component.
//
//   bp5_elasticity <p> <nx> <ny> <nz> <deform_amp> <lambda> <mu> <rel_tol>
#include <cstdio>
#include <cstdlib>

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
  bp5_mesh_desc md{};
  md.degree = atoi(argv[1]);
  for (int d = 0; d < 3; ++d) md.cells[d] = (uint32_t)atoi(argv[2 + d]);
  md.h = 1.0; md.deform_amp = atof(argv[5]); md.n_ranks = 1;
  const double lambda = atof(argv[6]), mu = atof(argv[7]), rel_tol = atof(argv[8]);
  bp5_mesh *mesh;
  CHECK(bp5_mesh_create_brick(&md, &mesh));
  bp5_mesh_view mv;
  CHECK(bp5_mesh_view_get(mesh, &mv));
  bp5_mf_desc d{};
  d.dim = 3; d.degree = mv.degree; d.quadrature = BP5_QUAD_GAUSS; d.coefficient = BP5_COEF_STEP64;
  d.n_cells = mv.n_cells; d.n_interior_cells = mv.n_interior_cells; d.n_owned = mv.n_owned; d.n_ghost = mv.n_ghost;
  d.local_to_global_host = mv.local_to_global_host; d.node_coords_host = mv.node_coords_host;
  d.constrained_host = mv.constrained_host; d.n_constrained = mv.n_constrained;
  d.n_cell_blocks = mv.n_cell_blocks; d.cell_block_offsets_host = mv.cell_block_offsets_host;
  bp5_mf *mf;
  CHECK(bp5_mf_create(&d, &mf));

  const size_t n_local = (size_t)mv.n_owned + mv.n_ghost, ld = n_local + (n_local & 1);
  size_t n_coef;
  CHECK(bp5_elasticity_coef_size(mf, &n_coef));
  double *coef, *b, *x, *inv_diag;
  CHECK(bp5_vec_alloc(n_coef, &coef));
  CHECK(bp5_vec_alloc(3 * ld, &b));
  CHECK(bp5_vec_alloc(3 * ld, &x));
  CHECK(bp5_vec_alloc(3 * ld, &inv_diag));
  CHECK(bp5_elasticity_compute_metric(mf, coef));
  CHECK(bp5_elasticity_compute_diagonal(mf, coef, lambda, mu, ld, inv_diag, 1));

  // body force (0, 0, -1): b_2 = -int phi_i, zero on the clamped DoFs
  CHECK(bp5_vec_fill(mf, b, 0.0, 3 * ld));
  CHECK(bp5_vec_fill(mf, x, 0.0, 3 * ld));
  CHECK(bp5_assemble_rhs(mf, x));                       // (x as scratch: the solver zeroes its owned entries)
  CHECK(bp5_vec_axpy(mf, b + 2 * ld, -1.0, x, n_local));
  double nb;
  CHECK(bp5_vec_l2_norm(mf, b + 2 * ld, mv.n_owned, &nb));

  bp5_cg_params prm{};
  prm.variant = BP5_CG_PLAIN; prm.max_iter = 10000; prm.abs_tol = rel_tol * nb; prm.check_every = 0;
  bp5_cg_result res{};
  CHECK(bp5_cg_solve_elasticity(mf, coef, lambda, mu, ld, inv_diag, b, x, &prm, &res));
  double l2[3];
  for (int c = 0; c < 3; ++c) CHECK(bp5_l2_norm_solution(mf, x + c * ld, &l2[c]));
  CHECK(bp5_mf_sync(mf));
  printf("dofs %llu\niterations %d\nresidual %.6e\n", 3ull * (unsigned long long)mv.n_global_dofs, res.iterations, res.residual);
  for (int c = 0; c < 3; ++c) printf("l2_norm_%d %.15e\n", c, l2[c]);
  printf("apply_kernel %s\n", res.apply_kernel);

  bp5_vec_free(coef); bp5_vec_free(b); bp5_vec_free(x); bp5_vec_free(inv_diag);
  bp5_mf_destroy(mf);
  bp5_mesh_destroy(mesh);
  return 0;
}
