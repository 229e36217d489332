// The trilinear geometry mode on the C ABI directly (include/bp5.h: BP5_GEOM_TRILINEAR; deal.II's default mapping MappingQ1): (grad v, grad u) = (v, 1)
// with zero Dirichlet values on n^3 straight-sided, skewed cells of the unit cube at degree p, one rank.  The mesh is the generator's sine mesh with
// every cell's nodes moved onto the trilinear image of its eight vertices -- what a hex mesh generator writes.  Solved twice with Jacobi-CG: on a
// handle that computes the metric from the cells' vertices inside the operator kernel (no metric array exists, coef = NULL), and on the default
// handle with its six stored planes.  Prints both iteration counts and both L2 norms of the solution.
//
//   bp5_q1_mapping <p> <n> <rel_tol> [deform_amp = 0.04]
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

// every cell's nodes onto the trilinear image of its vertices (the local entries (0|p, 0|p, 0|p)); cells that share a node agree on it
static void trilinearise(int p, uint32_t n_cells, const uint32_t *l2g, const double *nodes, std::vector<double> &X)
{
  const int n = p + 1, n3 = n * n * n;
  const std::vector<double> X0(X);
  for (uint32_t c = 0; c < n_cells; ++c) {
    const uint32_t *row = l2g + (size_t)c * n3;
    for (int k = 0; k < n; ++k)
      for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i)
          for (int e = 0; e < 3; ++e) {
            double x = 0.0;
            for (int v = 0; v < 8; ++v) {
              const int a = v & 1, b = (v >> 1) & 1, cc = v >> 2;
              const double w = (a ? nodes[i] : 1.0 - nodes[i]) * (b ? nodes[j] : 1.0 - nodes[j]) * (cc ? nodes[k] : 1.0 - nodes[k]);
              x += w * X0[3 * (size_t)row[a * p + n * (b * p + n * cc * p)] + e];
            }
            X[3 * (size_t)row[i + n * (j + n * k)] + e] = x;
          }
  }
}

int main(int argc, char **argv)
{
  if (argc < 4) {
    fprintf(stderr, "usage: %s p n rel_tol [deform_amp]\n", argv[0]);
    return 2;
  }
  bp5_mesh_desc md{};
  md.degree = atoi(argv[1]);
  const uint32_t n = (uint32_t)atoi(argv[2]);
  for (int d = 0; d < 3; ++d) md.cells[d] = n;
  md.h = 1.0 / n; md.deform_amp = argc > 4 ? atof(argv[4]) : 0.04; md.n_ranks = 1;
  const double rel_tol = atof(argv[3]);
  bp5_mesh *mesh;
  CHECK(bp5_mesh_create_brick(&md, &mesh));
  bp5_mesh_view mv;
  CHECK(bp5_mesh_view_get(mesh, &mv));
  const int p = mv.degree, n1 = p + 1;
  std::vector<double> nodes(n1), pts(n1), w(n1), N(n1 * n1), D(n1 * n1);
  CHECK(bp5_shape_tables(p, BP5_QUAD_GAUSS, nodes.data(), pts.data(), w.data(), N.data(), D.data()));
  const size_t n_local = (size_t)mv.n_owned + mv.n_ghost;
  std::vector<double> coords(mv.node_coords_host, mv.node_coords_host + 3 * n_local);
  trilinearise(p, mv.n_cells, mv.local_to_global_host, nodes.data(), coords);

  bp5_mf_desc d{};
  d.dim = 3; d.degree = p; d.quadrature = BP5_QUAD_GAUSS; d.coefficient = BP5_COEF_ONE;
  d.n_cells = mv.n_cells; d.n_interior_cells = mv.n_interior_cells; d.n_owned = mv.n_owned; d.n_ghost = mv.n_ghost;
  d.local_to_global_host = mv.local_to_global_host; d.node_coords_host = coords.data();
  d.constrained_host = mv.constrained_host; d.n_constrained = mv.n_constrained;
  d.n_cell_blocks = mv.n_cell_blocks; d.cell_block_offsets_host = mv.cell_block_offsets_host;

  printf("dofs=%llu\n", (unsigned long long)mv.n_global_dofs);
  const char *names[2] = {"trilinear", "merged6"};
  for (int run = 0; run < 2; ++run) {
    bp5_mf *mf;
    CHECK(bp5_mf_create(&d, &mf));
    double *coef = nullptr, *b, *x, *inv_diag;
    if (run == 0) {
      CHECK(bp5_mf_set_geometry_mode(mf, BP5_GEOM_TRILINEAR)); // checks the mesh: BP5_ERR_UNSUPPORTED "mesh is not trilinear" otherwise
    } else {
      size_t n_coef;
      CHECK(bp5_mf_coef_size(mf, &n_coef));
      CHECK(bp5_vec_alloc(n_coef, &coef));
      CHECK(bp5_mf_compute_merged_metric(mf, coef));
    }
    CHECK(bp5_vec_alloc(n_local, &b));
    CHECK(bp5_vec_alloc(n_local, &x));
    CHECK(bp5_vec_alloc(n_local, &inv_diag));
    CHECK(bp5_assemble_rhs(mf, b));
    CHECK(bp5_compute_diagonal(mf, coef, inv_diag, 1));
    double nb;
    CHECK(bp5_vec_l2_norm(mf, b, mv.n_owned, &nb));
    bp5_cg_params prm{};
    prm.variant = BP5_CG_PLAIN; prm.max_iter = 10000; prm.abs_tol = rel_tol * nb; prm.check_every = 0;
    bp5_cg_result res{};
    CHECK(bp5_cg_solve(mf, coef, inv_diag, b, x, &prm, &res));
    double l2;
    CHECK(bp5_l2_norm_solution(mf, x, &l2));
    CHECK(bp5_mf_sync(mf));
    printf("iterations_%s=%d\nresidual_%s=%.6e\nl2_norm_%s=%.15e\napply_kernel_%s=%s\n", names[run], res.iterations, names[run], res.residual, names[run], l2,
           names[run], res.apply_kernel);
    bp5_vec_free(b); bp5_vec_free(x); bp5_vec_free(inv_diag);
    if (coef) bp5_vec_free(coef);
    bp5_mf_destroy(mf);
  }
  bp5_mesh_destroy(mesh);
  return 0;
}
