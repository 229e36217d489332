// Multigrid-preconditioned CG written like the solve of deal.II's step-37 (Poisson with step-64's kappa), against the deal.II-shaped
// facade (include/bp5_dealii_facade.hpp): the operators of the levels p, p / 2, ..., 1 on the same cells, then up to h_levels degree-1
// levels on 2:1 coarser meshes (step-75's global coarsening), PreconditionMG (V-cycle, Chebyshev smoothers, Chebyshev coarse solver),
// SolverCG.  Prints the iteration count, the levels and the solution's norm.
//
//   bp5_multigrid <p> <nx> <ny> <nz> <deform> <rel_tol> [coefficient] [h_levels] [metric_precision]
//     coefficient: 0 = kappa 1, 1 = step-64's kappa (default)
//     h_levels: h-levels below degree 1 (default 0); coarsening stops at an odd cell count or below 4 cells in a direction
//     metric_precision: float64 (default) | float32 = the level operators of the preconditioner keep their metric planes as floats
//       (step-37's mixed-precision multigrid as far as the planes go); the outer CG runs on an FP64 operator of the fine level
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "bp5_dealii_facade.hpp"

using namespace bp5::dealii_facade;

// the library's own Poisson operator on a brick mesh: handle() + coef() make the facade's solvers and PreconditionMG run it natively
class LaplaceOperator {
public:
  LaplaceOperator(const bp5_mesh_view &mv, int coefficient, int metric_precision = BP5_METRIC_F64)
  {
    bp5_mf_desc d{};
    d.dim = 3; d.degree = mv.degree; d.quadrature = BP5_QUAD_GAUSS; d.coefficient = coefficient;
    d.n_cells = mv.n_cells; d.n_interior_cells = mv.n_interior_cells; d.n_owned = mv.n_owned; d.n_ghost = mv.n_ghost;
    d.local_to_global_host = mv.local_to_global_host; d.node_coords_host = mv.node_coords_host;
    d.constrained_host = mv.constrained_host; d.n_constrained = mv.n_constrained;
    d.n_cell_blocks = mv.n_cell_blocks; d.cell_block_offsets_host = mv.cell_block_offsets_host;
    mf_data.reinit(d);
    if (metric_precision != BP5_METRIC_F64) mf_data.set_metric_precision(metric_precision);
    n_owned = mv.n_owned;
    size_t nc;
    check(bp5_mf_coef_size(mf_data.handle(), &nc));
    check(bp5_vec_alloc(nc, &coef_));
    check(bp5_mf_compute_merged_metric(mf_data.handle(), coef_));
  }
  ~LaplaceOperator() { bp5_vec_free(coef_); }
  void vmult(double *dst, const double *src) const { check(bp5_apply(mf_data.handle(), coef_, src, dst, 1)); }
  void initialize_dof_vector(double **v) const { mf_data.initialize_dof_vector(v); }
  // == MatrixFreeOperators::Base::compute_diagonal + inverse (step-37: the Jacobi part of the Chebyshev smoother)
  void compute_diagonal(double *diag, bool invert) const { check(bp5_compute_diagonal(mf_data.handle(), coef_, diag, invert ? 1 : 0)); }
  bp5_mf *handle() const { return mf_data.handle(); }
  const double *coef() const { return coef_; }
  size_t n_owned = 0;

private:
  CUDAWrappers::MatrixFree<3, double> mf_data;
  double *coef_ = nullptr;
};

int main(int argc, char **argv)
{
  if (argc < 7) {
    fprintf(stderr, "usage: %s p nx ny nz deform rel_tol [coefficient] [h_levels] [float64|float32]\n", argv[0]);
    return 2;
  }
  try {
    const int coefficient = argc > 7 ? atoi(argv[7]) : BP5_COEF_STEP64;
    const int h_levels = argc > 8 ? atoi(argv[8]) : 0;
    if (argc > 9 && std::string(argv[9]) != "float32" && std::string(argv[9]) != "float64") {
      fprintf(stderr, "unknown metric precision '%s'\nusage: %s p nx ny nz deform rel_tol [coefficient] [h_levels] [float64|float32]\n", argv[9], argv[0]);
      return 2;
    }
    const int precision = argc > 9 && std::string(argv[9]) == "float32" ? BP5_METRIC_F32 : BP5_METRIC_F64;
    std::vector<bp5_mesh *> meshes;
    std::vector<bp5_mesh_view> views;
    for (int p = atoi(argv[1]);; p = p / 2 > 1 ? p / 2 : 1) { // the hierarchy p, p / 2, ..., 1 on the same cells
      bp5_mesh_desc md{};
      md.degree = p;
      for (int d = 0; d < 3; ++d) md.cells[d] = (uint32_t)atoi(argv[2 + d]);
      md.h = 1.0; md.deform_amp = atof(argv[5]); md.n_ranks = 1;
      bp5_mesh *mesh;
      check(bp5_mesh_create_brick(&md, &mesh));
      bp5_mesh_view mv;
      check(bp5_mesh_view_get(mesh, &mv));
      meshes.push_back(mesh);
      views.push_back(mv);
      if (p == 1) break;
    }
    // h-levels at degree 1 (BrickMesh.coarsen's rule on one rank), with the parent maps of their transfers
    std::vector<std::vector<uint32_t>> parents(views.size() - 1);
    std::vector<std::vector<uint8_t>> children(views.size() - 1);
    for (int k = 0; k < h_levels; ++k) {
      bp5_mesh_desc md{};
      md.degree = 1;
      md.h = double(2 << k); md.deform_amp = atof(argv[5]); md.n_ranks = 1;
      bool ok = true;
      for (int d = 0; d < 3; ++d) {
        const uint32_t n = views.back().global_dofs_per_dir[d] - 1; // cells of the level above (degree 1)
        ok = ok && n % 2 == 0 && n / 2 >= 4;
        md.cells[d] = n / 2;
      }
      if (!ok) break;
      bp5_mesh *mesh;
      check(bp5_mesh_create_brick(&md, &mesh));
      bp5_mesh_view mv;
      check(bp5_mesh_view_get(mesh, &mv));
      parents.emplace_back(views.back().n_cells);
      children.emplace_back(views.back().n_cells);
      check(bp5_mesh_parent_cells(meshes.back(), mesh, parents.back().data(), children.back().data()));
      meshes.push_back(mesh);
      views.push_back(mv);
    }
    {
      std::vector<std::unique_ptr<LaplaceOperator>> ops;
      std::vector<const LaplaceOperator *> levels;
      PreconditionMG::AdditionalData data;
      for (const bp5_mesh_view &mv : views) {
        ops.emplace_back(new LaplaceOperator(mv, coefficient, precision));
        levels.push_back(ops.back().get());
        data.start_ids_host.push_back(mv.global_ids_host);
      }
      // float planes on the levels: the outer CG's operator is an FP64 twin of level 0, so the solution is the FP64 solution
      std::unique_ptr<LaplaceOperator> outer;
      if (precision != BP5_METRIC_F64) outer.reset(new LaplaceOperator(views[0], coefficient));
      for (size_t l = 0; l < parents.size(); ++l) {
        data.parent_cells.push_back(parents[l].empty() ? nullptr : parents[l].data());
        data.child.push_back(children[l].empty() ? nullptr : children[l].data());
      }
      const LaplaceOperator &A = outer ? *outer : *ops[0];
      double *b, *x;
      A.initialize_dof_vector(&b); A.initialize_dof_vector(&x);
      check(bp5_assemble_rhs(A.handle(), b));
      PreconditionMG P;
      P.initialize(levels, data);
      double bnorm;
      check(bp5_vec_l2_norm(A.handle(), b, A.n_owned, &bnorm));
      SolverControl control(1000, atof(argv[6]) * bnorm);
      SolverCG cg(control);
      cg.solve(A, x, b, P);
      double xnorm;
      check(bp5_vec_l2_norm(A.handle(), x, A.n_owned, &xnorm));
      printf("dofs %llu\niterations %u\nresidual %.6e\n", (unsigned long long)views[0].n_global_dofs, control.last_step(), control.last_value());
      for (int l = 0; l < (int)levels.size(); ++l) {
        const bp5_mg_level o = P.level_info(l);
        printf("level%d %d %u %.12e %.12e\n", l, o.degree, o.n_owned, o.min_used, o.max_used);
      }
      if (outer) printf("metric_precision float32\n");
      printf("solution_norm %.15e\nsolve_ms %.3f\n", xnorm, cg.result.solve_ms);
      P.clear();
      bp5_vec_free(b); bp5_vec_free(x);
    }
    for (bp5_mesh *m : meshes) bp5_mesh_destroy(m);
  } catch (const std::exception &e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
