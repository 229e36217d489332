// CEED BP6 -- the three-component twin of BP5 -- against the deal.II-shaped facade (include/bp5_dealii_facade.hpp): a vector Poisson problem
// on BlockVectors over ONE scalar DoFHandler.  The operator's vmult(BlockVector &, const BlockVector &) runs all components through one pass
// over the metric (bp5_apply_components); SolverCG solves the stacked system in one Krylov space with the scalar operator's inverse diagonal
// (bp5_cg_solve_components).  Right-hand side of component c: b_i (1 + 0.5 sin(0.37 (c + 1) i)), b = the BP5 load vector, i = the DoF index.
// Prints the iteration count and, per component, the L2 norm of the solution.
//
//   bp5_bp6 <p> <nx> <ny> <nz> <deform> <rel_tol> [coefficient]
//     coefficient: 0 = kappa 1, 1 = step-64's kappa (default)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bp5_dealii_facade.hpp"

using namespace bp5::dealii_facade;
using BlockVectorType = LinearAlgebra::distributed::BlockVector<double, MemorySpace::CUDA>;
constexpr unsigned int n_components = 3;

// the library's own Poisson operator on a brick mesh, applied to every block of a BlockVector
class VectorLaplaceOperator {
public:
  VectorLaplaceOperator(const bp5_mesh_view &mv, int coefficient)
  {
    bp5_mf_desc d{};
    d.dim = 3; d.degree = mv.degree; d.quadrature = BP5_QUAD_GAUSS; d.coefficient = coefficient;
    d.n_cells = mv.n_cells; d.n_interior_cells = mv.n_interior_cells; d.n_owned = mv.n_owned; d.n_ghost = mv.n_ghost;
    d.local_to_global_host = mv.local_to_global_host; d.node_coords_host = mv.node_coords_host;
    d.constrained_host = mv.constrained_host; d.n_constrained = mv.n_constrained;
    d.n_cell_blocks = mv.n_cell_blocks; d.cell_block_offsets_host = mv.cell_block_offsets_host;
    mf_data.reinit(d);
    n_owned = mv.n_owned; n_ghost = mv.n_ghost;
    size_t nc;
    check(bp5_mf_coef_size(mf_data.handle(), &nc));
    check(bp5_vec_alloc(nc, &coef_));
    check(bp5_mf_compute_merged_metric(mf_data.handle(), coef_));
  }
  ~VectorLaplaceOperator() { bp5_vec_free(coef_); }
  void vmult(BlockVectorType &dst, const BlockVectorType &src) const
  {
    check(bp5_apply_components(mf_data.handle(), coef_, (int)src.n_blocks(), src.leading_dimension(), src.get_values(), dst.get_values(), 1));
  }
  void initialize_dof_vector(BlockVectorType &v) const { v.reinit(n_components, mf_data.handle(), n_owned, n_ghost); }
  void compute_diagonal(double *diag, bool invert) const { check(bp5_compute_diagonal(mf_data.handle(), coef_, diag, invert ? 1 : 0)); }
  bp5_mf *handle() const { return mf_data.handle(); }
  const double *coef() const { return coef_; }
  size_t n_owned = 0, n_ghost = 0;

private:
  CUDAWrappers::MatrixFree<3, double> mf_data;
  double *coef_ = nullptr;
};

int main(int argc, char **argv)
{
  if (argc < 7) {
    fprintf(stderr, "usage: %s p nx ny nz deform rel_tol [coefficient]\n", argv[0]);
    return 2;
  }
  try {
    bp5_mesh_desc md{};
    md.degree = atoi(argv[1]);
    for (int d = 0; d < 3; ++d) md.cells[d] = (uint32_t)atoi(argv[2 + d]);
    md.h = 1.0; md.deform_amp = atof(argv[5]); md.n_ranks = 1;
    bp5_mesh *mesh;
    check(bp5_mesh_create_brick(&md, &mesh));
    bp5_mesh_view mv;
    check(bp5_mesh_view_get(mesh, &mv));
    {
      VectorLaplaceOperator A(mv, argc > 7 ? atoi(argv[7]) : BP5_COEF_STEP64);
      BlockVectorType b, x, r;
      A.initialize_dof_vector(b); A.initialize_dof_vector(x); A.initialize_dof_vector(r);
      // the scalar load vector, then one modulated copy per component
      double *b0, *inv;
      check(bp5_vec_alloc(A.n_owned + A.n_ghost, &b0));
      check(bp5_vec_alloc(A.n_owned + A.n_ghost, &inv));
      check(bp5_assemble_rhs(A.handle(), b0));
      check(bp5_mf_sync(A.handle()));
      std::vector<double> h(A.n_owned), hc(A.n_owned);
      check(bp5_copy_d2h(h.data(), b0, h.size() * sizeof(double)));
      for (unsigned int c = 0; c < n_components; ++c) {
        for (size_t i = 0; i < h.size(); ++i) hc[i] = h[i] * (1.0 + 0.5 * std::sin(0.37 * (c + 1) * (double)i));
        check(bp5_copy_h2d(b.block(c).get_values(), hc.data(), hc.size() * sizeof(double)));
      }
      A.compute_diagonal(inv, true);
      DiagonalMatrix preconditioner;
      preconditioner.diag = inv;
      SolverControl control(10000, atof(argv[6]) * b.l2_norm());
      SolverCG cg(control);
      cg.solve(A, x, b, preconditioner);
      // the FP64 residual of the stacked system, recomputed: r = b - A x
      A.vmult(r, x);
      for (unsigned int c = 0; c < n_components; ++c) r.block(c).sadd(-1.0, 1.0, b.block(c));
      printf("dofs %llu\ncomponents %u\niterations %u\nresidual %.6e\ntrue_residual %.6e\ntolerance %.6e\n", (unsigned long long)mv.n_global_dofs, x.n_blocks(),
             control.last_step(), control.last_value(), r.l2_norm(), control.tolerance);
      for (unsigned int c = 0; c < n_components; ++c) {
        double l2;
        check(bp5_l2_norm_solution(A.handle(), x.block(c).get_values(), &l2));
        printf("l2_norm_%u %.15e\n", c, l2);
      }
      printf("apply_kernel %s\nsolve_ms %.3f\n", cg.result.apply_kernel, cg.result.solve_ms);
      bp5_vec_free(b0); bp5_vec_free(inv);
    }
    bp5_mesh_destroy(mesh);
  } catch (const std::exception &e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
