// CEED BP3 -- the Poisson problem with Gauss(p+2) quadrature -- against the deal.II-shaped facade (include/bp5_dealii_facade.hpp):
// (grad v, grad u) = (v, 1) with zero Dirichlet values on n^3 deformed cells of the unit cube at degree p, one rank.  PoissonOperatorBP3 is the
// library's native over-integrated kernel (quadrature BP5_QUAD_GAUSS_OVER: six planes of (p+2)^3 entries per cell) over the C ABI descriptor -- the
// facade's MatrixFree holds n_q_points_1d == p + 1 and refuses the id; the facade's Vector and SolverCG take the operator through handle() and
// coef(), with the inverse diagonal as DiagonalMatrix.  Prints the iteration count, the residual and the L2 norm of the solution.
//
//   bp5_bp3 <p> <n> <rel_tol> [deform_amp = 0.04]
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "bp5_dealii_facade.hpp"

using namespace bp5::dealii_facade;
using DeviceVector = LinearAlgebra::distributed::Vector<double, MemorySpace::CUDA>;

// == BP5::PoissonOperator (bp5/step-64.cu:198-276) with FEEvaluation<dim, p, p + 2> (bp5/fe_evaluation_gl.h:28)
class PoissonOperatorBP3 {
public:
  explicit PoissonOperatorBP3(const bp5_mesh_view &mv) : n_owned(mv.n_owned), n_ghost(mv.n_ghost)
  {
    bp5_mf_desc d{};
    d.dim = 3; d.degree = mv.degree; d.quadrature = BP5_QUAD_GAUSS_OVER; d.coefficient = BP5_COEF_ONE;
    d.n_cells = mv.n_cells; d.n_interior_cells = mv.n_interior_cells; d.n_owned = mv.n_owned; d.n_ghost = mv.n_ghost;
    d.local_to_global_host = mv.local_to_global_host; d.node_coords_host = mv.node_coords_host;
    d.constrained_host = mv.constrained_host; d.n_constrained = mv.n_constrained;
    d.n_cell_blocks = mv.n_cell_blocks; d.cell_block_offsets_host = mv.cell_block_offsets_host;
    check(bp5_mf_create(&d, &mf));
    size_t nc;
    check(bp5_mf_coef_size(mf, &nc)); // 6 n_cells (p+2)^3
    check(bp5_vec_alloc(nc, &planes));
    check(bp5_mf_compute_merged_metric(mf, planes));
  }
  ~PoissonOperatorBP3() { bp5_vec_free(planes); bp5_mf_destroy(mf); }
  PoissonOperatorBP3(const PoissonOperatorBP3 &) = delete;
  PoissonOperatorBP3 &operator=(const PoissonOperatorBP3 &) = delete;
  void vmult(DeviceVector &dst, const DeviceVector &src) const
  {
    check(bp5_apply(mf, planes, static_cast<const double *>(src.get_values()), dst.get_values(), 1));
  }
  void initialize_dof_vector(DeviceVector &v) const { v.reinit(mf, n_owned, n_ghost); }
  void compute_diagonal(double *diag, bool invert) const { check(bp5_compute_diagonal(mf, planes, diag, invert ? 1 : 0)); }
  bp5_mf *handle() const { return mf; }
  const double *coef() const { return planes; }

private:
  bp5_mf *mf = nullptr;
  double *planes = nullptr;
  size_t n_owned, n_ghost;
};

int main(int argc, char **argv)
{
  if (argc < 4) {
    fprintf(stderr, "usage: %s p n rel_tol [deform_amp]\n", argv[0]);
    return 2;
  }
  try {
    bp5_mesh_desc md{};
    md.degree = atoi(argv[1]);
    const uint32_t n = (uint32_t)atoi(argv[2]);
    for (int d = 0; d < 3; ++d) md.cells[d] = n;
    md.h = 1.0 / n; md.deform_amp = argc > 4 ? atof(argv[4]) : 0.04; md.n_ranks = 1;
    bp5_mesh *mesh;
    check(bp5_mesh_create_brick(&md, &mesh));
    bp5_mesh_view mv;
    check(bp5_mesh_view_get(mesh, &mv));
    {
      PoissonOperatorBP3 A(mv);
      DeviceVector b, x;
      A.initialize_dof_vector(b); A.initialize_dof_vector(x);
      check(bp5_assemble_rhs(A.handle(), b.get_values())); // b_i = int phi_i with Gauss(p+1): its definition, whatever the operator's quadrature
      const size_t n_local = (size_t)mv.n_owned + mv.n_ghost;
      double *inv;
      check(bp5_vec_alloc(n_local, &inv));
      A.compute_diagonal(inv, true);
      DiagonalMatrix preconditioner;
      preconditioner.diag = inv;
      SolverControl control(10000, atof(argv[3]) * b.l2_norm());
      SolverCG cg(control);
      cg.solve(A, x, b, preconditioner);
      double l2;
      check(bp5_l2_norm_solution(A.handle(), x.get_values(), &l2));
      check(bp5_mf_sync(A.handle()));
      printf("dofs=%llu\niterations=%u\nresidual=%.6e\nl2_norm=%.15e\napply_kernel=%s\n", (unsigned long long)mv.n_global_dofs, control.last_step(),
             control.last_value(), l2, cg.result.apply_kernel);
      bp5_vec_free(inv);
    }
    bp5_mesh_destroy(mesh);
  } catch (const std::exception &e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
