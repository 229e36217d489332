// CEED BP1 -- the mass problem -- against the deal.II-shaped facade (include/bp5_dealii_facade.hpp): the L2 projection M x = b of
// f(x, y, z) = sin(pi x) sin(pi y) sin(pi z) exp(x y - z) on n^3 cells of the unit cube at degree p, one rank.  b = M f_h with f_h the nodal interpolant of f
// (zero on the boundary, like f), so the exact solution of the linear system is f_h itself.  MassOperatorNative is the library's native mass
// kernel (bp5_mf_set_operator(BP5_OP_MASS): one plane rho JxW); the facade's SolverCG solves with the inverse diagonal as DiagonalMatrix.
// Prints the iteration count, the L2 norm of x and the relative difference between x and f at the nodes.
//
//   bp5_bp1 <p> <n> <rel_tol>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bp5_dealii_facade.hpp"

using namespace bp5::dealii_facade;
using DeviceVector = LinearAlgebra::distributed::Vector<double, MemorySpace::CUDA>;

// == MatrixFreeOperators::MassOperator on the library's native kernel: (v, u), rho = 1
class MassOperatorNative {
public:
  explicit MassOperatorNative(const bp5_mesh_view &mv)
  {
    bp5_mf_desc d{};
    d.dim = 3; d.degree = mv.degree; d.quadrature = BP5_QUAD_GAUSS; d.coefficient = BP5_COEF_ONE;
    d.n_cells = mv.n_cells; d.n_interior_cells = mv.n_interior_cells; d.n_owned = mv.n_owned; d.n_ghost = mv.n_ghost;
    d.local_to_global_host = mv.local_to_global_host; d.node_coords_host = mv.node_coords_host;
    d.constrained_host = mv.constrained_host; d.n_constrained = mv.n_constrained;
    d.n_cell_blocks = mv.n_cell_blocks; d.cell_block_offsets_host = mv.cell_block_offsets_host;
    mf_data.reinit(d);
    check(bp5_mf_set_operator(mf_data.handle(), BP5_OP_MASS));
    size_t nc;
    check(bp5_mf_coef_size(mf_data.handle(), &nc)); // one plane: rho JxW
    check(bp5_vec_alloc(nc, &plane));
    check(bp5_mf_compute_merged_metric(mf_data.handle(), plane));
  }
  ~MassOperatorNative() { bp5_vec_free(plane); }
  void vmult(DeviceVector &dst, const DeviceVector &src) const
  {
    check(bp5_apply(mf_data.handle(), plane, static_cast<const double *>(src.get_values()), dst.get_values(), 1));
  }
  void initialize_dof_vector(DeviceVector &v) const { mf_data.initialize_dof_vector(v); }
  void compute_diagonal(double *diag, bool invert) const { check(bp5_compute_diagonal(mf_data.handle(), plane, diag, invert ? 1 : 0)); }
  bp5_mf *handle() const { return mf_data.handle(); }
  const double *coef() const { return plane; }
  CUDAWrappers::MatrixFree<3, double> mf_data;

private:
  double *plane = nullptr;
};

int main(int argc, char **argv)
{
  if (argc < 4) {
    fprintf(stderr, "usage: %s p n rel_tol\n", argv[0]);
    return 2;
  }
  try {
    bp5_mesh_desc md{};
    md.degree = atoi(argv[1]);
    const uint32_t n = (uint32_t)atoi(argv[2]);
    for (int d = 0; d < 3; ++d) md.cells[d] = n;
    md.h = 1.0 / n; md.deform_amp = 0.0; md.n_ranks = 1;
    bp5_mesh *mesh;
    check(bp5_mesh_create_brick(&md, &mesh));
    bp5_mesh_view mv;
    check(bp5_mesh_view_get(mesh, &mv));
    {
      MassOperatorNative M(mv);
      DeviceVector f, b, x;
      M.initialize_dof_vector(f); M.initialize_dof_vector(b); M.initialize_dof_vector(x);
      const size_t n_local = (size_t)mv.n_owned + mv.n_ghost;
      const double pi = std::acos(-1.0);
      std::vector<double> fh(n_local);
      for (size_t i = 0; i < n_local; ++i) {
        const double X = mv.node_coords_host[3 * i], Y = mv.node_coords_host[3 * i + 1], Z = mv.node_coords_host[3 * i + 2];
        fh[i] = std::sin(pi * X) * std::sin(pi * Y) * std::sin(pi * Z) * std::exp(X * Y - Z);
      }
      check(bp5_copy_h2d(f.get_values(), fh.data(), n_local * sizeof(double)));
      M.vmult(b, f);
      check(bp5_set_constrained(M.handle(), 0.0, b.get_values())); // homogeneous Dirichlet rows, as assemble_rhs leaves them
      double *inv;
      check(bp5_vec_alloc(n_local, &inv));
      M.compute_diagonal(inv, true);
      DiagonalMatrix preconditioner;
      preconditioner.diag = inv;
      SolverControl control(10000, atof(argv[3]) * b.l2_norm());
      SolverCG cg(control);
      cg.solve(M, x, b, preconditioner);
      double l2;
      check(bp5_l2_norm_solution(M.handle(), x.get_values(), &l2));
      check(bp5_mf_sync(M.handle()));
      std::vector<double> xh(n_local);
      check(bp5_copy_d2h(xh.data(), x.get_values(), n_local * sizeof(double)));
      double num = 0, den = 0;
      for (size_t i = 0; i < mv.n_owned; ++i) { num += (xh[i] - fh[i]) * (xh[i] - fh[i]); den += fh[i] * fh[i]; }
      printf("dofs=%llu\niterations=%u\nresidual=%.6e\nl2_norm=%.15e\nrel_diff=%.3e\napply_kernel=%s\n", (unsigned long long)mv.n_global_dofs, control.last_step(),
             control.last_value(), l2, std::sqrt(num / den), cg.result.apply_kernel);
      bp5_vec_free(inv);
    }
    bp5_mesh_destroy(mesh);
  } catch (const std::exception &e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
