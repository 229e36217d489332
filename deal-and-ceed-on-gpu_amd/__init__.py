"""MI355X-native BP5 matrix-free operator + CG hot path (host-side mirror of the reference's
operator interface: PoissonOperator / MatrixFree / SolverCG / SolverCGFullMerge,
peterrum/deal-and-ceed-on-gpu bp5/step-64.cu, bp5/solver.h).

All compute goes through the C ABI of include/bp5.h (libbp5.so, hand-written HIP for gfx950).
There is NO CPU fallback: importing works anywhere, compute calls fail loudly without the
library or without a GPU."""
from ._lib import (BP5Error, QUAD_GAUSS, QUAD_GLL, QUAD_GAUSS_OVER, COEF_ONE, COEF_STEP64, CG_PLAIN, CG_MERGED, GEOM_MERGED6, GEOM_AFFINE, GEOM_TRILINEAR, OP_POISSON, OP_HELMHOLTZ, OP_MASS, build, lib,
                   lib_path, shape_tables, quadrature_points_1d, tridiagonal_eigenvalues, HEADER_SYMBOLS)
from .mesh import BrickMesh
from .matrix_free import (MatrixFree, PoissonOperator, HelmholtzOperator, MassOperator, ElasticityOperator, HyperelasticityOperator, NewtonSolver, DiagonalMatrix, IterationNumberControl, SolverControl,
                          SolverCG, SolverCGFullMerge, Communicator, Vector, PreconditionChebyshev,
                          MGTwoLevelTransfer, PreconditionMG, make_mg_hierarchy, mg_coarse_degrees,
                          ElasticityPreconditionChebyshev, ElasticityPreconditionMG, make_elasticity_mg_hierarchy)

__all__ = ["BP5Error", "QUAD_GAUSS", "QUAD_GLL", "QUAD_GAUSS_OVER", "COEF_ONE", "COEF_STEP64", "CG_PLAIN", "CG_MERGED", "GEOM_MERGED6", "GEOM_AFFINE", "GEOM_TRILINEAR", "OP_POISSON", "OP_HELMHOLTZ", "OP_MASS", "build", "lib",
           "lib_path", "shape_tables", "quadrature_points_1d", "HEADER_SYMBOLS", "BrickMesh", "MatrixFree", "PoissonOperator", "HelmholtzOperator", "MassOperator", "ElasticityOperator", "HyperelasticityOperator", "NewtonSolver",
           "DiagonalMatrix", "IterationNumberControl", "SolverControl", "SolverCG", "SolverCGFullMerge",
           "Communicator", "Vector", "PreconditionChebyshev", "tridiagonal_eigenvalues",
           "MGTwoLevelTransfer", "PreconditionMG", "make_mg_hierarchy", "mg_coarse_degrees",
           "ElasticityPreconditionChebyshev", "ElasticityPreconditionMG", "make_elasticity_mg_hierarchy"]
