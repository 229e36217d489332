"""Which operator kernel a solve launches, pinned by name.

Variant 56 (the block kernel's default shape) picks one build out of a list that depends on the operator class (Poisson on double or
float metric planes, Helmholtz, hanging nodes, affine geometry), on the plan (every block a lattice block, or packed indices), on what
the solver asks for (dot products fused into the write-out) and on the streaming policy.  The names below are what
bp5_cg_result.apply_kernel reports, spelled out as literals: a change of the dispatch that launches another build for the same input
fails here.  Every case also compares the solution with the same solve through the handle's own atomic pencil kernel (whose name is
pinned too): a right name on a wrong launch does not pass.

The meshes are the smallest with several bricks, partial bricks and a plan that fits LDS (those of
test_lattice_blocks_need_no_index_stream); eight workgroups, two CG iterations.  Both solvers take d.h from the block kernel when fusion
is on (the plain solver wants p.v only), so the rows are: SolverCGFullMerge fused, SolverCG fused, SolverCG with fusion switched off."""
import functools

import pytest

import bp5_pkg
from test_gpu_parity import _hanging_namespace, _refined, _with_cell_blocks

pytestmark = pytest.mark.gpu
pkg = bp5_pkg.load()
INVALID, UNSUPPORTED = 1, 5                       # bp5.h: BP5_ERR_INVALID, BP5_ERR_UNSUPPORTED
ITS = 2

# degree -> (cells, cell block)
BRICKS = {1: ((17, 9, 10), (8, 8, 8)), 2: ((9, 8, 5), (8, 8, 4)), 3: ((9, 5, 6), (8, 4, 4)), 4: ((9, 8, 6), (4, 4, 4)),
          5: ((7, 5, 3), (6, 4, 2)), 6: ((5, 4, 3), (4, 4, 2)), 7: ((5, 3, 3), (4, 2, 2)), 8: ((3, 3, 3), (2, 2, 2))}
# degree -> (pattern, deformation, cells per group): the 2:1 meshes of test_hanging_nodes_in_the_deterministic_block_kernel
HANGING = {1: ("stairs", 0.0, 3), 2: ("stairs", 0.03, 3), 3: ("L", 0.0, 2), 4: ("L", 0.02, 2), 5: ("stairs", 0.0, 3), 6: ("L", 0.02, 2),
           7: ("L", 0.0, 2), 8: ("L", 0.02, 1)}

# (class, degree, quadrature) -> {(fused, lattice_indices, streaming): kernel}, variant 56
BLOCK_KERNEL = {
    ("poisson", 1, 0): {
        (1, 1, 0): "apply_block_kernel<1,false,4,1,18114560>", (1, 1, 1): "apply_block_kernel<1,false,4,1,18114560>",
        (1, 0, 0): "apply_block_kernel<1,false,4,1,1337344>", (1, 0, 1): "apply_block_kernel<1,false,4,1,1337344>",
        (0, 1, 0): "apply_block_kernel<1,false,4,1,17065984>", (0, 1, 1): "apply_block_kernel<1,false,4,1,17065984>",
        (0, 0, 0): "apply_block_kernel<1,false,4,1,288768>", (0, 0, 1): "apply_block_kernel<1,false,4,1,288768>",
    },
    ("poisson", 1, 1): {
        (1, 1, 0): "apply_block_kernel<1,true,4,1,18114560>", (1, 1, 1): "apply_block_kernel<1,true,4,1,18114560>",
        (1, 0, 0): "apply_block_kernel<1,true,4,1,1337344>", (1, 0, 1): "apply_block_kernel<1,true,4,1,1337344>",
        (0, 1, 0): "apply_block_kernel<1,true,4,1,17065984>", (0, 1, 1): "apply_block_kernel<1,true,4,1,17065984>",
        (0, 0, 0): "apply_block_kernel<1,true,4,1,288768>", (0, 0, 1): "apply_block_kernel<1,true,4,1,288768>",
    },
    ("poisson", 2, 0): {
        (1, 1, 0): "apply_block_kernel<2,false,9,1,18114560>", (1, 1, 1): "apply_block_kernel<2,false,9,1,18114560>",
        (1, 0, 0): "apply_block_kernel<2,false,9,1,1337344>", (1, 0, 1): "apply_block_kernel<2,false,9,1,1337344>",
        (0, 1, 0): "apply_block_kernel<2,false,9,1,17065984>", (0, 1, 1): "apply_block_kernel<2,false,9,1,17065984>",
        (0, 0, 0): "apply_block_kernel<2,false,9,1,288768>", (0, 0, 1): "apply_block_kernel<2,false,9,1,288768>",
    },
    ("poisson", 2, 1): {
        (1, 1, 0): "apply_block_kernel<2,true,9,1,18114560>", (1, 1, 1): "apply_block_kernel<2,true,9,1,18114560>",
        (1, 0, 0): "apply_block_kernel<2,true,9,1,1337344>", (1, 0, 1): "apply_block_kernel<2,true,9,1,1337344>",
        (0, 1, 0): "apply_block_kernel<2,true,9,1,17065984>", (0, 1, 1): "apply_block_kernel<2,true,9,1,17065984>",
        (0, 0, 0): "apply_block_kernel<2,true,9,1,288768>", (0, 0, 1): "apply_block_kernel<2,true,9,1,288768>",
    },
    ("poisson", 3, 0): {
        (1, 1, 0): "apply_block_kernel<3,false,16,1,18114560>", (1, 1, 1): "apply_block_kernel<3,false,16,1,18114560>",
        (1, 0, 0): "apply_block_kernel<3,false,16,1,1337344>", (1, 0, 1): "apply_block_kernel<3,false,16,1,1337344>",
        (0, 1, 0): "apply_block_kernel<3,false,16,1,17065984>", (0, 1, 1): "apply_block_kernel<3,false,16,1,17065984>",
        (0, 0, 0): "apply_block_kernel<3,false,16,1,288768>", (0, 0, 1): "apply_block_kernel<3,false,16,1,288768>",
    },
    ("poisson", 3, 1): {
        (1, 1, 0): "apply_block_kernel<3,true,16,1,18114560>", (1, 1, 1): "apply_block_kernel<3,true,16,1,18114560>",
        (1, 0, 0): "apply_block_kernel<3,true,16,1,1337344>", (1, 0, 1): "apply_block_kernel<3,true,16,1,1337344>",
        (0, 1, 0): "apply_block_kernel<3,true,16,1,17065984>", (0, 1, 1): "apply_block_kernel<3,true,16,1,17065984>",
        (0, 0, 0): "apply_block_kernel<3,true,16,1,288768>", (0, 0, 1): "apply_block_kernel<3,true,16,1,288768>",
    },
    ("poisson", 4, 0): {
        (1, 1, 0): "apply_block_kernel<4,false,32,1,286550016>", (1, 1, 1): "apply_block_kernel<4,false,32,1,286582784>",
        (1, 0, 0): "apply_block_kernel<4,false,32,1,1337344>", (1, 0, 1): "apply_block_kernel<4,false,32,1,1337344>",
        (0, 1, 0): "apply_block_kernel<4,false,32,1,285501440>", (0, 1, 1): "apply_block_kernel<4,false,32,1,285534208>",
        (0, 0, 0): "apply_block_kernel<4,false,32,1,288768>", (0, 0, 1): "apply_block_kernel<4,false,32,1,288768>",
    },
    ("poisson", 4, 1): {
        (1, 1, 0): "apply_block_kernel<4,true,32,1,286550016>", (1, 1, 1): "apply_block_kernel<4,true,32,1,286550016>",
        (1, 0, 0): "apply_block_kernel<4,true,32,1,1337344>", (1, 0, 1): "apply_block_kernel<4,true,32,1,1337344>",
        (0, 1, 0): "apply_block_kernel<4,true,32,1,285501440>", (0, 1, 1): "apply_block_kernel<4,true,32,1,285501440>",
        (0, 0, 0): "apply_block_kernel<4,true,32,1,288768>", (0, 0, 1): "apply_block_kernel<4,true,32,1,288768>",
    },
    ("poisson", 5, 0): {
        (1, 1, 0): "apply_block_kernel<5,false,36,1,18114560>", (1, 1, 1): "apply_block_kernel<5,false,36,1,18114560>",
        (1, 0, 0): "apply_block_kernel<5,false,36,1,1337344>", (1, 0, 1): "apply_block_kernel<5,false,36,1,1337344>",
        (0, 1, 0): "apply_block_kernel<5,false,36,1,17065984>", (0, 1, 1): "apply_block_kernel<5,false,36,1,17065984>",
        (0, 0, 0): "apply_block_kernel<5,false,36,1,288768>", (0, 0, 1): "apply_block_kernel<5,false,36,1,288768>",
    },
    ("poisson", 5, 1): {
        (1, 1, 0): "apply_block_kernel<5,true,36,1,18114560>", (1, 1, 1): "apply_block_kernel<5,true,36,1,18114560>",
        (1, 0, 0): "apply_block_kernel<5,true,36,1,1337344>", (1, 0, 1): "apply_block_kernel<5,true,36,1,1337344>",
        (0, 1, 0): "apply_block_kernel<5,true,36,1,17065984>", (0, 1, 1): "apply_block_kernel<5,true,36,1,17065984>",
        (0, 0, 0): "apply_block_kernel<5,true,36,1,288768>", (0, 0, 1): "apply_block_kernel<5,true,36,1,288768>",
    },
    ("poisson", 6, 0): {
        (1, 1, 0): "apply_block_kernel<6,false,64,1,18114560>", (1, 1, 1): "apply_block_kernel<6,false,64,1,18114560>",
        (1, 0, 0): "apply_block_kernel<6,false,64,1,1337344>", (1, 0, 1): "apply_block_kernel<6,false,64,1,1337344>",
        (0, 1, 0): "apply_block_kernel<6,false,64,1,17065984>", (0, 1, 1): "apply_block_kernel<6,false,64,1,17065984>",
        (0, 0, 0): "apply_block_kernel<6,false,64,1,288768>", (0, 0, 1): "apply_block_kernel<6,false,64,1,288768>",
    },
    ("poisson", 6, 1): {
        (1, 1, 0): "apply_block_kernel<6,true,64,1,18114560>", (1, 1, 1): "apply_block_kernel<6,true,64,1,18114560>",
        (1, 0, 0): "apply_block_kernel<6,true,64,1,1337344>", (1, 0, 1): "apply_block_kernel<6,true,64,1,1337344>",
        (0, 1, 0): "apply_block_kernel<6,true,64,1,17065984>", (0, 1, 1): "apply_block_kernel<6,true,64,1,17065984>",
        (0, 0, 0): "apply_block_kernel<6,true,64,1,288768>", (0, 0, 1): "apply_block_kernel<6,true,64,1,288768>",
    },
    ("poisson", 7, 0): {
        (1, 1, 0): "apply_block_kernel<7,false,64,1,18114560>", (1, 1, 1): "apply_block_kernel<7,false,64,1,18114560>",
        (1, 0, 0): "apply_block_kernel<7,false,64,1,1337344>", (1, 0, 1): "apply_block_kernel<7,false,64,1,1337344>",
        (0, 1, 0): "apply_block_kernel<7,false,64,1,17065984>", (0, 1, 1): "apply_block_kernel<7,false,64,1,17065984>",
        (0, 0, 0): "apply_block_kernel<7,false,64,1,288768>", (0, 0, 1): "apply_block_kernel<7,false,64,1,288768>",
    },
    ("poisson", 7, 1): {
        (1, 1, 0): "apply_block_kernel<7,true,64,1,18114560>", (1, 1, 1): "apply_block_kernel<7,true,64,1,18114560>",
        (1, 0, 0): "apply_block_kernel<7,true,64,1,1337344>", (1, 0, 1): "apply_block_kernel<7,true,64,1,1337344>",
        (0, 1, 0): "apply_block_kernel<7,true,64,1,17065984>", (0, 1, 1): "apply_block_kernel<7,true,64,1,17065984>",
        (0, 0, 0): "apply_block_kernel<7,true,64,1,288768>", (0, 0, 1): "apply_block_kernel<7,true,64,1,288768>",
    },
    ("poisson", 8, 0): {
        (1, 1, 0): "apply_block_kernel<8,false,81,1,18114560>", (1, 1, 1): "apply_block_kernel<8,false,81,1,18114560>",
        (1, 0, 0): "apply_block_kernel<8,false,81,1,1337344>", (1, 0, 1): "apply_block_kernel<8,false,81,1,1337344>",
        (0, 1, 0): "apply_block_kernel<8,false,81,1,17065984>", (0, 1, 1): "apply_block_kernel<8,false,81,1,17065984>",
        (0, 0, 0): "apply_block_kernel<8,false,81,1,288768>", (0, 0, 1): "apply_block_kernel<8,false,81,1,288768>",
    },
    ("poisson", 8, 1): {
        (1, 1, 0): "apply_block_kernel<8,true,81,1,18114560>", (1, 1, 1): "apply_block_kernel<8,true,81,1,18114560>",
        (1, 0, 0): "apply_block_kernel<8,true,81,1,1337344>", (1, 0, 1): "apply_block_kernel<8,true,81,1,1337344>",
        (0, 1, 0): "apply_block_kernel<8,true,81,1,17065984>", (0, 1, 1): "apply_block_kernel<8,true,81,1,17065984>",
        (0, 0, 0): "apply_block_kernel<8,true,81,1,288768>", (0, 0, 1): "apply_block_kernel<8,true,81,1,288768>",
    },
    ("f32", 1, 0): {
        (0, 1, 0): "apply_block_kernel<1,false,4,1,553936896>", (0, 1, 1): "apply_block_kernel<1,false,4,1,553936896>",
        (0, 0, 0): "apply_block_kernel<1,false,4,1,537159680>", (0, 0, 1): "apply_block_kernel<1,false,4,1,537159680>",
    },
    ("f32", 1, 1): {
        (0, 1, 0): "apply_block_kernel<1,true,4,1,553936896>", (0, 1, 1): "apply_block_kernel<1,true,4,1,553936896>",
        (0, 0, 0): "apply_block_kernel<1,true,4,1,537159680>", (0, 0, 1): "apply_block_kernel<1,true,4,1,537159680>",
    },
    ("f32", 2, 0): {
        (0, 1, 0): "apply_block_kernel<2,false,9,1,553936896>", (0, 1, 1): "apply_block_kernel<2,false,9,1,553936896>",
        (0, 0, 0): "apply_block_kernel<2,false,9,1,537159680>", (0, 0, 1): "apply_block_kernel<2,false,9,1,537159680>",
    },
    ("f32", 2, 1): {
        (0, 1, 0): "apply_block_kernel<2,true,9,1,553936896>", (0, 1, 1): "apply_block_kernel<2,true,9,1,553936896>",
        (0, 0, 0): "apply_block_kernel<2,true,9,1,537159680>", (0, 0, 1): "apply_block_kernel<2,true,9,1,537159680>",
    },
    ("f32", 3, 0): {
        (0, 1, 0): "apply_block_kernel<3,false,16,1,553936896>", (0, 1, 1): "apply_block_kernel<3,false,16,1,553936896>",
        (0, 0, 0): "apply_block_kernel<3,false,16,1,537159680>", (0, 0, 1): "apply_block_kernel<3,false,16,1,537159680>",
    },
    ("f32", 3, 1): {
        (0, 1, 0): "apply_block_kernel<3,true,16,1,553936896>", (0, 1, 1): "apply_block_kernel<3,true,16,1,553936896>",
        (0, 0, 0): "apply_block_kernel<3,true,16,1,537159680>", (0, 0, 1): "apply_block_kernel<3,true,16,1,537159680>",
    },
    ("f32", 4, 0): {
        (0, 1, 0): "apply_block_kernel<4,false,32,1,822372352>", (0, 1, 1): "apply_block_kernel<4,false,32,1,822372352>",
        (0, 0, 0): "apply_block_kernel<4,false,32,1,537159680>", (0, 0, 1): "apply_block_kernel<4,false,32,1,537159680>",
    },
    ("f32", 4, 1): {
        (0, 1, 0): "apply_block_kernel<4,true,32,1,822372352>", (0, 1, 1): "apply_block_kernel<4,true,32,1,822372352>",
        (0, 0, 0): "apply_block_kernel<4,true,32,1,537159680>", (0, 0, 1): "apply_block_kernel<4,true,32,1,537159680>",
    },
    ("f32", 5, 0): {
        (0, 1, 0): "apply_block_kernel<5,false,36,1,553936896>", (0, 1, 1): "apply_block_kernel<5,false,36,1,553936896>",
        (0, 0, 0): "apply_block_kernel<5,false,36,1,537159680>", (0, 0, 1): "apply_block_kernel<5,false,36,1,537159680>",
    },
    ("f32", 5, 1): {
        (0, 1, 0): "apply_block_kernel<5,true,36,1,553936896>", (0, 1, 1): "apply_block_kernel<5,true,36,1,553936896>",
        (0, 0, 0): "apply_block_kernel<5,true,36,1,537159680>", (0, 0, 1): "apply_block_kernel<5,true,36,1,537159680>",
    },
    ("f32", 6, 0): {
        (0, 1, 0): "apply_block_kernel<6,false,64,1,553936896>", (0, 1, 1): "apply_block_kernel<6,false,64,1,553936896>",
        (0, 0, 0): "apply_block_kernel<6,false,64,1,537159680>", (0, 0, 1): "apply_block_kernel<6,false,64,1,537159680>",
    },
    ("f32", 6, 1): {
        (0, 1, 0): "apply_block_kernel<6,true,64,1,553936896>", (0, 1, 1): "apply_block_kernel<6,true,64,1,553936896>",
        (0, 0, 0): "apply_block_kernel<6,true,64,1,537159680>", (0, 0, 1): "apply_block_kernel<6,true,64,1,537159680>",
    },
    ("f32", 7, 0): {
        (0, 1, 0): "apply_block_kernel<7,false,64,1,553936896>", (0, 1, 1): "apply_block_kernel<7,false,64,1,553936896>",
        (0, 0, 0): "apply_block_kernel<7,false,64,1,537159680>", (0, 0, 1): "apply_block_kernel<7,false,64,1,537159680>",
    },
    ("f32", 7, 1): {
        (0, 1, 0): "apply_block_kernel<7,true,64,1,553936896>", (0, 1, 1): "apply_block_kernel<7,true,64,1,553936896>",
        (0, 0, 0): "apply_block_kernel<7,true,64,1,537159680>", (0, 0, 1): "apply_block_kernel<7,true,64,1,537159680>",
    },
    ("f32", 8, 0): {
        (0, 1, 0): "apply_block_kernel<8,false,81,1,553936896>", (0, 1, 1): "apply_block_kernel<8,false,81,1,553936896>",
        (0, 0, 0): "apply_block_kernel<8,false,81,1,537159680>", (0, 0, 1): "apply_block_kernel<8,false,81,1,537159680>",
    },
    ("f32", 8, 1): {
        (0, 1, 0): "apply_block_kernel<8,true,81,1,553936896>", (0, 1, 1): "apply_block_kernel<8,true,81,1,553936896>",
        (0, 0, 0): "apply_block_kernel<8,true,81,1,537159680>", (0, 0, 1): "apply_block_kernel<8,true,81,1,537159680>",
    },
    ("helmholtz", 1, 0): {
        (1, 1, 0): "apply_block_kernel<1,false,4,1,9725952>", (1, 1, 1): "apply_block_kernel<1,false,4,1,9725952>",
        (1, 0, 0): "apply_block_kernel<1,false,4,1,9725952>", (1, 0, 1): "apply_block_kernel<1,false,4,1,9725952>",
        (0, 1, 0): "apply_block_kernel<1,false,4,1,8677376>", (0, 1, 1): "apply_block_kernel<1,false,4,1,8677376>",
        (0, 0, 0): "apply_block_kernel<1,false,4,1,8677376>", (0, 0, 1): "apply_block_kernel<1,false,4,1,8677376>",
    },
    ("helmholtz", 1, 1): {
        (1, 1, 0): "apply_block_kernel<1,true,4,1,9725952>", (1, 1, 1): "apply_block_kernel<1,true,4,1,9725952>",
        (1, 0, 0): "apply_block_kernel<1,true,4,1,9725952>", (1, 0, 1): "apply_block_kernel<1,true,4,1,9725952>",
        (0, 1, 0): "apply_block_kernel<1,true,4,1,8677376>", (0, 1, 1): "apply_block_kernel<1,true,4,1,8677376>",
        (0, 0, 0): "apply_block_kernel<1,true,4,1,8677376>", (0, 0, 1): "apply_block_kernel<1,true,4,1,8677376>",
    },
    ("helmholtz", 2, 0): {
        (1, 1, 0): "apply_block_kernel<2,false,9,1,9725952>", (1, 1, 1): "apply_block_kernel<2,false,9,1,9725952>",
        (1, 0, 0): "apply_block_kernel<2,false,9,1,9725952>", (1, 0, 1): "apply_block_kernel<2,false,9,1,9725952>",
        (0, 1, 0): "apply_block_kernel<2,false,9,1,8677376>", (0, 1, 1): "apply_block_kernel<2,false,9,1,8677376>",
        (0, 0, 0): "apply_block_kernel<2,false,9,1,8677376>", (0, 0, 1): "apply_block_kernel<2,false,9,1,8677376>",
    },
    ("helmholtz", 2, 1): {
        (1, 1, 0): "apply_block_kernel<2,true,9,1,9725952>", (1, 1, 1): "apply_block_kernel<2,true,9,1,9725952>",
        (1, 0, 0): "apply_block_kernel<2,true,9,1,9725952>", (1, 0, 1): "apply_block_kernel<2,true,9,1,9725952>",
        (0, 1, 0): "apply_block_kernel<2,true,9,1,8677376>", (0, 1, 1): "apply_block_kernel<2,true,9,1,8677376>",
        (0, 0, 0): "apply_block_kernel<2,true,9,1,8677376>", (0, 0, 1): "apply_block_kernel<2,true,9,1,8677376>",
    },
    ("helmholtz", 3, 0): {
        (1, 1, 0): "apply_block_kernel<3,false,16,1,9725952>", (1, 1, 1): "apply_block_kernel<3,false,16,1,9725952>",
        (1, 0, 0): "apply_block_kernel<3,false,16,1,9725952>", (1, 0, 1): "apply_block_kernel<3,false,16,1,9725952>",
        (0, 1, 0): "apply_block_kernel<3,false,16,1,8677376>", (0, 1, 1): "apply_block_kernel<3,false,16,1,8677376>",
        (0, 0, 0): "apply_block_kernel<3,false,16,1,8677376>", (0, 0, 1): "apply_block_kernel<3,false,16,1,8677376>",
    },
    ("helmholtz", 3, 1): {
        (1, 1, 0): "apply_block_kernel<3,true,16,1,9725952>", (1, 1, 1): "apply_block_kernel<3,true,16,1,9725952>",
        (1, 0, 0): "apply_block_kernel<3,true,16,1,9725952>", (1, 0, 1): "apply_block_kernel<3,true,16,1,9725952>",
        (0, 1, 0): "apply_block_kernel<3,true,16,1,8677376>", (0, 1, 1): "apply_block_kernel<3,true,16,1,8677376>",
        (0, 0, 0): "apply_block_kernel<3,true,16,1,8677376>", (0, 0, 1): "apply_block_kernel<3,true,16,1,8677376>",
    },
    ("helmholtz", 4, 0): {
        (1, 1, 0): "apply_block_kernel<4,false,32,1,9725952>", (1, 1, 1): "apply_block_kernel<4,false,32,1,9725952>",
        (1, 0, 0): "apply_block_kernel<4,false,32,1,9725952>", (1, 0, 1): "apply_block_kernel<4,false,32,1,9725952>",
        (0, 1, 0): "apply_block_kernel<4,false,32,1,8677376>", (0, 1, 1): "apply_block_kernel<4,false,32,1,8677376>",
        (0, 0, 0): "apply_block_kernel<4,false,32,1,8677376>", (0, 0, 1): "apply_block_kernel<4,false,32,1,8677376>",
    },
    ("helmholtz", 4, 1): {
        (1, 1, 0): "apply_block_kernel<4,true,32,1,9725952>", (1, 1, 1): "apply_block_kernel<4,true,32,1,9725952>",
        (1, 0, 0): "apply_block_kernel<4,true,32,1,9725952>", (1, 0, 1): "apply_block_kernel<4,true,32,1,9725952>",
        (0, 1, 0): "apply_block_kernel<4,true,32,1,8677376>", (0, 1, 1): "apply_block_kernel<4,true,32,1,8677376>",
        (0, 0, 0): "apply_block_kernel<4,true,32,1,8677376>", (0, 0, 1): "apply_block_kernel<4,true,32,1,8677376>",
    },
    ("helmholtz", 5, 0): {
        (1, 1, 0): "apply_block_kernel<5,false,36,1,9725952>", (1, 1, 1): "apply_block_kernel<5,false,36,1,9725952>",
        (1, 0, 0): "apply_block_kernel<5,false,36,1,9725952>", (1, 0, 1): "apply_block_kernel<5,false,36,1,9725952>",
        (0, 1, 0): "apply_block_kernel<5,false,36,1,8677376>", (0, 1, 1): "apply_block_kernel<5,false,36,1,8677376>",
        (0, 0, 0): "apply_block_kernel<5,false,36,1,8677376>", (0, 0, 1): "apply_block_kernel<5,false,36,1,8677376>",
    },
    ("helmholtz", 5, 1): {
        (1, 1, 0): "apply_block_kernel<5,true,36,1,9725952>", (1, 1, 1): "apply_block_kernel<5,true,36,1,9725952>",
        (1, 0, 0): "apply_block_kernel<5,true,36,1,9725952>", (1, 0, 1): "apply_block_kernel<5,true,36,1,9725952>",
        (0, 1, 0): "apply_block_kernel<5,true,36,1,8677376>", (0, 1, 1): "apply_block_kernel<5,true,36,1,8677376>",
        (0, 0, 0): "apply_block_kernel<5,true,36,1,8677376>", (0, 0, 1): "apply_block_kernel<5,true,36,1,8677376>",
    },
    ("helmholtz", 6, 0): {
        (1, 1, 0): "apply_block_kernel<6,false,64,1,9725952>", (1, 1, 1): "apply_block_kernel<6,false,64,1,9725952>",
        (1, 0, 0): "apply_block_kernel<6,false,64,1,9725952>", (1, 0, 1): "apply_block_kernel<6,false,64,1,9725952>",
        (0, 1, 0): "apply_block_kernel<6,false,64,1,8677376>", (0, 1, 1): "apply_block_kernel<6,false,64,1,8677376>",
        (0, 0, 0): "apply_block_kernel<6,false,64,1,8677376>", (0, 0, 1): "apply_block_kernel<6,false,64,1,8677376>",
    },
    ("helmholtz", 6, 1): {
        (1, 1, 0): "apply_block_kernel<6,true,64,1,9725952>", (1, 1, 1): "apply_block_kernel<6,true,64,1,9725952>",
        (1, 0, 0): "apply_block_kernel<6,true,64,1,9725952>", (1, 0, 1): "apply_block_kernel<6,true,64,1,9725952>",
        (0, 1, 0): "apply_block_kernel<6,true,64,1,8677376>", (0, 1, 1): "apply_block_kernel<6,true,64,1,8677376>",
        (0, 0, 0): "apply_block_kernel<6,true,64,1,8677376>", (0, 0, 1): "apply_block_kernel<6,true,64,1,8677376>",
    },
    ("helmholtz", 7, 0): {
        (1, 1, 0): "apply_block_kernel<7,false,64,1,9725952>", (1, 1, 1): "apply_block_kernel<7,false,64,1,9725952>",
        (1, 0, 0): "apply_block_kernel<7,false,64,1,9725952>", (1, 0, 1): "apply_block_kernel<7,false,64,1,9725952>",
        (0, 1, 0): "apply_block_kernel<7,false,64,1,8677376>", (0, 1, 1): "apply_block_kernel<7,false,64,1,8677376>",
        (0, 0, 0): "apply_block_kernel<7,false,64,1,8677376>", (0, 0, 1): "apply_block_kernel<7,false,64,1,8677376>",
    },
    ("helmholtz", 7, 1): {
        (1, 1, 0): "apply_block_kernel<7,true,64,1,9725952>", (1, 1, 1): "apply_block_kernel<7,true,64,1,9725952>",
        (1, 0, 0): "apply_block_kernel<7,true,64,1,9725952>", (1, 0, 1): "apply_block_kernel<7,true,64,1,9725952>",
        (0, 1, 0): "apply_block_kernel<7,true,64,1,8677376>", (0, 1, 1): "apply_block_kernel<7,true,64,1,8677376>",
        (0, 0, 0): "apply_block_kernel<7,true,64,1,8677376>", (0, 0, 1): "apply_block_kernel<7,true,64,1,8677376>",
    },
    ("helmholtz", 8, 0): {
        (1, 1, 0): "apply_block_kernel<8,false,81,1,9725952>", (1, 1, 1): "apply_block_kernel<8,false,81,1,9725952>",
        (1, 0, 0): "apply_block_kernel<8,false,81,1,9725952>", (1, 0, 1): "apply_block_kernel<8,false,81,1,9725952>",
        (0, 1, 0): "apply_block_kernel<8,false,81,1,8677376>", (0, 1, 1): "apply_block_kernel<8,false,81,1,8677376>",
        (0, 0, 0): "apply_block_kernel<8,false,81,1,8677376>", (0, 0, 1): "apply_block_kernel<8,false,81,1,8677376>",
    },
    ("helmholtz", 8, 1): {
        (1, 1, 0): "apply_block_kernel<8,true,81,1,9725952>", (1, 1, 1): "apply_block_kernel<8,true,81,1,9725952>",
        (1, 0, 0): "apply_block_kernel<8,true,81,1,9725952>", (1, 0, 1): "apply_block_kernel<8,true,81,1,9725952>",
        (0, 1, 0): "apply_block_kernel<8,true,81,1,8677376>", (0, 1, 1): "apply_block_kernel<8,true,81,1,8677376>",
        (0, 0, 0): "apply_block_kernel<8,true,81,1,8677376>", (0, 0, 1): "apply_block_kernel<8,true,81,1,8677376>",
    },
    ("hanging", 1, 0): {
        (1, 1, 0): "apply_block_kernel<1,false,4,1,3434496>", (1, 1, 1): "apply_block_kernel<1,false,4,1,3434496>",
        (1, 0, 0): "apply_block_kernel<1,false,4,1,3434496>", (1, 0, 1): "apply_block_kernel<1,false,4,1,3434496>",
        (0, 1, 0): "apply_block_kernel<1,false,4,1,2385920>", (0, 1, 1): "apply_block_kernel<1,false,4,1,2385920>",
        (0, 0, 0): "apply_block_kernel<1,false,4,1,2385920>", (0, 0, 1): "apply_block_kernel<1,false,4,1,2385920>",
    },
    ("hanging", 1, 1): {
        (1, 1, 0): "apply_block_kernel<1,true,4,1,3434496>", (1, 1, 1): "apply_block_kernel<1,true,4,1,3434496>",
        (1, 0, 0): "apply_block_kernel<1,true,4,1,3434496>", (1, 0, 1): "apply_block_kernel<1,true,4,1,3434496>",
        (0, 1, 0): "apply_block_kernel<1,true,4,1,2385920>", (0, 1, 1): "apply_block_kernel<1,true,4,1,2385920>",
        (0, 0, 0): "apply_block_kernel<1,true,4,1,2385920>", (0, 0, 1): "apply_block_kernel<1,true,4,1,2385920>",
    },
    ("hanging", 2, 0): {
        (1, 1, 0): "apply_block_kernel<2,false,9,1,3434496>", (1, 1, 1): "apply_block_kernel<2,false,9,1,3434496>",
        (1, 0, 0): "apply_block_kernel<2,false,9,1,3434496>", (1, 0, 1): "apply_block_kernel<2,false,9,1,3434496>",
        (0, 1, 0): "apply_block_kernel<2,false,9,1,2385920>", (0, 1, 1): "apply_block_kernel<2,false,9,1,2385920>",
        (0, 0, 0): "apply_block_kernel<2,false,9,1,2385920>", (0, 0, 1): "apply_block_kernel<2,false,9,1,2385920>",
    },
    ("hanging", 2, 1): {
        (1, 1, 0): "apply_block_kernel<2,true,9,1,3434496>", (1, 1, 1): "apply_block_kernel<2,true,9,1,3434496>",
        (1, 0, 0): "apply_block_kernel<2,true,9,1,3434496>", (1, 0, 1): "apply_block_kernel<2,true,9,1,3434496>",
        (0, 1, 0): "apply_block_kernel<2,true,9,1,2385920>", (0, 1, 1): "apply_block_kernel<2,true,9,1,2385920>",
        (0, 0, 0): "apply_block_kernel<2,true,9,1,2385920>", (0, 0, 1): "apply_block_kernel<2,true,9,1,2385920>",
    },
    ("hanging", 3, 0): {
        (1, 1, 0): "apply_block_kernel<3,false,16,1,3434496>", (1, 1, 1): "apply_block_kernel<3,false,16,1,3434496>",
        (1, 0, 0): "apply_block_kernel<3,false,16,1,3434496>", (1, 0, 1): "apply_block_kernel<3,false,16,1,3434496>",
        (0, 1, 0): "apply_block_kernel<3,false,16,1,2385920>", (0, 1, 1): "apply_block_kernel<3,false,16,1,2385920>",
        (0, 0, 0): "apply_block_kernel<3,false,16,1,2385920>", (0, 0, 1): "apply_block_kernel<3,false,16,1,2385920>",
    },
    ("hanging", 3, 1): {
        (1, 1, 0): "apply_block_kernel<3,true,16,1,3434496>", (1, 1, 1): "apply_block_kernel<3,true,16,1,3434496>",
        (1, 0, 0): "apply_block_kernel<3,true,16,1,3434496>", (1, 0, 1): "apply_block_kernel<3,true,16,1,3434496>",
        (0, 1, 0): "apply_block_kernel<3,true,16,1,2385920>", (0, 1, 1): "apply_block_kernel<3,true,16,1,2385920>",
        (0, 0, 0): "apply_block_kernel<3,true,16,1,2385920>", (0, 0, 1): "apply_block_kernel<3,true,16,1,2385920>",
    },
    ("hanging", 4, 0): {
        (1, 1, 0): "apply_block_kernel<4,false,32,1,3434496>", (1, 1, 1): "apply_block_kernel<4,false,32,1,3467264>",
        (1, 0, 0): "apply_block_kernel<4,false,32,1,3434496>", (1, 0, 1): "apply_block_kernel<4,false,32,1,3467264>",
        (0, 1, 0): "apply_block_kernel<4,false,32,1,2385920>", (0, 1, 1): "apply_block_kernel<4,false,32,1,2418688>",
        (0, 0, 0): "apply_block_kernel<4,false,32,1,2385920>", (0, 0, 1): "apply_block_kernel<4,false,32,1,2418688>",
    },
    ("hanging", 4, 1): {
        (1, 1, 0): "apply_block_kernel<4,true,32,1,3434496>", (1, 1, 1): "apply_block_kernel<4,true,32,1,3434496>",
        (1, 0, 0): "apply_block_kernel<4,true,32,1,3434496>", (1, 0, 1): "apply_block_kernel<4,true,32,1,3434496>",
        (0, 1, 0): "apply_block_kernel<4,true,32,1,2385920>", (0, 1, 1): "apply_block_kernel<4,true,32,1,2385920>",
        (0, 0, 0): "apply_block_kernel<4,true,32,1,2385920>", (0, 0, 1): "apply_block_kernel<4,true,32,1,2385920>",
    },
    ("hanging", 5, 0): {
        (1, 1, 0): "apply_block_kernel<5,false,36,1,3434496>", (1, 1, 1): "apply_block_kernel<5,false,36,1,3434496>",
        (1, 0, 0): "apply_block_kernel<5,false,36,1,3434496>", (1, 0, 1): "apply_block_kernel<5,false,36,1,3434496>",
        (0, 1, 0): "apply_block_kernel<5,false,36,1,2385920>", (0, 1, 1): "apply_block_kernel<5,false,36,1,2385920>",
        (0, 0, 0): "apply_block_kernel<5,false,36,1,2385920>", (0, 0, 1): "apply_block_kernel<5,false,36,1,2385920>",
    },
    ("hanging", 5, 1): {
        (1, 1, 0): "apply_block_kernel<5,true,36,1,3434496>", (1, 1, 1): "apply_block_kernel<5,true,36,1,3434496>",
        (1, 0, 0): "apply_block_kernel<5,true,36,1,3434496>", (1, 0, 1): "apply_block_kernel<5,true,36,1,3434496>",
        (0, 1, 0): "apply_block_kernel<5,true,36,1,2385920>", (0, 1, 1): "apply_block_kernel<5,true,36,1,2385920>",
        (0, 0, 0): "apply_block_kernel<5,true,36,1,2385920>", (0, 0, 1): "apply_block_kernel<5,true,36,1,2385920>",
    },
    ("hanging", 6, 0): {
        (1, 1, 0): "apply_block_kernel<6,false,64,1,3434496>", (1, 1, 1): "apply_block_kernel<6,false,64,1,3434496>",
        (1, 0, 0): "apply_block_kernel<6,false,64,1,3434496>", (1, 0, 1): "apply_block_kernel<6,false,64,1,3434496>",
        (0, 1, 0): "apply_block_kernel<6,false,64,1,2385920>", (0, 1, 1): "apply_block_kernel<6,false,64,1,2385920>",
        (0, 0, 0): "apply_block_kernel<6,false,64,1,2385920>", (0, 0, 1): "apply_block_kernel<6,false,64,1,2385920>",
    },
    ("hanging", 6, 1): {
        (1, 1, 0): "apply_block_kernel<6,true,64,1,3434496>", (1, 1, 1): "apply_block_kernel<6,true,64,1,3434496>",
        (1, 0, 0): "apply_block_kernel<6,true,64,1,3434496>", (1, 0, 1): "apply_block_kernel<6,true,64,1,3434496>",
        (0, 1, 0): "apply_block_kernel<6,true,64,1,2385920>", (0, 1, 1): "apply_block_kernel<6,true,64,1,2385920>",
        (0, 0, 0): "apply_block_kernel<6,true,64,1,2385920>", (0, 0, 1): "apply_block_kernel<6,true,64,1,2385920>",
    },
    ("hanging", 7, 0): {
        (1, 1, 0): "apply_block_kernel<7,false,64,1,3434496>", (1, 1, 1): "apply_block_kernel<7,false,64,1,3434496>",
        (1, 0, 0): "apply_block_kernel<7,false,64,1,3434496>", (1, 0, 1): "apply_block_kernel<7,false,64,1,3434496>",
        (0, 1, 0): "apply_block_kernel<7,false,64,1,2385920>", (0, 1, 1): "apply_block_kernel<7,false,64,1,2385920>",
        (0, 0, 0): "apply_block_kernel<7,false,64,1,2385920>", (0, 0, 1): "apply_block_kernel<7,false,64,1,2385920>",
    },
    ("hanging", 7, 1): {
        (1, 1, 0): "apply_block_kernel<7,true,64,1,3434496>", (1, 1, 1): "apply_block_kernel<7,true,64,1,3434496>",
        (1, 0, 0): "apply_block_kernel<7,true,64,1,3434496>", (1, 0, 1): "apply_block_kernel<7,true,64,1,3434496>",
        (0, 1, 0): "apply_block_kernel<7,true,64,1,2385920>", (0, 1, 1): "apply_block_kernel<7,true,64,1,2385920>",
        (0, 0, 0): "apply_block_kernel<7,true,64,1,2385920>", (0, 0, 1): "apply_block_kernel<7,true,64,1,2385920>",
    },
    ("hanging", 8, 0): {
        (1, 1, 0): "apply_block_kernel<8,false,81,1,3434496>", (1, 1, 1): "apply_block_kernel<8,false,81,1,3434496>",
        (1, 0, 0): "apply_block_kernel<8,false,81,1,3434496>", (1, 0, 1): "apply_block_kernel<8,false,81,1,3434496>",
        (0, 1, 0): "apply_block_kernel<8,false,81,1,2385920>", (0, 1, 1): "apply_block_kernel<8,false,81,1,2385920>",
        (0, 0, 0): "apply_block_kernel<8,false,81,1,2385920>", (0, 0, 1): "apply_block_kernel<8,false,81,1,2385920>",
    },
    ("hanging", 8, 1): {
        (1, 1, 0): "apply_block_kernel<8,true,81,1,3434496>", (1, 1, 1): "apply_block_kernel<8,true,81,1,3434496>",
        (1, 0, 0): "apply_block_kernel<8,true,81,1,3434496>", (1, 0, 1): "apply_block_kernel<8,true,81,1,3434496>",
        (0, 1, 0): "apply_block_kernel<8,true,81,1,2385920>", (0, 1, 1): "apply_block_kernel<8,true,81,1,2385920>",
        (0, 0, 0): "apply_block_kernel<8,true,81,1,2385920>", (0, 0, 1): "apply_block_kernel<8,true,81,1,2385920>",
    },
    ("affine", 4, 0): {
        (0, 1, 0): "apply_block_kernel<4,false,32,1,289792>", (0, 1, 1): "apply_block_kernel<4,false,32,1,289792>",
        (0, 0, 0): "apply_block_kernel<4,false,32,1,289792>", (0, 0, 1): "apply_block_kernel<4,false,32,1,289792>",
    },
    ("affine", 4, 1): {
        (0, 1, 0): "apply_block_kernel<4,true,32,1,289792>", (0, 1, 1): "apply_block_kernel<4,true,32,1,289792>",
        (0, 0, 0): "apply_block_kernel<4,true,32,1,289792>", (0, 0, 1): "apply_block_kernel<4,true,32,1,289792>",
    },
}
# (class, degree, quadrature) -> the degree's default pencil kernel (the atomic reference of every case)
PENCIL_KERNEL = {
    ("poisson", 1, 0): "apply_pencil_kernel<1,false,1,4,4,true,0>", ("poisson", 1, 1): "apply_pencil_kernel<1,true,1,4,4,true,0>",
    ("poisson", 2, 0): "apply_pencil_kernel<2,false,1,9,4,true,0>", ("poisson", 2, 1): "apply_pencil_kernel<2,true,1,9,4,true,0>",
    ("poisson", 3, 0): "apply_pencil_kernel<3,false,1,16,4,true,0>", ("poisson", 3, 1): "apply_pencil_kernel<3,true,1,16,4,true,0>",
    ("poisson", 4, 0): "apply_pencil_kernel<4,false,4,25,1,true,0>", ("poisson", 4, 1): "apply_pencil_kernel<4,true,4,25,1,true,0>",
    ("poisson", 5, 0): "apply_pencil_kernel<5,false,4,36,1,true,0>", ("poisson", 5, 1): "apply_pencil_kernel<5,true,4,36,1,true,0>",
    ("poisson", 6, 0): "apply_pencil_kernel<6,false,4,49,1,true,0>", ("poisson", 6, 1): "apply_pencil_kernel<6,true,4,49,1,true,0>",
    ("poisson", 7, 0): "apply_pencil_kernel<7,false,4,64,1,true,0>", ("poisson", 7, 1): "apply_pencil_kernel<7,true,4,64,1,true,0>",
    ("poisson", 8, 0): "apply_pencil_kernel<8,false,4,81,1,true,0>", ("poisson", 8, 1): "apply_pencil_kernel<8,true,4,81,1,true,0>",
    ("f32", 1, 0): "apply_pencil_kernel<1,false,1,4,4,true,536870912>", ("f32", 1, 1): "apply_pencil_kernel<1,true,1,4,4,true,536870912>",
    ("f32", 2, 0): "apply_pencil_kernel<2,false,1,9,4,true,536870912>", ("f32", 2, 1): "apply_pencil_kernel<2,true,1,9,4,true,536870912>",
    ("f32", 3, 0): "apply_pencil_kernel<3,false,1,16,4,true,536870912>", ("f32", 3, 1): "apply_pencil_kernel<3,true,1,16,4,true,536870912>",
    ("f32", 4, 0): "apply_pencil_kernel<4,false,4,25,1,true,536870912>", ("f32", 4, 1): "apply_pencil_kernel<4,true,4,25,1,true,536870912>",
    ("f32", 5, 0): "apply_pencil_kernel<5,false,4,36,1,true,536870912>", ("f32", 5, 1): "apply_pencil_kernel<5,true,4,36,1,true,536870912>",
    ("f32", 6, 0): "apply_pencil_kernel<6,false,4,49,1,true,536870912>", ("f32", 6, 1): "apply_pencil_kernel<6,true,4,49,1,true,536870912>",
    ("f32", 7, 0): "apply_pencil_kernel<7,false,4,64,1,true,536870912>", ("f32", 7, 1): "apply_pencil_kernel<7,true,4,64,1,true,536870912>",
    ("f32", 8, 0): "apply_pencil_kernel<8,false,4,81,1,true,536870912>", ("f32", 8, 1): "apply_pencil_kernel<8,true,4,81,1,true,536870912>",
    ("helmholtz", 1, 0): "apply_pencil_kernel<1,false,1,4,4,true,8388608>", ("helmholtz", 1, 1): "apply_pencil_kernel<1,true,1,4,4,true,8388608>",
    ("helmholtz", 2, 0): "apply_pencil_kernel<2,false,1,9,4,true,8388608>", ("helmholtz", 2, 1): "apply_pencil_kernel<2,true,1,9,4,true,8388608>",
    ("helmholtz", 3, 0): "apply_pencil_kernel<3,false,1,16,4,true,8388608>", ("helmholtz", 3, 1): "apply_pencil_kernel<3,true,1,16,4,true,8388608>",
    ("helmholtz", 4, 0): "apply_pencil_kernel<4,false,4,25,1,true,8388608>", ("helmholtz", 4, 1): "apply_pencil_kernel<4,true,4,25,1,true,8388608>",
    ("helmholtz", 5, 0): "apply_pencil_kernel<5,false,4,36,1,true,8388608>", ("helmholtz", 5, 1): "apply_pencil_kernel<5,true,4,36,1,true,8388608>",
    ("helmholtz", 6, 0): "apply_pencil_kernel<6,false,4,49,1,true,8388608>", ("helmholtz", 6, 1): "apply_pencil_kernel<6,true,4,49,1,true,8388608>",
    ("helmholtz", 7, 0): "apply_pencil_kernel<7,false,4,64,1,true,8388608>", ("helmholtz", 7, 1): "apply_pencil_kernel<7,true,4,64,1,true,8388608>",
    ("helmholtz", 8, 0): "apply_pencil_kernel<8,false,4,81,1,true,8388608>", ("helmholtz", 8, 1): "apply_pencil_kernel<8,true,4,81,1,true,8388608>",
    ("hanging", 1, 0): "apply_pencil_kernel<1,false,1,4,4,true,2097152>", ("hanging", 1, 1): "apply_pencil_kernel<1,true,1,4,4,true,2097152>",
    ("hanging", 2, 0): "apply_pencil_kernel<2,false,1,9,4,true,2097152>", ("hanging", 2, 1): "apply_pencil_kernel<2,true,1,9,4,true,2097152>",
    ("hanging", 3, 0): "apply_pencil_kernel<3,false,1,16,4,true,2097152>", ("hanging", 3, 1): "apply_pencil_kernel<3,true,1,16,4,true,2097152>",
    ("hanging", 4, 0): "apply_pencil_kernel<4,false,4,25,1,true,2097152>", ("hanging", 4, 1): "apply_pencil_kernel<4,true,4,25,1,true,2097152>",
    ("hanging", 5, 0): "apply_pencil_kernel<5,false,4,36,1,true,2097152>", ("hanging", 5, 1): "apply_pencil_kernel<5,true,4,36,1,true,2097152>",
    ("hanging", 6, 0): "apply_pencil_kernel<6,false,4,49,1,true,2097152>", ("hanging", 6, 1): "apply_pencil_kernel<6,true,4,49,1,true,2097152>",
    ("hanging", 7, 0): "apply_pencil_kernel<7,false,4,64,1,true,2097152>", ("hanging", 7, 1): "apply_pencil_kernel<7,true,4,64,1,true,2097152>",
    ("hanging", 8, 0): "apply_pencil_kernel<8,false,4,81,1,true,2097152>", ("hanging", 8, 1): "apply_pencil_kernel<8,true,4,81,1,true,2097152>",
    ("affine", 4, 0): "apply_pencil_kernel<4,false,4,25,1,true,1024>", ("affine", 4, 1): "apply_pencil_kernel<4,true,4,25,1,true,1024>",
}
# variant 0 on these meshes (too few bricks for the block kernel to pay): (class, degree, quadrature) -> kernel.  The team kernel's name ends at its
# scatter mode; the affine pencil kernel keeps four waves per workgroup at every degree
VARIANT_0 = {
    ("poisson", 1, 0): "apply_team_kernel<1,false,4,4,true,", ("poisson", 1, 1): "apply_team_kernel<1,true,4,4,true,",
    ("poisson", 2, 0): "apply_pencil_kernel<2,false,1,9,4,true,0>", ("poisson", 2, 1): "apply_pencil_kernel<2,true,1,9,4,true,0>",
    ("poisson", 3, 0): "apply_team_kernel<3,false,4,16,true,", ("poisson", 3, 1): "apply_team_kernel<3,true,4,16,true,",
    ("poisson", 4, 0): "apply_pencil_kernel<4,false,4,25,1,true,0>", ("poisson", 4, 1): "apply_pencil_kernel<4,true,4,25,1,true,0>",
    ("poisson", 5, 0): "apply_pencil_kernel<5,false,4,36,1,true,0>", ("poisson", 5, 1): "apply_pencil_kernel<5,true,4,36,1,true,0>",
    ("poisson", 6, 0): "apply_pencil_kernel<6,false,4,49,1,true,0>", ("poisson", 6, 1): "apply_pencil_kernel<6,true,4,49,1,true,0>",
    ("poisson", 7, 0): "apply_pencil_kernel<7,false,4,64,1,true,0>", ("poisson", 7, 1): "apply_pencil_kernel<7,true,4,64,1,true,0>",
    ("poisson", 8, 0): "apply_pencil_kernel<8,false,4,81,1,true,0>", ("poisson", 8, 1): "apply_pencil_kernel<8,true,4,81,1,true,0>",
    ("f32", 1, 0): "apply_pencil_kernel<1,false,1,4,4,true,536870912>", ("f32", 1, 1): "apply_pencil_kernel<1,true,1,4,4,true,536870912>",
    ("f32", 2, 0): "apply_pencil_kernel<2,false,1,9,4,true,536870912>", ("f32", 2, 1): "apply_pencil_kernel<2,true,1,9,4,true,536870912>",
    ("f32", 3, 0): "apply_pencil_kernel<3,false,1,16,4,true,536870912>", ("f32", 3, 1): "apply_pencil_kernel<3,true,1,16,4,true,536870912>",
    ("f32", 4, 0): "apply_pencil_kernel<4,false,4,25,1,true,536870912>", ("f32", 4, 1): "apply_pencil_kernel<4,true,4,25,1,true,536870912>",
    ("f32", 5, 0): "apply_pencil_kernel<5,false,4,36,1,true,536870912>", ("f32", 5, 1): "apply_pencil_kernel<5,true,4,36,1,true,536870912>",
    ("f32", 6, 0): "apply_pencil_kernel<6,false,4,49,1,true,536870912>", ("f32", 6, 1): "apply_pencil_kernel<6,true,4,49,1,true,536870912>",
    ("f32", 7, 0): "apply_pencil_kernel<7,false,4,64,1,true,536870912>", ("f32", 7, 1): "apply_pencil_kernel<7,true,4,64,1,true,536870912>",
    ("f32", 8, 0): "apply_pencil_kernel<8,false,4,81,1,true,536870912>", ("f32", 8, 1): "apply_pencil_kernel<8,true,4,81,1,true,536870912>",
    ("helmholtz", 1, 0): "apply_pencil_kernel<1,false,1,4,4,true,8388608>", ("helmholtz", 1, 1): "apply_pencil_kernel<1,true,1,4,4,true,8388608>",
    ("helmholtz", 2, 0): "apply_pencil_kernel<2,false,1,9,4,true,8388608>", ("helmholtz", 2, 1): "apply_pencil_kernel<2,true,1,9,4,true,8388608>",
    ("helmholtz", 3, 0): "apply_pencil_kernel<3,false,1,16,4,true,8388608>", ("helmholtz", 3, 1): "apply_pencil_kernel<3,true,1,16,4,true,8388608>",
    ("helmholtz", 4, 0): "apply_pencil_kernel<4,false,4,25,1,true,8388608>", ("helmholtz", 4, 1): "apply_pencil_kernel<4,true,4,25,1,true,8388608>",
    ("helmholtz", 5, 0): "apply_pencil_kernel<5,false,4,36,1,true,8388608>", ("helmholtz", 5, 1): "apply_pencil_kernel<5,true,4,36,1,true,8388608>",
    ("helmholtz", 6, 0): "apply_pencil_kernel<6,false,4,49,1,true,8388608>", ("helmholtz", 6, 1): "apply_pencil_kernel<6,true,4,49,1,true,8388608>",
    ("helmholtz", 7, 0): "apply_pencil_kernel<7,false,4,64,1,true,8388608>", ("helmholtz", 7, 1): "apply_pencil_kernel<7,true,4,64,1,true,8388608>",
    ("helmholtz", 8, 0): "apply_pencil_kernel<8,false,4,81,1,true,8388608>", ("helmholtz", 8, 1): "apply_pencil_kernel<8,true,4,81,1,true,8388608>",
    ("hanging", 1, 0): "apply_pencil_kernel<1,false,1,4,4,true,2097152>", ("hanging", 1, 1): "apply_pencil_kernel<1,true,1,4,4,true,2097152>",
    ("hanging", 2, 0): "apply_pencil_kernel<2,false,1,9,4,true,2097152>", ("hanging", 2, 1): "apply_pencil_kernel<2,true,1,9,4,true,2097152>",
    ("hanging", 3, 0): "apply_pencil_kernel<3,false,1,16,4,true,2097152>", ("hanging", 3, 1): "apply_pencil_kernel<3,true,1,16,4,true,2097152>",
    ("hanging", 4, 0): "apply_pencil_kernel<4,false,4,25,1,true,2097152>", ("hanging", 4, 1): "apply_pencil_kernel<4,true,4,25,1,true,2097152>",
    ("hanging", 5, 0): "apply_pencil_kernel<5,false,4,36,1,true,2097152>", ("hanging", 5, 1): "apply_pencil_kernel<5,true,4,36,1,true,2097152>",
    ("hanging", 6, 0): "apply_pencil_kernel<6,false,4,49,1,true,2097152>", ("hanging", 6, 1): "apply_pencil_kernel<6,true,4,49,1,true,2097152>",
    ("hanging", 7, 0): "apply_pencil_kernel<7,false,4,64,1,true,2097152>", ("hanging", 7, 1): "apply_pencil_kernel<7,true,4,64,1,true,2097152>",
    ("hanging", 8, 0): "apply_pencil_kernel<8,false,4,81,1,true,2097152>", ("hanging", 8, 1): "apply_pencil_kernel<8,true,4,81,1,true,2097152>",
    ("affine", 1, 0): "apply_pencil_kernel<1,false,4,4,1,true,1024>", ("affine", 1, 1): "apply_pencil_kernel<1,true,4,4,1,true,1024>",
    ("affine", 2, 0): "apply_pencil_kernel<2,false,4,9,1,true,1024>", ("affine", 2, 1): "apply_pencil_kernel<2,true,4,9,1,true,1024>",
    ("affine", 3, 0): "apply_pencil_kernel<3,false,4,16,1,true,1024>", ("affine", 3, 1): "apply_pencil_kernel<3,true,4,16,1,true,1024>",
    ("affine", 4, 0): "apply_team_kernel<4,false,4,25,true,", ("affine", 4, 1): "apply_team_kernel<4,true,4,25,true,",
    ("affine", 5, 0): "apply_pencil_kernel<5,false,4,36,1,true,1024>", ("affine", 5, 1): "apply_pencil_kernel<5,true,4,36,1,true,1024>",
    ("affine", 6, 0): "apply_pencil_kernel<6,false,4,49,1,true,1024>", ("affine", 6, 1): "apply_pencil_kernel<6,true,4,49,1,true,1024>",
    ("affine", 7, 0): "apply_pencil_kernel<7,false,4,64,1,true,1024>", ("affine", 7, 1): "apply_pencil_kernel<7,true,4,64,1,true,1024>",
    ("affine", 8, 0): "apply_pencil_kernel<8,false,4,81,1,true,1024>", ("affine", 8, 1): "apply_pencil_kernel<8,true,4,81,1,true,1024>",
    ("hanging_affine", 1, 0): "apply_pencil_kernel<1,false,1,4,4,true,2098176>", ("hanging_affine", 1, 1): "apply_pencil_kernel<1,true,1,4,4,true,2098176>",
    ("hanging_affine", 2, 0): "apply_pencil_kernel<2,false,1,9,4,true,2098176>", ("hanging_affine", 2, 1): "apply_pencil_kernel<2,true,1,9,4,true,2098176>",
    ("hanging_affine", 3, 0): "apply_pencil_kernel<3,false,1,16,4,true,2098176>", ("hanging_affine", 3, 1): "apply_pencil_kernel<3,true,1,16,4,true,2098176>",
    ("hanging_affine", 4, 0): "apply_pencil_kernel<4,false,4,25,1,true,2098176>", ("hanging_affine", 4, 1): "apply_pencil_kernel<4,true,4,25,1,true,2098176>",
    ("hanging_affine", 5, 0): "apply_pencil_kernel<5,false,4,36,1,true,2098176>", ("hanging_affine", 5, 1): "apply_pencil_kernel<5,true,4,36,1,true,2098176>",
    ("hanging_affine", 6, 0): "apply_pencil_kernel<6,false,4,49,1,true,2098176>", ("hanging_affine", 6, 1): "apply_pencil_kernel<6,true,4,49,1,true,2098176>",
    ("hanging_affine", 7, 0): "apply_pencil_kernel<7,false,4,64,1,true,2098176>", ("hanging_affine", 7, 1): "apply_pencil_kernel<7,true,4,64,1,true,2098176>",
    ("hanging_affine", 8, 0): "apply_pencil_kernel<8,false,4,81,1,true,2098176>", ("hanging_affine", 8, 1): "apply_pencil_kernel<8,true,4,81,1,true,2098176>",
}
# cell-interior DoFs numbered first, p >= 5: plain stores for the entries a cell owns alone
INTERIOR_STORES = {(5, 0): "apply_pencil_kernel<5,false,4,36,1,true,32>", (5, 1): "apply_pencil_kernel<5,true,4,36,1,true,32>", (6, 0): "apply_pencil_kernel<6,false,4,49,1,true,32>", (6, 1): "apply_pencil_kernel<6,true,4,49,1,true,32>", (7, 0): "apply_pencil_kernel<7,false,4,64,1,true,32>", (7, 1): "apply_pencil_kernel<7,true,4,64,1,true,32>", (8, 0): "apply_pencil_kernel<8,false,4,81,1,true,32>", (8, 1): "apply_pencil_kernel<8,true,4,81,1,true,32>"}
# p = 4 without packed indices: run-length write-out with list loads, list write-out
P4_RUNS = ["apply_block_kernel<4,false,32,1,26624>", "apply_block_kernel<4,true,32,1,26624>"]
P4_LISTS = ["apply_block_kernel<4,false,32,1,10240>", "apply_block_kernel<4,true,32,1,10240>"]


@functools.lru_cache(maxsize=None)
def _mesh(cls, p):
    if cls == "hanging":
        kind, amp, group = HANGING[p]
        return _with_cell_blocks(_refined(kind, p, amp), group)[0]
    cells, block = BRICKS[p]
    return pkg.BrickMesh(p, cells, h=0.2, deform_amp=0.0 if cls == "affine" else 0.03, cell_block=block, dof_numbering=1, cell_block_order=1)


def _operator(cls, mesh, quad):
    if cls == "helmholtz":
        return pkg.HelmholtzOperator(mesh, quad)
    if cls == "f32":
        return pkg.PoissonOperator(mesh, quad, pkg.COEF_STEP64, metric_precision="float32")
    if cls == "affine":
        return pkg.PoissonOperator(mesh, quad, pkg.COEF_STEP64, geometry=pkg.GEOM_AFFINE)
    return pkg.PoissonOperator(mesh, quad, pkg.COEF_STEP64)


def _solve(op, b, solver):
    x = op.initialize_dof_vector()
    ctl = pkg.IterationNumberControl(ITS, 0.0)
    solver(ctl).solve(op, x, b, pkg.DiagonalMatrix())
    assert ctl.last_step() == ITS
    return x, ctl


def _close(x, ref):
    return float((x - ref).abs().max()) < 1e-12 * float(ref.abs().max())


def _pencil_variant(cls, p):
    """the variant number that runs the degree's default pencil shape with atomics on this handle"""
    if cls == "hanging":
        return 90
    if cls == "poisson":
        return 1 if p in (1, 3) else 3 if p == 4 else 0     # (0 would resolve to the team kernel at p = 1, 3; 3 is p = 4's default shape)
    return 3 if cls == "affine" else 0


CASES = [(cls, p, quad) for cls in ("poisson", "f32", "helmholtz", "hanging") for p in range(1, 9) for quad in (0, 1)] + [("affine", 4, 0), ("affine", 4, 1)]


@pytest.mark.parametrize("cls,p,quad", CASES)
def test_variant_56_launches_the_pinned_build(cls, p, quad):
    """every build of the default block kernel: operator class x degree x quadrature, then lattice or packed indices, the three solver rows,
    both streaming policies and (p = 4) the face carry on and off"""
    mesh = _mesh(cls, p)
    want = BLOCK_KERNEL[cls, p, quad]
    # (solver, bp5_mf_set_cg_fusion, the dot products are fused); no fused build reads float planes or the affine geometry: the request is not made
    if cls in ("f32", "affine"):
        rows = [(pkg.SolverCGFullMerge, 1, 0), (pkg.SolverCG, 1, 0)]
    else:
        rows = [(pkg.SolverCGFullMerge, 1, 1), (pkg.SolverCG, 1, 1), (pkg.SolverCG, 0, 0)]
    for lattice in (1, 0):
        op = _operator(cls, mesh, quad)
        mf = op.mf_data
        mf.set_tuning("lattice_indices", lattice)
        mf.set_block_workgroups(8)
        b = op.assemble_rhs()
        mf.set_apply_variant(_pencil_variant(cls, p))
        ref = {}
        for solver in (pkg.SolverCGFullMerge, pkg.SolverCG):
            ref[solver], ctl = _solve(op, b, solver)
            assert ctl.apply_kernel == PENCIL_KERNEL[cls, p, quad] and not ctl.dot_products_fused
        assert _close(ref[pkg.SolverCG], ref[pkg.SolverCGFullMerge])
        mf.set_apply_variant(56)
        nb, _, packed = mf.block_plan_info()
        assert packed and (cls == "hanging" or mf.block_plan_lattice() == (nb if lattice else 0))   # (bricks: every block a lattice block)
        for solver, fusion, fused in rows:
            mf.set_cg_fusion(fusion)
            for streaming in (0, 1):
                mf.set_streaming(streaming)
                for carry in ((0, 1) if p == 4 else (1,)):
                    mf.set_tuning("face_carry", carry)
                    x, ctl = _solve(op, b, solver)
                    where = (cls, p, quad, solver.__name__, fusion, lattice, streaming, carry)
                    assert ctl.apply_kernel == want[fused, lattice, streaming], where
                    assert ctl.dot_products_fused == bool(fused), where
                    assert _close(x, ref[solver]), where


@pytest.mark.parametrize("quad", [0, 1])
def test_p4_plans_without_packed_indices_take_the_two_fallbacks(quad):
    """p = 4 keeps a kernel for plans without packed indices: the run-length write-out with list loads while a block has at most 128 runs
    (variant 49 asks for it on any plan), the list write-out beyond (lexicographic numbering: hundreds of short runs per brick).  No fused
    build among them: the solver forms its dot products itself."""
    for numbering, variant, name in ((1, 49, P4_RUNS[quad]), (0, 56, P4_LISTS[quad])):
        mesh = pkg.BrickMesh(4, (9, 5, 6), h=0.2, deform_amp=0.03, cell_block=(4, 4, 4), dof_numbering=numbering, cell_block_order=1)
        op = pkg.PoissonOperator(mesh, quad, pkg.COEF_STEP64)
        mf = op.mf_data
        mf.set_block_workgroups(8)
        _, max_runs, packed = mf.block_plan_info()
        assert packed == (numbering == 1) and (max_runs > 128) == (numbering == 0)
        b = op.assemble_rhs()
        mf.set_apply_variant(3)
        ref, _ = _solve(op, b, pkg.SolverCGFullMerge)
        mf.set_apply_variant(variant)
        x, ctl = _solve(op, b, pkg.SolverCGFullMerge)
        assert ctl.apply_kernel == name and not ctl.dot_products_fused
        assert _close(x, ref)


@pytest.mark.parametrize("p", range(1, 9))
@pytest.mark.parametrize("quad", [0, 1])
def test_variant_0_launches_the_default_pencil_shape(p, quad):
    """variant 0 on meshes too small for the block kernel to pay: the degree's default pencil shape in the build of the operator class (the
    team kernel for Poisson at p = 1, 3 and for the affine geometry at p = 4); with the cell-interior DoFs numbered first, p >= 5 stores them plainly"""
    for cls in ("poisson", "f32", "helmholtz", "hanging", "affine", "hanging_affine"):
        team = (cls == "poisson" and p in (1, 3)) or (cls == "affine" and p == 4)
        if cls == "hanging_affine":                  # undeformed 2:1 meshes: per-cell K K^T + one scalar plane, pencil kernel only
            kind, _, group = HANGING[p]
            op = _operator("affine", _with_cell_blocks(_refined(kind, p, 0.0), group)[0], quad)
        elif team:                                   # x-row teams: a lexicographic cell order (test_default_variant_resolution)
            op = _operator(cls, pkg.BrickMesh(p, (3, 3, 3), h=0.2, deform_amp=0.0 if cls == "affine" else 0.03), quad)
        else:
            op = _operator(cls, _mesh(cls, p), quad)
        mf = op.mf_data
        mf.set_block_workgroups(8)
        b = op.assemble_rhs()
        assert mf.get_apply_variant() == (90 if cls.startswith("hanging") else 10 if team else 0)
        x, ctl = _solve(op, b, pkg.SolverCGFullMerge)
        assert ctl.apply_kernel == VARIANT_0[cls, p, quad], (cls, p, quad)
        if cls == "hanging_affine" or (cls == "affine" and p != 4):
            continue                                 # (one kernel for every variant: nothing to compare with)
        mf.set_apply_variant(_pencil_variant(cls, p) if team else 56)
        y, _ = _solve(op, b, pkg.SolverCGFullMerge)
        assert _close(y, x), (cls, p, quad)
    if p >= 5:
        mesh = pkg.BrickMesh(p, (3, 3, 2), h=0.25, deform_amp=0.03, dof_numbering=2)
        op = pkg.PoissonOperator(mesh, quad, pkg.COEF_STEP64)
        b = op.assemble_rhs()
        x, ctl = _solve(op, b, pkg.SolverCGFullMerge)
        assert ctl.apply_kernel == INTERIOR_STORES[p, quad]
        op.mf_data.set_tuning("interior_stores", 0)
        y, ctl = _solve(op, b, pkg.SolverCGFullMerge)
        assert ctl.apply_kernel == PENCIL_KERNEL["poisson", p, quad] and _close(x, y)


def _refused(op, status):
    d = op.initialize_dof_vector()
    with pytest.raises(pkg.BP5Error) as e:
        op.vmult(d, op.assemble_rhs())
    assert e.value.status == status, str(e.value)


@pytest.mark.parametrize("p", [2, 4])
def test_refusals_keep_their_status_codes(p):
    """what variant 56 refuses: a mesh without cell blocks (INVALID: no cell range is aligned with blocks), a plan without packed indices
    away from p = 4 Poisson (UNSUPPORTED), hanging nodes in the affine geometry mode (UNSUPPORTED at the request); and the operator classes
    with two kernels refuse every other variant at the request (UNSUPPORTED)"""
    for cls in ("poisson", "f32", "helmholtz"):
        op = _operator(cls, pkg.BrickMesh(p, (3, 3, 2), h=0.2, deform_amp=0.03), 0)
        op.mf_data.set_apply_variant(56)
        _refused(op, INVALID)
        cells, block = BRICKS[p]                     # lexicographic numbering: a run per x-line of a brick, more than 128 of them
        lexicographic = pkg.BrickMesh(p, cells, h=0.2, deform_amp=0.03, cell_block=block, dof_numbering=0)
        op = _operator(cls, lexicographic, 0)
        assert not op.mf_data.block_plan_info()[2]
        op.mf_data.set_apply_variant(56)
        if (cls, p) != ("poisson", 4):
            _refused(op, UNSUPPORTED)
        if cls != "poisson":
            with pytest.raises(pkg.BP5Error) as e:
                op.mf_data.set_apply_variant(10)
            assert e.value.status == UNSUPPORTED
    kind, _, group = HANGING[p]
    flat = _with_cell_blocks(_refined(kind, p, 0.0), group)[0]
    op = pkg.PoissonOperator(flat, 0, pkg.COEF_STEP64, geometry=pkg.GEOM_AFFINE)
    with pytest.raises(pkg.BP5Error) as e:
        op.mf_data.set_apply_variant(56)
    assert e.value.status == UNSUPPORTED
    op = pkg.PoissonOperator(_hanging_namespace(_refined(kind, p, 0.0)), 0, pkg.COEF_STEP64)
    op.mf_data.set_apply_variant(56)                 # hanging nodes without cell blocks
    _refused(op, INVALID)
    with pytest.raises(pkg.BP5Error) as e:
        op.mf_data.set_apply_variant(3)
    assert e.value.status == UNSUPPORTED
