"""Static checks of the gfx950 ISA of the FP32-metric builds of the fused operator (BLK_F32M, bp5_mf_set_metric_precision; no GPU needed):
the p = 4 builds use no scratch and stay within the register budget of three waves per SIMD -- the default shapes run three workgroups per
CU.  Same files and the same regular expression as tests/test_isa_checks.py."""
import re

from test_isa_checks import _isa

F32M = 536870912                                                 # bp5_kernels.hpp: BLK_F32M
PACKED = 2048 + 8192 + 16384 + 262144 + F32M                     # BLK_DEFAULT | BLK_F32M
LATTICE_CARRY = PACKED + 16777216 + 268435456                    # ... | BLK_LATT | BLK_CARRY


def test_p4_f32_metric_kernels_do_not_spill():
    text = "".join(open(f).read() for f in _isa())
    want = []
    for coll in (0, 1):                                          # both quadratures are instantiated for every shape
        for scatter in (1, 2, 3, 4):                             # owner stores set / add, with and without atomics for shared DoFs (cell ranges)
            want += [f"apply_block_kernelILi4ELb{coll}ELi32ELi{scatter}ELi{PACKED}E", f"apply_block_kernelILi4ELb{coll}ELi32ELi{scatter}ELi{LATTICE_CARRY}E"]
        want.append(f"apply_pencil_kernelILi4ELb{coll}ELi4ELi25ELi1ELb1ELi{F32M}E")
    for key in want:
        m = re.search(r"\.name:\s+_ZN3bp5\d+" + re.escape(key) + r"\w*\n\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n){1,8}?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
        assert m, key
        assert int(m.group(1)) == 0 and int(m.group(3)) == 0, (key, m.groups())
        assert int(m.group(2)) <= 168, (key, m.groups())
