"""Register budget of the fused-update builds of the p = 4 lattice block kernel (BLK_UPD, BP5_TUNE_FUSED_UPDATE), from the metadata of the code
object the library was built from (no GPU needed; csrc/Makefile keeps the assembly of the device compile).  The kernel lives on three
workgroups per CU: at most 168 VGPRs, no scratch, nothing spilled -- with the vector update of a brick's interior inlined into its pass loop."""
import os
import re

import pytest

import bp5_pkg

ISA = os.path.join(bp5_pkg.ROOT, "deal-and-ceed-on-gpu_amd", "csrc", "bp5_apply_p4-hip-amdgcn-amd-amdhsa-gfx950.s")
BASE = 286550016                      # fused dot products, lattice blocks, face carry (the bench's kernel)
BUILDS = [(coll, BASE + 131072 + ntm) for coll in (0, 1) for ntm in (0, 32768)]   # + BLK_UPD, with and without non-temporal metric loads


@pytest.mark.parametrize("coll,mask", BUILDS)
def test_fused_update_builds_keep_three_workgroups_per_cu(coll, mask):
    assert os.path.exists(ISA), f"device ISA {ISA} missing: run __graft_entry__.build() (make -C deal-and-ceed-on-gpu_amd/csrc)"
    text = open(ISA).read()
    key = f"apply_block_kernelILi4ELb{coll}ELi32ELi1ELi{mask}E"
    m = re.search(r"\.name:\s+_ZN3bp5\d+" + re.escape(key) + r"\w*\n\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n){1,8}?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert m, key
    scratch, vgprs, spilled = (int(g) for g in m.groups())
    assert scratch == 0 and spilled == 0 and vgprs <= 168, (key, scratch, vgprs, spilled)
