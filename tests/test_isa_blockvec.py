"""Static checks of the gfx950 ISA of the pointwise and transfer kernels (chebyshev_step_kernel, mg_prolongate / mg_restrict / mg_combine_kernel,
the block form mg_restrict_components_kernel and the geometric pair; no GPU needed): the translation unit csrc/blockvec/bp5_blockvec is the
only one that instantiates them and keeps its ISA beside it (csrc/Makefile, --save-temps); __graft_entry__.build() produces it.  Every
instantiated build is present there and none is left in the device unit; none uses scratch or spills; the static LDS of every transfer kernel
is the figure that follows from its shape; the register table is printed (DESIGN 7k quotes it); tools/check_lds_barrier.py passes on the
file.  The pattern of tests/test_isa_elasticity.py."""
import os
import re
import sys

import bp5_pkg

CSRC = os.path.join(bp5_pkg.ROOT, "deal-and-ceed-on-gpu_amd", "csrc")
SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"
ISA = os.path.join(CSRC, "blockvec", "bp5_blockvec" + SUFFIX)
DEVICE_ISA = os.path.join(CSRC, "bp5_device" + SUFFIX)
sys.path.insert(0, os.path.join(bp5_pkg.ROOT, "tools"))

P_PAIRS = [(p + 1, max(1, p // 2) + 1) for p in range(2, 9)]       # (NF, NC) of the p-transfer pf -> max(1, pf / 2)
GEO_N = [p + 1 for p in range(1, 5)]                               # the geometric transfer, degree 1 .. 4


def _text(path=ISA):
    lib = os.path.join(bp5_pkg.ROOT, "deal-and-ceed-on-gpu_amd", "libbp5.so")
    assert os.path.exists(path), f"device ISA {path} missing: run __graft_entry__.build() (make -C deal-and-ceed-on-gpu_amd/csrc)"
    assert os.path.getmtime(path) <= os.path.getmtime(lib) + 1.0, "ISA is newer than libbp5.so: rebuild"
    return open(path).read()


def _metadata(text, key):
    """(static LDS bytes, scratch bytes, SGPRs, spilled SGPRs, VGPRs, spilled VGPRs) from the amdhsa.kernels entry of the kernel"""
    m = re.search(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n){1,9}?\s+\.name:\s+_ZN3bp5\d+" + re.escape(key) + r"\w*\n\s+\.private_segment_fixed_size:\s+(\d+)\n"
                  r"\s+\.sgpr_count:\s+(\d+)\n\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n){1,4}?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert m, key
    return tuple(int(g) for g in m.groups())


def mg_shape(nf, nc):
    """MgShape<NF, NC> (csrc/bp5_kernels.hpp): (cells per workgroup, doubles of LDS per cell)"""
    f3 = nf ** 3
    return (1 if f3 >= 256 else 256 // f3), f3 + nc * nf * nf + nc * nc * nf


def lds_bytes(nf, nc, geo):
    """8 * (CPB * MgShape::LDS + table entries) bytes, and 4 * CPB for the child codes of the geometric kernels; the compiler places each array on a
    16-byte boundary, which pads the cell tiles when their doubles are odd in number, and rounds the segment up to whole doubles"""
    cpb, per_cell = mg_shape(nf, nc)
    tiles, tables = 8 * cpb * per_cell, 8 * (2 * nf * nf if geo else nf * nc)
    return ((tiles + 15) // 16 * 16 + tables + (4 * cpb if geo else 0) + 7) // 8 * 8


def kernels():
    """{printed name: (mangled key, expected static LDS)} of every build the unit instantiates"""
    out = {}
    for form in range(4):
        for diag in (0, 1):
            for nt in (0, 1):
                out[f"chebyshev_step_kernel<{form},{diag},{nt}>"] = (f"chebyshev_step_kernelILi{form}ELb{diag}ELb{nt}EE", 0)
    for nf, nc in P_PAIRS:
        out[f"mg_prolongate_kernel<{nf},{nc}>"] = (f"mg_prolongate_kernelILi{nf}ELi{nc}EE", lds_bytes(nf, nc, False))
        for res in (0, 1):
            for form in ("", "_components"):      # the restriction alone keeps a body of its own for one component (csrc/bp5_kernels.hpp)
                out[f"mg_restrict{form}_kernel<{nf},{nc},{res}>"] = (f"mg_restrict{form}_kernelILi{nf}ELi{nc}ELb{res}EE", lds_bytes(nf, nc, False))
    for n in GEO_N:
        out[f"mg_geo_prolongate_kernel<{n}>"] = (f"mg_geo_prolongate_kernelILi{n}EE", lds_bytes(n, n, True))
        for res in (0, 1):
            out[f"mg_geo_restrict_kernel<{n},{res}>"] = (f"mg_geo_restrict_kernelILi{n}ELb{res}EE", lds_bytes(n, n, True))
    for add in (0, 1):
        out[f"mg_combine_kernel<{add}>"] = (f"mg_combine_kernelILb{add}EE", 0)
    return out


def test_every_step_and_transfer_kernel_is_here_without_scratch_and_with_the_lds_of_its_shape():
    text = _text()
    want = kernels()
    assert len(want) == 16 + 7 * (1 + 4) + 4 * 3 + 2
    print("kernel: VGPRs SGPRs static-LDS-B scratch-B")
    for name, (key, lds_want) in want.items():
        lds, scratch, sgpr, sspill, vgpr, vspill = _metadata(text, key)
        print(f"  {name:38s} {vgpr:4d} {sgpr:4d} {lds:6d} {scratch:3d}")
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        assert lds == lds_want, (name, lds, lds_want)
    # ... and nothing else of these families: one kernel per role and build
    names = set(re.findall(r"\.name:\s+(_ZN3bp5\d+(?:mg_|chebyshev_step)\w+)\n", text))
    assert len({n for n in names if not n.endswith(".kd")}) == len(want), sorted(names)


def test_the_device_unit_holds_no_step_or_transfer_kernel():
    names = re.findall(r"\.name:\s+(\S+)\n", _text(DEVICE_ISA))
    assert names and not [n for n in names if "mg_" in n or "chebyshev_step" in n]


def test_no_barrier_is_reached_with_an_lds_write_in_flight():
    import check_lds_barrier
    _text()
    assert check_lds_barrier.main(ISA) == 0
