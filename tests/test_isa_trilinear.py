"""Static checks of the gfx950 ISA of the trilinear geometry mode (BP5_GEOM_TRILINEAR; no GPU needed): the translation unit
csrc/trilinear/bp5_trilinear keeps its ISA beside it (csrc/Makefile, --save-temps); __graft_entry__.build() produces it.  The sixteen operator kernels
(p = 1 .. 8, Gauss and GLL, the degree's default pencil shape) and the setup and diagonal kernels of every degree are present, no kernel of p <= 4
uses scratch or spills, the register / LDS / scratch figures of every build are printed beside those of its apply_pencil_kernel twin (DESIGN 7l quotes
the table), and tools/check_lds_barrier.py passes on the file.  The pattern of tests/test_isa_overint.py."""
import os
import re
import sys

import bp5_pkg

CSRC = os.path.join(bp5_pkg.ROOT, "deal-and-ceed-on-gpu_amd", "csrc")
SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"
ISA = os.path.join(CSRC, "trilinear", "bp5_trilinear" + SUFFIX)
sys.path.insert(0, os.path.join(bp5_pkg.ROOT, "tools"))


def _text(path=ISA):
    lib = os.path.join(bp5_pkg.ROOT, "deal-and-ceed-on-gpu_amd", "libbp5.so")
    assert os.path.exists(path), f"device ISA {path} missing: run __graft_entry__.build() (make -C deal-and-ceed-on-gpu_amd/csrc)"
    assert os.path.getmtime(path) <= os.path.getmtime(lib) + 1.0, "ISA is newer than libbp5.so: rebuild"
    return open(path).read()


def shape(p):
    """DefaultPencil<p> (csrc/bp5_device.hpp): (TW, LPC, TPB)"""
    return (1 if p <= 3 else 4, (p + 1) ** 2, 4 if p <= 3 else 1)


def operator_key(p, coll):
    tw, lpc, tpb = shape(p)
    return f"apply_pencil_trilinear_kernelILi{p}ELb{coll}ELi{tw}ELi{lpc}ELi{tpb}EE"


def twin_key(p, coll):
    """apply_pencil_kernel<P, COLL, TW, LPC, TPB, PF = true, ABL = 0>: variant 0 of a MERGED6 handle"""
    tw, lpc, tpb = shape(p)
    return f"apply_pencil_kernelILi{p}ELb{coll}ELi{tw}ELi{lpc}ELi{tpb}ELb1ELi0EE"


def _metadata(text, key):
    """(static LDS bytes, scratch bytes, SGPRs, spilled SGPRs, VGPRs, spilled VGPRs) from the amdhsa.kernels entry of the kernel"""
    m = re.search(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n){1,9}?\s+\.name:\s+_ZN3bp5\d+" + re.escape(key) + r"\w*\n\s+\.private_segment_fixed_size:\s+(\d+)\n"
                  r"\s+\.sgpr_count:\s+(\d+)\n\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n){1,4}?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert m, key
    return tuple(int(g) for g in m.groups())


def lds_bytes(p):
    """dynamic LDS of one workgroup: TPB * CPT cell slots of LdsLayout<n, n^2>::CS doubles (csrc/bp5_kernels.hpp; n = 9: the generic layout)"""
    n = p + 1
    tw, lpc, tpb = shape(p)
    cs = {2: 36, 3: 169, 4: 240, 5: 377, 6: 648, 7: 1092, 8: 1728, 9: 3 * 9 * (81 + 1) + 1}[n]
    return tpb * (64 * tw // lpc) * cs * 8


def test_the_sixteen_operator_kernels_are_present_and_low_degrees_do_not_spill():
    text = _text()
    out = {(p, coll): _metadata(text, operator_key(p, coll)) for p in range(1, 9) for coll in (0, 1)}
    assert len(out) == 16
    print("apply_pencil_trilinear_kernel | apply_pencil_kernel twin: degree quadrature VGPRs spilled-VGPRs SGPRs spilled-SGPRs scratch-B | the same of the twin | LDS-B(dynamic)")
    for (p, coll), (lds, scratch, sgpr, sspill, vgpr, vspill) in sorted(out.items()):
        tl, ts, tsg, tss, tv, tvs = _metadata(_text(os.path.join(CSRC, f"bp5_apply_p{p}" + SUFFIX)), twin_key(p, coll))
        print(f"  p={p} {'GLL  ' if coll else 'Gauss'} {vgpr:4d} {vspill:3d} {sgpr:4d} {sspill:3d} {scratch:5d} | {tv:4d} {tvs:3d} {tsg:4d} {tss:3d} {ts:5d} | {lds_bytes(p):6d}")
        assert lds == 0 and tl == 0, (p, coll, lds, tl)         # the tiles are dynamic LDS, the same bytes in both
    for (p, coll), (lds, scratch, sgpr, sspill, vgpr, vspill) in out.items():
        if p <= 4:
            assert scratch == 0 and vspill == 0, (p, coll, scratch, vgpr, vspill)
    names = set(re.findall(r"\.name:\s+(_ZN3bp5\d+apply_pencil_trilinear_kernel\w+)\n", text))
    assert len({n for n in names if not n.endswith(".kd")}) == 16, sorted(names)


def test_the_setup_and_diagonal_kernels_of_every_degree_are_present():
    text = _text()
    for name in ("trilinear_setup_kernel", "trilinear_diagonal_kernel"):
        for p in range(1, 9):
            lds, scratch, sgpr, sspill, vgpr, vspill = _metadata(text, f"{name}ILi{p + 1}EE")
            print(f"{name} p={p}: {vgpr} VGPRs ({vspill} spilled), {sgpr} SGPRs ({sspill} spilled), static LDS {lds} B, scratch {scratch} B")
            if p <= 4:
                assert scratch == 0 and vspill == 0, (name, p, scratch, vspill)
        names = set(re.findall(r"\.name:\s+(_ZN3bp5\d+" + name + r"I\w+)\n", text))
        assert len({n for n in names if not n.endswith(".kd")}) == 8, (name, sorted(names))


def test_no_barrier_is_reached_with_an_lds_write_in_flight():
    import check_lds_barrier
    _text()
    assert check_lds_barrier.main(ISA) == 0


def test_cells_that_span_waves_use_the_workgroup_barrier_and_one_wave_teams_do_not():
    text = _text()
    for p in range(1, 9):
        tw = shape(p)[0]
        for coll in (0, 1):
            key = operator_key(p, coll)
            m = re.search(r"^(_ZN3bp5\d+" + re.escape(key) + r"\w*):[^\n]*\n(.*?)\n\s+s_endpgm", text, re.S | re.M)
            assert m, key
            assert ("s_barrier" in m.group(2)) == (tw > 1), (p, coll)
