"""Static checks of the gfx950 ISA of the neo-Hookean kernels (bp5_hyperelasticity_*; no GPU needed): the translation unit
csrc/hyperelasticity/bp5_hyperelasticity keeps its ISA beside it (csrc/Makefile, --save-temps); __graft_entry__.build() produces it.  The 32
operator kernels (p = 1 .. 8, Gauss and GLL, residual and tangent, the degree's default pencil shape) are present, no p <= 4 kernel uses scratch
or spills, the register / LDS / scratch figures of all of them are printed (DESIGN 7m quotes the table), and tools/check_lds_barrier.py passes on
the file.  The pattern of tests/test_isa_elasticity.py."""
import os
import re
import sys

import bp5_pkg

CSRC = os.path.join(bp5_pkg.ROOT, "deal-and-ceed-on-gpu_amd", "csrc")
ISA = os.path.join(CSRC, "hyperelasticity", "bp5_hyperelasticity-hip-amdgcn-amd-amdhsa-gfx950.s")
sys.path.insert(0, os.path.join(bp5_pkg.ROOT, "tools"))
MODES = {0: "residual", 1: "tangent"}


def _text():
    lib = os.path.join(bp5_pkg.ROOT, "deal-and-ceed-on-gpu_amd", "libbp5.so")
    assert os.path.exists(ISA), f"device ISA {ISA} missing: run __graft_entry__.build() (make -C deal-and-ceed-on-gpu_amd/csrc)"
    assert os.path.getmtime(ISA) <= os.path.getmtime(lib) + 1.0, "ISA is newer than libbp5.so: rebuild"
    return open(ISA).read()


def shape(p):
    """DefaultPencil<p> (csrc/bp5_device.hpp): (TW, LPC, TPB)"""
    return (1 if p <= 3 else 4, (p + 1) ** 2, 4 if p <= 3 else 1)


def operator_key(p, coll, mode):
    tw, lpc, tpb = shape(p)
    return f"apply_pencil_hyperelasticity_kernelILi{p}ELb{coll}ELi{tw}ELi{lpc}ELi{tpb}ELi{mode}EE"


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


def test_the_32_operator_kernels_are_present_and_low_degrees_do_not_spill():
    text = _text()
    out = {(p, coll, mode): _metadata(text, operator_key(p, coll, mode)) for p in range(1, 9) for coll in (0, 1) for mode in MODES}
    assert len(out) == 32
    print("apply_pencil_hyperelasticity_kernel: degree quadrature mode VGPRs spilled-VGPRs SGPRs spilled-SGPRs scratch-B LDS-B(dynamic) waves/SIMD(by VGPRs)")
    for (p, coll, mode), (lds, scratch, sgpr, sspill, vgpr, vspill) in sorted(out.items()):
        waves = min(8, 512 // max(vgpr, 1))
        print(f"  p={p} {'GLL  ' if coll else 'Gauss'} {MODES[mode]:8s} {vgpr:4d} {vspill:3d} {sgpr:4d} {sspill:3d} {scratch:5d} {lds_bytes(p):6d} {waves}")
        assert lds == 0, (p, coll, mode, lds)         # the tiles are dynamic LDS
    for (p, coll, mode), (lds, scratch, sgpr, sspill, vgpr, vspill) in out.items():
        if p <= 4:
            assert scratch == 0 and vspill == 0, (p, coll, mode, scratch, vgpr, vspill)
    names = set(re.findall(r"\.name:\s+(_ZN3bp5\d+apply_pencil_hyperelasticity_kernel\w+)\n", text))
    assert len({n for n in names if not n.endswith(".kd")}) == 32, sorted(names)


def test_no_barrier_is_reached_with_an_lds_write_in_flight():
    import check_lds_barrier
    _text()
    assert check_lds_barrier.main(ISA) == 0


def test_cells_that_span_waves_use_the_workgroup_barrier_and_one_wave_teams_do_not():
    text = _text()
    for p in range(1, 9):
        tw = shape(p)[0]
        for coll in (0, 1):
            for mode in MODES:
                key = operator_key(p, coll, mode)
                m = re.search(r"^(_ZN3bp5\d+" + re.escape(key) + r"\w*):[^\n]*\n(.*?)\n\s+s_endpgm", text, re.S | re.M)
                assert m, key
                assert ("s_barrier" in m.group(2)) == (tw > 1), (p, coll, mode)


def test_the_tangent_has_no_division_and_no_logarithm():
    """the tangent's quadrature-point function reads B and ln J from the state: no reciprocal, no division, no logarithm in its ISA (the residual
    has them)"""
    text = _text()
    for mode, expected in ((1, False), (0, True)):
        m = re.search(r"^(_ZN3bp5\d+" + re.escape(operator_key(2, 0, mode)) + r"\w*):[^\n]*\n(.*?)\n\s+s_endpgm", text, re.S | re.M)
        assert m
        found = any(op in m.group(2) for op in ("v_rcp_f64", "v_div_scale_f64", "v_div_fmas_f64", "v_frexp_mant_f64"))
        assert found == expected, (mode, found)
