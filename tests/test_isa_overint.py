"""Static checks of the gfx950 ISA of the Gauss(p+2) kernels (BP5_QUAD_GAUSS_OVER; no GPU needed): the translation unit csrc/overint/bp5_overint
keeps its ISA beside it (csrc/Makefile, --save-temps); __graft_entry__.build() produces it.  Every new kernel is present once per degree, none of
p <= 4 uses scratch or spills, the register / LDS / scratch figures of all of them are printed, and tools/check_lds_barrier.py passes on the
file.  The pattern of tests/test_isa_mass.py."""
import os
import re
import sys

import bp5_pkg

CSRC = os.path.join(bp5_pkg.ROOT, "deal-and-ceed-on-gpu_amd", "csrc")
ISA = os.path.join(CSRC, "overint", "bp5_overint-hip-amdgcn-amd-amdhsa-gfx950.s")
sys.path.insert(0, os.path.join(bp5_pkg.ROOT, "tools"))


def _text():
    lib = os.path.join(bp5_pkg.ROOT, "deal-and-ceed-on-gpu_amd", "libbp5.so")
    assert os.path.exists(ISA), f"device ISA {ISA} missing: run __graft_entry__.build() (make -C deal-and-ceed-on-gpu_amd/csrc)"
    assert os.path.getmtime(ISA) <= os.path.getmtime(lib) + 1.0, "ISA is newer than libbp5.so: rebuild"
    return open(ISA).read()


def shape(p):
    """OverintShape<p> (csrc/bp5_kernels.hpp): (TW, LPC, TPB, PF)"""
    one_wave = p <= 3 or p == 6
    return (1 if one_wave else 4, (p + 2) ** 2, 4 if one_wave else 1, 1 if p <= 4 else 0)


def kernels(p):
    """mangled-name keys of the four kernels of degree p"""
    tw, lpc, tpb, pf = shape(p)
    return {"apply_pencil_q_kernel": f"apply_pencil_q_kernelILi{p}ELi{tw}ELi{lpc}ELi{tpb}ELb{pf}EE",
            "apply_pencil_mass_q_kernel": f"apply_pencil_mass_q_kernelILi{p}ELi{tw}ELi{lpc}ELi{tpb}EE",
            "overint_metric_kernel": f"overint_metric_kernelILi{p + 1}EE",
            "overint_diagonal_kernel": f"overint_diagonal_kernelILi{p + 1}EE"}


def _metadata(text, key):
    """(static LDS bytes, scratch bytes, SGPRs, spilled SGPRs, VGPRs, spilled VGPRs) from the amdhsa.kernels entry of the kernel"""
    m = re.search(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n){1,9}?\s+\.name:\s+_ZN3bp5\d+" + re.escape(key) + r"\w*\n\s+\.private_segment_fixed_size:\s+(\d+)\n"
                  r"\s+\.sgpr_count:\s+(\d+)\n\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n){1,4}?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert m, key
    return tuple(int(g) for g in m.groups())


def test_every_degree_has_its_kernels_and_low_degrees_do_not_spill():
    text = _text()
    out = {}
    for p in range(1, 9):
        for name, key in kernels(p).items():
            out[(name, p)] = _metadata(text, key)
    assert len(out) == 32
    for (name, p), (lds, scratch, sgpr, sspill, vgpr, vspill) in sorted(out.items()):
        print(f"{name} p={p}: {vgpr} VGPRs ({vspill} spilled), {sgpr} SGPRs ({sspill} spilled to VGPR lanes), static LDS {lds} B, scratch {scratch} B")
    for (name, p), (lds, scratch, sgpr, sspill, vgpr, vspill) in out.items():
        if p <= 4:
            assert scratch == 0 and vspill == 0 and sspill == 0, (name, p, scratch, vspill, sspill)
        assert scratch == 0 and vspill == 0, (name, p, scratch, vspill)      # measured at the time of writing: no kernel of any degree touches scratch


def test_one_kernel_per_degree_and_class():
    text = _text()
    for name in ("apply_pencil_q_kernel", "apply_pencil_mass_q_kernel", "overint_metric_kernel", "overint_diagonal_kernel"):
        names = set(re.findall(r"\.name:\s+(_ZN3bp5\d+" + name + r"I\w+)\n", text))
        assert len({n for n in names if not n.endswith(".kd")}) == 8, (name, sorted(names))
    # the permutation to the reference layout is metric_permute_kernel taken at Q = 3 .. 10
    names = set(re.findall(r"\.name:\s+(_ZN3bp5\d+metric_permute_kernelILi\d+EdEE\w*)\n", text))
    assert len(names) == 8, sorted(names)


def test_no_barrier_is_reached_with_an_lds_write_in_flight():
    import check_lds_barrier
    _text()
    assert check_lds_barrier.main(ISA) == 0


def test_cells_that_span_waves_use_the_workgroup_barrier_and_one_wave_teams_do_not():
    text = _text()
    for p in range(1, 9):
        tw = shape(p)[0]
        for name in ("apply_pencil_q_kernel", "apply_pencil_mass_q_kernel"):
            key = kernels(p)[name]
            m = re.search(r"^(_ZN3bp5\d+" + re.escape(key) + r"\w*):[^\n]*\n(.*?)\n\s+s_endpgm", text, re.S | re.M)
            assert m, key
            assert ("s_barrier" in m.group(2)) == (tw > 1), (name, p)
