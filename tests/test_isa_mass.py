"""Static checks of the gfx950 ISA of the mass-operator kernels (BP5_OP_MASS; no GPU needed): one apply_pencil_mass_kernel per degree and quadrature
in the degree's default pencil shape and the BLK_MASS builds of the block kernel, plain and fused, per degree and quadrature; no scratch and no
spill for p <= 4, and the collocated pencil builds use no LDS at all.  Reads the register /
scratch / spill / LDS metadata only; the barrier pattern of these kernels is covered by tests/test_isa_checks.py, which walks every kernel of the
same files.  Same files and the same regular expression as tests/test_isa_checks.py."""
import re

from test_isa_checks import _isa


def _shape(p):
    """the default pencil shape of apply_degree_impl's variant 0: (TW, LPC, TPB)"""
    return (1 if p <= 3 else 4, (p + 1) ** 2, 4 if p <= 3 else 1)


def _builds():
    text = "".join(open(f).read() for f in _isa())
    out = {}
    for p in range(1, 9):
        tw, lpc, tpb = _shape(p)
        for coll in (0, 1):
            key = f"apply_pencil_mass_kernelILi{p}ELb{coll}ELi{tw}ELi{lpc}ELi{tpb}EE"
            m = re.search(r"\.name:\s+_ZN3bp5\d+" + re.escape(key) + r"\w*\n\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n){1,8}?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
            assert m, key
            out[(p, coll)] = tuple(int(g) for g in m.groups())      # (scratch bytes, VGPRs, spilled VGPRs)
    return out


def test_every_degree_and_quadrature_has_its_kernel_and_low_degrees_do_not_spill():
    builds = _builds()
    assert len(builds) == 16
    for (p, coll), (scratch, vgpr, spill) in sorted(builds.items()):
        print(f"apply_pencil_mass_kernel p={p} {'GLL' if coll else 'Gauss'}: {vgpr} VGPRs, scratch {scratch} B, {spill} spilled")
    for (p, coll), (scratch, vgpr, spill) in builds.items():
        if p <= 4:
            assert scratch == 0 and spill == 0, (p, coll, scratch, vgpr, spill)


BLOCK_LPC = {1: 4, 2: 9, 3: 16, 4: 32, 5: 36, 6: 64, 7: 64, 8: 81}
BLOCK_MASKS = {"plain": 2048 + 8192 + 16384 + 262144 + 1073741824, "fused": 2048 + 8192 + 16384 + 262144 + 1048576 + 1073741824}   # BLK_DEFAULT | BLK_MASS [| BLK_FUSE]


def test_block_builds_per_degree_and_quadrature_and_low_degrees_do_not_spill():
    """the overwrite launch (owner stores, SCATTER = 1) of every BLK_MASS build: 32 kernels"""
    text = "".join(open(f).read() for f in _isa())
    out = {}
    for p in range(1, 9):
        for coll in (0, 1):
            for kind, mask in BLOCK_MASKS.items():
                key = f"apply_block_kernelILi{p}ELb{coll}ELi{BLOCK_LPC[p]}ELi1ELi{mask}E"
                m = re.search(r"\.name:\s+_ZN3bp5\d+" + re.escape(key) + r"\w*\n\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n){1,8}?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
                assert m, key
                out[(p, coll, kind)] = tuple(int(g) for g in m.groups())
    assert len(out) == 32
    for (p, coll, kind), (scratch, vgpr, spill) in sorted(out.items()):
        print(f"apply_block_kernel BLK_MASS {kind} p={p} {'GLL' if coll else 'Gauss'}: {vgpr} VGPRs, scratch {scratch} B, {spill} spilled")
    for (p, coll, kind), (scratch, vgpr, spill) in out.items():
        if p <= 4:
            assert scratch == 0 and spill == 0, (p, coll, kind, scratch, vgpr, spill)


def test_one_kernel_per_degree_and_quadrature():
    text = "".join(open(f).read() for f in _isa())
    names = set(re.findall(r"\.name:\s+(_ZN3bp5\d+apply_pencil_mass_kernel\w+)\n", text))
    assert len({n for n in names if not n.endswith(".kd")}) == 16, sorted(names)


def test_collocated_builds_touch_no_lds_and_no_barrier():
    """GLL collocation: the operator is pointwise; the plane is read in the gather orientation, so there is no tile and no barrier"""
    text = "".join(open(f).read() for f in _isa())
    for p in range(1, 9):
        tw, lpc, tpb = _shape(p)
        name = rf"_ZN3bp5\d+apply_pencil_mass_kernelILi{p}ELb1ELi{tw}ELi{lpc}ELi{tpb}EE\w*"
        m = re.search(r"^(" + name + r"):[^\n]*\n(.*?)\n\s+s_endpgm", text, re.S | re.M)
        assert m, (p, name)
        body = m.group(2)
        assert "s_barrier" not in body and not re.search(r"\bds_(read|write|load|store)", body), p
