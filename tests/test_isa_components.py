"""Static checks of the gfx950 ISA of the block-vector operator kernel (apply_pencil_components_kernel, bp5_apply_components; no GPU needed):
one build per degree and quadrature in the degree's default pencil shape, and the p <= 4 builds use no scratch and spill nothing.  Reads the
register / scratch / spill metadata only; the barrier pattern of these kernels is covered by tests/test_isa_checks.py, which walks every kernel
of the same files.  Same files and the same regular expression as tests/test_isa_checks.py."""
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
            key = f"apply_pencil_components_kernelILi{p}ELb{coll}ELi{tw}ELi{lpc}ELi{tpb}EE"
            m = re.search(r"\.name:\s+_ZN3bp5\d+" + re.escape(key) + r"\w*\n\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n){1,8}?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
            assert m, key
            out[(p, coll)] = tuple(int(g) for g in m.groups())      # (scratch bytes, VGPRs, spilled VGPRs)
    return out


def test_every_degree_and_quadrature_has_its_kernel_and_low_degrees_do_not_spill():
    builds = _builds()
    assert len(builds) == 16
    for (p, coll), (scratch, vgpr, spill) in sorted(builds.items()):
        print(f"apply_pencil_components_kernel p={p} {'GLL' if coll else 'Gauss'}: {vgpr} VGPRs, scratch {scratch} B, {spill} spilled")
    for (p, coll), (scratch, vgpr, spill) in builds.items():
        if p <= 4:
            assert scratch == 0 and spill == 0, (p, coll, scratch, vgpr, spill)


def test_one_kernel_per_degree_and_quadrature():
    """the trip count over the components is a run-time argument: sixteen kernels, not sixteen per n_components"""
    text = "".join(open(f).read() for f in _isa())
    names = set(re.findall(r"\.name:\s+(_ZN3bp5\d+apply_pencil_components_kernel\w+)\n", text))
    assert len({n for n in names if not n.endswith(".kd")}) == 16, sorted(names)
