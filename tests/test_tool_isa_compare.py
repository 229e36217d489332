"""tools/isa_compare.py on small synthetic ISA texts (no GPU, no build needed)."""
import io
import os
import sys

import bp5_pkg

sys.path.insert(0, os.path.join(bp5_pkg.ROOT, "tools"))

OLD = ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "v_lshlrev_b32_e32 v2, 3, v0", ".LBB7_1: ; %loop", "global_load_dwordx2 v[0:1], v2, s[0:1]",
       "s_waitcnt vmcnt(0)", "v_fma_f64 v[4:5], v[0:1], v[0:1], v[4:5]", "v_mul_f64 v[4:5], v[4:5], 2.0", "s_cbranch_scc0 .LBB7_1", "s_endpgm"]


def _unit(tmp_path, side, kernels):
    d = tmp_path / side / "sub"
    d.mkdir(parents=True)
    text = "".join(f"{name}:\n" + "".join(f"\t{ln}\n" for ln in body) for name, body in kernels.items())
    (d / "unit-hip-amdgcn-amd-amdhsa-gfx950.s").write_text(text)
    return str(tmp_path / side)


def test_verdicts():
    """Label numbers and comments do not count; a changed address instruction is float-identical; a changed, added or
    reordered-into-another-opcode floating-point instruction differs."""
    import isa_compare
    renumbered = [ln.replace(".LBB7_1", ".LBB12_3").replace("; %loop", "; %for.body") for ln in OLD]
    assert isa_compare.verdict(OLD, renumbered) == "identical"
    address = [ln.replace("v_lshlrev_b32_e32 v2, 3, v0", "v_mul_u32_u24_e32 v2, 8, v0") for ln in OLD]
    assert isa_compare.verdict(OLD, address + ["s_nop 0"]) == "float-identical"
    assert isa_compare.verdict(OLD, [ln.replace("v_mul_f64", "v_add_f64") for ln in OLD]) == "differs"
    assert isa_compare.verdict(OLD, OLD[:6] + OLD[5:]) == "differs"            # one more v_fma_f64
    assert isa_compare.verdict(OLD, [ln.replace("v_fma_f64", "v_fma_f32") for ln in OLD]) == "differs"
    branch_elsewhere = OLD[:2] + [".LBB7_0:"] + OLD[2:7] + ["s_cbranch_scc0 .LBB7_0", "s_endpgm"]
    assert isa_compare.verdict(OLD, branch_elsewhere) == "float-identical"     # (not identical: the branch target moved)


def test_compare_fails_on_a_difference_and_on_a_missing_kernel(tmp_path):
    import isa_compare
    old = _unit(tmp_path, "old", {"_Z1aPd": OLD, "_Z1bPd": OLD})
    same = _unit(tmp_path, "same", {"_Z1bPd": [ln.replace(".LBB7_", ".LBB0_") for ln in OLD], "_Z1aPd": OLD})
    out = io.StringIO()
    assert isa_compare.compare(old, same, out) == 0
    assert out.getvalue().splitlines() == ["sub/unit _Z1aPd identical", "sub/unit _Z1bPd identical", "# identical: 2"]
    differs = _unit(tmp_path, "differs", {"_Z1aPd": OLD, "_Z1bPd": [ln.replace("v_mul_f64", "v_add_f64") for ln in OLD]})
    assert isa_compare.compare(old, differs, io.StringIO()) == 1
    fewer = _unit(tmp_path, "fewer", {"_Z1aPd": OLD})
    out = io.StringIO()
    assert isa_compare.compare(old, fewer, out) == 1 and "_Z1bPd missing in NEW" in out.getvalue()
    assert isa_compare.compare(fewer, old, io.StringIO()) == 1
    assert isa_compare.compare(old, str(tmp_path / "nothing_here"), io.StringIO()) == 2
