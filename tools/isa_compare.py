#!/usr/bin/env python3
"""Compare the gfx950 ISA of two builds of csrc/ kernel by kernel (the *-gfx950.s files that `make` keeps beside each unit):

    tools/isa_compare.py OLD_CSRC NEW_CSRC

Per kernel one verdict:
  identical        the same instructions in the same order, once the compiler's label numbers are normalised
  float-identical  the multiset of floating-point opcodes (mnemonic contains f64 or f32) is equal; only other instructions differ
  differs          anything else
Exit status 1 on any `differs` and on a kernel (or a whole unit) that only one side has.  What a refactor of the setup kernels
has to show: the arithmetic is the same even where address computation was scheduled differently."""
import collections
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_lds_barrier import functions  # noqa: E402

SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"


def instructions(body):
    """The kernel's instructions and labels, without comments and directives; .LBB<function>_<block> loses the function's
    number (its place in the unit) and the blocks are renumbered in order of appearance."""
    out, blocks = [], {}

    def block(m):
        return ".LBB_%d" % blocks.setdefault(m.group(0), len(blocks))

    lines = [ln.split(";")[0].strip() for ln in body]
    lines = [ln for ln in lines if ln and not (ln.startswith(".") and not ln.startswith(".LBB"))]
    for ln in lines:  # number the blocks where they are defined, so that a reference ahead of its label gets the same number
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            blocks.setdefault(m.group(1), len(blocks))
    for ln in lines:
        out.append(re.sub(r"\.LBB\d+_\d+", block, ln))
    return out


def float_opcodes(ins):
    ops = (ln.split()[0] for ln in ins if not ln.startswith(".LBB"))
    return collections.Counter(op for op in ops if "f64" in op or "f32" in op)


def verdict(old_body, new_body):
    old, new = instructions(old_body), instructions(new_body)
    if old == new:
        return "identical"
    if float_opcodes(old) == float_opcodes(new):
        return "float-identical"
    return "differs"


def units(csrc):
    files = glob.glob(os.path.join(csrc, "**", "*" + SUFFIX), recursive=True)
    return {os.path.relpath(f, csrc)[: -len(SUFFIX)]: f for f in files}


def compare(old_csrc, new_csrc, out=sys.stdout):
    """Prints `unit kernel verdict` lines and a count per verdict; returns the number of kernels that differ or are missing on a side."""
    old_units, new_units = units(old_csrc), units(new_csrc)
    count = collections.Counter()
    for unit in sorted(set(old_units) | set(new_units)):
        old = dict(functions(old_units[unit])) if unit in old_units else {}
        new = dict(functions(new_units[unit])) if unit in new_units else {}
        for name in sorted(set(old) | set(new)):
            v = "missing in OLD" if name not in old else "missing in NEW" if name not in new else verdict(old[name], new[name])
            count[v] += 1
            print(unit, name, v, file=out)
    print("# " + ", ".join(f"{k}: {count[k]}" for k in sorted(count)), file=out)
    return sum(c for v, c in count.items() if v not in ("identical", "float-identical"))


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(1 if compare(sys.argv[1], sys.argv[2]) or not units(sys.argv[1]) else 0)
