#!/usr/bin/env python3
"""Dump what the Chebyshev step and multigrid transfer kernels compute, for a byte-for-byte comparison of two builds of the library
(profiles/transfer_unify/README.md, section 2):

    BP5_LIB=<parent build>/libbp5.so python tools/transfer_bits.py --out A
    python tools/transfer_bits.py --out B
    python tools/transfer_bits.py --compare A B [--control A2]     # exit status 1 unless every compared array is byte-equal

Scalar prolongate_and_add / restrict_and_add at p = 2 .. 8 and geometric p = 1 .. 4, the block entries with 1 and 3 components on the same
transfers, PreconditionChebyshev vmult / step at degree 4 and 5 with given bounds (Poisson p = 2, 4; elasticity p = 2), one scalar V-cycle on
a brick-ordered mesh with the block kernel (owner stores: bitwise reproducible) and one elasticity V-cycle.  Everything that contains an
operator application is computed twice; where the two runs of ONE build differ (atomic scatter) the array is saved as *.not_compared.npy
and listed, not counted.  --control A2: a second dump of A's build from another process; what differs between A and A2 (a V-cycle whose
level diagonals and bounds were summed atomically at setup) is listed as not compared too."""
import argparse
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
AMP = 0.04


def compare(a, b, control=None):
    names = sorted({os.path.basename(f) for d in (a, b) for f in glob.glob(os.path.join(d, "*.npy"))})
    bad = skipped = 0
    for n in names:
        fa, fb = os.path.join(a, n), os.path.join(b, n)
        if n.endswith(".not_compared.npy") or not (os.path.exists(fa) and os.path.exists(fb)):
            skipped += 1
            print(f"{n}: not compared" + ("" if n.endswith(".not_compared.npy") else " (ONE SIDE ONLY)"))
            bad += not n.endswith(".not_compared.npy")
            continue
        if control and open(fa, "rb").read() != open(os.path.join(control, n), "rb").read():
            skipped += 1
            print(f"{n}: not compared (two processes of one build differ, max |a - a2| = %.3e)" % np.abs(np.load(fa) - np.load(os.path.join(control, n))).max())
            continue
        same = open(fa, "rb").read() == open(fb, "rb").read()
        bad += not same
        print(f"{n}: {'byte-equal' if same else 'DIFFERS, max |a - b| = %.3e' % np.abs(np.load(fa) - np.load(fb)).max()}")
    print(f"# {len(names) - skipped} arrays compared, {len(names) - skipped - bad} byte-equal, {skipped} not compared")
    return 1 if bad or not names else 0


def dump(out):
    import torch
    import bp5_pkg
    pkg = bp5_pkg.load()
    os.makedirs(out, exist_ok=True)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0")

    def save(name, fn, twice=False):
        a = fn().cpu().numpy()
        ok = not twice or np.array_equal(a, fn().cpu().numpy(), equal_nan=True)
        np.save(os.path.join(out, name + ("" if ok else ".not_compared") + ".npy"), a)

    def blockvec(v, n):                                     # (rows, ld) with ld = n rounded up to even, padding 0
        t = torch.zeros((v.shape[0], n + (n & 1)), dtype=torch.float64, device="cuda:0")
        t[:, :n] = dev(v)
        return t

    def applied(fn, dst, src):
        fn(dst, src)
        return dst

    cases = [("p", p, (3, 2, 2) if p <= 4 else (2, 2, 2)) for p in range(2, 9)] + [("h", p, (4, 4, 4) if p <= 2 else (2, 2, 2)) for p in range(1, 5)]
    for kind, p, cells in cases:
        mesh = pkg.BrickMesh(p, cells, deform_amp=AMP)
        fine = pkg.PoissonOperator(mesh, pkg.QUAD_GAUSS)
        cmesh = mesh.coarsen(1) if kind == "h" else pkg.BrickMesh(max(1, p // 2), cells, deform_amp=AMP)
        coarse = pkg.PoissonOperator(cmesh, pkg.QUAD_GAUSS)
        tr = pkg.MGTwoLevelTransfer(fine, coarse, geometric=kind == "h")
        nf, nc = fine.mf_data.n_local, coarse.mf_data.n_local
        rng = np.random.default_rng(10 * p + (kind == "h"))
        xf, xc = rng.uniform(-1, 1, (3, nf)), rng.uniform(-1, 1, (3, nc))
        tag = f"{kind}{p}"
        save(f"{tag}_prolongate_scalar", lambda: applied(tr.prolongate_and_add, dev(xf[0]), dev(xc[0])))
        save(f"{tag}_restrict_scalar", lambda: applied(tr.restrict_and_add, dev(xc[0]), dev(xf[0])))
        for k in (1, 3):
            save(f"{tag}_prolongate_components{k}", lambda: applied(tr.prolongate_and_add_components, blockvec(xf[:k], nf), blockvec(xc[:k], nc)))
            save(f"{tag}_restrict_components{k}", lambda: applied(tr.restrict_and_add_components, blockvec(xc[:k], nc), blockvec(xf[:k], nf)))
        tr.clear()

    def chebyshev(tag, op, make, vec):
        n = op.mf_data.n_local
        rng = np.random.default_rng(7)
        src, x0 = vec(rng.uniform(-1, 1, (3, n))), rng.uniform(-1, 1, (3, n))
        for degree in (4, 5):
            ch = make(degree)
            save(f"{tag}_vmult_degree{degree}", lambda: applied(ch.vmult, vec(np.full((3, n), 7.0)), src), twice=True)
            save(f"{tag}_step_degree{degree}", lambda: applied(ch.step, vec(x0), src), twice=True)
            ch.clear()

    for p in (2, 4):
        op = pkg.PoissonOperator(pkg.BrickMesh(p, (3, 2, 2), deform_amp=AMP), pkg.QUAD_GAUSS, pkg.COEF_STEP64)
        inv = pkg.DiagonalMatrix(op.compute_diagonal(invert=True))
        Ch = pkg.PreconditionChebyshev
        chebyshev(f"chebyshev_poisson_p{p}", op, lambda d: Ch().initialize(op, Ch.AdditionalData(degree=d, max_eigenvalue=2.1, min_eigenvalue=0.15, preconditioner=inv)),
                  lambda v: dev(v[0]))
    el = pkg.ElasticityOperator(pkg.BrickMesh(2, (3, 2, 2), deform_amp=AMP), pkg.QUAD_GAUSS, pkg.COEF_STEP64, lam=1.0, mu=1.0)
    n, ECh, inv = el.mf_data.n_local, pkg.ElasticityPreconditionChebyshev, pkg.DiagonalMatrix(el.compute_diagonal(invert=True))
    chebyshev("chebyshev_elasticity_p2", el, lambda d: ECh().initialize(el, ECh.AdditionalData(degree=d, max_eigenvalue=2.1, min_eigenvalue=0.15, preconditioner=inv)),
              lambda v: blockvec(v, n))

    fine = pkg.PoissonOperator(pkg.BrickMesh(4, (5, 4, 6), deform_amp=AMP, cell_block=(4, 4, 4), dof_numbering=1, cell_block_order=1), pkg.QUAD_GAUSS, pkg.COEF_STEP64)
    ops = pkg.make_mg_hierarchy(fine)
    for o in ops:
        o.mf_data.set_apply_variant(56)
    # the step kernel on the reproducible operator, with a diagonal that no kernel computed (compute_diagonal adds atomically)
    n = fine.mf_data.n_local
    inv = pkg.DiagonalMatrix(dev(np.random.default_rng(6).uniform(0.5, 1.5, n) * 1e-2))
    chebyshev("chebyshev_poisson_p4_block_kernel", fine, lambda d: Ch().initialize(fine, Ch.AdditionalData(degree=d, max_eigenvalue=2.1, min_eigenvalue=0.15, preconditioner=inv)),
              lambda v: dev(v[0]))
    mg = pkg.PreconditionMG(ops)
    np.save(os.path.join(out, "vcycle_poisson_p4_level_bounds.npy"), np.array([[d[k] for k in ("min_used", "max_used")] for d in mg.level_info()]))
    src = dev(np.random.default_rng(8).uniform(-1, 1, n))
    save("vcycle_poisson_p4_block_kernel", lambda: applied(mg.vmult, dev(np.zeros(n)), src), twice=True)
    mg.clear()
    ops = pkg.make_elasticity_mg_hierarchy(pkg.ElasticityOperator(pkg.BrickMesh(4, (3, 2, 2), deform_amp=AMP), pkg.QUAD_GAUSS, pkg.COEF_STEP64, lam=1.0, mu=1.0))
    n = ops[0].mf_data.n_local
    mg = pkg.ElasticityPreconditionMG(ops, ld=n + (n & 1))
    src = blockvec(np.random.default_rng(9).uniform(-1, 1, (3, n)), n)
    save("vcycle_elasticity_p4", lambda: applied(mg.vmult, blockvec(np.zeros((3, n)), n), src), twice=True)
    mg.clear()
    print(f"{len(glob.glob(os.path.join(out, '*.npy')))} arrays in {out}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--control", metavar="A2")
    args = ap.parse_args()
    sys.exit(compare(*args.compare, control=args.control) if args.compare else dump(args.out or "bench_out/transfer_bits"))
