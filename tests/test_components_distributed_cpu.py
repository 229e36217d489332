"""CPU checks of block vectors on more than one rank (bp5_halo_*_components, bp5_apply_components_distributed,
bp5_cg_solve_components_distributed): the entry points exist, have prototypes, and refuse every bad argument that can be stated without a
handle before anything touches a device -- with the words of the one-rank entry points (tests/test_components_cpu.py)."""
import ctypes as C

import numpy as np

import bp5_pkg

pkg = bp5_pkg.load()
INVALID = 1
HALO = ("bp5_halo_gather_components", "bp5_halo_scatter_add_components", "bp5_halo_zero_ghosts_components")
SYMBOLS = HALO + ("bp5_apply_components_distributed", "bp5_cg_solve_components_distributed")


def test_symbols_are_exported_and_listed():
    L = pkg.lib()
    for s in SYMBOLS:
        assert s in pkg.HEADER_SYMBOLS and hasattr(L, s) and s in L._protos, s
    # the one-rank entry points are still there, next to their twins
    for s in ("bp5_apply_components", "bp5_cg_solve_components"):
        assert s in pkg.HEADER_SYMBOLS and s in L._protos


def _buffers():
    """two 16-byte aligned host buffers: the refusals under test are decided before any pointer is dereferenced"""
    a = np.zeros(64 + 2)
    off = (-a.ctypes.data // 8) % 2
    return a.ctypes.data + 8 * off, a.ctypes.data + 8 * off + 8 * 32, a


def _vp(p):
    return C.c_void_p(p) if p else None


def test_operator_and_solver_refuse_invalid_arguments_without_a_device():
    """null, n_components 0 / 9 / -1, odd ld, misaligned, src == dst, null handle on both entries; null params / result, unknown variant and
    max_iter < 0 on the solver.  The layout checks come before the handle is looked at, so a NULL handle does not mask them."""
    L = pkg.lib()
    from deal_and_ceed_on_gpu_amd import _lib
    src, dst, keep = _buffers()
    null = C.c_void_p()
    prm, res = _lib.CGParams(_lib.CG_PLAIN, 10, 0.0, 0, 0), _lib.CGResult()

    def apply(nc=3, ld=8, s=src, d=dst):
        st = L.bp5_apply_components_distributed(null, C.c_void_p(src), nc, ld, _vp(s), _vp(d), 1)
        return st, L.bp5_last_error().decode()

    def solve(nc=3, ld=8, s=src, d=dst, p=prm, r=res):
        st = L.bp5_cg_solve_components_distributed(null, C.c_void_p(src), nc, ld, None, _vp(s), _vp(d), C.byref(p) if p is not None else None,
                                                   C.byref(r) if r is not None else None)
        return st, L.bp5_last_error().decode()

    for fn in (apply, solve):
        for kw, word in ((dict(nc=0), "n_components"), (dict(nc=9), "n_components"), (dict(nc=-1), "n_components"), (dict(ld=7), "even"),
                         (dict(s=src + 8), "aligned"), (dict(d=dst + 8), "aligned"), (dict(d=src), "overlap"), (dict(s=None), "null"),
                         (dict(d=None), "null"), (dict(), "null handle")):
            st, msg = fn(**kw)
            assert st == INVALID and word in msg, (fn.__name__, kw, st, msg)
    assert solve(p=None)[0] == INVALID and solve(r=None)[0] == INVALID
    st, msg = solve(p=_lib.CGParams(7, 10, 0.0, 0, 0))
    assert st == INVALID and "variant" in msg, msg
    st, msg = solve(p=_lib.CGParams(_lib.CG_PLAIN, -1, 0.0, 0, 0))
    assert st == INVALID and "max_iter" in msg, msg
    # a misaligned inverse diagonal, as on one rank
    st = L.bp5_cg_solve_components_distributed(null, C.c_void_p(src), 3, 8, C.c_void_p(src + 8), C.c_void_p(src), C.c_void_p(dst), C.byref(prm), C.byref(res))
    assert st == INVALID and "aligned" in L.bp5_last_error().decode()
    del keep


def test_halo_entries_refuse_invalid_arguments_without_a_device():
    """the three exchanges take ONE block vector: null, n_components 0 / 9 / -1, odd ld, misaligned, null handle"""
    L = pkg.lib()
    v, _, keep = _buffers()
    null = C.c_void_p()
    for name in HALO:
        fn = getattr(L, name)
        for kw, word in ((dict(nc=0), "n_components"), (dict(nc=9), "n_components"), (dict(nc=-1), "n_components"), (dict(ld=7), "even"),
                         (dict(p=v + 8), "aligned"), (dict(p=None), "null"), (dict(), "null handle")):
            a = dict(nc=3, ld=8, p=v)
            a.update(kw)
            st = fn(null, a["nc"], a["ld"], _vp(a["p"]))
            msg = L.bp5_last_error().decode()
            assert st == INVALID and word in msg, (name, kw, st, msg)
    del keep


def test_mirror_has_the_block_vector_exchanges():
    """MatrixFree carries the three exchanges of a block vector (the dispatch of vmult / solve on A.distributed is what
    tests/test_gpu_components_multirank.py runs)"""
    from deal_and_ceed_on_gpu_amd import matrix_free as M
    for name in ("update_ghost_values_block", "compress_add_block", "zero_out_ghosts_block"):
        assert callable(getattr(M.MatrixFree, name))
