"""The level-of-detail entries of the one-pass render (f2n_render_rays_lod, f2n_render_rays_head_lod,
f2n_render_rays_tail_lod) without a GPU: they parse from the header with a comment of their own, are
exported, take the arguments of the entries without the suffix with one more int L_active after L, and
answer an L_active outside [1, L] with F2N_E_INVALID_ARG before any HIP work -- after every check of
the entry without it.  (Registers, spills and the set of instantiations of the kernels behind them:
tests/test_render_rays_cpu.py and tests/test_render_rays_head_cpu.py, which compile the same files.)"""
import ctypes

import pytest

OK, INVALID, UNSUPPORTED = 0, -1, -3
PLAIN = {"f2n_render_rays_lod": "f2n_render_rays", "f2n_render_rays_head_lod": "f2n_render_rays_head",
         "f2n_render_rays_tail_lod": "f2n_render_rays_tail"}
PTR = 1 << 20       # fake, aligned, non-null: never dereferenced, validation answers first


def _call(c, entry, n_rays=4, S=128, L=16, L_active=16, F=2, T=1 << 19, stride=None, null=(),
          n_head=64, state=PTR):
    names = ["rays_o", "rays_d", "noise", "table", "primes", "bias", "mul", "w_h", "b_h", "w1", "b1",
             "w2", "b2"]
    a = [None if n in null or n == "noise" else PTR for n in names]
    a += [None, None, None, 0]
    a += [None if n in null else PTR for n in ("bg", "colors", "depths", "last_trans", "kept")]
    a += [None, n_rays, S, ctypes.c_float(1.0 / 64), L, L_active, F, T,
          T * F if stride is None else stride, ctypes.c_float(1e-4), ctypes.c_float(3.0),
          ctypes.c_float(1e-2)]
    if entry != "f2n_render_rays_lod":
        a += [n_head, state]
    return getattr(c, entry)(*a, None)


def test_entries_parse_export_and_carry_a_comment(capi):
    decls = capi.parse_header()
    cdll = ctypes.CDLL(capi.LIB_PATH)
    text = open(capi.HEADER).read()
    for lod, plain in PLAIN.items():
        assert lod in decls and hasattr(cdll, lod), lod
        names, base = [n for _, n in decls[lod][1]], [n for _, n in decls[plain][1]]
        i = base.index("L")
        assert names == base[:i + 1] + ["L_active"] + base[i + 1:], lod
        assert [t for t, _ in decls[lod][1]][i + 1] is ctypes.c_int
        pos = text.index("int %s(" % lod)
        start = text.rindex("/*", 0, pos)
        assert text[text.index("*/", start) + 2:pos].strip() == "", lod   # the comment is this entry's own
        block = text[start:pos]
        assert "L_active" in block and "src/renderer.cpp:33-123" in block, lod
    pos = text.index("int f2n_render_rays_lod(")
    assert "No counterpart in the reference" in text[text.rindex("/*", 0, pos):pos]
    assert capi.lib().cdll.f2n_abi_version() == 2


@pytest.mark.parametrize("entry", sorted(PLAIN))
def test_l_active_is_answered_before_any_hip_work(capi, entry):
    c = capi.lib().cdll
    call = lambda **kw: _call(c, entry, **kw)
    for L, F in ((16, 2), (8, 2), (8, 1), (16, 4), (32, 1)):
        for bad in (0, L + 1, -1, 1 << 20):
            assert call(L=L, F=F, L_active=bad) == INVALID, (L, F, bad)
            assert call(n_rays=0, L=L, F=F, L_active=bad) == INVALID, (L, F, bad)
        for good in (1, L // 2, L - 1, L):
            assert call(n_rays=0, L=L, F=F, L_active=good) == OK, (L, F, good)   # the empty call
    # the checks of the entry without it come first, with their own statuses
    assert call(L=16, F=3, L_active=0) == UNSUPPORTED
    assert call(L=12, F=2, L_active=13) == UNSUPPORTED
    assert call(L=33, F=2, L_active=0) == UNSUPPORTED
    assert call(n_rays=-1, L_active=0) == INVALID
    assert call(null=("table",), L_active=3) == INVALID
    assert call(S=0, L_active=3) == INVALID
    if entry != "f2n_render_rays_lod":
        assert call(n_head=100, L_active=3) == INVALID
        assert call(state=None, L_active=3) == INVALID
