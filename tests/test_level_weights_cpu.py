"""f2n_level_weights and the coarse-to-fine schedule without a GPU: the weights against the float64
restatement of tests/level_weights_model.py within one f32 ulp, exact zeros and ones outside the ramp,
monotone in alpha, l_active = min(L, ceil(alpha)); every documented bad argument answered with its
status; f2n::CoarseToFine::alpha_at at start, end and outside them.  Host arithmetic only."""
import ctypes
import math

import numpy as np
import pytest

from tests import level_weights_model as lm

OK, INVALID = 0, -1
LEVELS = (1, 4, 16, 32)


def _call(capi, alpha, L):
    w = (ctypes.c_float * max(L, 1))(*([-7.0] * max(L, 1)))
    la = ctypes.c_int(-7)
    st = capi.lib().cdll.f2n_level_weights(float(alpha), L, w, ctypes.byref(la))
    return st, np.array(w[:max(L, 0)], dtype=np.float32), la.value


def _sweep(L):
    """every integer and quarter, values just inside the ramp's ends, and past L"""
    a = [1.0 + 0.25 * k for k in range(4 * (L - 1) + 1)]
    a += [l + e for l in range(1, L) for e in (1e-3, 0.5 - 1e-3, 1.0 - 1e-3, 1.0 / 3.0)]
    a += [L + 0.5, L + 100.0]
    return sorted(a)


def test_entry_parses_exports_and_says_it_has_no_counterpart(capi):
    decls = capi.parse_header()
    assert "f2n_level_weights" in decls
    assert [n for _, n in decls["f2n_level_weights"][1]] == ["alpha", "L", "w_host", "l_active"]
    assert decls["f2n_level_weights"][1][0][0] is ctypes.c_double
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "f2n_level_weights")
    text = open(capi.HEADER).read()
    pos = text.index("int f2n_level_weights(")
    block = text[text.rindex("/*", 0, pos):pos]
    assert "No counterpart in the reference" in block and "no HIP work" in block
    assert capi.lib().cdll.f2n_abi_version() == 2


@pytest.mark.parametrize("L", LEVELS)
def test_weights_match_the_model(capi, L):
    prev = np.zeros(L, dtype=np.float32)
    for alpha in _sweep(L):
        st, w, la = _call(capi, alpha, L)
        assert st == OK, alpha
        ref = lm.weights(alpha, L)
        err = np.abs(w.astype(np.float64) - ref)
        assert (err <= lm.ulp32(ref)).all(), (alpha, w, ref)
        d = min(alpha, L) - np.arange(L)
        assert (w[d <= 0] == 0.0).all() and (w[d >= 1] == 1.0).all(), (alpha, w)
        inside = (d > 0) & (d < 1)
        assert ((w[inside] > 0.0) & (w[inside] < 1.0)).all(), (alpha, w)
        assert (w >= prev).all(), (alpha, w, prev)          # monotone in alpha, level by level
        prev = w
        assert la == lm.active_levels(ref) == lm.ceil_alpha(alpha, L), (alpha, la)
        assert la >= 1
    # alpha > L is alpha = L: all ones
    assert (_call(capi, L + 3.0, L)[1] == 1.0).all()


def test_bad_arguments(capi):
    for L in (0, -1, 33, 1 << 20):
        assert _call(capi, 1.0, L)[0] == INVALID, L
    for alpha in (0.999, 0.0, -2.0, float("nan"), float("inf"), -float("inf")):
        st, w, la = _call(capi, alpha, 8)
        assert st == INVALID, alpha
        assert (w == -7.0).all() and la == -7               # nothing written
    c = capi.lib().cdll
    la = ctypes.c_int(0)
    w = (ctypes.c_float * 8)()
    assert c.f2n_level_weights(2.0, 8, None, ctypes.byref(la)) == INVALID
    assert c.f2n_level_weights(2.0, 8, w, None) == INVALID
    st, w1, la1 = _call(capi, 1.0, 1)
    assert st == OK and w1.tolist() == [1.0] and la1 == 1
    assert _call(capi, 32.0, 32)[2] == 32


def test_alpha_at(pkg):
    H = pkg.load_host()
    c2f = H.CoarseToFine(start=100.0, end=500.0, base=2.0)
    L = 16
    assert c2f.alpha_at(100.0, L) == 2.0 and c2f.alpha_at(500.0, L) == 16.0
    assert c2f.alpha_at(0.0, L) == 2.0 and c2f.alpha_at(-5.0, L) == 2.0
    assert c2f.alpha_at(501.0, L) == 16.0 and c2f.alpha_at(1e9, L) == 16.0
    for it in (150.0, 300.0, 499.0):
        want = lm.alpha_at(it, L, 100.0, 500.0, 2.0)
        assert math.isclose(c2f.alpha_at(it, L), want, rel_tol=1e-15), it
    assert (c2f.start, c2f.end, c2f.base) == (100.0, 500.0, 2.0)
    # the host's wrapper of the entry: a CPU tensor and l_active
    w, la = H.level_weights(2.5, 8)
    assert la == 3 and w.dtype.is_floating_point and tuple(w.shape) == (8,)
    assert np.array_equal(w.numpy(), lm.weights(2.5, 8).astype(np.float32))
    with pytest.raises(RuntimeError):
        H.level_weights(0.5, 8)


def test_field_keeps_weights_on_the_host_side(pkg):
    """Hash3DAnchored's bookkeeping on a CPU field: the host copy, active_levels, head_weight is the
    parameter itself without weights and the model's fold with them, clear goes back."""
    import torch

    H = pkg.load_host()
    f = H.Hash3DAnchored(n_levels=4, n_channels=2, log2_table=8, device="cpu")
    W = f.named_parameters()["mlp.weight"]
    assert f.level_weights() is None and f.active_levels() == 4 and f.skip_masked_levels
    assert f.head_weight().data_ptr() == W.data_ptr()
    lw = torch.tensor([1.0, 0.5, 0.0, 0.0])
    f.set_level_weights(lw)
    assert torch.equal(f.level_weights(), lw) and f.active_levels() == 2
    got = f.head_weight()
    assert got.requires_grad
    ref = lm.fold(W.detach().numpy(), lw.numpy(), 2)
    assert np.array_equal(got.detach().numpy().astype(np.float64), ref)     # products by 1, .5, 0: exact
    got.sum().backward()
    assert torch.equal(W.grad, torch.from_numpy(lm.cols(lw.numpy(), 2)).float().expand(16, 8))
    for bad in (torch.tensor([1.0, -0.1, 0, 0]), torch.tensor([1.0, float("nan"), 0, 0]),
                torch.zeros(4), torch.ones(3)):
        with pytest.raises(RuntimeError):
            f.set_level_weights(bad)
    assert f.active_levels() == 2                                           # a rejected call changes nothing
    f.clear_level_weights()
    assert f.level_weights() is None and f.active_levels() == 4
    assert f.head_weight().data_ptr() == W.data_ptr()
