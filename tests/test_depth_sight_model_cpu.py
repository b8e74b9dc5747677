"""The power of tests/test_gpu_depth_sight.py, checked without a GPU: the model of
tests/depth_sight_model.py agrees with a brute-force statement of the definition and with central
differences, its assertions accept the f32 restatement of the kernels' order and reject every
mutant, and the constant K is re-derived."""
import math

import numpy as np
import pytest

from tests import depth_sight_model as dm
from tests import ragged_cases as rc

CASES = [(name, variant, eps) for name in dm.LAYOUTS for variant in dm.T_VARIANTS
         for eps in dm.EPS_VALUES]


def _f32(out):
    return {k: np.asarray(v, dtype=np.float32) for k, v in out.items() if k in ("out", "dw")}


def test_inputs_are_what_the_docstring_says():
    for name, variant, eps in CASES:
        lay, case, ref = dm.shared(name, variant, eps)
        assert lay.n_rays == len(dm.LENGTHS) * len(dm.KINDS)
        assert sorted(set(lay.len.tolist())) == sorted(dm.LENGTHS)
        assert {(int(l), k) for l, k in zip(lay.len, lay.kind)} == {
            (l, k) for l in dm.LENGTHS for k in dm.KINDS}
        w, t, dt, z = (case[k].numpy() for k in ("weights", "t", "dt", "z"))
        assert w.dtype == t.dtype == dt.dtype == z.dtype == np.float32
        m32 = dm.midpoints32(t, dt)
        seen_straddle = 0
        for r in range(lay.n_rays):
            s, e = int(lay.start[r]), int(lay.end[r])
            kind = lay.kind[r]
            if kind in dm.INVALID_KINDS:
                assert not dm.ray_valid(z[r])
                continue
            assert dm.ray_valid(z[r])
            if e == s:
                continue
            for lo in range(s, e, rc.WAVE):                     # every stride carries weight
                assert w[lo:min(lo + rc.WAVE, e)].sum() > 1e-4
            assert 0.45 < w[s:e].sum() < 1.01
            front, band = dm.membership(m32[s:e], z[r], eps)
            if kind == "before":
                assert not front.any() and not band.any()
            elif kind == "beyond":
                assert front.all()
            elif kind == "inside":
                assert band[(e - s) // 2]
            elif kind == "edge":
                j = (e - s) // 3
                assert band[j] and m32[s + j] == np.float32(z[r] - np.float32(eps))
            else:
                assert band[min(rc.WAVE - 1, e - s - 1)]
                if eps > 0 and e - s > rc.WAVE and variant == "contiguous":
                    assert band[:rc.WAVE].any() and band[rc.WAVE:].any()   # both strides
                    seen_straddle += 1
        if eps > 0 and variant == "contiguous":
            assert seen_straddle == 3                           # the rays of 65, 129 and 200 samples
        if name == "gaps":
            assert lay.len[0] == 0 and lay.len[-1] == 0 and (~lay.inside).sum() > rc.WAVE


@pytest.mark.parametrize("name,variant,eps", CASES)
def test_model_is_the_brute_force_definition(name, variant, eps):
    lay, case, ref = dm.shared(name, variant, eps)
    w, t, dt, z, g = (case[k].numpy() for k in ("weights", "t", "dt", "z", "d_out"))
    for r in range(lay.n_rays):
        s, e = int(lay.start[r]), int(lay.end[r])
        out, dw = dm.brute_force(w[s:e], t[s:e], dt[s:e], z[r], case["eps"], g[r].astype(np.float64))
        assert np.allclose(ref["out"][r], out, rtol=1e-12, atol=1e-300), (r, lay.kind[r])
        assert np.allclose(ref["dw"][s:e], dw, rtol=1e-11, atol=1e-15), (r, lay.kind[r])
    assert (ref["dw"][~lay.inside] == dm.SENTINEL).all()
    # the corner values: invalid -> zeros; valid and empty -> (0, 1, z^2)
    for r in range(lay.n_rays):
        if lay.kind[r] in dm.INVALID_KINDS:
            assert (ref["out"][r] == 0).all()
        elif lay.len[r] == 0:
            assert tuple(ref["out"][r]) == (0.0, 1.0, float(z[r]) ** 2)


def test_model_gradient_is_the_central_difference():
    """out is a quadratic in the weights once the membership is fixed (it does not depend on them), so
    a central difference in float64 is exact up to rounding"""
    lay, case, ref = dm.shared("gaps", "thinned", dm.EPS_VALUES[1])
    w = case["weights"].numpy().astype(np.float64)
    g = case["d_out"].numpy().astype(np.float64)
    rng = np.random.RandomState(5)
    h = 2.0 ** -12                       # exactly representable next to an f32 weight in float64
    checked = 0
    for r in np.flatnonzero(lay.len > 0):
        if lay.kind[r] in dm.INVALID_KINDS:
            continue
        s, e = int(lay.start[r]), int(lay.end[r])
        for k in set(rng.randint(s, e, size=3).tolist()) | {s, e - 1}:
            vals = []
            for sign in (+1.0, -1.0):
                moved = dict(case)
                w2 = w.copy()
                w2[k] += sign * h
                moved["weights"] = _AsF64(w2)
                vals.append(float(dm.sight_ref(lay, moved)["out"][r] @ g[r]))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - ref["dw"][k]) <= 1e-9 * (1.0 + abs(ref["dw"][k])), (r, k, fd, ref["dw"][k])
            checked += 1
    assert checked > 100


class _AsF64:
    """a stand-in for a torch tensor holding float64 weights (rc._np64 calls detach().cpu().numpy())"""

    def __init__(self, a):
        self.a = a

    def detach(self):
        return self

    def cpu(self):
        return self

    def numpy(self):
        return self.a


@pytest.mark.parametrize("name,variant,eps", CASES)
def test_assertions_accept_the_f32_restatement(name, variant, eps):
    lay, case, ref = dm.shared(name, variant, eps)
    for strided in (False, True):
        got = _f32(dm.sight_f32(lay, case, strided))
        assert got["out"].dtype == np.float32
        rc.assert_no_failures(dm.sight_failures(lay, case, got, ref),
                              "%s %s eps=%g strided=%s" % (name, variant, eps, strided))
    # the assertions themselves: a write outside the ranges, a non-zero invalid ray, a negative zero
    got = _f32(dm.sight_f32(lay, case, True))
    gap = np.flatnonzero(~lay.inside)
    if gap.size:
        got["dw"][gap[0]] = 0.0
        assert any(f[3].startswith("written outside") for f in dm.sight_failures(lay, case, got, ref))
    inval = [r for r in range(lay.n_rays) if lay.kind[r] in dm.INVALID_KINDS]
    got["out"][inval[0], 1] = 1e-30
    got["out"][inval[1], 2] = -0.0
    fails = [f for f in dm.sight_failures(lay, case, got, ref) if f[3].startswith("invalid ray")]
    assert {f[0] for f in fails} == {inval[0], inval[1]}


def test_measured_K():
    """K_SIGHT = 4 x the largest (err / u - len M_sum) / M_op of the f32 restatement, rounded up to a
    power of two.  Prints the figures the module docstring quotes."""
    worst = {}
    for name, variant, eps in CASES:
        lay, case, ref = dm.shared(name, variant, eps)
        for strided in (False, True):
            for out, (ratio, _) in dm.ratios(lay, case, dm.sight_f32(lay, case, strided), ref).items():
                key = (name, out, strided)
                worst[key] = max(worst.get(key, -np.inf), float(ratio.max()))
    for key in sorted(worst):
        print("  %-5s %-3s strided=%-5s %.3f" % (key + (worst[key],)))
    top = max(worst.values())
    assert top > 0
    K = max(1.0, 2.0 ** math.ceil(math.log2(4.0 * top)))
    assert K == dm.K_SIGHT, (top, K)


@pytest.mark.parametrize("name,variant,eps", CASES)
def test_every_mutant_is_rejected(name, variant, eps):
    lay, case, ref = dm.shared(name, variant, eps)
    kinds = np.array(lay.kind)
    valid = ~np.isin(kinds, dm.INVALID_KINDS)
    long_rays = set(np.flatnonzero(valid & (lay.len > rc.WAVE)).tolist())
    partial = set(np.flatnonzero(valid & (lay.len % rc.WAVE != 0)).tolist())
    for mutant in dm.SIGHT_MUTANTS:
        fails = dm.sight_failures(lay, case, _f32(dm.sight_ref(lay, case, mutant=mutant)), ref)
        rays = {f[0] for f in fails}
        fwd = {f[0] for f in fails if f[1] == "out"}
        bwd = {f[0] for f in fails if f[1] == "dw"}
        if mutant == "sight_carry_d":      # every valid ray of more than one stride, both directions
            assert fwd == long_rays and bwd == long_rays, (mutant, sorted(fwd), sorted(bwd))
        elif mutant == "sight_carry_w":    # those whose band reaches into a stride that is not the last
            want = {r for r in long_rays if _band_before_last_stride(lay, case, r)}
            # (the backward shows it on the band's samples alone, scaled by d_out[r, 1]: a ray whose
            # g1 happens to be tiny may hide it there)
            assert want and fwd == want, (mutant, sorted(fwd), sorted(want))
            assert bwd <= want and len(bwd) >= len(want) - 1, (mutant, sorted(bwd), sorted(want))
        elif mutant == "sight_tail":       # every valid ray whose last stride is partial
            assert rays == partial and bwd == partial
            assert fwd == partial, sorted(partial - fwd)
        elif mutant == "sight_edge":       # the rays with a sample ON the band's lower edge
            on_edge = {r for r in np.flatnonzero(valid & (lay.len > 0)) if _sample_on_lo(lay, case, r)}
            assert on_edge and rays == on_edge and fwd == on_edge and bwd == on_edge
            assert {r for r in on_edge if kinds[r] == "edge"} == set(
                np.flatnonzero((kinds == "edge") & (lay.len > 0)).tolist())
        elif mutant == "sight_invalid":    # the backward alone, every invalid ray that has samples
            assert not fwd and bwd == set(np.flatnonzero(~valid & (lay.len > 0)).tolist())
        else:
            assert mutant == "sight_mid"   # every valid ray with a sample
            assert fwd == bwd == set(np.flatnonzero(valid & (lay.len > 0)).tolist())


def _band_before_last_stride(lay, case, r):
    s, e = int(lay.start[r]), int(lay.end[r])
    m32 = dm.midpoints32(case["t"].numpy()[s:e], case["dt"].numpy()[s:e])
    _, band = dm.membership(m32, case["z"].numpy()[r], case["eps"])
    return bool(band[:max(e - s - rc.WAVE, 0)].any())


def _sample_on_lo(lay, case, r):
    s, e = int(lay.start[r]), int(lay.end[r])
    m32 = dm.midpoints32(case["t"].numpy()[s:e], case["dt"].numpy()[s:e])
    z = case["z"].numpy()[r]
    return bool((m32 == np.float32(z - np.float32(case["eps"]))).any())
