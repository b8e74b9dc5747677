"""The power of tests/test_gpu_weight_dist.py, checked without a GPU: the assertions of
tests/dist_cases.py accept the f32 restatement of the kernels' O(n) form and reject every mutant, the
constant K is re-derived, the closed forms anchor the double sum, and the two C entries are declared,
exported, cited and validate their arguments before any HIP work."""
import ctypes
import math
import re

import numpy as np
import pytest

from tests import dist_cases as dc
from tests import ragged_cases as rc

CASES = [(name, variant) for name in rc.LAYOUTS for variant in dc.T_VARIANTS]


def _f32(out):
    return {k: np.asarray(v, dtype=np.float32) for k, v in out.items()}


def test_inputs_are_what_the_docstring_says():
    for name, variant in CASES:
        lay, case, ref = dc.shared(name, variant)
        assert lay.n_rays == 72 and int(lay.len.sum()) == 32176
        assert sorted(set(lay.len.tolist())) == sorted(rc.LENGTHS)
        t, dt, w = (case[k].numpy() for k in ("t", "dt", "weights"))
        assert t.dtype == dt.dtype == w.dtype == np.float32
        step_over_dt = []
        for r in range(lay.n_rays):
            s, e = int(lay.start[r]), int(lay.end[r])
            if e <= s:
                continue
            m = t[s:e].astype(np.float64) - 0.5 * dt[s:e].astype(np.float64)
            assert (np.diff(m) >= 0).all()                         # the kernels' precondition
            assert case["offset"][r] <= dc.MAX_OFFSET
            if lay.tau[r] in (0.7, 3.0):                           # every stride carries weight
                for lo in range(s, e, rc.WAVE):
                    assert w[lo:min(lo + rc.WAVE, e)].sum() > 0
            big = dt[s + 1:e] > 64 * np.spacing(t[s + 1:e])        # (steps that f32 t resolves)
            step_over_dt.append((np.diff(t[s:e].astype(np.float64)) / dt[s + 1:e])[big])
        ratio = np.concatenate(step_over_dt)
        if variant == "contiguous":
            assert np.all(np.abs(ratio - 1.0) < 0.05)
        else:
            far = ratio > 3.5
            assert 0.15 < far.mean() < 0.25 and ratio[far].max() < 41.5
        if name != "tile":                  # samples outside the ranges hold ordinary values
            assert (w[~lay.inside] > 0).all() and (t[~lay.inside] >= 1).all()


def test_closed_forms_anchor_the_double_sum():
    rng = np.random.RandomState(3)
    w, dt = rng.rand(2) + 0.1, rng.rand(2) + 0.1
    m = np.array([5.25, 5.25 + rng.rand()])
    D1, g1 = dc.double_sum(w[:1], m[:1], dt[:1])
    want_D, want_g = dc.closed_form_one(w[0], dt[0])
    assert abs(D1 - want_D) <= 1e-15 and np.allclose(g1, want_g, rtol=1e-14, atol=0)
    D2, g2 = dc.double_sum(w, m, dt)
    want_D, want_g = dc.closed_form_two(w, m, dt)
    assert abs(D2 - want_D) <= 1e-15 and np.allclose(g2, want_g, rtol=1e-14, atol=0)
    # ... and on the rays of length 1 and 2 of a case, through dist_ref
    lay, case, ref = dc.shared("gaps", "thinned")
    w, t, dt, d_out = (case[k].numpy().astype(np.float64) for k in ("weights", "t", "dt", "d_out"))
    seen = set()
    for r in np.flatnonzero(lay.len <= 2):
        s, e = int(lay.start[r]), int(lay.end[r])
        if e - s == 1:
            D, g = dc.closed_form_one(w[s], dt[s])
        elif e - s == 2:
            D, g = dc.closed_form_two(w[s:e], t[s:e] - 0.5 * dt[s:e], dt[s:e])
        else:
            assert ref["D"][r] == 0.0
            continue
        seen.add(e - s)
        assert abs(ref["D"][r] - D) <= 1e-14 * abs(D)
        assert np.allclose(ref["dw"][s:e], d_out[r] * g, rtol=1e-13, atol=0)
    assert seen == {1, 2}


def test_linear_form_in_float64_is_the_double_sum():
    """the O(n) algebra itself (no defect, float64) agrees with the definition far inside the bound"""
    lay, case, ref = dc.shared("unordered", "thinned")
    for strided in (False, True):
        got = dc.dist_linear(lay, case, np.float64, strided)
        for name, (ratio, _) in dc.ratios(lay, got, ref).items():
            assert ratio.max() < 1e-3, (name, strided, ratio.max())


@pytest.mark.parametrize("name,variant", CASES)
def test_assertions_accept_the_f32_restatement(name, variant):
    lay, case, ref = dc.shared(name, variant)
    for strided in (False, True):
        got = _f32(dc.dist_f32(lay, case, strided))
        assert got["D"].dtype == np.float32
        rc.assert_no_failures(dc.dist_failures(lay, got, ref), "%s %s strided=%s" % (name, variant, strided))
    # the assertions themselves: a write outside the ranges and a non-zero empty ray are caught
    got = _f32(dc.dist_f32(lay, case, True))
    gap = np.flatnonzero(~lay.inside)
    if gap.size:
        got["dw"][gap[0]] = 0.0
        assert any(f[3].startswith("written outside") for f in dc.dist_failures(lay, got, ref))
    empty = np.flatnonzero(lay.len == 0)
    got["D"][empty[0]] = 1e-30
    assert any(f[3].startswith("empty ray") for f in dc.dist_failures(lay, got, ref))


def test_measured_K():
    """K_DIST = 4 x the largest (err / u - len M_sum) / M_op of the f32 restatement, rounded up to a
    power of two.  Prints the figures the module docstring and NOTES.md quote."""
    worst, worst_short = 0.0, 0.0
    for name in rc.LAYOUTS:
        row = {}
        for strided in (False, True):
            for out in ("D", "dw"):
                row[(strided, out)] = -np.inf
        short = -np.inf
        for variant in dc.T_VARIANTS:
            lay, case, ref = dc.shared(name, variant)
            for strided in (False, True):
                for out, (ratio, ray) in dc.ratios(lay, dc.dist_f32(lay, case, strided), ref).items():
                    row[(strided, out)] = max(row[(strided, out)], float(ratio.max()))
                    short = max(short, float(ratio[lay.len[ray] <= 2].max()))
        print("  %-9s forward serial %.3f strided %.3f | backward serial %.3f strided %.3f | "
              "len <= 2: %.3f" % (name, row[(False, "D")], row[(True, "D")], row[(False, "dw")],
                                  row[(True, "dw")], short))
        worst = max(worst, *row.values())
        worst_short = max(worst_short, short)
    assert worst > 0 and worst_short > 0
    K = 2.0 ** math.ceil(math.log2(4.0 * max(worst, worst_short)))
    assert K == dc.K_DIST, (worst, worst_short, K)


@pytest.mark.parametrize("name,variant", CASES)
def test_every_mutant_is_rejected(name, variant):
    lay, case, ref = dc.shared(name, variant)
    long_rays = set(np.flatnonzero(lay.len > rc.WAVE).tolist())          # more than one stride
    partial = set(np.flatnonzero(lay.len % rc.WAVE != 0).tolist())
    for mutant in dc.DIST_MUTANTS:
        fails = dc.dist_failures(lay, _f32(dc.dist_linear(lay, case, mutant=mutant)), ref)
        rays = {f[0] for f in fails}
        fwd = {f[0] for f in fails if f[1] == "D"}
        bwd = {f[0] for f in fails if f[1] == "dw"}
        if mutant == "dist_carry":         # every ray of more than one stride, both directions
            assert bwd == long_rays and len(fwd) >= len(long_rays) - 1 and fwd <= long_rays
        elif mutant == "dist_suffix":      # the backward alone
            assert not fwd and len(bwd) >= len(long_rays) - 1 and bwd <= long_rays
        elif mutant == "dist_tail":        # rays whose last stride is partial
            assert rays <= partial and len(rays) >= 0.9 * len(partial)
            assert len(fwd) >= 0.9 * len(partial)
        elif mutant == "dist_self":        # at least every ray of one or two samples
            assert set(np.flatnonzero((lay.len >= 1) & (lay.len <= 2)).tolist()) <= (fwd & bwd)
            assert len(rays) >= 50
        elif mutant == "dist_mid":
            assert len(bwd) >= 60 and len(fwd) >= 36
        else:
            # no anchoring costs precision only where the offset is large against the ray's extent:
            # the contiguous rays (extent = sum of dt, a fraction of a unit) show it at offsets of up
            # to 5; the thinned ones (extents of tens of units) show it once they lie 50 further out
            assert mutant == "dist_anchor"
            if variant == "contiguous":
                assert rays, "no ray shows the missing anchor"
                assert min(case["offset"][r] for r in rays) > 1.0
            else:
                far = dc.far_case(lay, case)
                far_ref = dc.dist_ref(lay, far)
                for strided in (False, True):        # the anchored form pays nothing for the offset
                    rc.assert_no_failures(
                        dc.dist_failures(lay, _f32(dc.dist_f32(lay, far, strided)), far_ref), "far")
                bad = dc.dist_failures(lay, _f32(dc.dist_linear(lay, far, mutant=mutant)), far_ref)
                assert len({f[0] for f in bad}) >= 3, "no thinned ray shows the missing anchor"


# ---- the C entries -------------------------------------------------------------------------------

ENTRIES = ("f2n_weight_dist_fwd", "f2n_weight_dist_bwd")


def test_entries_are_declared_exported_and_cited(capi):
    decls = capi.parse_header()
    P, I = ctypes.c_void_p, ctypes.c_int
    assert [t for t, _ in decls["f2n_weight_dist_fwd"][1]] == [P, P, P, P, P, I, P]
    assert [t for t, _ in decls["f2n_weight_dist_bwd"][1]] == [P, P, P, P, P, P, I, P]
    assert [n for _, n in decls["f2n_weight_dist_fwd"][1]] == [
        "weights", "t", "dt", "idx", "out", "n_rays", "stream"]
    assert [n for _, n in decls["f2n_weight_dist_bwd"][1]] == [
        "weights", "t", "dt", "idx", "d_out", "dw", "n_rays", "stream"]
    cdll = ctypes.CDLL(capi.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(cdll, name), name
    assert capi.lib().cdll.f2n_abi_version() == 2          # entries added, nothing else changed
    text = open(capi.HEADER).read()
    pos = text.index("f2n_weight_dist_fwd(")
    block = text[text.rindex("/*", 0, pos):pos]
    assert text.index("ragged per-ray ops") < pos < text.index("scatter (row A9)")
    for site in ("src/CustomOps/CustomOps.cu:13-67", "src/main_functions/train_manager.cpp:80-93"):
        assert site in block, site
    flat = " ".join(block.split())
    assert re.search(r"reference has NO such kernel", flat)
    assert "non-decreasing" in flat and "no gradient" in flat


def test_argument_validation_without_gpu(capi):
    c = capi.lib().cdll
    fake = 0x1000
    fwd, bwd = c.f2n_weight_dist_fwd, c.f2n_weight_dist_bwd
    assert fwd(fake, fake, fake, None, fake, 4, None) == -1        # null idx
    assert fwd(fake, fake, fake, fake, None, 4, None) == -1        # null output
    assert fwd(fake, fake, fake, fake, fake, -1, None) == -1       # negative count
    assert fwd(None, None, None, None, None, 0, None) == -1        # idx required even when empty
    assert fwd(fake, fake, fake, fake, fake, 0, None) == 0         # no rays: nothing is launched
    assert bwd(fake, fake, fake, None, fake, fake, 4, None) == -1
    assert bwd(fake, fake, fake, fake, fake, None, 4, None) == -1
    assert bwd(fake, fake, fake, fake, fake, fake, -1, None) == -1
    assert bwd(fake, fake, fake, fake, fake, fake, 0, None) == 0


def test_host_op_refuses_cpu_tensors(pkg):
    import torch

    H = pkg.load_host()
    w = torch.ones(4)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        H.weight_dist(w, w, w, torch.tensor([[0, 4]], dtype=torch.int32))
