"""The power of tests/test_gpu_ragged_edges.py, checked without a GPU: the float64 closed forms of
tests/ragged_cases.py against autograd, the constant K measured on the f32 oracle, the oracle passing
every assertion the GPU tests make, every mutant failing them on every eligible ray, the share of
density-scan rays that lie within rounding of the threshold, and the Hilbert restatement."""
import math

import numpy as np
import pytest
import torch

from oracle import kernels as K
from tests import ragged_cases as rc
from tests.test_gpu_fused import _composite_oracle

_cache = {}


def _setup(name):
    """(layout, case, float64 forward reference) per bounds layout, built once."""
    if name not in _cache:
        lay = rc.layout(name)
        case = rc.composite_case(lay)
        _cache[name] = (lay, case, rc.composite_fwd_ref(lay, case))
    return _cache[name]


def _fill_outside(lay, a):
    """The oracle's ops allocate their outputs; what the kernels must leave alone is set here."""
    a = a.detach().numpy().copy()
    a[~lay.inside] = rc.SENTINEL
    return a


def _oracle_composite(lay, case):
    """The oracle's f32 op-by-op composition (renderer.cpp:93,107-118) and its autograd backward."""
    key = ("oracle", id(lay))
    if key in _cache:
        return _cache[key]
    logit = case["logit"].clone().requires_grad_(True)
    rgb = case["rgb"].clone().requires_grad_(True)
    idx = lay.bounds
    colors, depths, weights, last_trans = _composite_oracle(logit, rgb, case["dt"], case["t"], idx,
                                                            case["bg"])
    d_w = torch.where(torch.from_numpy(lay.inside), case["d_weights"], torch.zeros(()))
    (colors * case["d_colors"]).sum().add((depths * case["d_depths"]).sum()).add(
        (weights * d_w).sum()).backward()
    got = dict(weights=_fill_outside(lay, weights), last_trans=last_trans.detach().numpy(),
               colors=colors.detach().numpy(), depths=depths.detach().numpy(),
               d_rgb=_fill_outside(lay, rgb.grad), d_logit=_fill_outside(lay, logit.grad))
    _cache[key] = got
    return got


# ---- closed form against autograd ----------------------------------------------------------------

class _TruncExp64(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(x.clamp(-100.0, 5.0))


@pytest.mark.parametrize("name", ["tile", "unordered"])
def test_closed_form_backward_is_autograd_of_the_forward(name):
    lay, case, fwd = _setup(name)
    ref = rc.merge_refs(fwd, rc.composite_bwd_ref(lay, case, fwd["weights"], fwd["last_trans"]))
    logit = case["logit"].double().requires_grad_(True)
    rgb = case["rgb"].double().requires_grad_(True)
    dt, t = case["dt"].double(), case["t"].double()
    loss = torch.zeros((), dtype=torch.float64)
    for r in range(lay.n_rays):
        s, e = int(lay.start[r]), int(lay.end[r])
        if e <= s:
            continue
        sec = _TruncExp64.apply(logit[s:e] - rc.DENSITY_SHIFT) * dt[s:e]
        acc = torch.cumsum(sec, 0) - sec
        w = torch.exp(-acc) * -torch.expm1(-sec)
        tl = torch.exp(-sec.sum())
        colors = (w[:, None] * rgb[s:e]).sum(0) + tl * case["bg"][r].double()
        depth = (w * (t[s:e] + rc.T_SHIFT)).sum() / (1.0 - tl + 1e-4)
        np.testing.assert_allclose(colors.detach().numpy(), ref["colors"][r], rtol=1e-11, atol=0)
        np.testing.assert_allclose(depth.item(), ref["depths"][r], rtol=1e-11, atol=0)
        loss = loss + (colors * case["d_colors"][r].double()).sum() + depth * case["d_depths"][r].double() \
            + (w * case["d_weights"][s:e].double()).sum()
    loss.backward()
    inside = lay.inside
    # 1e-11 of the element; where its terms cancel (an element of 1e-10 from terms of 0.06 occurs)
    # float64 itself resolves it only to 2^-53 of the terms' magnitude, which M_op bounds from above
    for name, got in (("d_logit", logit.grad.numpy()), ("d_rgb", rgb.grad.numpy())):
        a, b, m = got[inside], ref[name][inside], ref["mop"][name][inside]
        assert np.all(np.abs(a - b) <= 1e-11 * np.abs(a) + 1e-15 * m), name


# ---- K -------------------------------------------------------------------------------------------

def _measure(name):
    lay, case, fwd = _setup(name)
    got = _oracle_composite(lay, case)
    _, ref = rc.composite_check(lay, case, got, fwd)
    worst_all, worst_short, by_len = -np.inf, -np.inf, {}
    for out, (ratio, ray) in rc.ratios(lay, got, ref).items():
        worst_all = max(worst_all, float(ratio.max()))
        short = lay.len[ray] <= 2
        worst_short = max(worst_short, float(ratio[short].max()))
        # the single-M figure for the record: err / (u (M_sum + M_op)), to be compared with len_r
        g = np.asarray(got[out], dtype=np.float64)
        rr = rc._ray_index(lay, out, g.shape)
        sel = (rr >= 0) & (lay.len[np.maximum(rr, 0)] > 0)
        one = rc.safe_ratio(np.abs(g - ref[out])[sel],
                            rc.U * (ref["msum"][out][sel] + ref["mop"][out][sel]))
        for ln in np.unique(lay.len[rr[sel]]):
            by_len[int(ln)] = max(by_len.get(int(ln), 0.0), float(one[lay.len[rr[sel]] == ln].max()))
    return worst_all, worst_short, by_len


def test_measured_K():
    """K_COMPOSITE is 4 x the oracle's largest (err/u - len M_sum) / M_op, up to a power of two."""
    worst = 0.0
    for name in rc.LAYOUTS:
        all_, short, by_len = _measure(name)
        print("%s: all rays %.3f, len <= 2: %.3f; err/(u(M_sum+M_op)) by length: %s" % (
            name, all_, short, " ".join("%d:%.2f" % kv for kv in sorted(by_len.items()))))
        worst = max(worst, all_, short)
        # weight_var (M_sum = M_op = M): err / (u M) - len_r
        lay = _setup(name)[0]
        _, w, dv = rc.segment_inputs(lay)
        wr = rc.weight_var_ref(lay, w, dv)
        some = lay.len > 0
        e_var = np.abs(K.weight_var_fwd(w, lay.bounds).numpy() - wr["var"])[some]
        k_var = rc.safe_ratio(e_var - lay.len[some] * rc.U * wr["m_var"][some], rc.U * wr["m_var"][some])
        dw = K.weight_var_bwd(w, lay.bounds, dv).numpy().astype(np.float64)
        ins = lay.inside
        k_dw = rc.safe_ratio(np.abs(dw - wr["dw"])[ins] - lay.len_of[ins] * rc.U * wr["m_dw"][ins],
                             rc.U * wr["m_dw"][ins])
        short = lay.len[some] <= 2
        print("  weight_var: all rays %.3f / %.3f (fwd / bwd), len <= 2: %.3f / %.3f" % (
            k_var.max(), k_dw.max(), k_var[short].max(), k_dw[lay.len_of[ins] <= 2].max()))
        worst = max(worst, float(k_var.max()), float(k_dw.max()))
    assert worst > 0
    assert rc.K_COMPOSITE == 2 ** math.ceil(math.log2(4.0 * worst)), worst


# ---- the oracle passes ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", rc.LAYOUTS)
def test_oracle_passes_the_composite_assertions(name):
    lay, case, fwd = _setup(name)
    rc.assert_no_failures(rc.composite_check(lay, case, _oracle_composite(lay, case), fwd)[0], name)


def _scan_failing_rays(lay, got, want, bound):
    """rays with an element off by more than its bound, or written outside (owner of the gap)."""
    got = np.asarray(got, dtype=np.float64)
    bad_in = lay.inside & ~(np.abs(got - want) <= bound)
    bad_out = ~lay.inside & (got != rc.SENTINEL)
    return set(lay.ray_of[bad_in].tolist()) | set(lay.owner_of_gap[bad_out].tolist())


@pytest.mark.parametrize("name", rc.LAYOUTS)
def test_oracle_passes_the_segment_assertions(name):
    lay, case, ref = _setup(name)
    val, w, dv = rc.segment_inputs(lay)
    want, bound = rc.seg_sum_ref(lay, val)
    assert np.all(np.abs(K.seg_sum_fwd(val, lay.bounds).numpy() - want) <= bound)
    for vec in (3, 16, 64):
        v = torch.randn(lay.n_total, vec, generator=torch.Generator().manual_seed(vec))
        want, bound = rc.seg_sum_ref(lay, v)
        assert np.all(np.abs(K.seg_sum_fwd(v, lay.bounds).numpy() - want) <= bound), vec
    for inc in (0, 1):
        for bwd in (False, True):
            fn = K.seg_scan_bwd if bwd else K.seg_scan_fwd
            want, bound = rc.seg_scan_ref(lay, val, inc, backward=bwd)
            got = _fill_outside(lay, fn(val, lay.bounds, inc))
            assert not _scan_failing_rays(lay, got, want, bound), (inc, bwd)
    wr = rc.weight_var_ref(lay, w, dv)
    tol = (lay.len + rc.K_COMPOSITE) * rc.U * wr["m_var"]
    assert np.all(np.abs(K.weight_var_fwd(w, lay.bounds).numpy() - wr["var"]) <= tol)
    got = _fill_outside(lay, K.weight_var_bwd(w, lay.bounds, dv))
    tol = (lay.len_of + rc.K_COMPOSITE) * rc.U * wr["m_dw"]
    assert not _scan_failing_rays(lay, got, wr["dw"], tol)


# ---- every mutant fails --------------------------------------------------------------------------

def _eligible(lay, mutant, clamped=None):
    ln, tau = lay.len, lay.tau
    mid = (tau == 0.7) | (tau == 3.0)
    if mutant == "tail":
        return set(np.flatnonzero(ln % rc.WAVE != 0).tolist())
    if mutant == "noclamp":   # rays that hold a clamped sample
        return {int(r) for r in np.unique(lay.ray_of[clamped & lay.inside]) if tau[r] <= 3.0}
    if mutant == "var_tail":   # a whole number of strides has no tail to lose
        return set(np.flatnonzero((ln > rc.WAVE) & (ln % rc.WAVE != 0) & mid).tolist())
    return set(np.flatnonzero((ln > rc.WAVE) & mid).tolist())


# (tail on tiling bounds is left out: a write past a ray's end lands in the next ray there)
@pytest.mark.parametrize("mutant,name", [(m, n) for m in rc.COMPOSITE_MUTANTS for n in rc.LAYOUTS
                                         if not (m == "tail" and n == "tile")])
def test_composite_mutant_fails_on_every_eligible_ray(mutant, name):
    lay, case, fwd = _setup(name)
    mut = rc.composite_ref(lay, case, with_dw=True, mutant=mutant)
    got = {k: mut[k].astype(np.float32) for k in rc.PER_SAMPLE + rc.PER_RAY}
    fails, _ = rc.composite_check(lay, case, got, fwd)
    caught = {f[0] for f in fails}
    want = _eligible(lay, mutant, case["clamped"])
    assert want and want <= caught, sorted(want - caught)
    if mutant == "noclamp":   # every clamped sample of a tau <= 3 ray, not merely every ray
        hit = {f[2] for f in fails if f[1] == "d_logit"}
        need = {int(i) for i in np.flatnonzero(case["clamped"] & lay.inside)
                if lay.tau[lay.ray_of[i]] <= 3.0}
        assert need and need <= hit, len(need - hit)
    if mutant == "tail":      # through the written-outside check wherever a gap follows the ray
        outside = {f[0] for f in fails if f[3].startswith("written outside")}
        gap_after = {r for r in want if lay.end[r] < lay.n_total and lay.ray_of[lay.end[r]] < 0}
        assert gap_after and gap_after <= outside
    print("%s / %s: %d of %d eligible rays caught" % (mutant, name, len(want & caught), len(want)))


@pytest.mark.parametrize("name", rc.LAYOUTS)
def test_scan_and_var_mutants_fail_on_every_eligible_ray(name):
    lay, case, ref = _setup(name)
    val, w, dv = rc.segment_inputs(lay)
    want = _eligible(lay, "scan_carry")
    for inc in (0, 1):
        for bwd in (False, True):
            good, bound = rc.seg_scan_ref(lay, val, inc, backward=bwd)
            bad, _ = rc.seg_scan_ref(lay, val, inc, backward=bwd, mutant="scan_carry")
            caught = _scan_failing_rays(lay, bad.astype(np.float32), good, bound)
            assert want and want <= caught, (inc, bwd, sorted(want - caught))
    good = rc.weight_var_ref(lay, w, dv)
    bad = rc.weight_var_ref(lay, w, dv, mutant="var_tail")
    want = _eligible(lay, "var_tail")
    tol = (lay.len + rc.K_COMPOSITE) * rc.U * good["m_var"]
    caught = set(np.flatnonzero(~(np.abs(bad["var"].astype(np.float32) - good["var"]) <= tol)).tolist())
    assert want and want <= caught, sorted(want - caught)      # the forward alone sees every one
    tol = (lay.len_of + rc.K_COMPOSITE) * rc.U * good["m_dw"]
    caught_bwd = _scan_failing_rays(lay, bad["dw"].astype(np.float32), good["dw"], tol)
    # the backward too, except where the tail is a single sample of thousands: the mean moves by
    # less than the any-order bound of its own sum
    assert {r for r in want if lay.len[r] < 1000} <= caught_bwd


def test_the_old_inputs_hide_the_suffix_carry():
    """What test_composite_fwd_bwd cannot see, restated on this module's machinery: with every
    seventh logit at 9.5 and dt ~ U(0, 0.01) a ray is opaque within its first stride, and the
    backward without its suffix carry stays inside that test's tolerance."""
    lay = rc.uniform_layout(8, 257)
    case = rc.composite_case(lay)
    g = torch.Generator().manual_seed(0)
    case["dt"] = torch.rand(lay.n_total, generator=g) * 0.01
    ref = rc.composite_ref(lay, case)["d_logit"]
    mut = rc.composite_ref(lay, case, mutant="suffix")["d_logit"]
    assert np.any(mut != ref)
    assert np.all(np.abs(mut - ref) <= 1e-3 * np.abs(ref) + 1e-4 * np.abs(ref).max())


# ---- density scan: rays within rounding of the threshold ------------------------------------------

def test_density_scan_cases_stay_clear_of_the_threshold():
    n_rays = n_band = 0
    for S in rc.SCAN_S:
        for C in rc.SCAN_C:
            case = rc.density_scan_case(S, C)
            kept, in_band = rc.density_scan_ref(case)
            assert np.array_equal(kept, case["target"]), (S, C)       # the cases are what they claim
            assert in_band.mean() <= 0.02, (S, C)
            n_rays += kept.shape[0]
            n_band += int(in_band.sum())
    assert n_band <= 0.02 * n_rays


# ---- ray keys: the Hilbert restatement ------------------------------------------------------------

def test_hilbert_restatement_is_a_curve():
    bits = 4
    n = 1 << bits
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    d = rc.hilbert_index(x.reshape(-1), y.reshape(-1), bits).astype(np.int64)
    assert np.array_equal(np.sort(d), np.arange(n * n))               # a bijection
    order = np.argsort(d)
    xs, ys = x.reshape(-1)[order], y.reshape(-1)[order]
    step = np.abs(np.diff(xs)) + np.abs(np.diff(ys))
    assert np.all(step == 1)                                           # consecutive: 4-neighbours


def test_ray_keys_restatement_edges():
    d = np.array([[0, 0, 0], [np.inf, 1, 0], [1, -np.inf, 0], [np.nan, 1, 0], [1, np.nan, 0],
                  [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, -1], [1, 1, 1], [-1, -1, 1]], np.float32)
    k = rc.ray_keys_ref(d)
    assert np.all(k[:5] == 0) and np.all(k[5:] > 0) and np.all(k >= 0)
    assert list(k[5:] >> 28) == [0, 1, 2, 5, 0, 1]                     # ties: x over y over z
    assert (k[9] & ((1 << 28) - 1)) == int(rc.hilbert_index([16383], [16383])[0])   # u = v = 1: clamped
