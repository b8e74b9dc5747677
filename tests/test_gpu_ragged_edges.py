"""The per-ray kernels (one wavefront per ray, 64-sample strides linked by a scalar carry) at the
lengths where a stride walk goes wrong, on bounds that tile, leave gaps or are out of order, against
float64 references with a tolerance per element (tests/ragged_cases.py; the power of these assertions
is checked on the CPU by tests/test_ragged_cases_cpu.py).  Every output is pre-filled with a sentinel
and must still hold it outside the rays' ranges."""
import math

import numpy as np
import pytest
import torch

from tests import ragged_cases as rc
from tests import util

pytestmark = pytest.mark.gpu

F2N_E_UNSUPPORTED = -3
WAVES_PER_BLOCK = 4          # F2N_WAVES_PER_BLOCK: rays per workgroup

_cache = {}


def _setup(name):
    if name not in _cache:
        lay = rc.layout(name)
        case = rc.composite_case(lay)
        _cache[name] = (lay, case, rc.composite_fwd_ref(lay, case))
    return _cache[name]


def _status(capi, name, *args):
    """The raw status of f2n_<name> (capi.call raises on anything but F2N_OK)."""
    fn = getattr(capi.lib().cdll, "f2n_" + name)
    return fn(*[capi._ptr(a) for a in args], capi.current_stream())


def _sent(dev, *shape, dtype=torch.float32):
    return torch.full(shape, rc.SENTINEL, dtype=dtype, device=dev)


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))


def _assert_within(lay, got, want, bound, what):
    """|got - want| <= bound inside the ranges, the sentinel bit for bit outside."""
    got = got.cpu().numpy()
    out = ~lay.inside
    assert _bits_equal(got[out], np.full(int(out.sum()), rc.SENTINEL, np.float32)), \
        "%s: written outside every range" % what
    err = np.abs(got.astype(np.float64) - want)[lay.inside]
    bad = ~(err <= bound[lay.inside])
    assert not bad.any(), "%s: %d elements beyond their bound, first: sample %d err %.3e bound %.3e" % (
        what, int(bad.sum()), int(np.flatnonzero(lay.inside)[np.flatnonzero(bad)[0]]),
        err[bad][0], bound[lay.inside][bad][0])


def _run_composite(capi, dev, lay, case, logit_ld, with_dw, n_rays=None, rows=None):
    """composite_fwd then composite_bwd on its outputs, everything pre-filled with the sentinel."""
    n, R = lay.n_total, lay.n_rays if n_rays is None else n_rays
    rows = lay.n_rays if rows is None else rows
    if logit_ld == 1:
        d_logit_in = case["logit"].to(dev)
    else:
        g = torch.Generator().manual_seed(logit_ld)
        feat = torch.randn(n, logit_ld, generator=g)
        feat[:, 0] = case["logit"]
        d_logit_in = feat.to(dev)
    dv = {k: case[k].to(dev).contiguous() for k in ("rgb", "dt", "t", "bg", "d_colors", "d_depths",
                                                    "d_weights")}
    bounds = lay.bounds.to(dev)
    o_c, o_d, o_lt, o_w = _sent(dev, rows, 3), _sent(dev, rows), _sent(dev, rows), _sent(dev, n)
    capi.call("composite_fwd", d_logit_in, logit_ld, dv["rgb"], dv["dt"], dv["t"], bounds, dv["bg"],
              o_c, o_d, o_w, o_lt, R, rc.DENSITY_SHIFT, rc.T_SHIFT)
    g_logit, g_rgb = _sent(dev, n), _sent(dev, n, 3)
    capi.call("composite_bwd", d_logit_in, logit_ld, dv["rgb"], dv["dt"], dv["t"], bounds, dv["bg"],
              o_w, o_lt, dv["d_colors"], dv["d_depths"], dv["d_weights"] if with_dw else None,
              g_logit, g_rgb, R, rc.DENSITY_SHIFT, rc.T_SHIFT)
    return dict(weights=o_w.cpu().numpy(), last_trans=o_lt.cpu().numpy(), colors=o_c.cpu().numpy(),
                depths=o_d.cpu().numpy(), d_rgb=g_rgb.cpu().numpy(), d_logit=g_logit.cpu().numpy())


def _report(lay, got, ref, what):
    worst = {k: float(v[0].max()) for k, v in rc.ratios(lay, got, ref).items() if v[0].size}
    print("%s: largest (err/u - len M_sum)/M_op per output: %s (K = %d)" % (
        what, " ".join("%s %.2f" % kv for kv in worst.items()), rc.K_COMPOSITE))


@pytest.mark.parametrize("with_dw", [True, False])
@pytest.mark.parametrize("logit_ld", [1, 16])
@pytest.mark.parametrize("name", rc.LAYOUTS)
def test_composite_fwd_bwd_per_element(capi, dev, name, logit_ld, with_dw):
    """weights, last_trans, colors, depths, d_rgb and d_logit within u (len_r M_sum + K M_op) of the
    float64 closed forms, element by element; empty rays: colors == bg, last_trans == 1,
    depths == 0 exactly; nothing written outside the ranges, forward or backward."""
    lay, case, fwd = _setup(name)
    got = _run_composite(capi, dev, lay, case, logit_ld, with_dw)
    fails, ref = rc.composite_check(lay, case, got, fwd, with_dw)
    _report(lay, got, ref, "%s ld %d dw %d" % (name, logit_ld, with_dw))
    rc.assert_no_failures(fails, "composite on %s bounds" % name)


@pytest.mark.parametrize("n_rays", [1, WAVES_PER_BLOCK - 1, WAVES_PER_BLOCK, WAVES_PER_BLOCK + 1])
def test_ray_count_edges(capi, dev, n_rays):
    """The last wave of the last block is sometimes absent: rays and samples past n_rays stay
    untouched (the buffers hold eight rays of 65 samples; the kernels are told of n_rays)."""
    full = rc.uniform_layout(8, 65)
    case = rc.composite_case(full)
    lay = rc.Layout(full.bounds[:n_rays].contiguous(), full.tau[:n_rays], full.n_total)
    sub = dict(case)
    for k in ("bg", "d_colors", "d_depths"):
        sub[k] = case[k][:n_rays]
    fwd = rc.composite_fwd_ref(lay, sub)
    got = _run_composite(capi, dev, full, case, 1, True, n_rays=n_rays, rows=8)
    for k in rc.PER_RAY:
        tail = got[k][n_rays:]
        assert _bits_equal(tail, np.full(tail.shape, rc.SENTINEL, np.float32)), k
        got[k] = got[k][:n_rays]
    fails, _ = rc.composite_check(lay, sub, got, fwd, True)
    rc.assert_no_failures(fails, "composite, %d rays" % n_rays)
    val, _, _ = rc.segment_inputs(full)
    for inc in (0, 1):
        for bwd in (False, True):
            out = _sent(dev, full.n_total)
            capi.call("seg_scan_bwd" if bwd else "seg_scan_fwd", val.to(dev), full.bounds.to(dev), out,
                      n_rays, inc)
            want, bound = rc.seg_scan_ref(lay, val, inc, backward=bwd)
            _assert_within(lay, out, want, bound, "seg_scan inc %d bwd %d" % (inc, bwd))


@pytest.mark.parametrize("name", rc.LAYOUTS)
def test_segment_sums_and_scans(capi, dev, name):
    """seg_sum, seg_sum_vec, seg_scan: within the any-order bound len_r u sum|x| of the float64 value,
    per element and with no global scale; the backward copies bit-equal."""
    lay = _setup(name)[0]
    val, _, _ = rc.segment_inputs(lay)
    R, n = lay.n_rays, lay.n_total
    bounds = lay.bounds.to(dev)
    g = torch.Generator().manual_seed(9)

    out = _sent(dev, R)
    capi.call("seg_sum_fwd", val.to(dev), bounds, out, R)
    want, bound = rc.seg_sum_ref(lay, val)
    err = np.abs(out.cpu().numpy().astype(np.float64) - want)
    assert np.all(err <= bound), int(np.argmax(err - bound))
    dsum = torch.randn(R, generator=g)
    dval = _sent(dev, n)
    capi.call("seg_sum_bwd", dsum.to(dev), bounds, dval, R)
    assert _bits_equal(dval.cpu().numpy(), rc.seg_sum_bwd_ref(lay, dsum))

    for vec in (3, 16, 64):
        v = torch.randn(n, vec, generator=g)
        out = _sent(dev, R, vec)
        capi.call("seg_sum_vec_fwd", v.to(dev), bounds, out, R, vec)
        want, bound = rc.seg_sum_ref(lay, v)
        err = np.abs(out.cpu().numpy().astype(np.float64) - want)
        assert np.all(err <= bound), (vec, int(np.argmax(err - bound)))
        ds = torch.randn(R, vec, generator=g)
        dv = _sent(dev, n, vec)
        capi.call("seg_sum_vec_bwd", ds.to(dev), bounds, dv, R, vec)
        assert _bits_equal(dv.cpu().numpy(), rc.seg_sum_bwd_ref(lay, ds)), vec

    for inc in (0, 1):
        for bwd in (False, True):
            out = _sent(dev, n)
            capi.call("seg_scan_bwd" if bwd else "seg_scan_fwd", val.to(dev), bounds, out, R, inc)
            want, bound = rc.seg_scan_ref(lay, val, inc, backward=bwd)
            _assert_within(lay, out, want, bound, "seg_scan inc %d bwd %d" % (inc, bwd))


def test_seg_sum_vec_above_the_cap_is_unsupported(capi, dev):
    lay = rc.uniform_layout(3, 5)
    v, out = torch.zeros(lay.n_total, 65, device=dev), _sent(dev, 3, 65)
    assert _status(capi, "seg_sum_vec_fwd", v, lay.bounds.to(dev), out, 3, 65) == F2N_E_UNSUPPORTED
    assert _status(capi, "seg_sum_vec_bwd", out, lay.bounds.to(dev), v, 3, 65) == F2N_E_UNSUPPORTED
    assert bool((out == rc.SENTINEL).all()) and bool((v == 0).all())


@pytest.mark.parametrize("name", rc.LAYOUTS)
def test_weight_var_per_element(capi, dev, name):
    lay = _setup(name)[0]
    _, w, dvars = rc.segment_inputs(lay)
    ref = rc.weight_var_ref(lay, w, dvars)
    bounds = lay.bounds.to(dev)
    out = _sent(dev, lay.n_rays)
    capi.call("weight_var_fwd", w.to(dev), bounds, out, lay.n_rays)
    got = out.cpu().numpy().astype(np.float64)
    assert np.all(got[lay.len == 0] == 0.0)
    tol = (lay.len + rc.K_COMPOSITE) * rc.U * ref["m_var"]
    assert np.all(np.abs(got - ref["var"]) <= tol), int(np.argmax(np.abs(got - ref["var"]) - tol))
    dw = _sent(dev, lay.n_total)
    capi.call("weight_var_bwd", w.to(dev), bounds, dvars.to(dev), dw, lay.n_rays)
    _assert_within(lay, dw, ref["dw"], (lay.len_of + rc.K_COMPOSITE) * rc.U * ref["m_dw"], "weight_var_bwd")


# ---- density_scan --------------------------------------------------------------------------------

def _scan(capi, dev, case, thresh=rc.SCAN_THRESH):
    kept = torch.full((case["n_rays"],), -1, dtype=torch.int32, device=dev)
    capi.call("density_scan", case["enc"].to(dev), case["C"], case["dt"].to(dev), case["w0"].to(dev),
              case["b0"].to(dev), kept, case["n_rays"], case["S"], thresh, rc.DENSITY_SHIFT)
    return kept.cpu().numpy()


@pytest.mark.parametrize("C", rc.SCAN_C)
@pytest.mark.parametrize("S", rc.SCAN_S)
def test_density_scan_against_the_float64_rule(capi, dev, S, C):
    """kept = the number of leading samples with T_k > thresh, rays built to stop at 1, 63, 64, 65,
    S - 1 and S samples; a ray whose decision lies within the f32 rounding of the exclusive depth may
    differ by one, and at most 2 % of the rays may be such."""
    case = rc.density_scan_case(S, C)
    want, in_band = rc.density_scan_ref(case)
    got = _scan(capi, dev, case)
    assert in_band.mean() <= 0.02
    assert np.array_equal(got[~in_band], want[~in_band]), (got, want)
    assert np.all(np.abs(got[in_band] - want[in_band]) <= 1)
    if S == 65:   # T_0 = 1 is not above a threshold of 1: nothing is kept
        assert np.array_equal(_scan(capi, dev, case, 1.0), np.zeros(case["n_rays"], np.int32))


@pytest.mark.parametrize("C", [1, 4, 12, 24, 48, 256])
def test_density_scan_other_widths_are_unsupported(capi, dev, C):
    S, R = 8, 3
    kept = torch.full((R,), -1, dtype=torch.int32, device=dev)
    st = _status(capi, "density_scan", torch.zeros(C, R * S, device=dev), C, torch.ones(R * S, device=dev),
                 torch.zeros(C, device=dev), torch.zeros(1, device=dev), kept, R, S, 1e-4, 3.0)
    assert st == F2N_E_UNSUPPORTED
    assert bool((kept == -1).all())


@pytest.mark.parametrize("S,step,bias0", [(128, 4.0 / 128, 6.0), (100, 0.04, 6.0), (128, 4.0 / 128, 0.0)])
def test_density_scan_on_the_hash_encoding_is_the_march(capi, dev, S, step, bias0):
    """f2n_density_scan on f2n_hash_fwd's channel-major encoding of all samples gives
    f2n_density_march's counts exactly, on every MARCH route (the claim of include/f2nerf_hip.h)."""
    n_rays, L, F = 150, 16, 2
    fld = util.make_field(L, F, 19, seed=S)
    g = torch.Generator().manual_seed(S + 1)
    C = L * F
    w0 = ((torch.rand(C, generator=g) * 2 - 1) / math.sqrt(C)).to(dev)
    b0 = torch.tensor([bias0], device=dev)
    o = (torch.randn(n_rays, 3, generator=g) * 0.25).to(dev)
    d = torch.randn(n_rays, 3, generator=g).to(dev)
    noise = (torch.rand(n_rays, S, generator=g) + 0.5).to(dev)
    table16, primes = fld["table16"].to(dev), fld["primes"].to(dev)
    bias, mul = fld["bias"].to(dev), fld["mul"].to(dev)
    n_all = n_rays * S
    pts, dirs = torch.empty(n_all, 3, device=dev), torch.empty(n_all, 3, device=dev)
    dt, t = torch.empty(n_all, device=dev), torch.empty(n_all, device=dev)
    bounds = torch.zeros(n_rays, 2, dtype=torch.int32, device=dev)
    capi.call("sample_rays", o, d, noise, pts, dirs, dt, t, bounds, n_rays, S, step)
    x = torch.empty_like(pts)
    capi.call("contract_fwd", pts, x, n_all)
    enc_cm = torch.empty(C, n_all, device=dev)
    capi.call("hash_fwd", x, table16, primes, bias, mul, enc_cm, 1, n_all, None, n_all, L, F,
              fld["T"], fld["stride"])
    scan = torch.full((n_rays,), -1, dtype=torch.int32, device=dev)
    capi.call("density_scan", enc_cm, C, dt, w0, b0, scan, n_rays, S, 1e-4, 3.0)
    for route in (0, 1, 2):
        kept = torch.full((n_rays,), -1, dtype=torch.int32, device=dev)
        with capi.option("MARCH", route):
            capi.call("density_march", o, d, noise, table16, primes, bias, mul, w0, b0, kept, n_rays, S,
                      step, L, F, fld["T"], fld["stride"], 1e-4, 3.0)
        assert torch.equal(kept, scan), route
    if bias0 >= 6.0:
        assert bool((scan < S).any()) and bool((scan >= 1).all())
    else:
        assert bool((scan == S).all())


# ---- density_margin ------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 63, 65])
def test_density_margin_short_and_ragged_strides(capi, dev, S):
    """test_density_margin_flag at S = 1, 63, 65: one stride, a partial one, one sample into the
    second.  The deepest ray is the last one (a block of its own partial wave set) and sits 0.1 %
    below or above the limit: far beyond the rounding of a 65-term f32 sum."""
    g = torch.Generator().manual_seed(S)
    n_rays, limit = 37, 8.7
    logit = torch.randn(n_rays, S, generator=g) * 1.5
    dt = torch.rand(n_rays, S, generator=g) * 0.04 + 0.001
    depth = (torch.exp(logit.double() - 3.0) * dt.double()).sum(1)
    dt = dt * (0.5 * limit / depth).float().unsqueeze(1)          # every ray at half the limit
    for last, poison, want in ((0.999, None, 0), (1.001, None, 1), (0.5, 11, 1), (0.5, None, 0)):
        d = dt.clone()
        d[-1] *= 2.0 * last
        lg = logit.clone()
        if poison is not None:
            lg[poison, S - 1] = float("nan")
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        capi.call("density_margin", lg.reshape(-1).to(dev), d.reshape(-1).to(dev), flag, n_rays, S, 3.0,
                  limit)
        assert int(flag.item()) == want, (last, poison)


# ---- compact_rows_cm -----------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 32])
def test_compact_rows_cm(capi, dev, C):
    """dst[c, start_r + k] == src[c, r S + k] bit for bit; gaps between the destinations and the
    padding behind them keep the sentinel."""
    S = 100
    counts = np.array([0, 1, 64, 65, S, 37, 0, 99, S, 63], dtype=np.int64)
    gaps = np.array([2, 0, 1, 5, 0, 0, 3, 1, 0, 4], dtype=np.int64)
    R = counts.shape[0]
    start = np.cumsum(counts + gaps) - counts
    n_src, n_dst = R * S, int(start[-1] + counts[-1]) + 70
    bounds = torch.from_numpy(np.stack([start, start + counts], 1).astype(np.int32))
    g = torch.Generator().manual_seed(C)
    src = torch.randn(C, n_src, generator=g)
    dst = _sent(dev, C, n_dst)
    capi.call("compact_rows_cm", src.to(dev), n_src, dst, n_dst, C, bounds.to(dev), R, S)
    want = np.full((C, n_dst), rc.SENTINEL, np.float32)
    for r in range(R):
        want[:, start[r]:start[r] + counts[r]] = src.numpy()[:, r * S:r * S + counts[r]]
    assert _bits_equal(dst.cpu().numpy(), want)


# ---- sample_compact ------------------------------------------------------------------------------

@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("S", [100, 192])
def test_sample_compact_rows_are_sample_rays_rows(capi, dev, S, with_noise):
    """The first cnt_r rows f2n_sample_compact writes for ray r are f2n_sample_rays' rows
    r S .. r S + cnt_r bit for bit, in pts, dirs, dt and t (the claim of include/f2nerf_hip.h), at the
    counts where a stride walk goes wrong; behind the last ray the sentinel stays."""
    counts = np.array([0, 1, 8, 63, 64, 65, 72, S - 1, S], dtype=np.int64)
    R, step, pad = counts.shape[0], 4.0 / S, 70
    g = torch.Generator().manual_seed(S)
    o = (torch.randn(R, 3, generator=g) * 0.25).to(dev)
    d = torch.randn(R, 3, generator=g).to(dev)
    noise = (torch.rand(R, S, generator=g) + 0.5).to(dev) if with_noise else None
    full = [_sent(dev, R * S, 3), _sent(dev, R * S, 3), _sent(dev, R * S), _sent(dev, R * S)]
    capi.call("sample_rays", o, d, noise, *full, torch.zeros(R, 2, dtype=torch.int32, device=dev), R, S,
              step)
    start = np.cumsum(counts) - counts
    n = int(counts.sum())
    bounds = torch.from_numpy(np.stack([start, start + counts], 1).astype(np.int32)).to(dev)
    got = [_sent(dev, n + pad, 3), _sent(dev, n + pad, 3), _sent(dev, n + pad), _sent(dev, n + pad)]
    capi.call("sample_compact", o, d, noise, bounds, *got, R, S, step)
    for what, a, b in zip(("pts", "dirs", "dt", "t"), got, full):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        want = np.full_like(a, rc.SENTINEL)
        for r in range(R):
            want[start[r]:start[r] + counts[r]] = b[r * S:r * S + counts[r]]
        assert _bits_equal(a, want), what
