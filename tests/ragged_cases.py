"""Inputs, float64 references, per-element bounds and mutants for the per-ray kernels (one 64-lane
wavefront per ray, 64-sample strides linked by a scalar carry): composite_fwd/bwd, seg_sum(_vec),
seg_scan, weight_var, density_scan.  No tests in here; tests/test_ragged_cases_cpu.py checks on the
CPU that the assertions built from this module reject every mutant, tests/test_gpu_ragged_edges.py
makes them against the HIP kernels.

Bounds.  stride_edge_bounds: every length in LENGTHS (the edges of a 64-sample stride walk) paired
with every total optical depth in TAUS, shuffled; tiling, with gaps of 0 / 1 / 5 unused samples, or
with gaps and the ranges laid out in non-monotonic order.  Outputs are pre-filled with SENTINEL and
everything outside the rays' ranges must still hold it.

Compositing case.  dt is rescaled per ray so that sum exp(logit - 3) dt = tau_r: every stride of a
tau = 0.7 or 3 ray carries weight, which is what makes a dropped stride carry visible.  Every
seventh sample has logit 9.5 (x = 6.5 > 5: the clamp of TruncExp::backward) with dt shrunk by
exp(1 - 9.5), so that its optical depth stays ordinary.

Tolerance of a float output element of ray r:

    tol = u (len_r M_sum + K M_op),   u = 2^-24

M_sum and M_op are float64 conditioning numbers: sums of the absolute values of the terms that enter
the element, each with the fixed amplification of its f32 formula.  M_sum holds what a sum over the
ray's samples contributes (len_r u sum|x| is the any-order bound for adding len_r terms: it holds for
the reference's serial order and for every stride and DPP tree); M_op holds what the roundings that
are not the sum contribute (the expf's, the products, the divide), and K is their count.  It is the
form (len_r + K) u M with the two kinds of term kept apart, and never wider than that form with
M = M_sum + M_op: alpha = 1 - expf(-sec) carries an absolute error of about u whatever sec is, so a
weight is known to u T_k only, and charging that per-op error len_r times as well would leave a
4097-sample colour a tolerance of order 0.1.

K is MEASURED against the oracle's f32 op-by-op composition (never against the HIP kernels), by
tests/test_ragged_cases_cpu.py::test_measured_K: the largest (err / u - len_r M_sum) / M_op over all
elements of all outputs, and the same over rays of length <= 2 where sums play no part; K = 4 x the
larger of the two, rounded up to a power of two (4: the device's expf may be an ulp looser than the
host's, and the kernel fuses where the oracle does not).

    measured on the three layouts (tiling / gapped / out of order), composite outputs:
      all rays 0.997 / 0.995 / 0.994 (d_rgb = w dC: one product, one rounding, so just below 1),
      rays of length <= 2: 0.778 / 0.835 / 0.828;
    weight_var (M_sum = M_op = M, err / (u M) - len_r): forward -1.0 / -0.4 / -1.0, backward
      -1.5 / -1.8 / -1.8: the oracle's serial sums stay below the any-order term alone.
    4 x 0.997 rounds up to K_COMPOSITE = 4.  As one number M = M_sum + M_op, the oracle's largest
    err / (u M) by ray length is 0.5-0.8 (1, 2), 0.9-1.0 (63 .. 129), 1.0-2.3 (191 .. 257), 1.5-3.4
    (1000), 2.2-4.3 (1024), 5.2-6.3 (4097): far below len_r; NOTES.md section 12 has the table.

Mutants (CPU only, float64, one defect each): suffix, depth, nd, tail, noclamp (compositing),
scan_carry (seg_scan), var_tail (weight_var); see MUTANTS.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
SENTINEL = 7.0
WAVE = 64
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1000, 1024, 4097)
TAUS = (0.05, 0.7, 3.0, 12.0)
LAYOUTS = ("tile", "gaps", "unordered")
K_COMPOSITE = 4          # see the module docstring; test_measured_K re-derives it
DENSITY_SHIFT = 3.0
T_SHIFT = 1e-2

COMPOSITE_MUTANTS = ("suffix", "depth", "nd", "tail", "noclamp")
MUTANTS = COMPOSITE_MUTANTS + ("scan_carry", "var_tail")


# ---------------------------------------------------------------------------------- bounds --------

class Layout:
    """bounds [n_rays, 2] int32, tau [n_rays] float64, n_total (buffer length in samples), and
    ray_of [n_total] (index of the ray that owns the sample, or -1), owner_of_gap [n_total] (for a
    sample outside every range: the ray whose range ends closest before it, else -1)."""

    def __init__(self, bounds, tau, n_total):
        self.bounds = bounds
        self.tau = tau
        self.n_total = n_total
        b = bounds.numpy().astype(np.int64)
        self.start, self.end = b[:, 0], b[:, 1]
        self.len = self.end - self.start
        self.n_rays = b.shape[0]
        self.ray_of = np.full(n_total, -1, dtype=np.int64)
        for r in range(self.n_rays):
            assert (self.ray_of[self.start[r]:self.end[r]] == -1).all(), "ranges overlap"
            self.ray_of[self.start[r]:self.end[r]] = r
        self.inside = self.ray_of >= 0
        self.owner_of_gap = np.full(n_total, -1, dtype=np.int64)
        by_end = sorted((int(self.end[r]), r) for r in range(self.n_rays) if self.len[r] > 0)
        for end, r in by_end:
            i = end
            while i < n_total and self.ray_of[i] < 0:
                self.owner_of_gap[i] = r
                i += 1
        self.len_of = np.where(self.inside, self.len[np.maximum(self.ray_of, 0)], 0)


def stride_edge_layout(seed, gaps, unordered=False, empty_ends=False):
    rng = np.random.RandomState(seed)
    pairs = [(l, t) for l in LENGTHS for t in TAUS]
    order = rng.permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    if empty_ends:   # the first and the last ray are empty
        empties = [i for i, p in enumerate(pairs) if p[0] == 0]
        for pos, i in ((0, empties[0]), (len(pairs) - 1, empties[-1])):
            pairs[pos], pairs[i] = pairs[i], pairs[pos]
    n_rays = len(pairs)
    lens = np.array([p[0] for p in pairs], dtype=np.int64)
    tau = np.array([p[1] for p in pairs], dtype=np.float64)
    place = rng.permutation(n_rays) if unordered else np.arange(n_rays)   # memory order of the rays
    gap = rng.choice([0, 1, 5], size=n_rays) if gaps else np.zeros(n_rays, dtype=np.int64)
    start = np.zeros(n_rays, dtype=np.int64)
    pos = int(gap[0]) if gaps else 0
    for r in place:
        start[r] = pos
        pos += int(lens[r]) + int(gap[r])
    n_total = pos + (WAVE if gaps else 0)     # room behind the last ray stays sentinel too
    bounds = torch.from_numpy(np.stack([start, start + lens], 1).astype(np.int32)).contiguous()
    return Layout(bounds, tau, n_total)


def stride_edge_bounds(seed, gaps, unordered=False, empty_ends=False):
    """[n_rays, 2] int32 bounds of stride_edge_layout."""
    return stride_edge_layout(seed, gaps, unordered, empty_ends).bounds


def layout(name, seed=0):
    """'tile': the ranges tile the array in ray order; 'gaps': 0, 1 or 5 unused samples between
    consecutive rays, first and last ray empty; 'unordered': gaps, starts not sorted."""
    if name == "tile":
        return stride_edge_layout(seed, False)
    if name == "gaps":
        return stride_edge_layout(seed, True, empty_ends=True)
    assert name == "unordered"
    return stride_edge_layout(seed, True, unordered=True)


def uniform_layout(n_rays, length):
    start = np.arange(n_rays, dtype=np.int64) * length
    bounds = torch.from_numpy(np.stack([start, start + length], 1).astype(np.int32)).contiguous()
    return Layout(bounds, np.resize(np.array(TAUS[:3]), n_rays).astype(np.float64), n_rays * length)


# ---------------------------------------------------------------------------------- inputs --------

CASE_SEED = 2   # seeds 0 and 1 each hold one clamped sample whose d_logit cancels to below its own
                # bound (1e-10 from terms of 1e-3): the missing clamp cannot show on that sample


def composite_case(lay, seed=CASE_SEED):
    """f32 inputs of composite_fwd/bwd on a Layout (torch CPU tensors; samples outside the ranges
    hold ordinary values too, so that a kernel reading past a ray's end computes with them)."""
    g = torch.Generator().manual_seed(1000 + seed)
    n, R = lay.n_total, lay.n_rays
    logit = (torch.randn(n, generator=g, dtype=torch.float64) * 1.5 + 1.0)
    dt = torch.rand(n, generator=g, dtype=torch.float64) * 0.8 + 0.2
    clamped = torch.zeros(n, dtype=torch.bool)
    clamped[::7] = True
    logit[clamped] = 9.5
    dt[clamped] *= math.exp(1.0 - 9.5)
    logit = logit.float()
    sig = torch.exp(logit.double() - DENSITY_SHIFT)
    scale = torch.full((n,), 1e-3, dtype=torch.float64)
    for r in range(R):
        s, e = int(lay.start[r]), int(lay.end[r])
        if e > s:
            scale[s:e] = lay.tau[r] / float((sig[s:e] * dt[s:e]).sum())
    dt = (dt * scale).float()
    assert bool((dt > 0).all())
    case = dict(
        logit=logit, dt=dt, clamped=clamped.numpy(),
        rgb=torch.rand(n, 3, generator=g), t=torch.rand(n, generator=g) * 4.0,
        bg=torch.rand(R, 3, generator=g), d_colors=torch.randn(R, 3, generator=g),
        d_depths=torch.randn(R, generator=g) * 0.1, d_weights=torch.randn(n, generator=g) * 0.1)
    return case


def _np64(x):
    return x.detach().cpu().numpy().astype(np.float64)


# ---------------------------------------------------------------------------------- compositing ---

def _excl_cumsum(a):
    c = np.cumsum(a)
    return c - a


def _suffix_excl(a):
    """out[k] = sum_{j>k} a[j]"""
    c = np.cumsum(a[::-1])[::-1]
    return c - a


def _stride_local(a, fn):
    out = np.empty_like(a)
    for c in range(0, a.shape[0], WAVE):
        out[c:c + WAVE] = fn(a[c:c + WAVE])
    return out


def _ray_range(lay, r, mutant):
    s, e = int(lay.start[r]), int(lay.end[r])
    if e > s and mutant == "tail":   # the last partial stride handled as if it were full
        e = min(s + -(-(e - s) // WAVE) * WAVE, lay.n_total)
    return s, e


def composite_fwd_ref(lay, case, mutant=None):
    """The forward's closed form (include/f2nerf_hip.h, composite.hip; appendix A.7) in float64 on
    the f32 inputs -> dict: weights [n] (SENTINEL outside the ranges), last_trans [R], colors [R,3],
    depths [R], and 'msum' / 'mop': the conditioning numbers of each, same shapes."""
    assert mutant in (None,) + COMPOSITE_MUTANTS
    n, R = lay.n_total, lay.n_rays
    logit, dt, rgb, t, bg = (_np64(case[k]) for k in ("logit", "dt", "rgb", "t", "bg"))
    out = dict(weights=np.full(n, SENTINEL), last_trans=np.ones(R), colors=bg.copy(),
               depths=np.zeros(R))
    msum = {k: np.zeros_like(v) for k, v in out.items()}
    mop = {k: np.zeros_like(v) for k, v in out.items()}
    for r in range(R):
        s, e = _ray_range(lay, r, mutant)
        if e <= s:
            continue
        sl = slice(s, e)
        x = logit[sl] - DENSITY_SHIFT
        ax = np.abs(x)
        sec = np.exp(x) * dt[sl]
        acc = _excl_cumsum(sec)
        tau = float(sec.sum())
        T = np.exp(-(_stride_local(sec, _excl_cumsum) if mutant == "depth" else acc))
        w = T * -np.expm1(-sec)
        Tl = math.exp(-tau)
        den = 1.0 - Tl + 1e-4
        tp = t[sl] + T_SHIFT
        Nd = float((w * tp).sum())
        out["weights"][sl] = w
        out["last_trans"][r] = Tl
        out["colors"][r] = (w[:, None] * rgb[sl]).sum(0) + Tl * bg[r]
        out["depths"][r] = Nd / den
        # sec_j = expf(fl(logit_j - shift)) dt_j carries a relative error of (|x_j| + 2) u; the
        # exclusive sum acc_k adds len u acc_k; T_k = expf(-acc_k) turns both into relative errors
        accx, taux = _excl_cumsum(sec * (2.0 + ax)), float((sec * (2.0 + ax)).sum())
        m_w_sum = w * acc
        # alpha = 1 - expf(-sec): an absolute error of u whatever sec is, so w is known to u T
        m_w_op = T * (1.0 + (2.0 + ax) * np.minimum(sec, 1.0)) + w * (2.0 + accx)
        m_Tl_sum, m_Tl_op = Tl * tau, Tl * (1.0 + taux)
        msum["weights"][sl], mop["weights"][sl] = m_w_sum, m_w_op
        msum["last_trans"][r], mop["last_trans"][r] = m_Tl_sum, m_Tl_op
        msum["colors"][r] = ((m_w_sum + w)[:, None] * rgb[sl]).sum(0) + (m_Tl_sum + Tl) * bg[r]
        mop["colors"][r] = (m_w_op[:, None] * rgb[sl]).sum(0) + (m_Tl_op + Tl) * bg[r]
        m_Nd_sum, m_Nd_op = float(((m_w_sum + w) * tp).sum()), float(((m_w_op + w) * tp).sum())
        depth = Nd / den                 # den = 1 - T_last + 1e-4: the factor (1 + 1/den)
        msum["depths"][r] = m_Nd_sum / den + depth * m_Tl_sum / den
        mop["depths"][r] = m_Nd_op / den + depth * (m_Tl_op / den + 3.0)
    out["msum"], out["mop"] = msum, mop
    return out


def composite_bwd_ref(lay, case, weights, last_trans, with_dw=True, mutant=None):
    """The backward's closed form (composite.hip, appendix A.8) in float64.  weights [n] and
    last_trans [R] are INPUTS of f2n_composite_bwd (f32, what the forward under test wrote) and are
    taken as given here too; T_k is re-derived from logit and dt as the kernel does.
    -> dict d_rgb [n,3], d_logit [n] (SENTINEL outside the ranges), 'msum' / 'mop'."""
    assert mutant in (None,) + COMPOSITE_MUTANTS
    n, R = lay.n_total, lay.n_rays
    logit, dt, rgb, t = (_np64(case[k]) for k in ("logit", "dt", "rgb", "t"))
    bg, dC, dD = _np64(case["bg"]), _np64(case["d_colors"]), _np64(case["d_depths"])
    dW = _np64(case["d_weights"]) if with_dw else np.zeros(n)
    w_in = np.asarray(weights, dtype=np.float64)
    tl_in = np.asarray(last_trans, dtype=np.float64)
    out = dict(d_rgb=np.full((n, 3), SENTINEL), d_logit=np.full(n, SENTINEL))
    msum = {k: np.zeros_like(v) for k, v in out.items()}
    mop = {k: np.zeros_like(v) for k, v in out.items()}
    for r in range(R):
        s, e = _ray_range(lay, r, mutant)
        if e <= s:
            continue
        sl = slice(s, e)
        x = logit[sl] - DENSITY_SHIFT
        ax = np.abs(x)
        sec = np.exp(x) * dt[sl]
        acc = _excl_cumsum(sec)
        T = np.exp(-(_stride_local(sec, _excl_cumsum) if mutant == "depth" else acc))
        w, Tl = w_in[sl], float(tl_in[r])
        den = 1.0 - Tl + 1e-4
        tp = t[sl] + T_SHIFT
        Nd = float((w * tp).sum())
        dw = rgb[sl] @ dC[r] + dD[r] * tp / den + dW[sl]
        q = dw * w
        later = _stride_local(q, _suffix_excl) if mutant == "suffix" else _suffix_excl(q)
        Nd_b = float((w[:WAVE] * tp[:WAVE]).sum()) if mutant == "nd" else Nd
        d_tl = float(dC[r] @ bg[r]) + dD[r] * Nd_b / (den * den)
        d_total = -Tl * d_tl
        d_sec = dw * (T - w) - later + d_total
        fac = dt[sl] * np.exp(x if mutant == "noclamp" else np.clip(x, -100.0, 5.0))
        out["d_logit"][sl] = d_sec * fac
        out["d_rgb"][sl] = w[:, None] * dC[r][None, :]
        # ---- conditioning numbers (module docstring) ----
        accx = _excl_cumsum(sec * (2.0 + ax))
        m_T_sum, m_T_op = T * acc, T * (1.0 + accx)
        mop["d_rgb"][sl] = np.abs(w)[:, None] * np.abs(dC[r])[None, :]       # one product
        a_dep = np.abs(dD[r]) * tp / den
        adw = rgb[sl] @ np.abs(dC[r]) + a_dep + np.abs(dW[sl])
        m_dw_op = 3.0 * adw + 3.0 * a_dep            # the dot's three terms; t + shift, den, divide
        aq = np.abs(dw * w)
        a_nd = float((np.abs(w) * tp).sum())
        k_nd = abs(dD[r]) / (den * den)
        a_tl = float(np.abs(dC[r]) @ bg[r]) + k_nd * a_nd
        m_ds_sum = np.abs(dw) * m_T_sum + _suffix_excl(aq) + abs(Tl) * k_nd * a_nd
        m_ds_op = (m_dw_op * np.abs(T - w) + np.abs(dw) * (m_T_op + T + np.abs(w))
                   + _suffix_excl(m_dw_op * np.abs(w) + aq) + abs(Tl) * (4.0 * a_tl + 8.0 * k_nd * a_nd))
        a_ds = np.abs(dw * (T - w)) + _suffix_excl(aq) + abs(d_total)
        msum["d_logit"][sl] = fac * m_ds_sum
        mop["d_logit"][sl] = fac * (m_ds_op + a_ds * (4.0 + ax))
    out["msum"], out["mop"] = msum, mop
    return out


def merge_refs(*refs):
    out = {"msum": {}, "mop": {}}
    for ref in refs:
        for k, v in ref.items():
            if k in ("msum", "mop"):
                out[k].update(v)
            else:
                out[k] = v
    return out


def composite_ref(lay, case, with_dw=True, mutant=None):
    """Forward, then the backward on the forward's own weights and last_trans rounded to f32 (what a
    kernel with the same defect, or none, would hand its backward)."""
    fwd = composite_fwd_ref(lay, case, mutant)
    bwd = composite_bwd_ref(lay, case, fwd["weights"].astype(np.float32),
                            fwd["last_trans"].astype(np.float32), with_dw, mutant)
    return merge_refs(fwd, bwd)


PER_SAMPLE = ("weights", "d_rgb", "d_logit")
PER_RAY = ("last_trans", "colors", "depths")


def _ray_index(lay, name, shape):
    """ray index of every element of output `name` (-1: outside every range)."""
    if name in PER_SAMPLE:
        idx = lay.ray_of
    else:
        idx = np.arange(lay.n_rays)
    return idx if len(shape) == 1 else np.broadcast_to(idx[:, None], shape)


def safe_ratio(num, den):
    """num / den where den > 0; an element without a bound (den == 0) must be exact: -inf if
    num <= 0, else +inf."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.where(num <= 0, -np.inf, np.inf)
    pos = den > 0
    out[pos] = num[pos] / den[pos]
    return out


def ratios(lay, got, ref, names=None):
    """(err / u - len_r M_sum) / M_op per element of each output (what K has to cover), as
    dict name -> (ratio array, ray index array) over the elements inside the ranges."""
    res = {}
    for name in (names or PER_SAMPLE + PER_RAY):
        if name not in got:
            continue
        g = np.asarray(got[name], dtype=np.float64)
        ray = _ray_index(lay, name, g.shape)
        sel = (ray >= 0) & (lay.len[np.maximum(ray, 0)] > 0)
        err = np.abs(g - ref[name])[sel]
        ln = lay.len[ray[sel]].astype(np.float64)
        res[name] = (safe_ratio(err / U - ln * ref["msum"][name][sel], ref["mop"][name][sel]),
                     ray[sel])
    return res


def composite_failures(lay, got, ref, K=K_COMPOSITE):
    """Every assertion the GPU test makes on composite outputs, as a list of
    (ray, output name, flat element index, message); empty = all hold.  got: name -> f32 array
    (any subset of the outputs; per-sample arrays were pre-filled with SENTINEL)."""
    fails = []
    sent = np.float32(SENTINEL)
    for name, g32 in got.items():
        g32 = np.asarray(g32, dtype=np.float32)
        assert g32.shape == ref[name].shape, (name, g32.shape, ref[name].shape)
        g = g32.astype(np.float64)
        ray = _ray_index(lay, name, g.shape)
        if name in PER_SAMPLE:    # written outside every range: charged to the ray in front of it
            own = lay.owner_of_gap if g.ndim == 1 else np.broadcast_to(
                lay.owner_of_gap[:, None], g.shape)
            bad = (ray < 0) & (g32.view(np.int32) != sent.view(np.int32))
            for i in np.flatnonzero(bad.reshape(-1)):
                fails.append((int(own.reshape(-1)[i]), name, int(i), "written outside every range"))
        rr = np.maximum(ray, 0)
        ln = lay.len[rr].astype(np.float64)
        empty = (ray >= 0) & (lay.len[rr] == 0)
        bad = empty & (g != ref[name])       # colors == bg, last_trans == 1, depths == 0: exactly
        for i in np.flatnonzero(bad.reshape(-1)):
            fails.append((int(ray.reshape(-1)[i]), name, int(i), "empty ray: not the exact value"))
        tol = U * (ln * ref["msum"][name] + K * ref["mop"][name])
        err = np.abs(g - ref[name])
        bad = (ray >= 0) & ~empty & ~(err <= tol)
        for i in np.flatnonzero(bad.reshape(-1)):
            fails.append((int(ray.reshape(-1)[i]), name, int(i), "err %.3e > tol %.3e (ref %.6e)" % (
                err.reshape(-1)[i], tol.reshape(-1)[i], ref[name].reshape(-1)[i])))
    return fails


def composite_check(lay, case, got, fwd_ref, with_dw=True, K=K_COMPOSITE):
    """composite_failures of a full set of outputs: the forward's against fwd_ref, the backward's
    against the closed form on the weights and last_trans that `got` itself holds (they are the
    backward's inputs).  -> (failures, the merged reference)."""
    bwd = composite_bwd_ref(lay, case, got["weights"], got["last_trans"], with_dw)
    ref = merge_refs(fwd_ref, bwd)
    return composite_failures(lay, got, ref, K), ref


def assert_no_failures(fails, what=""):
    if fails:
        rays = sorted({f[0] for f in fails})
        raise AssertionError("%s: %d elements fail on %d rays; first: ray %d, %s[%d]: %s" % (
            (what, len(fails), len(rays)) + tuple(fails[0])))


# ---------------------------------------------------------------------------------- seg ops -------

def seg_sum_ref(lay, val):
    """val [n] or [n, vec] f32 -> (sum float64 [R(, vec)], bound = len_r u sum|x|)."""
    v = _np64(val)
    shape = (lay.n_rays,) + v.shape[1:]
    out, bound = np.zeros(shape), np.zeros(shape)
    for r in range(lay.n_rays):
        s, e = int(lay.start[r]), int(lay.end[r])
        out[r] = v[s:e].sum(0)
        bound[r] = (e - s) * U * np.abs(v[s:e]).sum(0)
    return out, bound


def seg_sum_bwd_ref(lay, dsum):
    """the copy dval[i] = dsum[ray of i] as f32, SENTINEL outside the ranges (bit-equal)."""
    d = dsum.detach().cpu().numpy().astype(np.float32)
    out = np.full((lay.n_total,) + d.shape[1:], SENTINEL, dtype=np.float32)
    out[lay.inside] = d[lay.ray_of[lay.inside]]
    return out


def seg_scan_ref(lay, val, include_this, backward=False, mutant=None):
    """FlexAccumulateSum forward (prefix sums) or backward (suffix sums) in float64 ->
    (out [n] SENTINEL outside, bound [n] = len_r u sum|x| over the terms of the element)."""
    assert mutant in (None, "scan_carry")
    v = _np64(val)
    out, bound = np.full(lay.n_total, SENTINEL), np.zeros(lay.n_total)

    def scan(a):
        c = np.cumsum(a)
        return c if include_this else c - a

    for r in range(lay.n_rays):
        s, e = int(lay.start[r]), int(lay.end[r])
        if e <= s:
            continue
        a = v[s:e][::-1] if backward else v[s:e]     # the backward's strides start at the ray's end
        res = _stride_local(a, scan) if mutant == "scan_carry" else scan(a)
        bnd = (e - s) * U * scan(np.abs(a))
        out[s:e] = res[::-1] if backward else res
        bound[s:e] = bnd[::-1] if backward else bnd
    return out, bound


def segment_inputs(lay, seed=3):
    """val [n] ~ N(0, 1) for the sums and scans, and for weight_var w [n] = U(0.5, 1.5) / len_r
    (every sample of a ray counts, the last one included) with dvars [R] ~ N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    val = torch.randn(lay.n_total, generator=g)
    w = torch.rand(lay.n_total, generator=g) + 0.5
    w = (w / torch.from_numpy(np.maximum(lay.len_of, 1)).float()).contiguous()
    return val, w, torch.randn(lay.n_rays, generator=g)


def weight_var_ref(lay, w, dvars=None, mutant=None):
    """WeightVarLoss forward and, with dvars, backward as the reference codes it (quirk Q9:
    dw_i = g (b_i^2 - tmp x_i / wsum), tmp = 2 sum w_j b_j), float64, x_i = i / 16.
    -> dict var [R], dw [n] (SENTINEL outside), m_var, m_dw: conditioning numbers for
    tol = (len_r + K) u M (M_sum = M_op = M)."""
    assert mutant in (None, "var_tail")
    wv = _np64(w)
    R = lay.n_rays
    res = dict(var=np.zeros(R), m_var=np.zeros(R), dw=np.full(lay.n_total, SENTINEL),
               m_dw=np.zeros(lay.n_total))
    g = None if dvars is None else _np64(dvars)
    for r in range(R):
        s, e = int(lay.start[r]), int(lay.end[r])
        if e <= s:
            continue
        m = (e - s) // WAVE * WAVE if mutant == "var_tail" else e - s   # samples the sums see
        x = np.arange(e - s, dtype=np.float64) / 16.0
        ww = wv[s:e]
        wsum = 1e-6 + ww[:m].sum()
        mean = (ww[:m] * x[:m]).sum() / wsum
        b = x - mean
        res["var"][r] = (ww[:m] * b[:m] * b[:m]).sum()
        a_mean = (np.abs(ww) * x).sum() / wsum           # magnitude of the mean's terms
        m_mean = a_mean + abs(mean)                      # numerator's sum, denominator's sum
        awb = (np.abs(ww) * np.abs(b)).sum()
        tmp = 2.0 * (ww[:m] * b[:m]).sum()
        # d var / d mean = -tmp, which is 2e-6 mean at the weighted mean: the mean's error enters
        # through that factor only; what is left is the sum of the terms w b^2 themselves
        res["m_var"][r] = (np.abs(ww) * b * b).sum() + abs(tmp) * m_mean
        if g is not None:
            res["dw"][s:e] = g[r] * (b * b - tmp * x / wsum)
            m_tmp = 2.0 * (awb + np.abs(ww).sum() * m_mean)     # tmp = 2 sum w b cancels to ~0
            res["m_dw"][s:e] = abs(g[r]) * (b * b + 2.0 * np.abs(b) * m_mean + x / wsum * m_tmp)
    return res


# ---------------------------------------------------------------------------------- density scan --

SCAN_S = (1, 63, 64, 65, 100, 128, 1024)
SCAN_C = (8, 16, 32, 64, 128)
SCAN_THRESH = 1e-4
SCAN_RAYS_PER_TARGET = 3


def scan_targets(S):
    """kept counts the rays of a density_scan case are built to stop at (kept >= 1 always: the
    exclusive depth of sample 0 is 0; kept = 0 needs t_thresh >= 1 and is asserted apart)."""
    return sorted({m for m in (1, 63, 64, 65, S - 1, S) if 1 <= m <= S})


def density_scan_case(S, C, seed=0):
    """Channel-major encoding [C, n_rays S], dt, w0, b0 (f32 torch) and target [n_rays]: ray r is
    scaled (a per-ray density scale ln c_r / w0[0] added to channel 0) so that its transmittance
    crosses the threshold in the middle of sample target_r - 1; target S: it never does."""
    g = torch.Generator().manual_seed(77 * S + C + seed)
    targets = scan_targets(S)
    target = np.repeat(np.array(targets, dtype=np.int64), SCAN_RAYS_PER_TARGET)
    target = np.concatenate([target, [S]])        # + 1: the last block is not full
    R = target.shape[0]
    n = R * S
    enc = torch.randn(C, n, generator=g) * 0.3
    w0 = torch.randn(C, generator=g) * (0.8 / math.sqrt(C))
    w0[0] = 0.5
    b0 = torch.tensor([0.5])
    dt = torch.rand(n, generator=g) * 0.03 + 0.01
    limit = -math.log(float(np.float32(SCAN_THRESH)))
    logit = (b0.double() + (enc.double() * w0.double()[:, None]).sum(0)).numpy()
    sec = (np.exp(logit - DENSITY_SHIFT) * dt.double().numpy()).reshape(R, S)
    for r in range(R):
        m = int(target[r])
        if m == S:
            c = 0.5 * limit / sec[r].sum()
        else:   # sum of the first m-1 plus half of sample m-1 = the limit
            c = limit / (sec[r, :m - 1].sum() + 0.5 * sec[r, m - 1])
        enc[0, r * S:(r + 1) * S] += math.log(c) / 0.5
    return dict(enc=enc.contiguous(), dt=dt, w0=w0, b0=b0, target=target, n_rays=R, S=S, C=C)


def density_scan_ref(case, thresh=SCAN_THRESH):
    """kept [R] by the float64 rule, and in_band [R]: some sample's exclusive depth lies within the
    any-order f32 bound of the decision -ln(thresh): band_k = u (k depth_k + sum_{j<k} sec_j e_j + 4)
    with e_j = (C + 1) A_j + |x_j| + 4 the relative error of sec_j (A_j = |b0| + sum_c |enc w0|, the
    magnitude of the FMA chain; x_j = logit_j - shift; 4: the two expf's and the product)."""
    R, S, C = case["n_rays"], case["S"], case["C"]
    enc, w0 = case["enc"].double().numpy(), case["w0"].double().numpy()
    b0 = float(case["b0"][0])
    prod = enc * w0[:, None]
    logit = b0 + prod.sum(0)
    A = abs(b0) + np.abs(prod).sum(0)
    x = logit - DENSITY_SHIFT
    sec = (np.exp(x) * case["dt"].double().numpy()).reshape(R, S)
    e_rel = ((C + 1) * A + np.abs(x) + 4.0).reshape(R, S)
    return keep_rule(sec, e_rel, thresh)


def keep_rule(sec, e_rel, thresh=SCAN_THRESH):
    """The keep decision of density_scan_ref on sec [R, S] (float64; 0 where a sample contributes
    nothing) with the relative error e_rel [R, S] of each sec, in units of u -> kept [R], in_band [R].
    tests/render_model.py applies it to the one-pass render's chain."""
    S = sec.shape[1]
    depth = np.cumsum(sec, 1) - sec
    limit = -math.log(float(np.float32(thresh)))
    keep = np.exp(-depth) > float(np.float32(thresh))
    kept = np.where(keep.all(1), S, np.argmin(keep, 1)).astype(np.int32)
    k = np.arange(S, dtype=np.float64)[None, :]
    band = U * (k * depth + (np.cumsum(sec * e_rel, 1) - sec * e_rel) + 4.0)
    in_band = (np.abs(depth - limit) <= band).any(1)
    return kept, in_band


# ---------------------------------------------------------------------------------- ray keys ------

KEY_CELL_BITS = 14


def hilbert_index(x, y, bits=KEY_CELL_BITS):
    """Index of cell (x, y) of a 2^bits x 2^bits grid along the Hilbert curve (numpy uint32)."""
    x, y = np.asarray(x, dtype=np.uint32).copy(), np.asarray(y, dtype=np.uint32).copy()
    d = np.zeros_like(x, dtype=np.uint32)
    s = np.uint32(1 << (bits - 1))
    while s > 0:
        rx, ry = ((x & s) != 0).astype(np.uint32), ((y & s) != 0).astype(np.uint32)
        d = d + s * s * ((np.uint32(3) * rx) ^ ry)
        reflect = (ry == 0) & (rx == 1)
        x, y = np.where(reflect, x ^ (s - np.uint32(1)), x), np.where(reflect, y ^ (s - np.uint32(1)), y)
        x, y = np.where(ry == 0, y, x), np.where(ry == 0, x, y)
        s = np.uint32(s >> 1)
    return d


def _quantise(u):
    """(u/2 + 1/2) 2^14 clamped to [0, 16383] and truncated, in f32 (the multiply by 1/2, the add and
    the power-of-two scale are exact or correctly rounded in numpy as on the device)."""
    q = (u * np.float32(0.5) + np.float32(0.5)) * np.float32(1 << KEY_CELL_BITS)
    return np.clip(q, np.float32(0.0), np.float32((1 << KEY_CELL_BITS) - 1)).astype(np.uint32)


def ray_keys_ref(d):
    """f2n_ray_keys restated in numpy f32: d [n, 3] -> int32 keys.  The dominant axis (ties: x over
    y over z, `>=`), u and v = the next two components cyclically over |d_axis|, each quantised to 14
    bits, the pair in Hilbert order, face = 2 axis + (d_axis < 0) in bits 28-30.  A zero direction
    or one with an infinite or NaN component has key 0."""
    d = np.asarray(d, dtype=np.float32)
    n = d.shape[0]
    a = np.abs(d)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ax = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0,
                      np.where(a[:, 1] >= a[:, 2], 1, 2))
        rows = np.arange(n)
        m = a[rows, ax]
        ok = (m > 0) & (m <= np.float32(3.4e38)) & ~np.isnan(a).any(1)
        msafe = np.where(ok, m, np.float32(1.0))
        dz = np.where(ok[:, None], d, np.float32(0.0))
        u = dz[rows, (ax + 1) % 3] / msafe
        v = dz[rows, (ax + 2) % 3] / msafe
        face = (2 * ax + (d[rows, ax] < 0)).astype(np.uint32)
        key = (face << np.uint32(2 * KEY_CELL_BITS)) | hilbert_index(_quantise(u), _quantise(v))
    return np.where(ok, key, np.uint32(0)).astype(np.int32)
