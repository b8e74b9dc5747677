"""Inputs, float64 references, per-element bounds and mutants for the distortion-loss kernels
(f2n_weight_dist_fwd / f2n_weight_dist_bwd: one 64-lane wavefront per ray, 64-sample strides, two
scalar carries P and Q between strides).  No tests in here: tests/test_dist_cases_cpu.py checks on the
CPU that the assertions built from this module accept an f32 restatement of the kernels' O(n) form
and reject every mutant, tests/test_gpu_weight_dist.py makes them against the HIP kernels.

Inputs.  tests/ragged_cases.py's layouts ("tile", "gaps", "unordered": 72 rays of the stride-edge
lengths at four optical depths, 32 176 samples).  The weights are the float64 compositing weights of
ragged_cases.composite_case rounded to f32, so every stride of a tau = 0.7 or 3 ray carries weight; dt
is that case's dt; t (the interval END) is a per-ray running sum from an offset of up to 5 (every
fourth ray: exactly 5):
    "contiguous"  t_k - t_{k-1} = dt_k;
    "thinned"     about a fifth of the steps are dt_k (1 + J), J in [3, 40): the list neighbours an
                  occupancy grid leaves behind, far apart without dt growing.
The f32 t is then raised by single ulps wherever its rounding would make the midpoint m = t - dt/2
(exact in float64) step back: the kernels' precondition, m non-decreasing, holds for the f32 inputs
exactly and dist_case asserts it.  Samples outside the ranges hold ordinary values; dw is pre-filled
with SENTINEL by the callers.

Reference.  dist_ref: the literal double sum D_r = sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 dt_i and
dD_r/dw_i = 2 sum_j w_j |m_i - m_j| + 2/3 w_i dt_i in float64 on the f32 inputs, O(n^2) -- on purpose
NOT the prefix-sum algebra the kernels use.  closed_form_one / closed_form_two anchor it.

Bound of an element of ray r:   tol = u (len_r M_sum + K M_op),   u = 2^-24.
With x_i = m_i - m_s >= 0, P_i = sum_{j<i} w_j, Q_i = sum_{j<i} w_j x_j (float64, of |w|):
  forward   D = sum_i [2 w_i (x_i P_i - Q_i) + 1/3 w_i^2 dt_i] is a sum of len_r terms whose P_i, Q_i are
            themselves sums of up to len_r terms; the any-order bound len u sum|terms| applies once to
            the prefix sums and once to the outer sum, so
            M_sum = 2 sum_i 2 w_i (x_i P_i + Q_i) + sum_i 1/3 w_i^2 dt_i;
  backward  g_i = 2 [(x_i P_i - Q_i) + (Q_tot - Q_<=i) - x_i (P_tot - P_<=i)] + 2/3 w_i dt_i: four sums,
            no outer one,  M_sum_i = |d_out| 2 [x_i P_i + Q_i + Q_tot + Q_<=i + x_i (P_tot + P_<=i)];
  M_op      the same magnitudes once (the products, subtractions and the final scale: K counts
            them) plus the self term, plus what the anchored positions carry: x_i is known to
            u e_i, e_i = |m_i| + |m_s| + |x_i| (m_i rounded, m_s rounded, one subtraction), which enters
            wherever x_i does: e_i in place of x_i, E = prefix sums of w e in place of Q.
K is MEASURED on the CPU against dist_f32 -- an f32 numpy restatement of the O(n) form, serial and
in 64-sample strides with carries -- never against the HIP kernels
(tests/test_dist_cases_cpu.py::test_measured_K): the largest (err / u - len_r M_sum) / M_op over all
elements, layouts and t variants; K_DIST = 4 x that, rounded up to a power of two, as
ragged_cases fixes K_COMPOSITE (4: the device fuses multiply-adds where numpy does not, and its DPP
tree adds in another order).

    measured, "tile" / "gaps" / "unordered", larger of the two t variants (serial and strided agree
    to the digits shown: the largest ratios sit on rays of one or two samples, where there is no sum
    to re-order; on longer rays len_r M_sum alone covers the error and the ratio is negative):
      forward   0.046 / 0.244 / 0.083,   backward  0.078 / 0.164 / 0.070,
      rays of length <= 2 alone: 0.078 / 0.244 / 0.083.
    The largest is 0.244: 4 x 0.244 = 0.98 rounds up to K_DIST = 1.

Mutants (CPU only, one defect each; float64 except dist_anchor): see DIST_MUTANTS.
  dist_carry   the P, Q carry is dropped at every stride boundary
  dist_suffix  the backward's suffix half takes its totals from the sample's own stride
  dist_tail    the last partial stride is treated as full (reads past the ray's end)
  dist_self    the 1/3, 2/3 self term is missing
  dist_mid     t is used in place of the midpoint
  dist_anchor  no anchoring at the ray's first midpoint.  In float64 that changes nothing, so this
               one is dist_f32 (serial) with x_i = m_i: the defect is the f32 cancellation it causes,
               and it shows through the bound on rays that start at an offset that is large against
               their extent: contiguous rays at the offsets of up to 5, thinned rays (tens of units
               long) once they are moved 50 further out (far_case).
"""
import functools

import numpy as np
import torch

from tests import ragged_cases as rc

U = rc.U
SENTINEL = rc.SENTINEL
WAVE = rc.WAVE
T_VARIANTS = ("contiguous", "thinned")
DIST_MUTANTS = ("dist_carry", "dist_suffix", "dist_tail", "dist_self", "dist_mid", "dist_anchor")
K_DIST = 1               # see the module docstring; test_measured_K re-derives it
MAX_OFFSET = 5.0
FAR_OFFSET = 50.0         # far_case: the anchoring check on thinned rays


# ---------------------------------------------------------------------------------- inputs --------

def _midpoints64(t32, dt32):
    return t32.astype(np.float64) - 0.5 * dt32.astype(np.float64)


def _hold_precondition(lay, t, dt):
    """the precondition, exactly, for the f32 inputs: where rounding t made m step back, t is raised
    by single ulps until it does not"""
    same_ray = lay.inside[1:] & (lay.ray_of[1:] == lay.ray_of[:-1])
    for _ in range(4096):
        m = _midpoints64(t, dt)
        back = np.flatnonzero(same_ray & (m[1:] < m[:-1])) + 1
        if back.size == 0:
            break
        t[back] = np.nextafter(t[back], np.float32(np.inf))
    m = _midpoints64(t, dt)
    assert not (same_ray & (m[1:] < m[:-1])).any(), "m must be non-decreasing along every ray"
    return t


def far_case(lay, case, extra=FAR_OFFSET):
    """`case` with every ray moved `extra` further out (t + extra, rounded to f32 again, the
    precondition held again): rays whose offset is large against their extent even when thinned.  For
    the anchoring contract alone (tests/test_dist_cases_cpu.py); K is not measured on it."""
    t = (case["t"].numpy().astype(np.float64) + extra).astype(np.float32)
    far = dict(case)
    far["t"] = torch.from_numpy(_hold_precondition(lay, t, case["dt"].numpy()))
    far["offset"] = case["offset"] + extra
    return far


def dist_case(lay, variant, seed=rc.CASE_SEED):
    """f32 inputs on a Layout -> dict of torch CPU tensors: weights, t, dt [n_total], d_out [R]."""
    assert variant in T_VARIANTS
    case = rc.composite_case(lay, seed)
    fwd = rc.composite_fwd_ref(lay, case)
    rng = np.random.RandomState(4000 + seed + (17 if variant == "thinned" else 0))
    n, R = lay.n_total, lay.n_rays
    w = fwd["weights"].copy()
    w[~lay.inside] = 0.01 * rng.rand(int((~lay.inside).sum()))
    w = w.astype(np.float32)
    dt = case["dt"].numpy().astype(np.float32)
    step = dt.astype(np.float64)
    if variant == "thinned":
        jump = rng.rand(n) < 0.2
        step = step * (1.0 + jump * (3.0 + 37.0 * rng.rand(n)))
    offset = rng.rand(R) * MAX_OFFSET
    offset[::4] = MAX_OFFSET
    t = 1.0 + 3.0 * rng.rand(n)                       # outside the ranges: ordinary values
    for r in range(R):
        s, e = int(lay.start[r]), int(lay.end[r])
        t[s:e] = offset[r] + np.cumsum(step[s:e])
    t = t.astype(np.float32)
    t = _hold_precondition(lay, t, dt)
    g = torch.Generator().manual_seed(500 + seed)
    return dict(weights=torch.from_numpy(w), t=torch.from_numpy(t), dt=torch.from_numpy(dt),
                d_out=torch.randn(R, generator=g), offset=offset)


# ---------------------------------------------------------------------------------- reference -----

def closed_form_one(w, dt):
    """a single sample: D = 1/3 w^2 dt, dD/dw = 2/3 w dt"""
    return w * w * dt / 3.0, np.array([2.0 * w * dt / 3.0])


def closed_form_two(w, m, dt):
    """two samples: D = 2 w0 w1 (m1 - m0) + 1/3 (w0^2 dt0 + w1^2 dt1)"""
    gap = abs(m[1] - m[0])
    D = 2.0 * w[0] * w[1] * gap + (w[0] ** 2 * dt[0] + w[1] ** 2 * dt[1]) / 3.0
    g = np.array([2.0 * w[1] * gap + 2.0 * w[0] * dt[0] / 3.0,
                  2.0 * w[0] * gap + 2.0 * w[1] * dt[1] / 3.0])
    return D, g


def double_sum(w, m, dt, rows=1024):
    """The definition, literally: (D, dD/dw) of one ray in float64, O(n^2)."""
    n = w.shape[0]
    D, g = 0.0, np.empty(n)
    for i0 in range(0, n, rows):
        i1 = min(n, i0 + rows)
        aw = np.abs(m[i0:i1, None] - m[None, :]) @ w
        D += float(w[i0:i1] @ aw)
        g[i0:i1] = 2.0 * aw
    return D + float((w * w * dt).sum()) / 3.0, g + 2.0 * w * dt / 3.0


def _excl(a):
    c = np.cumsum(a)
    return c - a


def dist_ref(lay, case):
    """-> dict D [R], dw [n_total] (= d_out[r] dD_r/dw, SENTINEL outside the ranges) in float64 by
    the double sum, and 'msum' / 'mop': the conditioning numbers of each (module docstring)."""
    w_all, dt_all = rc._np64(case["weights"]), rc._np64(case["dt"])
    m_all = _midpoints64(case["t"].numpy(), case["dt"].numpy())
    d_out = rc._np64(case["d_out"])
    R, n = lay.n_rays, lay.n_total
    out = dict(D=np.zeros(R), dw=np.full(n, SENTINEL))
    msum = dict(D=np.zeros(R), dw=np.zeros(n))
    mop = dict(D=np.zeros(R), dw=np.zeros(n))
    for r in range(R):
        s, e = int(lay.start[r]), int(lay.end[r])
        if e <= s:
            continue
        w, m, dt = w_all[s:e], m_all[s:e], dt_all[s:e]
        D, g = double_sum(w, m, dt)
        out["D"][r] = D
        out["dw"][s:e] = d_out[r] * g
        aw = np.abs(w)
        x = m - m[0]
        err = np.abs(m) + abs(m[0]) + np.abs(x)           # x_i is known to u err_i
        P, Q, E = _excl(aw), _excl(aw * x), _excl(aw * err)
        Pi, Qi, Ei = P + aw, Q + aw * x, E + aw * err
        Pt, Qt, Et = Pi[-1], Qi[-1], Ei[-1]
        self_f, self_b = aw * aw * dt / 3.0, 2.0 * aw * dt / 3.0
        pair = 2.0 * aw * (x * P + Q)
        msum["D"][r] = 2.0 * pair.sum() + self_f.sum()
        mop["D"][r] = pair.sum() + self_f.sum() + (2.0 * aw * (err * P + E)).sum()
        four = 2.0 * (x * P + Q + Qt + Qi + x * (Pt + Pi))
        pos = 2.0 * (err * P + E + Et + Ei + err * (Pt + Pi))
        msum["dw"][s:e] = abs(d_out[r]) * four
        mop["dw"][s:e] = abs(d_out[r]) * (four + self_b + pos)
    out["msum"], out["mop"] = msum, mop
    return out


@functools.lru_cache(maxsize=None)
def shared(layout_name, variant):
    """(Layout, case, reference) of one layout and t variant, computed once per process and shared:
    nobody writes into them."""
    lay = rc.layout(layout_name)
    case = dist_case(lay, variant)
    return lay, case, dist_ref(lay, case)


# ---------------------------------------------------------------------------------- O(n) forms ----

def _prefix(a, strided, carry=True):
    """exclusive and inclusive prefix sums of a, in a's dtype: serial, or per 64-sample stride with
    a scalar carry between strides (carry = False: the carry is dropped)."""
    if not strided:
        incl = np.cumsum(a, dtype=a.dtype)
        return np.concatenate([[a.dtype.type(0)], incl[:-1]]), incl
    excl, incl = np.empty_like(a), np.empty_like(a)
    c = a.dtype.type(0)
    for lo in range(0, a.shape[0], WAVE):
        loc = np.cumsum(a[lo:lo + WAVE], dtype=a.dtype)
        incl[lo:lo + WAVE] = c + loc
        excl[lo:lo + WAVE] = c + np.concatenate([[a.dtype.type(0)], loc[:-1]])
        if carry:
            c = c + loc[-1]
    return excl, incl


def _total(a, strided):
    """sum of a in its dtype: serial, or one accumulator per lane over the strides, then the lanes"""
    if not strided:
        return np.cumsum(a, dtype=a.dtype)[-1]
    pad = np.zeros(-(-a.shape[0] // WAVE) * WAVE, dtype=a.dtype)
    pad[:a.shape[0]] = a
    lanes = np.add.reduce(pad.reshape(-1, WAVE), axis=0, dtype=a.dtype)
    return np.cumsum(lanes, dtype=a.dtype)[-1]


def dist_linear(lay, case, dtype=np.float64, strided=True, mutant=None):
    """The kernels' O(n) form in `dtype` -> dict D [R], dw [n_total] (SENTINEL outside).  float32:
    the restatement K is measured on (every operation rounded as the kernels round it, up to fused
    multiply-adds and the order inside a stride).  mutant: one of DIST_MUTANTS (module docstring)."""
    assert mutant in (None,) + DIST_MUTANTS
    if mutant == "dist_anchor":
        dtype, strided = np.float32, False
    f = dtype
    w_all = case["weights"].numpy().astype(f)
    t_all, dt_all = case["t"].numpy().astype(f), case["dt"].numpy().astype(f)
    d_out = case["d_out"].numpy().astype(f)
    R, n = lay.n_rays, lay.n_total
    out = dict(D=np.zeros(R, dtype=f), dw=np.full(n, SENTINEL, dtype=f))
    third, two = f(1.0) / f(3.0), f(2.0)
    for r in range(R):
        s, e = int(lay.start[r]), int(lay.end[r])
        if e <= s:
            continue
        e_sum = e
        if mutant == "dist_tail":
            e_sum = min(s + -(-(e - s) // WAVE) * WAVE, n)
        w, dt = w_all[s:e_sum], dt_all[s:e_sum]
        m = t_all[s:e_sum] if mutant == "dist_mid" else t_all[s:e_sum] - f(0.5) * dt
        x = m if mutant == "dist_anchor" else m - m[0]
        wx = w * x
        carry = mutant != "dist_carry"
        P, Pi = _prefix(w, strided or not carry, carry)
        Q, Qi = _prefix(wx, strided or not carry, carry)
        before = x * P - Q
        self_f = w * w * dt * (f(0.0) if mutant == "dist_self" else f(1.0))
        out["D"][r] = two * _total(w * before, strided) + _total(self_f, strided) * third
        Pt, Qt = _total(w, strided), _total(wx, strided)
        if mutant == "dist_suffix":       # totals of the sample's own stride only
            Pt, Qt = np.empty_like(w), np.empty_like(w)
            for lo in range(0, w.shape[0], WAVE):
                Pt[lo:lo + WAVE] = Pi[min(lo + WAVE, w.shape[0]) - 1]
                Qt[lo:lo + WAVE] = Qi[min(lo + WAVE, w.shape[0]) - 1]
        after = (Qt - Qi) - x * (Pt - Pi)
        self_b = (f(0.0) if mutant == "dist_self" else two * third) * w * dt
        g = d_out[r] * (two * (before + after) + self_b)
        out["dw"][s:e] = g[:e - s]
    return out


def dist_f32(lay, case, strided):
    return dist_linear(lay, case, np.float32, strided)


# ---------------------------------------------------------------------------------- assertions ----

def _ray_index(lay, name):
    return np.arange(lay.n_rays) if name == "D" else lay.ray_of


def ratios(lay, got, ref):
    """(err / u - len_r M_sum) / M_op per element inside the ranges (what K has to cover):
    dict name -> (ratio array, ray index array)."""
    res = {}
    for name in ("D", "dw"):
        if name not in got:
            continue
        g = np.asarray(got[name], dtype=np.float64)
        ray = _ray_index(lay, name)
        sel = (ray >= 0) & (lay.len[np.maximum(ray, 0)] > 0)
        err = np.abs(g - ref[name])[sel]
        ln = lay.len[ray[sel]].astype(np.float64)
        res[name] = (rc.safe_ratio(err / U - ln * ref["msum"][name][sel], ref["mop"][name][sel]),
                     ray[sel])
    return res


def dist_failures(lay, got, ref, K=K_DIST):
    """Every assertion the GPU test makes on the outputs 'D' [R] and / or 'dw' [n_total] (f32; dw
    pre-filled with SENTINEL), as a list of (ray, output name, element index, message)."""
    fails = []
    sent = np.float32(SENTINEL)
    for name, g32 in got.items():
        g32 = np.asarray(g32, dtype=np.float32)
        assert g32.shape == ref[name].shape, (name, g32.shape, ref[name].shape)
        g = g32.astype(np.float64)
        ray = _ray_index(lay, name)
        if name == "dw":
            bad = (ray < 0) & (g32.view(np.int32) != sent.view(np.int32))
            for i in np.flatnonzero(bad):
                fails.append((int(lay.owner_of_gap[i]), name, int(i), "written outside every range"))
        rr = np.maximum(ray, 0)
        empty = (ray >= 0) & (lay.len[rr] == 0)
        for i in np.flatnonzero(empty & (g != 0.0)):
            fails.append((int(ray[i]), name, int(i), "empty ray: not exactly 0"))
        tol = U * (lay.len[rr] * ref["msum"][name] + K * ref["mop"][name])
        err = np.abs(g - ref[name])
        for i in np.flatnonzero((ray >= 0) & ~empty & ~(err <= tol)):
            fails.append((int(ray[i]), name, int(i), "err %.3e > tol %.3e (ref %.6e)" % (
                err[i], tol[i], ref[name][i])))
    return fails
