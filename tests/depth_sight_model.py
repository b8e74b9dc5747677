"""Inputs, float64 model, per-element bounds and mutants for the line-of-sight depth kernels
(f2n_depth_sight_fwd / f2n_depth_sight_bwd: one 64-lane wavefront per ray, 64-sample strides, one
accumulator per lane and sum, a DPP reduction after the strided loop).  No tests in here:
tests/test_depth_sight_model_cpu.py checks on the CPU that the assertions built from this module accept
an f32 restatement of the kernels' order and reject every mutant; tests/test_gpu_depth_sight.py and
tests/test_gpu_depth_routes.py make them against the HIP kernels.  Method and layouts follow
tests/dist_cases.py / tests/ragged_cases.py.

Inputs.  sight_layout: one ray for every length in LENGTHS (the edges of a 64-sample stride walk: 0, 1,
2, 63, 64, 65, 129, 200) and every target kind in KINDS, shuffled; "tile" (the ranges tile the array) or
"gaps" (0 / 1 / 5 unused samples between rays, first and last ray empty, 64 behind the last).  Weights
are positive and sum to an opacity in [0.5, 1] per ray, so every stride of every ray carries weight; dt
in [0.005, 0.025]; t (the interval END) is a per-ray running sum from an offset in [0.5, 3]:
    "contiguous"  t_k - t_{k-1} = dt_k;
    "thinned"     about a fifth of the steps are dt_k (1 + J), J in [3, 40): the neighbours an occupancy
                  grid leaves behind.
Samples outside the ranges hold ordinary values; dw is pre-filled with SENTINEL by the callers.
Targets z [R] f32 by kind, for the call's eps (EPS_VALUES = 0 and 0.03), m32 = f32(t - 0.5 dt):
    "before"    z in front of every sample (below m32[0] - eps): every sample lies behind the band;
    "beyond"    z behind every sample: every sample is front;
    "inside"    z = m32[len // 2] exactly: with eps = 0 that sample IS the band (m == lo == hi);
    "straddle"  z = m32[min(63, len - 1)]: with eps = 0.03 the band holds samples on both sides of the
                boundary between the first and the second stride (rays longer than 64);
    "edge"      eps > 0: z such that f32(z - eps) == m32[j] exactly, j = len // 3: a sample ON the lower
                boundary belongs to the band (eps = 0: as "inside", at j);
    "zero", "neg", "nan", "inf"   invalid rays: z = 0, -1.5, NaN, +inf.
An empty ray of a valid kind has z = 1.5.

Model.  sight_ref: membership by the kernels' own f32 comparisons (m32 < lo32, m32 >= lo32 and m32 <=
hi32, with lo32 = f32(z - eps), hi32 = f32(z + eps)); the sums E = sum_front w^2, W = sum_band w, d = sum
w m in float64 with m = t - dt / 2 exact; out = (E, (1 - W)^2, (d - z)^2); dw = g0 2 w [front] - g1 2 (1 -
W) [band] + g2 2 (d - z) m.  An invalid ray: out = 0 and dw = 0 over its range.  brute_force restates
this sample by sample in Python floats; central differences check dw.

Bound of an element of ray r:   tol = u (len_r M_sum + K M_op),   u = 2^-24, counted from the header
comment of depth_sight.hip.  With S_b = sum_band |w|, S_m = sum |w m|, a = 1 - W, x = d - z:
  E        a sum of len_r products:              M_sum = M_op = sum_front w^2
  N = a^2  W is a sum (len u S_b), a one rounding, the square one:
                                                 M_sum = 2 |a| S_b,  M_op = 3 a^2 + u (len S_b + |a|)^2
           (the last term is the square of a's own error: what is left when a itself is ~0)
  X = x^2  d is a sum of products of w with m, m one rounding each (u S_m, not times len):
                                                 M_sum = 2 |x| S_m,
                                                 M_op = 2 |x| (S_m + |x|) + x^2 + u ((len + 1) S_m + |x|)^2
  dw_k     c1 = g1 2a and c2 = g2 2x inherit the sums' errors, then one product and one FMA:
           M_sum = [band] 2 |g1| S_b + |m_k| 2 |g2| S_m
           M_op  = [front] |2 g0 w_k| + [band] (2 |g1 a| + |c1|) + |m_k| (2 |g2| (S_m + |x|) + 2 |c2|)
                   + |dw_k|
K is MEASURED on the CPU against sight_f32 -- an f32 numpy restatement, serial and in the kernel's
strided order (per-lane accumulators over the strides, then the lanes) -- never against the HIP
kernels (test_measured_K): K_SIGHT = 4 x the largest (err / u - len_r M_sum) / M_op, rounded up to a
power of two (the device fuses multiply-adds where numpy does not, and its DPP tree adds the lanes in
another order).
    measured (layouts tile / gaps, both t variants, both eps; serial and strided agree to the digits):
      out 0.117 / 0.230,  dw 0.164 / 0.258;   4 x 0.258 = 1.03 rounds up to K_SIGHT = 2.

Mutants (CPU only, float64, one defect each): see SIGHT_MUTANTS.
  sight_carry_w  W keeps only what the lanes saw last (the accumulator is overwritten at every stride)
  sight_carry_d  the same for d
  sight_tail     the last partial stride is ignored (sums and dw)
  sight_edge     front is m <= lo instead of m < lo: a sample on the boundary changes sides
  sight_invalid  an invalid ray's range of dw is left unwritten
  sight_mid      t is used in place of the midpoint
"""
import functools

import numpy as np
import torch

from tests import ragged_cases as rc

U = rc.U
SENTINEL = rc.SENTINEL
WAVE = rc.WAVE
LENGTHS = (0, 1, 2, 63, 64, 65, 129, 200)
VALID_KINDS = ("before", "beyond", "inside", "straddle", "edge")
INVALID_KINDS = ("zero", "neg", "nan", "inf")
KINDS = VALID_KINDS + INVALID_KINDS
LAYOUTS = ("tile", "gaps")
T_VARIANTS = ("contiguous", "thinned")
EPS_VALUES = (0.0, 0.03)
SIGHT_MUTANTS = ("sight_carry_w", "sight_carry_d", "sight_tail", "sight_edge", "sight_invalid",
                 "sight_mid")
K_SIGHT = 2              # see the module docstring; test_measured_K re-derives it
F32 = np.float32


# ---------------------------------------------------------------------------------- inputs --------

class SightLayout(rc.Layout):
    """rc.Layout plus kind [n_rays]: the target kind of every ray."""

    def __init__(self, bounds, n_total, kinds):
        super().__init__(bounds, np.ones(bounds.shape[0]), n_total)
        self.kind = kinds


@functools.lru_cache(maxsize=None)
def sight_layout(name, seed=0):
    assert name in LAYOUTS
    rng = np.random.RandomState(70 + seed)
    pairs = [(l, k) for l in LENGTHS for k in KINDS]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    gaps = name == "gaps"
    if gaps:   # the first and the last ray are empty
        empties = [i for i, p in enumerate(pairs) if p[0] == 0]
        for pos, i in ((0, empties[0]), (len(pairs) - 1, empties[-1])):
            pairs[pos], pairs[i] = pairs[i], pairs[pos]
    lens = np.array([p[0] for p in pairs], dtype=np.int64)
    gap = rng.choice([0, 1, 5], size=len(pairs)) if gaps else np.zeros(len(pairs), dtype=np.int64)
    start = np.zeros(len(pairs), dtype=np.int64)
    pos = int(gap[0]) if gaps else 0
    for r in range(len(pairs)):
        start[r] = pos
        pos += int(lens[r]) + int(gap[r])
    n_total = pos + (WAVE if gaps else 0)
    bounds = torch.from_numpy(np.stack([start, start + lens], 1).astype(np.int32)).contiguous()
    return SightLayout(bounds, n_total, [p[1] for p in pairs])


def midpoints32(t32, dt32):
    """m as the kernels form it: 0.5f * dt is exact, one rounding"""
    return (t32 - F32(0.5) * dt32).astype(F32)


def _edge_target(m_j, eps):
    """z (f32) with f32(z - eps) == m_j exactly"""
    z = F32(m_j + eps)
    for _ in range(64):
        lo = F32(z - eps)
        if lo == m_j:
            return z
        z = np.nextafter(z, F32(np.inf) if lo < m_j else F32(-np.inf))
    raise AssertionError("no f32 target puts the band's lower edge on the sample")


def targets(lay, t32, dt32, eps):
    eps = F32(eps)
    z = np.zeros(lay.n_rays, dtype=F32)
    m_all = midpoints32(t32, dt32)
    for r in range(lay.n_rays):
        kind, n = lay.kind[r], int(lay.len[r])
        m = m_all[int(lay.start[r]):int(lay.end[r])]
        if kind in INVALID_KINDS:
            z[r] = {"zero": 0.0, "neg": -1.5, "nan": np.nan, "inf": np.inf}[kind]
        elif n == 0:
            z[r] = 1.5
        elif kind == "before":
            z[r] = F32(m[0] - F32(2) * eps - F32(0.05))
        elif kind == "beyond":
            z[r] = F32(m[-1] + F32(2) * eps + F32(0.05))
        elif kind == "inside":
            z[r] = m[n // 2]
        elif kind == "straddle":
            z[r] = m[min(WAVE - 1, n - 1)]
        else:
            z[r] = m[n // 3] if eps == 0 else _edge_target(m[n // 3], eps)
        assert kind in INVALID_KINDS or (np.isfinite(z[r]) and z[r] > 0), (kind, z[r])
    return z


def sight_case(lay, variant, eps, seed=0):
    """f32 inputs on a SightLayout -> dict of torch CPU tensors: weights, t, dt [n_total], z [R],
    d_out [R, 3], and eps (float)."""
    assert variant in T_VARIANTS
    rng = np.random.RandomState(9000 + seed + (17 if variant == "thinned" else 0))
    n, R = lay.n_total, lay.n_rays
    w = 0.01 * rng.rand(n) + 1e-4
    dt = 0.005 + 0.02 * rng.rand(n)
    step = dt.copy()
    if variant == "thinned":
        jump = rng.rand(n) < 0.2
        step = step * (1.0 + jump * (3.0 + 37.0 * rng.rand(n)))
    t = 1.0 + 3.0 * rng.rand(n)
    for r in range(R):
        s, e = int(lay.start[r]), int(lay.end[r])
        if e > s:
            raw = rng.rand(e - s) + 0.05
            w[s:e] = raw / raw.sum() * (0.5 + 0.5 * rng.rand())
            t[s:e] = 0.5 + 2.5 * rng.rand() + np.cumsum(step[s:e])
    w, t, dt = w.astype(F32), t.astype(F32), dt.astype(F32)
    z = targets(lay, t, dt, eps)
    g = torch.Generator().manual_seed(600 + seed)
    return dict(weights=torch.from_numpy(w), t=torch.from_numpy(t), dt=torch.from_numpy(dt),
                z=torch.from_numpy(z), d_out=torch.randn(R, 3, generator=g), eps=float(F32(eps)))


def ray_valid(z):
    z = np.asarray(z)
    return np.isfinite(z) & (z > 0)


def membership(m32, z, eps):
    """(front, band) of samples with f32 midpoints m32 for the f32 target z: the kernels' own
    comparisons, on the kernels' own f32 values"""
    lo, hi = F32(F32(z) - F32(eps)), F32(F32(z) + F32(eps))
    front = m32 < lo
    band = (m32 >= lo) & (m32 <= hi)
    return front, band


# ---------------------------------------------------------------------------------- model ---------

def sight_ref(lay, case, mutant=None):
    """-> dict out [R, 3], dw [n_total] (SENTINEL outside the ranges) in float64, and 'msum' / 'mop':
    the conditioning numbers of each (module docstring).  mutant: one of SIGHT_MUTANTS."""
    assert mutant in (None,) + SIGHT_MUTANTS
    w_all, dt_all = rc._np64(case["weights"]), rc._np64(case["dt"])
    t32, dt32 = case["t"].numpy(), case["dt"].numpy()
    m32_all = t32 if mutant == "sight_mid" else midpoints32(t32, dt32)
    m_all = t32.astype(np.float64) - (0.0 if mutant == "sight_mid" else 0.5) * dt_all
    z_all, g_all, eps = case["z"].numpy(), rc._np64(case["d_out"]), case["eps"]
    R, n = lay.n_rays, lay.n_total
    out = dict(out=np.zeros((R, 3)), dw=np.full(n, SENTINEL))
    msum = dict(out=np.zeros((R, 3)), dw=np.zeros(n))
    mop = dict(out=np.zeros((R, 3)), dw=np.zeros(n))
    for r in range(R):
        s, e = int(lay.start[r]), int(lay.end[r])
        ln = e - s
        if not ray_valid(z_all[r]):
            if mutant != "sight_invalid":
                out["dw"][s:e] = 0.0
            continue
        z = float(z_all[r])
        w, m = w_all[s:e], m_all[s:e]
        front, band = membership(m32_all[s:e], z_all[r], eps)
        if mutant == "sight_edge":
            lo = F32(z_all[r] - F32(eps))
            front, band = m32_all[s:e] <= lo, band & (m32_all[s:e] > lo)
        summed = np.ones(ln, dtype=bool)
        if mutant == "sight_tail":
            summed[(ln // WAVE) * WAVE:] = False
        last = np.arange(ln) + WAVE >= ln            # what each lane saw last
        in_w = summed & (last if mutant == "sight_carry_w" else True)
        in_d = summed & (last if mutant == "sight_carry_d" else True)
        E = float((w * w)[front & summed].sum())
        W = float(w[band & in_w].sum())
        d = float((w * m)[in_d].sum())
        a, x = 1.0 - W, d - z
        out["out"][r] = (E, a * a, x * x)
        g0, g1, g2 = g_all[r]
        c1, c2 = g1 * 2.0 * a, g2 * 2.0 * x
        dw = np.where(front, 2.0 * g0 * w, 0.0) - np.where(band, c1, 0.0) + c2 * m
        out["dw"][s:e][summed] = dw[summed]
        # conditioning
        aw, am = np.abs(w), np.abs(m)
        S_b, S_m = float(aw[band].sum()), float((aw * am).sum())
        msum["out"][r] = (E, 2.0 * abs(a) * S_b, 2.0 * abs(x) * S_m)
        mop["out"][r] = (E, 3.0 * a * a + U * (ln * S_b + abs(a)) ** 2,
                         2.0 * abs(x) * (S_m + abs(x)) + x * x + U * ((ln + 1) * S_m + abs(x)) ** 2)
        msum["dw"][s:e] = np.where(band, 2.0 * abs(g1) * S_b, 0.0) + am * 2.0 * abs(g2) * S_m
        mop["dw"][s:e] = (np.where(front, np.abs(2.0 * g0 * w), 0.0) +
                          np.where(band, 2.0 * abs(g1 * a) + abs(c1), 0.0) +
                          am * (2.0 * abs(g2) * (S_m + abs(x)) + 2.0 * abs(c2)) + np.abs(dw))
    out["msum"], out["mop"] = msum, mop
    return out


def brute_force(w, t, dt, z, eps, g):
    """The definition of one ray, sample by sample in Python floats on f32 inputs:
    ((E, N, X), dw) or ((0, 0, 0), zeros) for an invalid ray."""
    n = len(w)
    if not (np.isfinite(z) and z > 0):
        return (0.0, 0.0, 0.0), [0.0] * n
    lo, hi = F32(F32(z) - F32(eps)), F32(F32(z) + F32(eps))
    E = W = d = 0.0
    side = []
    for k in range(n):
        m32 = F32(F32(t[k]) - F32(0.5) * F32(dt[k]))
        m = float(t[k]) - 0.5 * float(dt[k])
        where = "front" if m32 < lo else ("band" if (m32 >= lo and m32 <= hi) else "behind")
        side.append((where, m))
        if where == "front":
            E += float(w[k]) ** 2
        if where == "band":
            W += float(w[k])
        d += float(w[k]) * m
    dw = []
    for k in range(n):
        where, m = side[k]
        v = g[2] * 2.0 * (d - float(z)) * m
        if where == "front":
            v += g[0] * 2.0 * float(w[k])
        if where == "band":
            v -= g[1] * 2.0 * (1.0 - W)
        dw.append(v)
    return (E, (1.0 - W) ** 2, (d - float(z)) ** 2), dw


@functools.lru_cache(maxsize=None)
def shared(layout_name, variant, eps):
    """(layout, case, reference) of one layout, t variant and eps, computed once per process and
    shared: nobody writes into them."""
    lay = sight_layout(layout_name)
    case = sight_case(lay, variant, eps)
    return lay, case, sight_ref(lay, case)


# ---------------------------------------------------------------------------------- f32 order -----

def _lane_total(a, strided):
    """sum of a in f32: serial, or one accumulator per lane over the strides in ascending order, then
    the lanes"""
    if a.shape[0] == 0:
        return F32(0)
    if not strided:
        return np.cumsum(a, dtype=F32)[-1]
    pad = np.zeros(-(-a.shape[0] // WAVE) * WAVE, dtype=F32)
    pad[:a.shape[0]] = a
    lanes = np.zeros(WAVE, dtype=F32)
    for row in pad.reshape(-1, WAVE):
        lanes = (lanes + row).astype(F32)
    return np.cumsum(lanes, dtype=F32)[-1]


def sight_f32(lay, case, strided):
    """The kernels' operations in float32, in the order of depth_sight.hip's header comment (up to
    fused multiply-adds and the order of the 64 lanes in the final reduction)."""
    w_all, t_all, dt_all = (case[k].numpy() for k in ("weights", "t", "dt"))
    z_all, g_all, eps = case["z"].numpy(), case["d_out"].numpy(), F32(case["eps"])
    R, n = lay.n_rays, lay.n_total
    out = dict(out=np.zeros((R, 3), dtype=F32), dw=np.full(n, SENTINEL, dtype=F32))
    zero = F32(0)
    for r in range(R):
        s, e = int(lay.start[r]), int(lay.end[r])
        z = z_all[r]
        if not ray_valid(z):
            out["dw"][s:e] = zero
            continue
        w = w_all[s:e]
        m = midpoints32(t_all[s:e], dt_all[s:e])
        front, band = membership(m, z, eps)
        E = _lane_total(np.where(front, w * w, zero).astype(F32), strided)
        W = _lane_total(np.where(band, w, zero).astype(F32), strided)
        d = _lane_total((w * m).astype(F32), strided)
        a, x = F32(F32(1) - W), F32(d - z)
        out["out"][r] = (E, F32(a * a), F32(x * x))
        g0, g1, g2 = g_all[r]
        c0, c1, c2 = F32(F32(2) * g0), F32(g1 * F32(F32(2) * a)), F32(g2 * F32(F32(2) * x))
        base = np.where(front, (c0 * w).astype(F32), np.where(band, -c1, zero)).astype(F32)
        out["dw"][s:e] = ((c2 * m).astype(F32) + base).astype(F32)
    return out


# ---------------------------------------------------------------------------------- assertions ----

def _ray_index(lay, name):
    if name == "out":
        return np.broadcast_to(np.arange(lay.n_rays)[:, None], (lay.n_rays, 3))
    return lay.ray_of


def ratios(lay, case, got, ref):
    """(err / u - len_r M_sum) / M_op per element of the valid rays (what K has to cover):
    dict name -> (ratio array, ray index array)."""
    res = {}
    valid = ray_valid(case["z"].numpy())
    for name in ("out", "dw"):
        if name not in got:
            continue
        g = np.asarray(got[name], dtype=np.float64)
        ray = _ray_index(lay, name)
        sel = (ray >= 0) & valid[np.maximum(ray, 0)]
        err = np.abs(g - ref[name])[sel]
        ln = lay.len[ray[sel]].astype(np.float64)
        res[name] = (rc.safe_ratio(err / U - ln * ref["msum"][name][sel], ref["mop"][name][sel]),
                     ray[sel])
    return res


def sight_failures(lay, case, got, ref, K=K_SIGHT):
    """Every assertion the GPU tests make on the outputs 'out' [R, 3] and / or 'dw' [n_total] (f32; dw
    pre-filled with SENTINEL), as a list of (ray, output name, flat element index, message)."""
    fails = []
    sent = F32(SENTINEL)
    valid = ray_valid(case["z"].numpy())
    for name, g32 in got.items():
        g32 = np.asarray(g32, dtype=F32)
        assert g32.shape == ref[name].shape, (name, g32.shape, ref[name].shape)
        g = g32.astype(np.float64).reshape(-1)
        ray = _ray_index(lay, name).reshape(-1)
        want = ref[name].reshape(-1)
        if name == "dw":
            bad = (ray < 0) & (g32.view(np.int32) != sent.view(np.int32))
            for i in np.flatnonzero(bad):
                fails.append((int(lay.owner_of_gap[i]), name, int(i), "written outside every range"))
        rr = np.maximum(ray, 0)
        inval = (ray >= 0) & ~valid[rr]
        zero_bits = g32.reshape(-1).view(np.int32) == 0
        for i in np.flatnonzero(inval & ~zero_bits):
            fails.append((int(ray[i]), name, int(i), "invalid ray: not exactly +0"))
        tol = U * (lay.len[rr] * ref["msum"][name].reshape(-1) + K * ref["mop"][name].reshape(-1))
        err = np.abs(g - want)
        for i in np.flatnonzero((ray >= 0) & ~inval & ~(err <= tol)):
            fails.append((int(ray[i]), name, int(i), "err %.3e > tol %.3e (ref %.6e)" % (
                err[i], tol[i], want[i])))
    return fails
