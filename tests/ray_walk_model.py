"""The ray walk of sampler.hiph -- load_ray, make_stride[_from], keep_step at 64, 16 and 8 lanes to a
ray -- restated from its float32 inputs: a float64 model with a first-order bound per element, a
float32 numpy restatement of the parts that are nothing but IEEE adds and one multiply (expected in
bits), the keep rule, rays designed to stop at a chosen sample, and mutants.  No tests in here:
tests/test_ray_walk_model_cpu.py checks the model, the bounds and the power of the assertions on the
CPU, tests/test_gpu_ray_walk.py makes the assertions against f2n_sample_rays, f2n_sample_dense,
f2n_ray_walk_probe and the real f2n_density_march[_occ].

Float64 model (walk_f64), from the f32 rays_o, rays_d, step multipliers and the f32 `step` the C ABI
receives (sampler.hiph:22-35, :229-265):

    d^ = d / |d|                       cum_k = sum_{j<=k} mult_j   (k + 1 without noise: exact)
    t_k = cum_k step                   p_k = o + d^ t_k
    dt_0 = 0,  dt_k = |p_k - p_{k-1}|  (quirk Q7: a difference of points)

With noise_affine the multiplier is the f32 value (u - .5f) + 1.f (numpy's f32 subtract and add are
IEEE, so it is an input here).  A zero direction gives NaN in d^, p and dt_k (k >= 1), a finite t.

Bounds, first order, per element, u = 2^-24, each line with the operations it stands for:

    E_dir  = 4 u |d^_c|                x x, fmaf, fmaf under the square root: 3 roundings of the sum of
                                       squares = 1.5 u of the norm; sqrtf: u; the division: u; 3.5 -> 4
    E_cum  = u D_k cum_k,  D_k = 7 + k // 64        (0 without noise)
                                       the multipliers are positive, so every partial sum is below
                                       cum_k and a term's error is at most u cum_k per addition it
                                       passes.  Longest chain inside a 64-sample block (sampler.hiph:48-52,
                                       common.hiph:33-42): four row_shr steps to the row total T0, T1 + T0,
                                       (rs + T2) + (T1 + T0): 6; carry + scan: 7 (sampler.hiph:246); the
                                       carry of a completed block is that sum (sampler.hiph:250), and every
                                       later block adds onto it once more: + k // 64
    E_t    = step E_cum + u t          the product cum * step (sampler.hiph:251)
    E_p    = t E_dir + |d^_c| E_t + u |d^_c t| + u |p_c|       d^ t, then o + (sampler.hiph:252-255)
    E_dt_k = || E_p_k + E_p_{k-1} + u |p_k - p_{k-1}| ||_2 + 3 u dt_k      the subtraction, then the
                                       norm as in E_dir without the division (sampler.hiph:259-260);
                                       E_dt_0 = 0: dt_0 is the constant +0

Exclusive optical depth of keep_step (sampler.hiph:300-315): depth_k = sum_{j<k} sec_j with the same
additions as the noise scan (scan, ds.carry + prev, ds.carry + ds.last), so E_depth = u D_k depth_k.

Bar: |got - f64| <= BAR E with BAR = 2 (as tests/ray_grad_model.py) for the second-order terms; where
E = 0 the values must be equal; where the model is NaN the value must be NaN.  Nothing here was fitted
on a kernel.

Float32 restatement (incl_in_block, cum_noise32, depth32, walk_f32).  The additions of
RayLanes<W>::scan as the header spells them: W = 64 the Kogge-Stone rows and the two row broadcasts of
wave_incl_scan; W = 16 the row scan with t0 / t1p / t2; W = 8 row_scan's two halves with the registers
pv / pa / pb / pc and the row_shl fills, and the (rs + T2) + (T1 + T0) association.  cum, t = cum * step
and keep_step's depth are f32 adds and one multiply and are expected in bits; d^, p and dt hold sqrt,
division and FMAs (numpy has no FMA: it is emulated through float64, a double rounding that can differ
in the last bit), so walk_f32's dirs, pts and dt are claimed within BAR E only.

Keep rule.  ragged_cases.keep_rule on sec = exp(b0 - shift) dt in float64, with the relative error of
sec_k in units of u:  e_rel_k = BAR E_dt_k / (u dt_k) + |b0 - shift| + 4  (dt's bound; expf of an
argument of that size, the product and the decision's own expf as in density_scan_ref).

Designed stops (stop_case).  A field with w0 = 0 has logit == b0 exactly, so sec_k = expf(b0 - shift) dt_k
whatever the table holds.  Ray r gets its own scale c_r on its noise row, solved in the float64 model so
that sum_{j < m-1} sec_j + sec_{m-1} / 2 = -ln(thresh): the transmittance crosses the threshold in the
middle of sample m - 1 and the ray keeps exactly m = target_r samples.  Targets: every member of
STOP_MARKS and S - 1, S that is <= S; three rays per target plus one where that makes the count even,
so the last wave of every mapping is partly empty.  Condition (asserted on the CPU): no designed ray in
the ambiguity band, and half the crossing sample's optical depth at least STOP_MARGIN = 4 bands.  At
S = 1024 the plain construction misses it for targets above ~500 (Q7's cancellation over that many
samples reaches half a sample's optical depth): the multiplier of the CROSSING sample of such a ray is
doubled until the condition holds (the choice made here; S is not lowered).

Mutants: see MUTANTS; each is the f32 restatement with one thing wrong, and names the assertion of the
GPU test that rejects it.
"""
import math

import numpy as np

from tests import ragged_cases as rc

U = rc.U
BAR = 2.0
WAVE = 64
WIDTHS = (64, 16, 8)
THRESH = 1e-4
DENSITY_SHIFT = 3.0

SAMPLE_S = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 100, 129, 1024)
SAMPLE_RAYS = (1, 5, 37)
STEPS = (1.0 / 256, 0.05, 0.04)
O_NORMS = (0.05, 0.3, 30.0)
D_NORMS = (1e-3, 1.0, 1e3)

STOP_S = (17, 100, 129, 1024)
STOP_MARKS = (2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 71, 72, 73, 127, 128, 129)
STOP_RAYS_PER_TARGET = 3
STOP_B0 = 8.0
STOP_FIELD = dict(L=4, F=2, log2_T=12)
STOP_MARGIN = 4.0
STOP_O_MAX = 0.3

F32 = np.float32


def D(k):
    """additions on the longest path of a term of cum_k / depth_k (module docstring)"""
    return 7 + np.asarray(k) // WAVE


# ---- float32: the additions of RayLanes<W>::scan -----------------------------------------------------

def _shr(a, n):
    """row_shr:n along the last axis, 0.f shifted in"""
    out = np.zeros_like(a)
    if n < a.shape[-1]:
        out[..., n:] = a[..., :a.shape[-1] - n]
    return out


def _row_scan(v):
    """the four row_shr steps on rows of 16 (last axis)"""
    for n in (1, 2, 4, 8):
        v = v + _shr(v, n)
    return v


def _scan64(v):
    """wave_incl_scan (common.hiph:33-42) of one block [R, 64]"""
    rs = _row_scan(v.reshape(-1, 4, 16))
    out = np.empty_like(rs)
    out[:, 0] = rs[:, 0]
    out[:, 1] = rs[:, 1] + rs[:, 0, 15:16]              # row_bcast15 into row 1
    out[:, 3] = rs[:, 3] + rs[:, 2, 15:16]              # ... and row 3
    out[:, 2] = rs[:, 2] + out[:, 1, 15:16]             # row_bcast31 into rows 2 and 3
    out[:, 3] = out[:, 3] + out[:, 1, 15:16]
    return out.reshape(-1, WAVE)


def _scan16(v, mut=None):
    """RayLanes<16>::scan over the four strides of one block [R, 64]"""
    out = np.empty_like(v)
    t0 = t1p = t2 = None
    for j in range(4):
        rs = _row_scan(v[:, 16 * j:16 * j + 16])
        tj = rs[:, 15]
        if j == 0:
            t0, ret = tj, rs
        elif j == 1:
            t1p = tj if mut == "w16_t1p" else tj + t0
            ret = rs + t0[:, None]
        elif j == 2:
            t2, ret = tj, rs + t1p[:, None]
        else:
            ret = (rs + t2[:, None]) + t1p[:, None]
        out[:, 16 * j:16 * j + 16] = ret
    return out


def _scan8(v, mut=None):
    """RayLanes<8>::scan over the eight strides of one block [R, 64]: row_scan's halves, then the
    totals of the completed rows"""
    out = np.empty_like(v)
    m = np.arange(8)
    t0 = t1p = t2 = pv = pa = pb = pc = None
    for s in range(8):
        j, h = s >> 1, s & 1
        x = v[:, 8 * s:8 * s + 8]
        if h == 0:
            a1 = x + _shr(x, 1)
            a2 = a1 + _shr(a1, 2)
            a4 = a2 + _shr(a2, 4)
            pv, pa, pb, pc = x, a1, a2, a4
            rs = a4
        else:
            top = 6 if mut == "w8_fill6" else 7
            f1 = pv[:, np.minimum(m + top, top)]        # row_shl:7 of pv: lane 0 reads lane 7
            a1 = x + np.where(m >= 1, _shr(x, 1), f1)
            f2 = pa[:, np.minimum(m + 6, 7)]            # row_shl:6 of pa: lanes 0, 1 read 6, 7
            a2 = a1 + np.where(m >= 2, _shr(a1, 2), f2)
            f4 = pb[:, np.minimum(m + 4, 7)]            # row_shl:4 of pb: lanes 0..3 read 4..7
            a4 = a2 + np.where(m >= 4, _shr(a2, 4), f4)
            rs = a4 if mut == "w8_no_pc" else a4 + pc
        if j == 0:
            inner = rs
        elif j == 1:
            inner = rs + t0[:, None]
        elif j == 2:
            inner = rs + t1p[:, None]
        else:
            inner = (rs + t2[:, None]) + t1p[:, None]
        if h == 1:
            tj = rs[:, 7]
            if j == 0:
                t0 = tj
            elif j == 1:
                t1p = tj + t0
            elif j == 2:
                t2 = tj
        out[:, 8 * s:8 * s + 8] = inner
    return out


def _pad(v):
    R, S = v.shape
    Sp = -(-S // WAVE) * WAVE
    out = np.zeros((R, Sp), dtype=F32)
    out[:, :S] = v
    return out


def incl_in_block(v, W, mut=None):
    """RayLanes<W>::scan of every stride: the inclusive f32 sum of v [R, S] INSIDE its 64-sample
    block (a lane without a sample holds 0.f) -> [R, S padded to a multiple of 64]"""
    v = _pad(np.asarray(v, dtype=F32))
    out = np.empty_like(v)
    for c in range(0, v.shape[1], WAVE):
        blk = v[:, c:c + WAVE]
        out[:, c:c + WAVE] = (_scan64(blk) if W == 64 else _scan16(blk, mut) if W == 16
                              else _scan8(blk, mut))
    assert out.dtype == F32
    return out


def cum_noise32(mult, W, mut=None):
    """make_stride_from's cum (sampler.hiph:246, :250) for multipliers mult [R, S] f32 -> [R, S] f32"""
    S = mult.shape[1]
    inc = incl_in_block(mult, W, mut)
    out = np.empty_like(inc)
    carry = np.zeros(inc.shape[0], dtype=F32)
    for c in range(0, inc.shape[1], WAVE):
        blk = inc[:, c:c + WAVE]
        if mut == "exclusive_noise":
            blk = np.concatenate([np.zeros_like(blk[:, :1]), blk[:, :-1]], 1)
        cum = blk if mut == "carry_dropped" else carry[:, None] + blk
        carry = cum[:, 62 if mut == "carry62" else 63]
        out[:, c:c + WAVE] = cum
    return out[:, :S]


def depth32(sec, W, mut=None):
    """keep_step's exclusive depth (sampler.hiph:306-309) of sec [R, S] f32 -> [R, S] f32"""
    S = sec.shape[1]
    inc = incl_in_block(sec, W, mut)
    out = np.empty_like(inc)
    carry = np.zeros(inc.shape[0], dtype=F32)
    last = np.zeros(inc.shape[0], dtype=F32)
    for c in range(0, inc.shape[1], WAVE):
        blk = inc[:, c:c + WAVE]
        fill = last if (mut == "keep_last_stale" and W < WAVE) else np.zeros_like(last)
        prev = blk if mut == "keep_inclusive" else np.concatenate([fill[:, None], blk[:, :-1]], 1)
        out[:, c:c + WAVE] = carry[:, None] + prev
        last = blk[:, 63]
        carry = carry + (blk[:, 62] if mut == "keep_carry62" else last)
        if mut == "keep_carry_twice":
            carry = carry + last
    return out[:, :S]


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _norm32(v):
    """sqrtf(fmaf(z, z, fmaf(y, y, x * x))) over the last axis"""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.sqrt(_fma32(z, z, _fma32(y, y, x * x)))


def multipliers(noise, affine=False):
    """the f32 step multipliers: noise itself, or (u - .5f) + 1.f"""
    if noise is None:
        return None
    n = np.asarray(noise, dtype=F32)
    return (n - F32(0.5)) + F32(1.0) if affine else n


def walk_f32(o, d, mult, S, step, W=64, mut=None):
    """load_ray and make_stride_from in numpy f32 at W lanes to a ray -> dict dirs [R, 3], t [R, S],
    pts [R, S, 3], dt [R, S].  `step` is the caller's Python number; the kernel sees float32(step)."""
    o, d = np.asarray(o, dtype=F32), np.asarray(d, dtype=F32)
    R = o.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        dirs = d if mut == "dir_raw" else d / _norm32(d)[:, None]
        if mult is None:
            cum = np.broadcast_to(np.arange(1, S + 1, dtype=F32), (R, S)).copy()
        else:
            mult = np.asarray(mult, dtype=F32)
            if mut == "noise_row_next":
                mult = np.roll(mult, -1, 0)
            if mut == "affine_twice":
                mult = (mult - F32(0.5)) + F32(1.0)
            cum = cum_noise32(mult, W, mut)
        if mut == "step_f64":
            t = (cum.astype(np.float64) * float(step)).astype(F32)
        else:
            t = cum * F32(step)
        pts = o[:, None, :] + dirs[:, None, :] * t[:, :, None]
        q = np.concatenate([np.zeros((R, 1, 3), dtype=F32), pts[:, :-1]], 1)   # carry.l* starts at 0
        if mut == "prev_own":
            ks = np.arange(S)
            own = (ks % W == 0) & (ks > 0)
            q[:, own] = pts[:, own]
        dt = _norm32(pts - q)
        if mut != "dt0":
            dt[:, 0] = 0.0
    assert t.dtype == F32 and pts.dtype == F32 and dt.dtype == F32
    return dict(dirs=dirs, t=t, pts=pts, dt=dt)


# ---- float64 model and bounds ---------------------------------------------------------------------------

def walk_f64(o, d, mult, S, step):
    """-> dict of float64 values dirs [R, 3], cum, t [R, S], pts [R, S, 3], dt [R, S] and their bounds
    E_dirs, E_t, E_pts, E_dt (module docstring).  mult: f32 multipliers or None."""
    o, d = np.asarray(o, dtype=F32).astype(np.float64), np.asarray(d, dtype=F32).astype(np.float64)
    R = o.shape[0]
    st = float(F32(step))
    k = np.arange(S)
    with np.errstate(divide="ignore", invalid="ignore"):
        dirs = d / np.sqrt((d * d).sum(1))[:, None]
        E_dirs = 4.0 * U * np.abs(dirs)
        if mult is None:
            cum = np.broadcast_to((k + 1).astype(np.float64), (R, S)).copy()
            E_cum = np.zeros((R, S))
        else:
            cum = np.cumsum(np.asarray(mult, dtype=F32).astype(np.float64), 1)
            E_cum = U * D(k)[None, :] * cum
        t = cum * st
        E_t = st * E_cum + U * t
        m = dirs[:, None, :] * t[:, :, None]
        pts = o[:, None, :] + m
        E_pts = (t[:, :, None] * E_dirs[:, None, :] + np.abs(dirs)[:, None, :] * E_t[:, :, None]
                 + U * np.abs(m) + U * np.abs(pts))
        diff = pts[:, 1:] - pts[:, :-1]
        dt = np.zeros((R, S))
        dt[:, 1:] = np.sqrt((diff * diff).sum(2))
        E_dt = np.zeros((R, S))
        e = E_pts[:, 1:] + E_pts[:, :-1] + U * np.abs(diff)
        E_dt[:, 1:] = np.sqrt((e * e).sum(2)) + 3.0 * U * dt[:, 1:]
    return dict(dirs=dirs, cum=cum, t=t, pts=pts, dt=dt, E_dirs=E_dirs, E_t=E_t, E_pts=E_pts,
                E_dt=E_dt)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.int32)


def bits_equal(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def within(got, ref, E):
    """element-wise: |got - ref| <= BAR E; equal where E == 0; NaN where the model is NaN"""
    g = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.abs(g - ref) <= BAR * E
    return np.where(np.isnan(ref), np.isnan(g), ok)


def ratio(got, ref, E):
    """largest |got - ref| / E over the elements with a bound (finite model, E > 0)"""
    g = np.asarray(got, dtype=np.float64)
    sel = np.isfinite(ref) & (E > 0)
    if not sel.any():
        return 0.0
    return float((np.abs(g - ref)[sel] / E[sel]).max())


SAMPLE_OUTPUTS = ("dirs", "pts", "dt")


def sample_failures(got, ref, t32):
    """The assertions of the GPU test on one set of samples, as a list of (name, message); empty =
    all hold.  got: dict of f32 arrays t [R, S], dt [R, S], pts [R, S, 3] and (optionally) dirs
    [R, S, 3] or [R, 3]; ref = walk_f64's dict; t32 = walk_f32's t.
      t_bits     t equals the f32 restatement bit for bit
      t_finite   t is finite on every ray, a zero direction included
      dirs_bar, pts_bar, dt_bar    within BAR E of the float64 model, NaN where it is NaN
      dt0_zero   dt at k = 0 is +0"""
    fails = []
    if not bits_equal(got["t"], t32):
        bad = np.argwhere(_bits(got["t"]) != _bits(t32))
        fails.append(("t_bits", "%d elements, first (ray, k) = %s" % (len(bad), tuple(bad[0]))))
    if not np.isfinite(np.asarray(got["t"])).all():
        fails.append(("t_finite", "a t is not finite"))
    for name in SAMPLE_OUTPUTS:
        if name not in got:
            continue
        g, r, E = np.asarray(got[name]), ref[name], ref["E_" + name]
        if name == "dirs" and g.ndim == 3:
            r, E = r[:, None, :], E[:, None, :]
        ok = within(g, r, E)
        if not ok.all():
            bad = np.argwhere(~ok)
            i = tuple(bad[0])
            fails.append((name + "_bar", "%d elements, first %s: got %r model %r E %r" % (
                len(bad), i, float(g[i]), float(np.broadcast_to(r, g.shape)[i]),
                float(np.broadcast_to(E, g.shape)[i]))))
    if (_bits(np.asarray(got["dt"])[:, 0]) != 0).any():
        fails.append(("dt0_zero", "dt at k = 0 is not +0"))
    return fails


def sample_ratios(got, ref):
    out = {}
    for name in SAMPLE_OUTPUTS + ("t",):
        if name in got:
            g, r, E = np.asarray(got[name]), ref[name], ref["E_" + name]
            if name == "dirs" and g.ndim == 3:
                r, E = np.broadcast_to(r[:, None, :], g.shape), np.broadcast_to(E[:, None, :], g.shape)
            out[name] = ratio(g, r, E)
    return out


def old_bar_passes(got, want):
    """The tolerances of tests/test_gpu_ops.py::test_sample_rays (torch.testing.assert_close:
    |got - want| <= atol + rtol |want|) on dirs, t, pts, dt against the f32 oracle's values `want`,
    and its dt[:, 0] == 0."""
    tol = dict(dirs=(1e-6, 1e-7), t=(1e-6, 1e-7), pts=(1e-5, 2e-6), dt=(1e-3, 2e-6))
    for name, (rtol, atol) in tol.items():
        g, w = np.asarray(got[name], dtype=np.float64), np.asarray(want[name], dtype=np.float64)
        if name == "dirs" and w.ndim == 3:
            g = np.broadcast_to(g[:, None, :], w.shape) if g.ndim == 2 else g
        if not (np.abs(g - w) <= atol + rtol * np.abs(w)).all():
            return False
    return bool((np.asarray(got["dt"])[:, 0] == 0).all())


# ---- cases of the samplers --------------------------------------------------------------------------------

def step_of(S):
    return STEPS[SAMPLE_S.index(S) % len(STEPS)] if S in SAMPLE_S else STEPS[S % len(STEPS)]


def sample_case(n_rays, S, with_noise, seed=0, zero_ray=None):
    """f32 rays with |o| cycling through O_NORMS and |d| through D_NORMS (every pair among nine
    consecutive rays), noise U[0, 1) + 0.5 or None; zero_ray: index of a ray whose direction is 0."""
    rng = np.random.RandomState(1000 * S + 10 * n_rays + seed)
    o = rng.standard_normal((n_rays, 3))
    d = rng.standard_normal((n_rays, 3))
    r = np.arange(n_rays)
    o *= (np.array(O_NORMS)[r % 3] / np.sqrt((o * o).sum(1)))[:, None]
    d *= (np.array(D_NORMS)[(r // 3) % 3] / np.sqrt((d * d).sum(1)))[:, None]
    noise = (rng.random_sample((n_rays, S)) + 0.5).astype(F32) if with_noise else None
    d = d.astype(F32)
    if zero_ray is not None:
        d[zero_ray] = 0.0
    return dict(o=o.astype(F32), d=d, noise=noise, n_rays=n_rays, S=S, step=step_of(S))


def random_sec(n_rays, S, seed=0):
    """positive f32 optical depths: ray r crosses the threshold after about S / 4 .. S samples, or not
    at all"""
    rng = np.random.RandomState(77 * S + n_rays + seed)
    limit = -math.log(float(F32(THRESH)))
    scale = limit / S * rng.choice([0.5, 1.0, 2.0, 4.0], size=n_rays)
    return (rng.random_sample((n_rays, S)) * 2.0 * scale[:, None] + 1e-6).astype(F32)


# ---- the keep rule ------------------------------------------------------------------------------------------

def depth_model(sec):
    """sec [R, S] (f32 values) -> float64 exclusive sum and its bound u D_k depth_k"""
    s = np.asarray(sec, dtype=np.float64)
    depth = np.cumsum(s, 1) - s
    return depth, U * D(np.arange(s.shape[1]))[None, :] * depth


def keep_model(sec, e_rel, thresh=THRESH):
    """ragged_cases.keep_rule per ray, and per sample: keep [R, S] by the float64 rule and band [R, S]
    (True where the sample's decision lies within the f32 rounding of its depth, same band)."""
    sec = np.asarray(sec, dtype=np.float64)
    kept, in_band = rc.keep_rule(sec, e_rel, thresh)
    S = sec.shape[1]
    depth = np.cumsum(sec, 1) - sec
    limit = -math.log(float(F32(thresh)))
    keep = np.exp(-depth) > float(F32(thresh))
    k = np.arange(S, dtype=np.float64)[None, :]
    band = U * (k * depth + (np.cumsum(sec * e_rel, 1) - sec * e_rel) + 4.0)
    near = np.abs(depth - limit) <= band
    assert np.array_equal(near.any(1), in_band)
    return dict(kept=kept, in_band=in_band, keep=keep, near=near, depth=depth, band=band, limit=limit)


def keep_failures(depth_got, keep_got, sec, W, designed=False):
    """The assertions of the GPU test on the probe's depth and keep for sec [R, S] f32 at width W:
      depth_bits   depth equals the f32 restatement bit for bit
      depth_bar    within BAR u D_k depth of the float64 exclusive sum
      keep_rule    keep follows the float64 rule outside the band
      band_cap     at most 2 % of the rays in the band (none of designed ones)"""
    fails = []
    if not bits_equal(depth_got, depth32(sec, 64)):
        bad = np.argwhere(_bits(depth_got) != _bits(depth32(sec, 64)))
        fails.append(("depth_bits", "W %d: %d elements, first (ray, k) = %s" % (W, len(bad), tuple(bad[0]))))
    d64, E = depth_model(sec)
    if not within(depth_got, d64, E).all():
        fails.append(("depth_bar", "W %d: worst ratio %.2f" % (W, ratio(depth_got, d64, E))))
    km = keep_model(sec, np.zeros_like(d64))
    wrong = (np.asarray(keep_got).astype(bool) != km["keep"]) & ~km["near"]
    if wrong.any():
        fails.append(("keep_rule", "W %d: %d samples, first (ray, k) = %s" % (
            W, int(wrong.sum()), tuple(np.argwhere(wrong)[0]))))
    cap = 0.0 if designed else 0.02
    if km["in_band"].mean() > cap:
        fails.append(("band_cap", "%d of %d rays in the band" % (int(km["in_band"].sum()), len(d64))))
    return fails


def kept_from_keep(keep):
    """leading samples kept, per ray"""
    k = np.asarray(keep).astype(bool)
    return np.where(k.all(1), k.shape[1], np.argmin(k, 1)).astype(np.int32)


# ---- designed stops -------------------------------------------------------------------------------------------

def stop_targets(S):
    return sorted({m for m in STOP_MARKS + (S - 1, S) if 2 <= m <= S})


def _stop_sec(case, c):
    noise = (c[:, None] * case["base"]).astype(F32)
    ref = walk_f64(case["o"], case["d"], noise, case["S"], case["step"])
    sigma = math.exp(STOP_B0 - DENSITY_SHIFT)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_rel = np.where(ref["dt"] > 0, BAR * ref["E_dt"] / (U * ref["dt"]), 0.0)
    e_rel = e_rel + np.where(ref["dt"] > 0, abs(STOP_B0 - DENSITY_SHIFT) + 4.0, 0.0)
    return noise, sigma * ref["dt"], e_rel


def stop_case(S, seed=0):
    """-> dict o, d [R, 3], noise [R, S] f32, step, target [R], base, boosted (rays whose crossing
    sample's multiplier was raised), and the float64 sec, e_rel the condition is checked on."""
    rng = np.random.RandomState(31 * S + seed)
    target = np.repeat(np.array(stop_targets(S), dtype=np.int64), STOP_RAYS_PER_TARGET)
    if target.shape[0] % 2 == 0:
        target = np.concatenate([target, [S]])
    R = target.shape[0]
    o = rng.standard_normal((R, 3))
    o *= (rng.uniform(0.05, STOP_O_MAX, R) / np.sqrt((o * o).sum(1)))[:, None]
    d = rng.standard_normal((R, 3))
    case = dict(o=o.astype(F32), d=d.astype(F32), S=S, step=step_of(S), target=target, n_rays=R,
                base=(rng.random_sample((R, S)) + 0.5))
    limit = -math.log(float(F32(THRESH)))
    rows = np.arange(R)
    boosted = np.zeros(R, dtype=np.int64)
    for _ in range(12):
        c = np.ones(R)
        for _ in range(4):
            noise, sec, e_rel = _stop_sec(case, c)
            csum = np.cumsum(sec, 1)
            half = 0.5 * sec[rows, target - 1]
            c = c * limit / (csum[rows, target - 1] - half)
        noise, sec, e_rel = _stop_sec(case, c)
        km = keep_model(sec, e_rel)
        half = 0.5 * sec[rows, target - 1]
        band = np.maximum(km["band"][rows, target - 1], km["band"][rows, np.minimum(target, S - 1)])
        thin = half < STOP_MARGIN * band
        if not thin.any():
            break
        case["base"][rows[thin], target[thin] - 1] *= 2.0
        boosted[thin] += 1
    case.update(noise=noise, sec=sec, e_rel=e_rel, boosted=boosted, c=c)
    return case


def stop_condition(case):
    """-> dict kept (float64 rule), in_band [R], margin [R] = band / (half the crossing sample's
    optical depth): the condition is kept == target, no ray in the band, margin <= 1 / STOP_MARGIN."""
    km = keep_model(case["sec"], case["e_rel"])
    rows, tg, S = np.arange(case["n_rays"]), case["target"], case["S"]
    half = 0.5 * case["sec"][rows, tg - 1]
    band = np.maximum(km["band"][rows, tg - 1], km["band"][rows, np.minimum(tg, S - 1)])
    return dict(kept=km["kept"], in_band=km["in_band"], margin=band / half)


def stop_sec32(case):
    """the designed optical depths as f32, for the probe's sec_in"""
    return case["sec"].astype(F32)


# ---- mutants -----------------------------------------------------------------------------------------------------

# name -> (what it breaks, the width forms it lives in, the assertion of the GPU test that rejects it)
MUTANTS = {
    "carry_dropped":    ("block carry of the noise scan dropped", WIDTHS, "t_bits"),
    "carry62":          ("block carry taken from lane 62", WIDTHS, "t_bits"),
    "exclusive_noise":  ("exclusive instead of inclusive noise sum", WIDTHS, "t_bits"),
    "prev_own":         ("prev at a stride start taken from the own lane", WIDTHS, "dt_bar"),
    "dt0":              ("dt_0 not zero", WIDTHS, "dt0_zero"),
    "dir_raw":          ("direction not normalised", WIDTHS, "dirs_bar"),
    "noise_row_next":   ("the noise row of ray r + 1", WIDTHS, "t_bits"),
    "affine_twice":     ("affine applied twice", (64,), "t_bits"),
    "step_f64":         ("float64 step", WIDTHS, "t_bits"),
    "w8_fill6":         ("RayLanes<8>: second half fills from lane 6", (8,), "probe_bits"),
    "w8_no_pc":         ("RayLanes<8>: pc not added", (8,), "probe_bits"),
    "w16_t1p":          ("RayLanes<16>: t1p without t0", (16,), "probe_bits"),
    "keep_inclusive":   ("keep_step: inclusive depth", WIDTHS, "depth_bits"),
    "keep_last_stale":  ("keep_step: ds.last not cleared at a block start", (16, 8), "depth_bits"),
    "keep_carry_twice": ("keep_step: block carry added twice", WIDTHS, "depth_bits"),
    "keep_carry62":     ("keep_step: block carry taken from lane 62", WIDTHS, "depth_bits"),
}
SAMPLE_MUTANTS = ("carry_dropped", "carry62", "exclusive_noise", "prev_own", "dt0", "dir_raw",
                  "noise_row_next", "affine_twice", "step_f64")
WIDTH_MUTANTS = ("w8_fill6", "w8_no_pc", "w16_t1p")
KEEP_MUTANTS = ("keep_inclusive", "keep_last_stale", "keep_carry_twice", "keep_carry62")
