"""Inputs, float64 references, per-element bounds, assertion functions and mutants for the kernels that
end a training step: f2n_adam_step (adam.hip) with FusedAdam, f2n_loss_fwd (loss.hip) and
f2n_scatter_add_bwd (scatter.hip).  No tests in here: tests/test_step_tail_cases_cpu.py checks on the
CPU that the assertion functions accept an f32 numpy restatement of each kernel and reject every
mutant, and re-measures the constants K; tests/test_gpu_adam.py, tests/test_gpu_loss.py and
tests/test_gpu_scatter_bwd.py call the same functions on what the HIP kernels return.

ADAM.  One step from a given f32 state (p, m, v, g) at a given step number: the bound is one step's
rounding, no trajectory is accumulated.  P = 256*16 blocks x 256 threads x 4 elements = 4 194 304 is
what one pass of the launcher's capped grid covers (adam.hip: grid = min(ceil(ceil(n/4)/256),
256*16), each thread a float4); the reference table has 4 P elements.
  Reference (adam_ref): LibTorch's rule as the header of adam.hip states it, in float64, with the f32
  scalars the ABI receives widened to double (1 - float32(beta) is exact in f32, so the reference
  uses the same number), bc1 = 1 - beta1^step and bc2 = 1 - beta2^step in double as in the launcher:
      g' = g + wd p;  M = b1 m + (1-b1) g';  V = b2 v + (1-b2) g'^2;
      D = sqrt(V)/sqrt(bc2) + eps;  P' = p - (lr/bc1) M / D.
  Inputs (adam_case), mixed within one tensor by a random category per element: |g| log-uniform
  1e-14..1e2 (sqrt(v) crosses eps), |m| log-uniform 1e-12..1e-1, v log-uniform 1e-30..1e-4, p normal
  0.1 or in the reference's initial table range (-1e-4..-0.8e-4: f16 subnormals and the smallest
  normals); g = 0 with m, v != 0; g = m = v = 0; g = -wd p (1 + d), |d| in 1e-7..1e-2 (g' cancels);
  g = m = v = 0 with p from CHOSEN_P (f16 ties, f16 subnormals, +-65504, +-65520, +-0, +-1e-8); and
  "nudged ties": p an f16 tie in 2^-6..2, g = v = 0, |m| in 1e-26..1e-24, so that with wd = 0 the
  update (<= 1e-10) is far below half an f32 ulp of p: the stored f32 p' is the tie and its RNE cast
  goes to the even neighbour, while a cast of the unrounded p' goes to the side the update points to.
  Bounds, u = 2^-24, A = 4 x 2^-149 (four f32 subnormal units), ag = |g| + |wd p|:
      |m' - M| <= K_M u M_m + A,   M_m = b1 |m| + (1-b1) ag
      |v' - V| <= K_V u M_v + A,   M_v = b2 |v| + (1-b2) (g'^2 + 2 |g'| ag)
                                   (ag enters through 2 |g'| dg', dg' ~ u ag)
      |p' - P'| <= u |P'| + K_P u s M_m / D_lo + s |M| (1/D_lo - 1/D) + A,   s = lr/bc1,
                                   D_lo = sqrt(max(V - dv, 0))/sqrt(bc2) + eps,  dv = K_V u M_v + A:
  the last rounding of p' alone, plus K_P times the update's conditioning, plus what v's error does to
  the denominator.  The denominator is taken as an interval (sqrt at V - dv), not to first order: where
  g cancels wd p, dv is of the size of V and a first-order term is several hundred times too small.
  Subnormals.  Whether the device flushes f32 subnormals in v or underflows gradually is not known,
  and either must pass.  adam_case keeps every non-zero input at or above 1e-30, and adam_failures
  asserts that no non-zero M or V of the reference lies below 2^-120: then no operation of the rule
  has a subnormal operand or result, both kinds of device round every operation alike, and A covers
  nothing but the last place of a result that is exactly zero in one arithmetic and not the other.
  Exact assertions: where g = m = v = 0 and wd = 0, p keeps its bits and m, v are +0; the shadow is
  the RNE f16 cast of the STORED f32 p, bit for bit, everywhere; with and without a shadow pointer
  p, m, v are bit-identical; GUARD = 64 elements of SENTINEL past n are intact in every buffer, the
  shadow included.
  K is MEASURED on the CPU against adam_f32, an f32 numpy restatement (every operation rounded; step
  size and 1/sqrt(bc2) rounded to f32 as the launcher does), never against the kernel
  (test_step_tail_cases_cpu.py::test_adam_measured_K).  The restatement fuses nothing but g' = wd p + g,
  which it rounds once as the kernel's fmaf(wd, p, g) does: rounded twice, g' is off by u ag where it
  cancels, its square by (u ag)^2, and M_v would need a second-order term the kernel has no use for.
  Measured: the largest (err - A)/(u M) of m and v, (err - A - u |P'| - denominator term)/(u s M_m/D_lo)
  of p, over all small sizes x steps x wds AND over the TILE-element draws every larger case repeats
  (all steps x wds: every element a GPU test sees is measured); K = 4 x that (the other fused
  multiply-adds, device sqrtf and divide), rounded up to a power of two.
      measured:  m 2.60,  v 1.95,  p 0.89 (with K_V = 8 in dv)   ->   K_M = 16, K_V = 8, K_P = 4.

LOSS.  Reference (loss_ref): train_manager's formula in float64 on the f32 inputs,
      color_loss = mean_{r,c} sqrt(e^2 + 1e-4), var_loss = mean_r sqrt(var + 1e-2),
      loss = color_loss + w var_loss, sq_err_sum = sum e^2,
      d_colors = e / sqrt(e^2 + 1e-4) / (3R),  d_var = w / (2 sqrt(var + 1e-2) R).
  Inputs (loss_case): "mixed" -- errors per element from {exact 0, +-1e-6, +-1e-3, O(1)}, var from
  {0, 1e-6, O(1)}; "zero" -- every error exactly 0; "spike" -- every error +-1e-3 and var 1e-6 but
  the LAST ray's, which are O(1): what the last block and the last partial hold then dominates
  sq_err_sum, so a dropped tail shows however many rays there are.
  Bounds: a gradient element K_LOSS u |value|; a sum of n terms the any-order bound n u sum|x| (scaled
  as the sum is) plus K_LOSS u |result|, n = 3R for color_loss and sq_err_sum, R for var_loss; the loss
  the two of its parts plus K_LOSS u |loss|.  Exact: e == 0 gives d_colors == 0, an all-zero error
  sq_err_sum == 0.  loss_nan_failures: a NaN colour makes loss, color_loss and sq_err_sum NaN, var_loss
  not, the poisoned d_colors element NaN and none outside its ray.
      measured (loss_f32: per-element f32, 256-ray partials, then the partials):
      d_colors 3.33, d_var 3.59; the sums' (err - n u sum|x|)/(u |result|) is negative everywhere (the
      any-order term alone covers them)  ->  4 x 3.59 = 14.4, K_LOSS = 16.

EMBEDDING GRADIENT.  The sum order is made irrelevant instead of bounded: dsum holds multiples of 2^-10
  with |x| <= 4 and every (image, channel) has sum |x| 2^10 < 2^24 (scatter_case asserts it), so every
  partial sum in any order is exact in f32 and any correct kernel equals the int64 reference
  (scatter_ref) BIT FOR BIT, atomics or not.  Layouts (scatter_ids): runs of {1, 63, 64, 65, 200}
  samples that start, end and cross at multiples of kSpan = 64, one run of id -1 and one of id n_emb
  (ignored), images 3 and 6 of the 8 never named (rows +0), cut to n_all in {1, 64, 65, 3000};
  C in {1, 3, 16, 17}.  demb is pre-filled with SENTINEL (overwritten, not accumulated into) and
  carries GUARD elements past n_emb C.

Mutants: ADAM_MUTANTS, LOSS_MUTANTS, SCATTER_MUTANTS below, one defect each, every one with the cases
on which the assertion function must reject it.
"""
import functools

import numpy as np

U = 2.0 ** -24
GUARD = 64
SENTINEL = 7.0
SENTINEL_H = int(np.float16(SENTINEL).view(np.uint16))
TINY = 4 * 2.0 ** -149               # A of the docstring
NO_SUBNORMAL_BELOW = 2.0 ** -120

# ---------------------------------------------------------------------------------- Adam ----------

ADAM_BLOCK, ADAM_VEC, ADAM_MAX_BLOCKS = 256, 4, 256 * 16     # adam.hip: F2N_BLOCK, float4, grid cap
P = ADAM_MAX_BLOCKS * ADAM_BLOCK * ADAM_VEC                   # elements per grid-stride pass
assert P == 4194304

LR, BETA1, BETA2, EPS = 1e-2, 0.9, 0.99, 1e-15
STEPS = (1, 2, 10, 1000, 100000)
WDS = (0.0, 1e-6, 1e-2)
SMALL_SIZES = (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025)
BIG_SIZES = (P - 1, P, P + 1, P + 5, 2 * P + 3, 4 * P)
# every big size runs one (step, wd) pair, different sizes different pairs
BIG_PAIRS = {P - 1: (1, 0.0), P: (2, 1e-6), P + 1: (10, 1e-2), P + 5: (1000, 0.0),
             2 * P + 3: (100000, 1e-6), 4 * P: (1, 1e-2)}
K_M, K_V, K_P = 16, 8, 4             # see the module docstring; test_adam_measured_K re-derives them

_T = 2.0 ** -24                       # the smallest f16 subnormal
CHOSEN_P = np.array([
    1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), -(1 + 3 * 2.0 ** -11),   # ties, normal
    0.5 * _T, 1.5 * _T, 2.5 * _T, -1.5 * _T, 1022.5 * _T,                           # ties, subnormal
    _T, 3 * _T, 1023 * _T, -_T, 6e-5, -9.3e-5, 2.0 ** -14,                          # subnormals, edge
    65504.0, -65504.0, 65520.0, -65520.0, 65519.996, 0.0, -0.0, 1e-8, -1e-8], dtype=np.float32)

ADAM_MUTANTS = ("no_bc2", "no_bc1", "eps_under_sqrt", "eps_scaled_by_bc2", "decoupled_wd",
                "wd_missing_in_v", "betas_swapped", "step_plus_one", "tail_skipped",
                "tail_without_wd", "pass_dropped", "pass_twice", "shadow_stale", "shadow_truncated",
                "shadow_single_rounding")


def adam_mutant_applies(mutant, n, step, wd):
    """the cases on which adam_failures must reject `mutant` (bc1 = 1 in double from step 1000 on,
    bc2 = 1 at step 100 000; one step more moves sqrt(bc2) by less than u at step 1000)"""
    if mutant == "no_bc2":
        return step <= 1000 and n >= 1023
    if mutant == "eps_scaled_by_bc2":     # (wd 1e-2 keeps sqrt(v) far above eps: 2e-5 of eps is nothing)
        return (step <= 10 or (step == 1000 and wd <= 1e-6)) and n >= 1023
    if mutant in ("no_bc1", "step_plus_one"):
        return step <= 10 and n >= 1023
    if mutant in ("decoupled_wd", "wd_missing_in_v"):
        return wd != 0 and n >= 1023
    if mutant == "tail_skipped":
        return n % ADAM_VEC != 0
    if mutant == "tail_without_wd":
        return n % ADAM_VEC != 0 and wd != 0 and n >= 1023
    if mutant in ("pass_dropped", "pass_twice"):
        return n > P
    if mutant == "shadow_single_rounding":
        return wd == 0 and n >= 1023
    return n >= 1023      # eps_under_sqrt, betas_swapped, shadow_stale, shadow_truncated


def adam_is_live(case, wd, sl=slice(None)):
    """elements of case[sl] that a step moves: with g = m = v = 0 and wd = 0 an untouched element is
    the right answer, and a mutant that skips it cannot show in p, m, v"""
    live = (case["g"][sl] != 0) | (case["m"][sl] != 0) | (case["v"][sl] != 0)
    return live | (np.float32(wd) != 0)


def _logu(rng, lo, hi, n):
    return 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)


def _sign(rng, n):
    return rng.randint(0, 2, n) * 2.0 - 1.0


TILE = 1000003                        # a prime: no multiple of it is a multiple of P or of a block


def adam_case(n, wd, seed=0):
    """-> dict of f32 numpy arrays p, g, m, v [n] and 'cat' (uint8 category per element).  Above TILE
    elements the case is TILE drawn ones repeated: element i and element i + k P (what a wrong
    stride or a pass taken twice confuses) still hold different values, TILE being prime."""
    if n > TILE:
        base = adam_case(TILE, wd, seed)
        return {k: np.resize(a, n) for k, a in base.items()}
    rng = np.random.RandomState((seed * 7919 + n * 31 + int(round(wd * 1e7))) % (2 ** 31))
    cat = rng.randint(0, 20, n).astype(np.uint8)
    wd32 = np.float64(np.float32(wd))
    p = rng.randn(n) * 0.1
    table = cat >= 18                                      # the reference's initial table range
    p[table] = -1e-4 + 0.2e-4 * rng.rand(int(table.sum()))
    p = p.astype(np.float32)
    g = _sign(rng, n) * _logu(rng, 1e-14, 1e2, n)
    m = _sign(rng, n) * _logu(rng, 1e-12, 1e-1, n)
    v = _logu(rng, 1e-30, 1e-4, n)
    g[(cat >= 9) & (cat <= 11)] = 0.0                     # zero gradient, live moments
    zero = (cat == 12) | (cat == 13)                       # nothing moves
    cancel = cat == 14
    d = _sign(rng, n) * _logu(rng, 1e-7, 1e-2, n)
    g[cancel] = (-wd32 * p.astype(np.float64) * (1.0 + d))[cancel]
    chosen = (cat == 15) | (cat == 16)
    p[chosen] = CHOSEN_P[rng.randint(0, CHOSEN_P.size, int(chosen.sum()))]
    nudge = cat == 17
    k = rng.randint(1024, 2048, n) + 0.5
    e = rng.randint(-6, 1, n)
    p[nudge] = (_sign(rng, n) * k * 2.0 ** (e - 10.0))[nudge].astype(np.float32)
    m[nudge] = (_sign(rng, n) * _logu(rng, 1e-26, 1e-24, n))[nudge]
    for a in (g, m, v):
        a[zero | chosen] = 0.0
    g[nudge] = 0.0
    v[nudge] = 0.0
    case = dict(p=p, g=g.astype(np.float32), m=m.astype(np.float32), v=v.astype(np.float32), cat=cat)
    for key in ("g", "m", "v"):
        a = np.abs(case[key])
        assert not ((a > 0) & (a < 1e-31)).any(), key
    return case


def _scalars(step, wd, lr):
    f = lambda x: np.float64(np.float32(x))
    b1, b2 = f(BETA1), f(BETA2)
    ob1 = np.float64(np.float32(1) - np.float32(BETA1))
    ob2 = np.float64(np.float32(1) - np.float32(BETA2))
    bc1, bc2 = 1.0 - b1 ** np.float64(step), 1.0 - b2 ** np.float64(step)
    return dict(b1=b1, b2=b2, ob1=ob1, ob2=ob2, eps=f(EPS), wd=f(wd), s=f(lr) / bc1,
                isb=1.0 / np.sqrt(bc2), bc1=bc1, bc2=bc2)


def adam_ref(p, g, m, v, step, wd, lr=LR):
    """One step in float64 -> dict P, M, V (the new p, m, v), D, and the conditioning numbers Mm, Mv
    of the module docstring, 's', 'isb', 'eps'."""
    c = _scalars(step, wd, lr)
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    wp = c["wd"] * p
    gp = g + wp
    ag = np.abs(g) + np.abs(wp)
    M = c["b1"] * m + c["ob1"] * gp
    V = c["b2"] * v + c["ob2"] * gp * gp
    Mm = c["b1"] * np.abs(m) + c["ob1"] * ag
    Mv = c["b2"] * np.abs(v) + c["ob2"] * (gp * gp + 2.0 * np.abs(gp) * ag)
    D = np.sqrt(V) * c["isb"] + c["eps"]
    return dict(P=p - c["s"] * M / D, M=M, V=V, D=D, Mm=Mm, Mv=Mv, s=c["s"], isb=c["isb"],
                eps=c["eps"], b1=c["b1"], b2=c["b2"])


def adam_tol(r, K=(K_M, K_V, K_P), dm_in=0.0, dv_in=0.0):
    """Bounds of one step from adam_ref's dict -> (tol_m, tol_v, tol_p, parts) with parts the pieces
    the ratios are measured on.  dm_in, dv_in: what the incoming m, v may already be off by (zero for
    one step from a given f32 state; FusedAdam's float64 trajectory carries them from step to step)."""
    km, kv, kp = K
    tm = km * U * r["Mm"] + TINY + r["b1"] * dm_in
    tv = kv * U * r["Mv"] + TINY + r["b2"] * dv_in
    d_lo = np.sqrt(np.maximum(r["V"] - tv, 0.0)) * r["isb"] + r["eps"]
    cond = r["s"] * r["Mm"] / d_lo
    eden = r["s"] * np.abs(r["M"]) * (1.0 / d_lo - 1.0 / r["D"]) + r["s"] * r["b1"] * dm_in / d_lo
    tp = U * np.abs(r["P"]) + kp * U * cond + eden + TINY
    return tm, tv, tp, dict(cond=cond, eden=eden)


def safe_ratio(num, den):
    """num / den where den > 0; without a bound (den == 0) the element must be exact"""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.where(num <= 0, -np.inf, np.inf)
    pos = den > 0
    out[pos] = num[pos] / den[pos]
    return out


def f16_rne_bits(p32):
    """RNE f16 cast of f32 values, as uint16 bits (numpy's cast rounds to nearest even, keeps
    subnormals and signed zeros, overflows to inf from 65520 on)"""
    with np.errstate(over="ignore"):
        return np.asarray(p32, dtype=np.float32).astype(np.float16).view(np.uint16)


def _f16_trunc_bits(p32):
    h = f16_rne_bits(p32).copy()
    with np.errstate(invalid="ignore"):
        up = np.abs(h.view(np.float16).astype(np.float64)) > np.abs(p32.astype(np.float64))
    h[up] -= 1                                           # one step toward zero (inf -> 65504)
    return h


def with_guard(a, n=None, fill=SENTINEL):
    """a [n] -> [n + GUARD], the tail filled with the sentinel"""
    a = np.asarray(a)
    out = np.full(a.shape[0] + GUARD, SENTINEL_H if a.dtype == np.uint16 else fill, dtype=a.dtype)
    out[:a.shape[0]] = a
    return out


def _adam_np(f, p, g, m, v, step, wd, lr, mutant=None):
    """the rule spelled in dtype f, every operation rounded in f -> (p', m', v')"""
    if mutant == "step_plus_one":
        step = step + 1
    c = _scalars(step, wd, lr)
    b1, b2, ob1, ob2 = (f(c[k]) for k in ("b1", "b2", "ob1", "ob2"))
    if mutant == "betas_swapped":
        b1, b2, ob1, ob2 = b2, b1, ob2, ob1
    s = f(c["s"]) if mutant != "no_bc1" else f(np.float32(lr))
    isb = f(c["isb"]) if mutant != "no_bc2" else f(1.0)
    eps, w = f(c["eps"]), f(c["wd"])
    p, g, m, v = (np.asarray(a).astype(f) for a in (p, g, m, v))
    # g' rounded once, as fmaf(wd, p, g): the product of two f32 is exact in float64
    gp = g if mutant == "decoupled_wd" else (np.float64(w) * p.astype(np.float64) + g.astype(np.float64)).astype(f)
    m2 = ob1 * gp + m * b1
    gv = g if mutant == "wd_missing_in_v" else gp
    v2 = (ob2 * gv) * gv + v * b2
    if mutant == "eps_under_sqrt":
        denom = np.sqrt(v2 * isb * isb + eps)
    elif mutant == "eps_scaled_by_bc2":
        denom = (np.sqrt(v2) + eps) * isb
    else:
        denom = np.sqrt(v2) * isb + eps
    base = p - f(np.float32(lr)) * w * p if mutant == "decoupled_wd" else p
    return base - s * (m2 / denom), m2, v2


def adam_f32(case, step, wd, lr=LR):
    """The restatement K is measured on -> got dict (p, m, v, shadow with guards)."""
    p, m, v = _adam_np(np.float32, case["p"], case["g"], case["m"], case["v"], step, wd, lr)
    return dict(p=with_guard(p), m=with_guard(m), v=with_guard(v), shadow=with_guard(f16_rne_bits(p)))


def adam_mutant(case, step, wd, mutant, shadow=True, lr=LR):
    """got dict of one mutant.  The arithmetic mutants are float64 restatements rounded to f32 at the
    end, the launch and shadow mutants start from adam_f32."""
    assert mutant in ADAM_MUTANTS
    n = case["p"].shape[0]
    args = (case["p"], case["g"], case["m"], case["v"])
    if mutant in ("no_bc2", "no_bc1", "eps_under_sqrt", "eps_scaled_by_bc2", "decoupled_wd",
                  "wd_missing_in_v", "betas_swapped", "step_plus_one"):
        p, m, v = (a.astype(np.float32) for a in _adam_np(np.float64, *args, step, wd, lr, mutant))
        h = f16_rne_bits(p)
    else:
        p64 = _adam_np(np.float64, *args, step, wd, lr)[0]
        p, m, v = _adam_np(np.float32, *args, step, wd, lr)
        h = f16_rne_bits(p)
        tail = slice(n - n % ADAM_VEC, n)
        if mutant == "tail_skipped":
            p[tail], m[tail], v[tail] = case["p"][tail], case["m"][tail], case["v"][tail]
            h[tail] = SENTINEL_H
        elif mutant == "tail_without_wd":
            p[tail], m[tail], v[tail] = _adam_np(np.float32, *(a[tail] for a in args), step, 0.0, lr)
            h[tail] = f16_rne_bits(p[tail])
        elif mutant == "pass_dropped":
            p[P:], m[P:], v[P:] = case["p"][P:], case["m"][P:], case["v"][P:]
            h[P:] = SENTINEL_H
        elif mutant == "pass_twice":
            p[P:], m[P:], v[P:] = _adam_np(np.float32, p[P:], case["g"][P:], m[P:], v[P:], step, wd, lr)
            h[P:] = f16_rne_bits(p[P:])
        elif mutant == "shadow_stale":
            h = f16_rne_bits(case["p"])
        elif mutant == "shadow_truncated":
            h = _f16_trunc_bits(p)
        elif mutant == "shadow_single_rounding":
            with np.errstate(over="ignore"):
                h = p64.astype(np.float16).view(np.uint16)
    got = dict(p=with_guard(p), m=with_guard(m), v=with_guard(v))
    got["shadow"] = with_guard(h) if shadow else None
    return got


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.uint16)


def p_update_ratio(err, r, parts, kp=K_P):
    """The part of p's bound that K_P scales, on its own: the largest (err - u |P'| - denominator term
    - A) / (K_P u s M_m / D_lo).  err / bound itself says little for p: u |P'| is p's last rounding,
    which half an ulp reaches whenever the significand of P' is near 1."""
    return float(safe_ratio(err - U * np.abs(r["P"]) - parts["eden"] - TINY, kp * U * parts["cond"]).max())


def adam_failures(case, step, wd, got, plain=None, lr=LR, K=(K_M, K_V, K_P), chunk=1 << 20, limit=8):
    """Every assertion on one step.  got: f32 'p', 'm', 'v' [n + GUARD] and uint16 'shadow'
    [n + GUARD] or None; plain: the same call's p, m, v without a shadow pointer, or None.
    -> (fails, worst): fails a list of (element, output, message), at most `limit` per kind; worst the
    largest err / bound of m, v, p and 'p_update' (p_update_ratio).  Works in chunks: 4 P elements never sit in float64 at once."""
    n = case["p"].shape[0]
    fails, worst = [], dict(m=0.0, v=0.0, p=0.0, p_update=-np.inf)
    count = {}

    def add(idx, name, msg):
        for i in np.atleast_1d(idx):
            count[(name, msg[:12])] = count.get((name, msg[:12]), 0) + 1
            if count[(name, msg[:12])] <= limit:
                fails.append((int(i), name, msg))

    for name in ("p", "m", "v", "shadow"):
        a = got[name]
        if a is None:
            continue
        assert a.shape[0] == n + GUARD, (name, a.shape, n)
        want = SENTINEL_H if name == "shadow" else np.float32(SENTINEL)
        add(n + np.flatnonzero(a[n:] != want), name, "guard past n overwritten")
        if plain is not None and name != "shadow":
            add(np.flatnonzero(_bits(a) != _bits(plain[name])), name, "differs without a shadow pointer")
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        sl = slice(lo, hi)
        p0, g0, m0, v0 = (case[k][sl] for k in ("p", "g", "m", "v"))
        r = adam_ref(p0, g0, m0, v0, step, wd, lr)
        for key in ("M", "V"):
            a = np.abs(r[key])
            assert not ((a > 0) & (a < NO_SUBNORMAL_BELOW)).any(), "subnormal %s in the reference" % key
        tm, tv, tp, parts = adam_tol(r, K)
        for name, ref, tol in (("m", r["M"], tm), ("v", r["V"], tv), ("p", r["P"], tp)):
            err = np.abs(got[name][sl].astype(np.float64) - ref)
            bad = ~(err <= tol)
            ratio = err / tol
            worst[name] = max(worst[name], float(np.nanmax(ratio)))
            if name == "p":
                worst["p_update"] = max(worst["p_update"], p_update_ratio(err, r, parts, K[2]))
            for i in np.flatnonzero(bad)[:limit]:
                add(lo + i, name, "err %.3e > tol %.3e (ref %.9e, got %.9e)" % (
                    err[i], tol[i], ref[i], got[name][lo + i]))
        if np.float32(wd) == 0:
            still = (g0 == 0) & (m0 == 0) & (v0 == 0)
            add(lo + np.flatnonzero(still & (_bits(got["p"][sl]) != _bits(p0))), "p",
                "nothing moves: p lost its bits")
            for name in ("m", "v"):
                add(lo + np.flatnonzero(still & (_bits(got[name][sl]) != 0)), name, "nothing moves: not +0")
        if got["shadow"] is not None:
            add(lo + np.flatnonzero(got["shadow"][sl] != f16_rne_bits(got["p"][sl])), "shadow",
                "not the RNE cast of the stored p")
    return fails, worst


def assert_none(fails, what=""):
    if fails:
        raise AssertionError("%s: %d failures; first: %s[%d]: %s" % (
            what, len(fails), fails[0][1], fails[0][0], fails[0][2]))


def adam_measure(case, step, wd, got, kv=K_V, lr=LR):
    """largest (err - A) / (u M) of m, v and (err - A - u |P'| - denominator term) / (u s M_m / D_lo) of p
    (what K_M, K_V, K_P have to cover; p with dv from kv)"""
    n = case["p"].shape[0]
    r = adam_ref(case["p"], case["g"], case["m"], case["v"], step, wd, lr)
    _, _, _, parts = adam_tol(r, (0.0, kv, 0.0))
    out = {}
    for name, ref, den, extra in (("m", r["M"], r["Mm"], 0.0), ("v", r["V"], r["Mv"], 0.0),
                                  ("p", r["P"], parts["cond"], parts["eden"] + U * np.abs(r["P"]))):
        err = np.abs(got[name][:n].astype(np.float64) - ref)
        out[name] = float(safe_ratio(err - TINY - extra, U * den).max())
    return out


# ---------------------------------------------------------------------------------- loss ----------

LOSS_BLOCK = 256                      # loss.hip: kLossBlock (one partial per block, one finish block)
LOSS_SIZES = (1, 63, 64, 255, 256, 257, 65280, 65536, 65537, 70001)
LOSS_WEIGHTS = (0.0, 1e-2, 0.3)
LOSS_KINDS = ("mixed", "zero", "spike")
K_LOSS = 16                           # see the module docstring; test_loss_measured_K re-derives it
LOSS_MUTANTS = ("mean_over_R", "no_floor", "d_var_without_half", "weight_missing_in_d_var",
                "partials_past_256_dropped", "last_block_tail_dropped", "sq_err_of_sqrt")
LOSS_OUT = ("loss", "color_loss", "var_loss", "sq_err_sum")


def loss_mutant_applies(mutant, n_rays, weight, kind):
    if mutant in ("d_var_without_half",):
        return weight != 0
    if mutant == "weight_missing_in_d_var":
        return True
    if mutant == "partials_past_256_dropped":          # the finish kernel's loop runs once only
        return n_rays > 256 * LOSS_BLOCK and kind == "spike"
    if mutant == "last_block_tail_dropped":             # the rays of a partial last block
        return n_rays % LOSS_BLOCK != 0 and kind == "spike"
    if mutant == "sq_err_of_sqrt":                      # 1e-4 per term against n u of terms of ~0.1
        return kind != "mixed" or n_rays <= 257
    return True


@functools.lru_cache(maxsize=None)
def loss_case(n_rays, kind, seed=0):
    """-> dict of f32 numpy arrays colors, gt [R, 3], var [R]; shared, nobody writes into them"""
    assert kind in LOSS_KINDS
    rng = np.random.RandomState(9000 + 13 * n_rays + seed)
    gt = rng.rand(n_rays, 3).astype(np.float32)
    sgn = _sign(rng, (n_rays, 3))
    big = rng.uniform(-1.0, 1.0, (n_rays, 3))
    pick = rng.randint(0, 4, (n_rays, 3))
    err = np.choose(pick, [np.zeros((n_rays, 3)), sgn * 1e-6, sgn * 1e-3, big])
    vpick = rng.randint(0, 3, n_rays)
    var = np.choose(vpick, [np.zeros(n_rays), np.full(n_rays, 1e-6), 2.0 * rng.rand(n_rays)])
    if kind == "zero":
        err[:] = 0.0
    elif kind == "spike":
        err = sgn * 1e-3
        err[-1] = (0.5, -0.7, 0.9)
        var[:] = 1e-6
        var[-1] = 1.5
    colors = (gt.astype(np.float64) + err).astype(np.float32)
    colors[err == 0] = gt[err == 0]
    return dict(colors=colors, gt=gt, var=var.astype(np.float32))


def _loss_formula(f, case, weight, mutant=None, blocked=False):
    """the formula in dtype f -> dict out4 [4] (LOSS_OUT), d_colors [R, 3], d_var [R].  blocked: the
    sums go through one partial per 256 rays, as the kernels' do; the sum mutants need it."""
    c, gt, var = (case[k].astype(f) for k in ("colors", "gt", "var"))
    R = c.shape[0]
    w = f(np.float32(weight))
    floor_c = f(0.0) if mutant == "no_floor" else f(np.float32(1e-4))
    e = c - gt
    e2 = e * e
    with np.errstate(invalid="ignore", divide="ignore"):
        rt = np.sqrt(e2 + floor_c)
        nc = f(R) if mutant == "mean_over_R" else f(3.0) * f(R)
        d_colors = e / rt * (f(1.0) / nc)
    rv = np.sqrt(var + f(np.float32(1e-2)))
    half = f(1.0) if mutant == "d_var_without_half" else f(0.5)
    wv = f(1.0) if mutant == "weight_missing_in_d_var" else w
    d_var = wv * half / rv * (f(1.0) / f(R))
    sq_terms = (e2 + floor_c) if mutant == "sq_err_of_sqrt" else e2

    def total(x):                       # x [R] per-ray terms
        if not blocked:
            return x.sum(dtype=f)
        nb = -(-R // LOSS_BLOCK)
        pad = np.zeros(nb * LOSS_BLOCK, dtype=f)
        pad[:R] = x
        if mutant == "last_block_tail_dropped" and R % LOSS_BLOCK:
            pad[(nb - 1) * LOSS_BLOCK:] = 0
        part = pad.reshape(nb, LOSS_BLOCK).sum(axis=1, dtype=f)
        if mutant == "partials_past_256_dropped":
            part = part[:256]
        return np.cumsum(part, dtype=f)[-1]

    a = total(((rt[:, 0] + rt[:, 1]) + rt[:, 2]).astype(f))
    b = total(rv)
    s = total(((sq_terms[:, 0] + sq_terms[:, 1]) + sq_terms[:, 2]).astype(f))
    cl, vl = a / nc, b / f(R)
    return dict(out4=np.array([cl + vl * w, cl, vl, s], dtype=f), d_colors=d_colors, d_var=d_var)


@functools.lru_cache(maxsize=None)
def loss_ref(n_rays, kind, weight, seed=0):
    """float64 reference and the bound of every output -> dict out4, d_colors, d_var, tol_out4"""
    case = loss_case(n_rays, kind, seed)
    r = _loss_formula(np.float64, case, weight)
    R = n_rays
    loss, cl, vl, sq = r["out4"]
    w = float(np.float32(weight))
    t_cl = U * (3 * R + K_LOSS) * cl          # every term positive: sum|x| is the sum
    t_vl = U * (R + K_LOSS) * vl
    r["tol_out4"] = np.array([t_cl + w * t_vl + K_LOSS * U * abs(loss), t_cl, t_vl,
                              U * (3 * R + K_LOSS) * sq])
    r["any_order"] = U * np.array([3 * R * cl + w * R * vl, 3 * R * cl, R * vl, 3 * R * sq])
    return r


def loss_f32(case, weight):
    return _loss_formula(np.float32, case, weight, blocked=True)


def loss_mutant(case, weight, mutant):
    assert mutant in LOSS_MUTANTS
    r = _loss_formula(np.float64, case, weight, mutant, blocked=True)
    with np.errstate(invalid="ignore"):
        return {k: v.astype(np.float32) for k, v in r.items()}


def loss_failures(case, ref, got, factor=1.0):
    """got: f32 out4 [4], d_colors [R, 3], d_var [R] (the gradients times `factor`, exact in f32: the
    upstream factor of host.train_loss) -> (fails, worst err / bound per output)"""
    fails, worst = [], {}
    err = np.abs(got["out4"].astype(np.float64) - ref["out4"])
    for i, name in enumerate(LOSS_OUT):
        worst[name] = float(safe_ratio(err[i], ref["tol_out4"][i]))
        if not err[i] <= ref["tol_out4"][i]:
            fails.append((i, name, "err %.3e > tol %.3e (ref %.9e)" % (err[i], ref["tol_out4"][i], ref["out4"][i])))
    for name in ("d_colors", "d_var"):
        want = ref[name].ravel() * factor
        g = got[name].astype(np.float64).ravel()
        e = np.abs(g - want)
        tol = (K_LOSS + (1 if factor != 1.0 else 0)) * U * np.abs(want)
        worst[name] = float(safe_ratio(e, tol).max())
        for i in np.flatnonzero(~(e <= tol))[:8]:
            fails.append((int(i), name, "err %.3e > tol %.3e (ref %.9e)" % (e[i], tol[i], want[i])))
    zero = (case["colors"] == case["gt"]).ravel()
    for i in np.flatnonzero(zero & (got["d_colors"].ravel() != 0))[:8]:
        fails.append((int(i), "d_colors", "zero error: not exactly 0"))
    if zero.all() and got["out4"][3] != 0:
        fails.append((3, "sq_err_sum", "all-zero error: not exactly 0"))
    return fails, worst


def loss_nan_failures(got, ray, channel):
    """colors[ray, channel] was NaN"""
    fails = []
    o = got["out4"]
    for i in (0, 1, 3):
        if not np.isnan(o[i]):
            fails.append((i, LOSS_OUT[i], "not NaN"))
    if np.isnan(o[2]):
        fails.append((2, "var_loss", "NaN"))
    nan = np.isnan(got["d_colors"])
    if not nan[ray, channel]:
        fails.append((3 * ray + channel, "d_colors", "the poisoned element is not NaN"))
    nan[ray] = False
    for i in np.flatnonzero(nan.ravel())[:8]:
        fails.append((int(i), "d_colors", "NaN outside the poisoned ray"))
    if np.isnan(got["d_var"]).any():
        fails.append((0, "d_var", "NaN"))
    return fails


# ---------------------------------------------------------------------------------- scatter -------

K_SPAN = 64                           # scatter.hip: kSpan
SCATTER_E = 8
SCATTER_UNNAMED = (3, 6)
SCATTER_C = (1, 3, 16, 17)
SCATTER_N = (1, 64, 65, 3000)
SCATTER_MUTANTS = ("span_first_dropped", "run_flush_missing_at_span_end", "accumulates_into_demb",
                   "channel_pad_leak")
# (length, id): positions in the comments.  Runs start, end and cross at multiples of 64.
_RUNS = ((64, 2), (1, 0), (63, 5), (65, 1), (63, 7), (200, 4), (56, 0), (64, -1), (64, 2), (65, 7),
         (63, SCATTER_E), (64, 1), (1, 5), (1, 4), (1, 5), (61, 0), (200, 2), (200, 1), (48, 5),
         (63, 4), (1, 7), (65, 0), (63, 2), (64, 5), (200, 7), (200, 0), (120, 4), (64, 1), (64, 1),
         (65, 5), (127, 2), (63, 0), (1, 4), (500, 7))


def scatter_mutant_applies(mutant, n_all, C):
    if mutant == "channel_pad_leak":
        return C & (C - 1) != 0 and n_all > 1           # cpad > C, and a sample behind the first
    return True


@functools.lru_cache(maxsize=None)
def scatter_ids(n_all):
    ids = np.concatenate([np.full(ln, e, dtype=np.int32) for ln, e in _RUNS])
    assert ids.shape[0] >= max(SCATTER_N) and n_all <= ids.shape[0]
    return ids[:n_all].copy()


@functools.lru_cache(maxsize=None)
def scatter_case(n_all, C, seed=0):
    """-> dict ids int32 [n_all], dsum f32 [n_all, C], k int64 (dsum 2^10)"""
    rng = np.random.RandomState(7000 + 17 * n_all + C + seed)
    ids = scatter_ids(n_all)
    k = rng.randint(-4096, 4097, (n_all, C)).astype(np.int64)
    dsum = (k / 1024.0).astype(np.float32)
    assert (dsum.astype(np.float64) * 1024 == k).all()
    for e in range(SCATTER_E):            # every partial sum, in any order, is exact in f32
        assert np.abs(k[ids == e]).sum(axis=0).max(initial=0) < 2 ** 24
    return dict(ids=ids, dsum=dsum, k=k)


def scatter_ref(case):
    """-> f32 [E, C], exact"""
    ids, k = case["ids"], case["k"]
    out = np.zeros((SCATTER_E, k.shape[1]), dtype=np.int64)
    ok = (ids >= 0) & (ids < SCATTER_E)
    np.add.at(out, ids[ok], k[ok])
    res = (out / 1024.0).astype(np.float32)
    assert (res.astype(np.float64) * 1024 == out).all()
    return res + np.float32(0.0)          # no -0


def scatter_layout_facts(n_all):
    """what the layout holds, for the CPU test: run starts / ends on, off and across span edges"""
    ids = scatter_ids(n_all)
    starts = np.flatnonzero(np.diff(ids, prepend=ids[0] - 1))
    ends = np.append(starts[1:], n_all)
    return dict(starts=starts, ends=ends, lengths=ends - starts,
                crossing=int(((starts // K_SPAN) != ((ends - 1) // K_SPAN)).sum()))


def scatter_mutant(case, mutant):
    """the kernel's span walk in int64 with one defect -> f32 [E C + GUARD] as the caller's buffer"""
    assert mutant in SCATTER_MUTANTS
    ids, k = case["ids"], case["k"]
    n_all, C = k.shape
    cpad = 1
    while cpad < C:
        cpad <<= 1
    flat = np.zeros(SCATTER_E * C + GUARD, dtype=np.int64)
    kf = np.append(k.ravel(), np.zeros(cpad, dtype=np.int64))
    chans = cpad if mutant == "channel_pad_leak" else C
    for lo in range(0, n_all, K_SPAN):
        hi = min(lo + K_SPAN, n_all)
        for c in range(chans):
            cur, acc = ids[lo], 0
            for p in range(lo, hi):
                if ids[p] != cur:
                    if 0 <= cur < SCATTER_E:
                        flat[cur * C + c] += acc
                    cur, acc = ids[p], 0
                if not (mutant == "span_first_dropped" and p == lo):
                    acc += kf[p * C + c]
            if 0 <= cur < SCATTER_E and mutant != "run_flush_missing_at_span_end":
                flat[cur * C + c] += acc
    out = (flat / 1024.0).astype(np.float32)
    out[SCATTER_E * C:] += np.float32(SENTINEL)
    if mutant == "accumulates_into_demb":
        out[:SCATTER_E * C] += np.float32(SENTINEL)
    return out


def scatter_failures(case, got):
    """got: f32 [E C + GUARD], pre-filled with SENTINEL before the call"""
    C = case["k"].shape[1]
    ref = scatter_ref(case).ravel()
    fails = []
    body, guard = got[:SCATTER_E * C], got[SCATTER_E * C:]
    assert guard.shape[0] == GUARD
    for i in np.flatnonzero(guard != np.float32(SENTINEL))[:8]:
        fails.append((SCATTER_E * C + int(i), "demb", "guard past n_emb C overwritten"))
    for i in np.flatnonzero(_bits(body) != _bits(ref))[:16]:
        what = "unnamed image: not +0" if i // C in SCATTER_UNNAMED else "not the exact sum"
        fails.append((int(i), "demb", "%s: got %r, want %r" % (what, float(body[i]), float(ref[i]))))
    return fails
