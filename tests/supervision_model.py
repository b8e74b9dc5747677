"""Numpy model, in exact integers and float64, of masked training's kernels: the mask pack and the
Philox draw of pixel_mask.hip (f2n_mask_pack, f2n_draw_pixels_masked) and the supervised loss of
loss_sup.hip (f2n_loss_sup_fwd) with its gradients and per-element bounds.  No tests in here:
tests/test_supervision_model_cpu.py checks the model on the CPU (known-answer vector, finite
differences, the formula of loss.hip); tests/test_gpu_pixel_mask.py, tests/test_gpu_loss_sup.py and
tests/test_gpu_supervised_step.py hold the HIP kernels to it.  Written from the definitions in
include/f2nerf_hip.h, not from the kernels.

PACK.  Global pixel g = (e*h + i)*w + j is bit (g & 31) of word (g >> 5).

DRAW.  Attempt a of ray r: Philox4x32-10, key (seed_lo, seed_hi), counter (r, a, 0, 0); cam = mulhi(x0,
E), i = mulhi(x1, h), j = mulhi(x2, w); the first attempt on a valid pixel is kept, tries = a + 1; all A
missed: tries = 0 and the last attempt stays.  philox4x32_10 is vectorised over uint64 arrays;
philox_scalar is the same algorithm in Python integers, the check of the vectorised one.

LOSS.  loss_ref evaluates the definition in float64 on the f32 inputs.  A ray with m == 0 contributes
nothing and has zero gradients whatever its other inputs hold.

Bounds, fixed before the first GPU run and counted from the EVALUATION ORDER in the header comment of
loss_sup.hip, u = 2^-24, first order in u and multiplied by 1 / (1 - 64 u) for the rest.  The weights
of the test cases are >= 0, so sum |m| = sum m.
  An element whose value v passes through k roundings, each relative to the running value, is within
  k u |v|; where a subtraction sits on the path (e = C - g) the absolute error of its operands is
  carried instead.  Per channel, alpha given:
      om (1), tb = om bg (1), g = fma(a, gt, tb) (1):  |dg| <= u G,  G = |a gt| + 3 |om bg|   (else G = 0)
      e = C - g (1):                                   |de| <= u Ee, Ee = |e| + G
      e2 = e e (1), rt = sqrt(e2 + 1e-4) (add 1, sqrt 1: the square root halves what came before):
                                                       |drt| <= u (|e| / rt Ee + 2 rt)
      q = e / rt (1):  dq/de = 1e-4 / rt^3:            |dq| <= u (1e-4 / rt^3 Ee + 3 |q|)
  Per-ray terms of the sums (two adds and the product with m: 3 more roundings):
      colour  T_r = |m| sum_c (|e| / rt Ee + 5 rt)
      sq_err  T_r = |m| sum_c (2 |e| Ee + 4 e2)
      var     rv = sqrt(var + 1e-2) (1.5), times m (1):        T_r = 2.5 |m| rv
      opac    do = O - a (1), do do (1 + 2 x 1), times m (1):  T_r = 4 |m| do^2
      sum_m   the terms are the inputs: T_r = 0
  A sum of terms t_r whose own errors are u T_r, each passing through at most
      D = 20 + ceil(n_blocks / 256)
  additions (6 in the DPP tree and 4 wave totals, twice, and the strided walk over the partials), is
  within u (sum T_r + D sum |t_r|): the worst case of any tree of that depth.
  Finish: W from sum_m (relative error rW = D u for m >= 0; none when W is replaced by 1);
      colour = s / (3 W): 2 roundings,  var = s / W, opac = s / W: 1 rounding
      |d colour| <= ds / (3 W) + |colour| (2 u + rW),   |d var| <= ds / W + |var| (u + rW), opac alike
      loss = (colour + var vw) + opac ow: 2 products, 2 adds:
      |d loss| <= dcolour + |vw| dvar + |ow| dopac + 3 u (|colour| + |var vw| + |opac ow|)
  Gradients (K_* below are the k of the issue's k u |value|):
      d_colors = (m q) i3,  i3 = 1 / (3 W): q (3, plus the carried 1e-4 / rt^3 Ee), m (1), i3 (2),
                 product (1):  K_DCOL = 7, plus rW |v| and u |m| 1e-4 / rt^3 Ee / (3 W)
      d_var    = (0.5 vw) / rv m i1: rv (1.5), division (1), m (1), i1 (1), product (1): K_DVAR = 6
                 (5.5 rounded up), plus rW |v|
      d_opac   = (2 ow) do m i1: do (1), product (1), m (1), i1 (1), product (1): K_DOP = 5, plus rW |v|
"""
import functools

import numpy as np

U = 2.0 ** -24
F32 = np.float32
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

# ---------------------------------------------------------------------------------- philox --------


def philox_scalar(counter, key):
    """Philox4x32-10 in Python integers: counter (c0, c1, c2, c3), key (k0, k1) -> (x0, x1, x2, x3)"""
    c0, c1, c2, c3 = (int(c) & MASK32 for c in counter)
    k0, k1 = (int(k) & MASK32 for k in key)
    for n in range(10):
        if n > 0:
            k0 = (k0 + W0) & MASK32
            k1 = (k1 + W1) & MASK32
        p0, p1 = M0 * c0, M1 * c2
        hi0, lo0 = p0 >> 32, p0 & MASK32
        hi1, lo1 = p1 >> 32, p1 & MASK32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return c0, c1, c2, c3


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """the same on uint64 arrays holding 32-bit values (broadcast against each other)"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK32) for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = np.uint64(k0 & MASK32), np.uint64(k1 & MASK32)
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for n in range(10):
        if n > 0:
            k0 = (k0 + np.uint64(W0)) & m32
            k1 = (k1 + np.uint64(W1)) & m32
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2     # < 2^64: no wrap
        hi0, lo0 = p0 >> s32, p0 & m32
        hi1, lo1 = p1 >> s32, p1 & m32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return c0, c1, c2, c3


def mulhi(x, n):
    return (np.asarray(x, dtype=np.uint64) * np.uint64(n)) >> np.uint64(32)


# ---------------------------------------------------------------------------------- masks ---------

E, H, W = 3, 5, 70                     # 1050 pixels: no multiple of 32 or 64, rows straddle words
MASKS = ("checker", "ones", "image1_off", "one_pixel")
ONE_PIXEL = (2, 3, 41)                 # the valid pixel of "one_pixel"
DRAW_SEED = 0x5EED0F2A9C3B7D11         # both halves of the key are used
DRAW_N = (1, 63, 257)
DRAW_A = (1, 32)


@functools.lru_cache(maxsize=None)
def mask(name):
    """uint8 [E, H, W], read-only"""
    assert name in MASKS
    e, i, j = np.meshgrid(np.arange(E), np.arange(H), np.arange(W), indexing="ij")
    if name == "checker":
        m = (e + i + j) % 2 == 0
    elif name == "ones":
        m = np.ones((E, H, W), dtype=bool)
    elif name == "image1_off":
        m = e != 1
    else:
        m = np.zeros((E, H, W), dtype=bool)
        m[ONE_PIXEL] = True
    m = (m * np.uint8(255 if name == "checker" else 1)).astype(np.uint8)   # any non-zero is valid
    m.setflags(write=False)
    return m


def pack(m):
    """uint8 / bool [E, h, w] -> (words uint32 [ceil(n / 32)], count int)"""
    flat = (np.asarray(m).reshape(-1) != 0)
    n = flat.shape[0]
    words = np.zeros((n + 31) // 32, dtype=np.uint64)
    g = np.flatnonzero(flat)
    np.bitwise_or.at(words, g >> 5, np.uint64(1) << (g & 31).astype(np.uint64))
    return words.astype(np.uint32), int(flat.sum())


def draw(m, n, seed, attempts):
    """-> cam [n] i32, ij [n, 2] i32, tries [n] i32 of the masked draw on the uint8 mask m"""
    m = np.asarray(m)
    e_, h_, w_ = m.shape
    valid = m.reshape(-1) != 0
    seed_lo, seed_hi = seed & MASK32, (seed >> 32) & MASK32
    r = np.arange(n, dtype=np.uint64)
    cam = np.zeros(n, dtype=np.int64)
    ij = np.zeros((n, 2), dtype=np.int64)
    tries = np.zeros(n, dtype=np.int64)
    for a in range(attempts):
        open_ = tries == 0
        if not open_.any():
            break
        x0, x1, x2, _ = philox4x32_10(r, a, 0, 0, seed_lo, seed_hi)
        c, i, j = mulhi(x0, e_).astype(np.int64), mulhi(x1, h_).astype(np.int64), mulhi(x2, w_).astype(np.int64)
        cam[open_], ij[open_, 0], ij[open_, 1] = c[open_], i[open_], j[open_]
        hit = open_ & valid[(c * h_ + i) * w_ + j]
        tries[hit] = a + 1
    return cam.astype(np.int32), ij.astype(np.int32), tries.astype(np.int32)


@functools.lru_cache(maxsize=None)
def shared_draw(name, n, attempts):
    """the model's draw of one GPU case, computed once (read-only arrays)"""
    out = draw(mask(name), n, DRAW_SEED, attempts)
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------- loss ----------

LOSS_SIZES = (1, 255, 257, 513)
LOSS_BLOCK = 256
WEIGHT_KINDS = (None, "mixed", "allzero")
VAR_WEIGHT = 0.3
OPACITY_WEIGHT = 0.7
K_DCOL, K_DVAR, K_DOP = 7, 6, 5
SLACK = 1.0 / (1.0 - 64 * U)
SENTINEL = -7777.0
GUARD = 8


def sum_depth(n_rays):
    n_blocks = -(-n_rays // LOSS_BLOCK)
    return 20 + -(-n_blocks // 256)


@functools.lru_cache(maxsize=None)
def loss_case(n, weight_kind, with_alpha, seed=0):
    """f32 inputs (read-only): colors, gt, bg [n, 3], var, opacity [n], and ray_weight / alpha [n] or
    None.  Some colours equal their target exactly, alphas include exact 0 and 1, weights include
    exact zeros, ones and fractions; the first masked ray's colour is NaN (a masked ray is not read)."""
    assert weight_kind in WEIGHT_KINDS
    rng = np.random.RandomState(4100 + 7 * n + seed)
    c = dict(colors=rng.rand(n, 3), gt=rng.rand(n, 3), bg=rng.rand(n, 3), var=0.05 * rng.rand(n),
             opacity=rng.rand(n))
    c = {k: v.astype(F32) for k, v in c.items()}
    alpha = None
    if with_alpha:
        alpha = rng.rand(n)
        pick = rng.rand(n)
        alpha[pick < 0.25] = 0.0
        alpha[pick > 0.75] = 1.0
        alpha = alpha.astype(F32)
        c["opacity"][::5] = alpha[::5]                      # O == a exactly
    same = rng.rand(n) < 0.1                                # C == gt' exactly (alpha 1 or none)
    if with_alpha:
        same &= alpha == 1
    c["colors"][same] = c["gt"][same]
    m = None
    if weight_kind == "mixed":
        m = rng.choice([0.0, 1.0, 0.25, 1.75, 0.6180339887], size=n)
        m[n // 2] = 0.0                                     # an exact zero whatever n is
        if n > 1:
            m[0] = 1.0
        m = m.astype(F32)
    elif weight_kind == "allzero":
        m = np.zeros(n, dtype=F32)
    if m is not None:
        c["colors"][np.flatnonzero(m == 0)[0], 1] = np.nan
    c["ray_weight"], c["alpha"] = m, alpha
    for v in c.values():
        if v is not None:
            v.setflags(write=False)
    return c


def loss_ref(case, var_weight, opacity_weight, with_opacity):
    """The definition in float64 -> dict of out [6], d_colors [n, 3], d_var [n], d_opacity [n] or None,
    and tol_* of the same shapes: the bounds of the module docstring."""
    f = lambda k: None if case[k] is None else case[k].astype(np.float64)
    C, gt, bg, var, O, m, a = (f(k) for k in ("colors", "gt", "bg", "var", "opacity", "ray_weight", "alpha"))
    n = C.shape[0]
    vw, ow = float(F32(var_weight)), float(F32(opacity_weight))
    if m is None:
        m = np.ones(n)
    on = m != 0
    with_op = a is not None and with_opacity
    if a is not None:
        om = 1.0 - a
        g = a[:, None] * gt + om[:, None] * bg
        G = np.abs(a[:, None] * gt) + 3.0 * np.abs(om[:, None] * bg)
    else:
        g, G = gt, np.zeros_like(gt)
    with np.errstate(invalid="ignore"):
        e = np.where(on[:, None], C - g, 0.0)               # a masked ray is not read
    G = np.where(on[:, None], G, 0.0)
    Ee = np.abs(e) + G
    rt = np.sqrt(e * e + 1e-4)
    q = e / rt
    rv = np.sqrt(var + 1e-2)
    mm = np.abs(m)
    t_col = m * rt.sum(1)
    t_sq = m * (e * e).sum(1)
    t_var = m * rv
    T_col = mm * (np.abs(e) / rt * Ee + 5.0 * rt).sum(1)
    T_sq = mm * (2.0 * np.abs(e) * Ee + 4.0 * e * e).sum(1)
    T_var = 2.5 * mm * rv
    if with_op:
        do = np.where(on, O - a, 0.0)
        t_op, T_op = m * do * do, 4.0 * mm * do * do
    else:
        t_op = T_op = np.zeros(n)
    D = sum_depth(n)
    s_m = m.sum()
    Wd = s_m if s_m > 0 else 1.0
    rW = D * U if s_m > 0 else 0.0

    def summed(t, T):
        return t.sum(), U * (T.sum() + D * np.abs(t).sum())

    s_col, ds_col = summed(t_col, T_col)
    s_var, ds_var = summed(t_var, T_var)
    s_op, ds_op = summed(t_op, T_op)
    s_sq, ds_sq = summed(t_sq, T_sq)
    colour, var_l, opac = s_col / (3.0 * Wd), s_var / Wd, s_op / Wd
    d_colour = ds_col / (3.0 * Wd) + abs(colour) * (2.0 * U + rW)
    d_varl = ds_var / Wd + abs(var_l) * (U + rW)
    d_opac = ds_op / Wd + abs(opac) * (U + rW)
    loss = colour + vw * var_l + ow * opac
    d_loss = (d_colour + abs(vw) * d_varl + abs(ow) * d_opac +
              3.0 * U * (abs(colour) + abs(var_l * vw) + abs(opac * ow)))
    out = np.array([loss, colour, var_l, opac, s_sq, s_m])
    tol_out = np.array([d_loss, d_colour, d_varl, d_opac, ds_sq, D * U * mm.sum()]) * SLACK
    d_colors = m[:, None] * q / (3.0 * Wd)
    tol_dc = (np.abs(d_colors) * (K_DCOL * U + rW) +
              U * mm[:, None] * (1e-4 / rt ** 3) * Ee / (3.0 * Wd)) * SLACK
    d_var = m * 0.5 * vw / rv / Wd
    tol_dv = np.abs(d_var) * (K_DVAR * U + rW) * SLACK
    res = dict(out=out, tol_out=tol_out, d_colors=d_colors, tol_d_colors=tol_dc, d_var=d_var,
               tol_d_var=tol_dv, d_opacity=None, tol_d_opacity=None, masked=~on)
    if with_op:
        res["d_opacity"] = m * 2.0 * ow * do / Wd
        res["tol_d_opacity"] = np.abs(res["d_opacity"]) * (K_DOP * U + rW) * SLACK
    return res


def loss_value(colors, var, opacity, case, var_weight, opacity_weight, with_opacity):
    """loss alone in float64 for other colours / var / opacity (finite differences)"""
    c = dict(case)
    c.update(colors=colors, var=var, opacity=opacity)
    return loss_ref(c, var_weight, opacity_weight, with_opacity)["out"][0]


def plain_loss(colors, gt, var, var_weight):
    """the formula of loss.hip in float64: {loss, color_loss, var_loss, sq_err_sum}"""
    C, gt, var = (np.asarray(x, dtype=np.float64) for x in (colors, gt, var))
    e = C - gt
    color_loss = np.sqrt(e * e + 1e-4).mean()
    var_loss = np.sqrt(var + 1e-2).mean()
    return np.array([color_loss + float(F32(var_weight)) * var_loss, color_loss, var_loss, (e * e).sum()])


def loss_failures(ref, got):
    """Every assertion the GPU tests make on one call: list of messages; and the largest
    error-to-bound ratio per output name."""
    fails, worst = [], {}
    for name in ("out", "d_colors", "d_var", "d_opacity"):
        want = ref[name]
        if want is None:
            continue
        g = np.asarray(got[name], dtype=np.float64)
        assert g.shape == want.shape, (name, g.shape, want.shape)
        tol = ref["tol_" + name]
        err = np.abs(g - want)
        bad = ~(err <= tol)
        for i in np.argwhere(bad)[:5]:
            i = tuple(i)
            fails.append("%s%s: got %.9g want %.9g err %.3e > tol %.3e" % (
                name, list(i), g[i], want[i], err[i], tol[i]))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
        worst[name] = float(ratio.max())
        if name != "out":
            rows = ref["masked"]
            bits = np.asarray(got[name], dtype=F32).view(np.int32)
            if bits[rows].any():
                fails.append("%s: a ray with weight 0 has a gradient that is not exactly +0" % name)
    return fails, worst
