"""Inputs, a float64 restatement and per-element rounding bounds for the density logit's spatial
gradient, f2n_density_grad, and the per-ray normals composited from it, f2n_ray_normals
(density_grad.hiph, density_grad.hip).  No tests in here: tests/test_density_grad_model_cpu.py checks
the restatement and the bounds on the CPU, tests/test_gpu_density_grad.py and
tests/test_gpu_render_normals.py hold the HIP kernels to them.  The helpers (fields, cells, the
value-and-bound arithmetic, the contraction's models, `ambiguous`) are tests/ray_grad_model.py's.

The function.  logit(p) = b0 + sum_l sum_k w0[lF+k] sum_d w_d(frac_l) f_{l,d,k}: x = contract(p),
pt_l = x mul_l + bias_l, frac_l = pt_l - floor(pt_l), the eight rows of the cell through the float32
chain of the kernels (oracle.kernels.hash_fwd(want_idx=True) at the float32 contracted point), f the f16
table rows.  Its gradient at the contracted point, per level and axis (corner d = 4dx + 2dy + dz,
s_d = sum_k w0[lF+k] f_{d,k}, a, b, c the fractions and a1, b1, c1 their complements):
  gx_l = mul_l [(s4-s0) b1 c1 + (s5-s1) b1 c + (s6-s2) b c1 + (s7-s3) b c], gy_l, gz_l likewise,
summed over the levels, then through the contraction's symmetric Jacobian at the float32 raw point
(ray_grad_model.contract_bwd_model: identity for |p| <= 1, a G + (a'/n)(p.G) p outside, NaN at
|p| == 0).  Per ray: n^ = 0 where g == 0 in all three, else -g / |g|; N_r = sum_k w_k n^_k.

Bound E, first order, per element, u = 2^-24, followed operation by operation through the
absolute-value form of each formula with ray_grad_model's _add .. _sqrt (propagated error plus
u |result| per float32 operation).  The operations, with the lines of density_grad.hiph they are:
  frac           the float32 pt carries E_pt = E_x mul + u |pt| (one fmaf, density_grad.hiph:48-50, the
                 same as hash_grid.hiph:69-71); pt - floorf(pt) is exact (:51)   -> (frac, E_pt)
  a1, b1, c1     1 - frac: one rounding each                               density_grad.hiph:52
  s_d            w0[0] f_0, then F - 1 fmaf                                density_grad.hiph:58-60
  per axis       four differences (1 rounding), four weight products (1), t = diff0 wgt0 (1), three
                 fmaf (1 each)                                             density_grad.hiph:62-73
  per level      g = fmaf(mul_l, t, g), levels in order, the first onto 0  density_grad.hiph:74-76, :91-95
  Jacobian       ray_grad_model.contract_bwd_model, the same operations as pose_grad.hip:104-120
                                                                           density_grad.hiph:96-112
  normal         |g|: x x, fmaf, fmaf, sqrtf; -g / |g|: one division       density_grad.hiph:124-127
  per ray        acc = fmaf(w, n^, acc) once per stride, then wave_sum (common.hiph:33-42, :78): the sum
                 takes gamma(ceil(len / 64) + 6) of its absolute terms     density_grad.hip:49-64
so the error of frac reaches the derivative through the weights, and the error of g reaches n^ through
the division and the norm.  Where the float32 norm of p may fall on the other side of 1 than the
float64 one, either branch is right (ray_grad_model._either).

Conditions on the inputs (caps, not measurements): no sample is ambiguous (ray_grad_model.ambiguous: a
cell face within twice the bound of pt at some level and axis), and no sample of a ray case has
|g| < 64 |E_g| (Euclidean norms; a shorter g makes n^ ill-conditioned), the deliberate exact-zero
samples (w0 = 0) and the NaN sample apart.  Offending samples are redrawn until none is left: cap 0.

Bar: |got - f64| <= BAR E with BAR = 2 for the second-order terms the rule drops; where E = 0 the
values are equal as numbers; NaN where the model is NaN.  The bound was fixed before any kernel was run
against it: nothing here was measured on a kernel.
"""
import collections
import functools

import numpy as np
import torch

from tests import ray_grad_model as R
from tests.ray_grad_model import (BAR, U, WAVE, SCAN_DEPTH, _add, _div, _fma, _mul, _norm, _sqrt, _sub, _v,  # noqa: F401
                                  ambiguous, contract_bwd_model, contract_f32, contract_fwd_model,
                                  corner_rows, gamma, ratio)

MIN_G_OVER_E = 64.0
SEG_LENGTHS = (0, 1, 2, 63, 64, 65, 129, 200)


def make_field(L, F, T, disjoint, seed):
    """ray_grad_model.make_field for a shape of our own (its table of shapes gets the entry for the
    duration of the call), plus w0 [L F], row 0 of a field head"""
    name = "_density_grad"
    R.FIELDS[name] = (L, F, T, disjoint)
    try:
        fld = R.make_field(name, seed)
    finally:
        del R.FIELDS[name]
    g = torch.Generator().manual_seed(seed + 7)
    fld["w0"] = (torch.randn(L * F, generator=g) * 0.5).contiguous()
    return fld


def K_RAY(length):
    """roundings on the longest path of one term of N_r: one fmaf per stride + the wave sum"""
    return (np.asarray(length) + WAVE - 1) // WAVE + SCAN_DEPTH


# corner pairs (hi, lo) and the two fractions whose weights they take, per axis
_PAIRS = (((4, 0), (5, 1), (6, 2), (7, 3)), ((2, 0), (3, 1), (6, 4), (7, 5)), ((1, 0), (3, 2), (5, 4), (7, 6)))
_OTHER = ((1, 2), (0, 2), (0, 1))          # x: (b, c), y: (a, c), z: (a, b)
_SIGN = np.array([[1.0 if d & bit else -1.0 for bit in (4, 2, 1)] for d in range(8)])


def _cells(fld, pts):
    """what every evaluation below reads: x (float64 contracted point, 0 in the |p| == 0 rows), E_x,
    zero, rows [n, L, 8] and the features [n, L, 8, F] as float64"""
    x, E_x, zero = contract_fwd_model(pts)
    x32 = contract_f32(pts)
    x32[zero] = 0.0          # any finite cell: the sample's gradient is NaN whatever it reads
    x = np.where(zero[:, None], 0.0, x)
    E_x = np.where(zero[:, None], 0.0, E_x)
    L, F, stride = fld["L"], fld["F"], fld["stride"]
    rows = corner_rows(fld, x32)
    tab = fld["table16"].numpy().view(np.float16)
    feat = np.stack([tab[stride * l + rows[:, l, :, None] * F + np.arange(F)].astype(np.float64)
                     for l in range(L)], 1)
    return x, E_x, zero, rows, feat


def _pos(fld, x, l):
    mul = float(fld["mul"][l])
    return x * mul + fld["bias"][l].numpy().astype(np.float64)[None]


def interpolant(fld, feat, x, w0, dx=0.0):
    """float64 restatement of the FORWARD: the trilinear blend of the cell's rows followed by w0, at the
    contracted points x + dx [n, 3], which stay inside the cells `feat` was read from at x -> [n].  The
    step is added to the fractions (dx mul_l), not to x: pt is of the order of 1000 and would lose a
    step of 1e-6 cells to its own rounding."""
    L, F = fld["L"], fld["F"]
    w0 = np.asarray(w0, dtype=np.float64).reshape(L, F)
    out = np.zeros(x.shape[0])
    for l in range(L):
        pos = _pos(fld, x, l)
        fr = (pos - np.floor(pos)) + dx * float(fld["mul"][l])
        for d in range(8):
            w = np.ones(x.shape[0])
            for ax, bit in enumerate((4, 2, 1)):
                w = w * (fr[:, ax] if d & bit else 1.0 - fr[:, ax])
            out += w * (feat[:, l, d, :] * w0[l]).sum(1)
    return out


def grad_values(fld, feat, x, w0, mut=None):
    """the closed form in float64 -> G [n, 3] at the contracted point.  mut (values only): 'q5' the
    other axes' weights dropped, ('flip', axis), ('no_mul', l), ('swap', l) the channels of level l
    reversed against w0."""
    L, F = fld["L"], fld["F"]
    w0 = np.asarray(w0, dtype=np.float64).reshape(L, F)
    G = np.zeros((x.shape[0], 3))
    for l in range(L):
        mul = 1.0 if mut == ("no_mul", l) else float(fld["mul"][l])
        wl = w0[l, ::-1] if mut == ("swap", l) else w0[l]
        s = (feat[:, l] * wl).sum(2)                      # [n, 8]
        pos = _pos(fld, x, l)
        fr = pos - np.floor(pos)
        for ax in range(3):
            if mut == "q5":
                G[:, ax] += mul * (s * _SIGN[:, ax]).sum(1)
                continue
            p, q = fr[:, _OTHER[ax][0]], fr[:, _OTHER[ax][1]]
            wg = ((1 - p) * (1 - q), (1 - p) * q, p * (1 - q), p * q)
            G[:, ax] += mul * sum((s[:, hi] - s[:, lo]) * wg[j] for j, (hi, lo) in enumerate(_PAIRS[ax]))
    if isinstance(mut, tuple) and mut[0] == "flip":
        G[:, mut[1]] *= -1.0
    return G


def grad_bound(fld, feat, x, E_x, w0):
    """the kernel's formula operation by operation -> (G, E_G) [n, 3]; G is grad_values' number"""
    L, F = fld["L"], fld["F"]
    w0 = np.asarray(w0, dtype=np.float64).reshape(L, F)
    n = x.shape[0]
    acc = [_v(np.zeros(n)) for _ in range(3)]
    one = _v(np.ones(n))
    for l in range(L):
        mul = float(fld["mul"][l])
        pos = _pos(fld, x, l)
        E_pos = E_x * mul + U * np.abs(pos)
        fr = [(pos[:, a] - np.floor(pos[:, a]), E_pos[:, a]) for a in range(3)]
        cm = [_sub(one, f) for f in fr]
        s = []
        for d in range(8):
            sd = _mul(_v(np.full(n, w0[l, 0])), _v(feat[:, l, d, 0]))
            for k in range(1, F):
                sd = _fma(_v(np.full(n, w0[l, k])), _v(feat[:, l, d, k]), sd)
            s.append(sd)
        for ax in range(3):
            p, q = _OTHER[ax]
            wg = (_mul(cm[p], cm[q]), _mul(cm[p], fr[q]), _mul(fr[p], cm[q]), _mul(fr[p], fr[q]))
            t = None
            for j, (hi, lo) in enumerate(_PAIRS[ax]):
                diff = _sub(s[hi], s[lo])
                t = _mul(diff, wg[j]) if t is None else _fma(diff, wg[j], t)
            acc[ax] = _fma(_v(np.full(n, mul)), t, acc[ax])
    return np.stack([a[0] for a in acc], 1), np.stack([a[1] for a in acc], 1)


def point_model(fld, pts, w0=None, mut=None):
    """-> dict: G, E_G (contracted point), g, E_g (raw point: f2n_density_grad's output), zero, pos_min"""
    w0 = fld["w0"].numpy() if w0 is None else np.asarray(w0)
    x, E_x, zero, rows, feat = _cells(fld, pts)
    G, E_G = grad_bound(fld, feat, x, E_x, w0)
    if mut is not None and mut != "identity_jac":
        G = grad_values(fld, feat, x, w0, mut)
    g, E_g = contract_bwd_model(pts, G, E_G)
    if mut == "identity_jac":
        g = np.where(zero[:, None], np.nan, G)
    pos_min = min(float(_pos(fld, x, l).min()) for l in range(fld["L"]))
    return dict(G=G, E_G=E_G, g=g, E_g=E_g, zero=zero, x=x, feat=feat, pos_min=pos_min)


def normal_model(g, E_g, mut=None):
    """n^ = -g / |g| (0 where g is zero in all three) -> (nh, E_nh) [n, 3].  mut: 'no_norm', 'plus_g'"""
    cols = [(g[:, a], E_g[:, a]) for a in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        ln = _norm(cols)
        nh = [_div(c, ln) for c in cols]
    v = -np.stack([c[0] for c in nh], 1)
    e = np.stack([c[1] for c in nh], 1)
    if mut == "no_norm":
        v = -g.copy()
    if mut == "plus_g":
        v = -v
    flat = (g == 0).all(1)
    v[flat] = 0.0
    e[flat] = 0.0
    return v, e


def ray_model(bounds, weights, nh, E_nh, mut=None):
    """N_r = sum_k w_k n^_k -> (N, E_N) [n_rays, 3].  mut: 'no_weight', 'drop_last_stride' (the samples
    of a last, partial 64-sample stride)"""
    b = bounds.numpy().astype(np.int64)
    n_rays, n = b.shape[0], nh.shape[0]
    length = b[:, 1] - b[:, 0]
    ray = np.repeat(np.arange(n_rays), length)
    w = weights.numpy().astype(np.float64)
    wv = np.ones(n) if mut == "no_weight" else w.copy()
    if mut == "drop_last_stride":
        k = np.arange(n) - b[ray, 0]
        wv[(length[ray] % WAVE != 0) & (k >= (length[ray] // WAVE) * WAVE)] = 0.0
    N, A, Ein = np.zeros((n_rays, 3)), np.zeros((n_rays, 3)), np.zeros((n_rays, 3))
    np.add.at(N, ray, wv[:, None] * nh)
    np.add.at(A, ray, np.abs(w[:, None] * nh))
    np.add.at(Ein, ray, np.abs(w)[:, None] * E_nh)
    return N, Ein + gamma(K_RAY(length))[:, None] * A


# ---- cases ----------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "kind F L T disjoint tag")

SHAPES = [(F, L) for F in (1, 2, 4, 8) for L in (4, 16)] + [(2, 32)]
TABLES = (1 << 14, 12289)


def _valid(F, T, disjoint):
    """the ABI wants level_stride a multiple of F (a row is one aligned load of 2 F bytes): overlapping
    windows of an odd T exist for F = 1 only"""
    return disjoint or T % F == 0


def cases():
    """'points': f2n_density_grad, one launch of n points (the fixed radii of ray_grad_model.fixed_points
    -- inside the ball, within an ulp of |p| = 1, far outside, the origin -- then random points);
    'rays': f2n_ray_normals.  Every (F, L) at both table sizes and both level strides as points (those the
    ABI accepts: _valid); as rays every (F, L), the table size and the stride taking turns."""
    out = []
    for F, L in SHAPES:
        for T in TABLES:
            for disjoint in (False, True):
                if _valid(F, T, disjoint):
                    out.append(Case("points", F, L, T, disjoint, "n200"))
    out += [Case("points", 2, 16, 1 << 14, False, "n%d" % n) for n in (1, 63, 64, 65, 1000)]
    for i, (F, L) in enumerate(SHAPES):
        T, disjoint = TABLES[i % 2], bool((i // 2) % 2)
        out.append(Case("rays", F, L, T, disjoint or not _valid(F, T, disjoint), "mixed130"))
    out.append(Case("rays", 1, 4, 12289, False, "mixed130"))
    out.append(Case("rays", 2, 16, 1 << 14, False, "one"))
    out.append(Case("rays", 2, 16, 12289, True, "nan"))
    out.append(Case("rays", 2, 16, 1 << 14, True, "w0zero"))
    return out


def case_id(c):
    return "%s-F%d-L%d-T%d-%s-%s" % (c.kind, c.F, c.L, c.T, "TF" if c.disjoint else "T", c.tag)


Built = collections.namedtuple("Built", "case fld pts bounds weights m redrawn")


def _seed(c):
    return 7919 * cases().index(c) + 11


def _too_flat(fld, pts):
    m = point_model(fld, pts)
    with np.errstate(invalid="ignore"):
        return np.linalg.norm(m["g"], axis=1) < MIN_G_OVER_E * np.linalg.norm(m["E_g"], axis=1)


@functools.lru_cache(maxsize=None)
def build_case(c):
    """-> Built (inputs as CPU tensors, the float64 model m, the share of samples redrawn).  Fixed
    seeds; ambiguous samples -- and, in ray cases, samples with |g| < 64 |E_g| -- are redrawn (fixed
    points: the field's seed is walked) until the case holds none."""
    seed = _seed(c)
    g = torch.Generator().manual_seed(seed)
    fld = make_field(c.L, c.F, c.T, c.disjoint, seed)
    n_fixed, lengths = 0, None
    if c.kind == "points":
        n = int(c.tag[1:])
        pts = R._anywhere(g, n)
        if n >= 200:
            fixed, _ = R.fixed_points()
            n_fixed = fixed.shape[0]
            pts[:n_fixed] = fixed
            for bump in range(1, 200):
                if not ambiguous(fld, pts[:n_fixed]).any():
                    break
                fld = make_field(c.L, c.F, c.T, c.disjoint, seed + 100000 * bump)
            else:
                raise AssertionError("no field without an ambiguous fixed point: " + case_id(c))
    else:
        if c.tag == "one":
            lengths = [129]
        elif c.tag == "nan":
            lengths = [65, 3, 200, 0, 64]
        else:
            lengths = [SEG_LENGTHS[(r + r // 8) % 8] for r in range(130)]
        n = sum(lengths)
        pts = R._anywhere(g, n)
    if c.tag == "w0zero":
        fld["w0"] = torch.zeros_like(fld["w0"])
    redrawn = 0
    for _ in range(200):
        bad = ambiguous(fld, pts)
        if c.kind == "rays" and c.tag != "w0zero":
            bad = bad | _too_flat(fld, pts)
        if not bad.any():
            break
        assert not bad[:n_fixed].any()
        k = int(bad.sum())
        redrawn += k
        pts[torch.from_numpy(bad)] = R._anywhere(g, k)
    else:
        raise AssertionError("samples that miss the input conditions left: " + case_id(c))
    nan_at = -1
    if c.tag == "nan":
        nan_at = lengths[0] + 1          # second sample of the middle ray of the first three
        pts[nan_at] = 0.0
    pts = pts.contiguous()
    m = point_model(fld, pts)
    m["nan_at"] = nan_at
    bounds = weights = None
    if c.kind == "rays":
        bounds = R._bounds(lengths)
        # independent of pts; the last sample of a ray is its surface hit and carries half the opacity,
        # so that a kernel which loses the last, partial stride cannot hide in the rounding of the rest
        weights = torch.rand(n, generator=g) * 0.05
        last = bounds[bounds[:, 1] > bounds[:, 0], 1].long() - 1
        weights[last] = 0.4 + 0.2 * torch.rand(last.shape[0], generator=g)
        weights = weights.contiguous()
        m["nh"], m["E_nh"] = normal_model(m["g"], m["E_g"])
        m["N"], m["E_N"] = ray_model(bounds, weights, m["nh"], m["E_nh"])
    return Built(c, fld, pts, bounds, weights, m, redrawn / max(n, 1))


def conditions(b):
    """-> (ambiguous samples, samples of a ray case with |g| < 64 |E_g|) left in a built case: both 0"""
    amb = ambiguous(b.fld, b.pts)
    flat = np.zeros(b.pts.shape[0], dtype=bool)
    if b.case.kind == "rays" and b.case.tag != "w0zero":
        flat = _too_flat(b.fld, b.pts)
        if b.m["nan_at"] >= 0:
            flat[b.m["nan_at"]] = False
    return int(amb.sum()), int(flat.sum())
