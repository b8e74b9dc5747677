"""Inputs, a float64 restatement and per-element rounding bounds for the encoding's true derivative with
respect to position as a vector-Jacobian product: f2n_hash_pts_grad_exact (one lane per point, at the
contracted point) and f2n_hash_rays_grad_exact (one wavefront per ray, through the contraction to
d(rays_o), d(rays_d)) in enc_grad.hip.  No tests in here: tests/test_enc_grad_model_cpu.py checks the
restatement and the bounds on the CPU, tests/test_gpu_enc_grad.py holds the HIP kernels to them.  The
cells, the interpolant, the closed form and the value-and-bound arithmetic are
tests/density_grad_model.py's; the contraction's models, the per-ray sums and `ambiguous` are
tests/ray_grad_model.py's.

The function.  enc[p, lF + k] = sum_d w_d(frac_l) f_{l,d,k} (the forward's interpolant, without the
per-channel f16 rounding of the blend), so for g = d(loss)/d(enc) [n, L F], at the contracted point,
  G[p] = sum_l mul_l [(s4-s0) b1 c1 + (s5-s1) b1 c + (s6-s2) b c1 + (s7-s3) b c], y and z likewise,
with s_d = sum_k g[p, lF + k] f_{l,d,k}: density_grad_model's closed form with the sample's own row of g
where that model has the uniform w0.  Then dp through the contraction's Jacobian at the float32 raw
point (ray_grad_model.contract_bwd_model, NaN at |p| == 0), and per ray d_o = sum dp, m = sum t dp,
d_d = (m - n (n.m)) / |d| exactly as ray_grad_model.ray_sums composes them.

Bound E, first order, per element, u = 2^-24: density_grad_model.grad_bound operation by operation
(density_grad.hiph's header: frac through one fmaf, 1 - frac, s_d = g_0 f_0 then F - 1 fmaf, per axis
four differences, four weight products, one product and three fmaf, per level one fmaf) with |g_k| in
place of |w0_k|; g is an exact float32 input (enc_grad.hip reads it unscaled, no f16 rounding).  The ray
part takes ray_grad_model's counts: the Jacobian's operations, K_RAY_O, K_RAY_M, the epilogue.
  f2n_hash_pts_grad_exact   the input IS the contracted float32 point: E_x = 0, no Jacobian
  f2n_hash_rays_grad_exact  the kernel contracts the raw point itself: E_x of contract_fwd_model

Ambiguous cells.  The face-normal component of the true gradient jumps at a cell face, so a sample
within twice its position bound of a face, on any level or axis, is redrawn until none is left
(ray_grad_model.ambiguous, with the raw point's E_x, the larger of the two): the cap is 0.

Bar: |got - f64| <= BAR E, BAR = 2; where E = 0 the values are equal as numbers; NaN where the model
has it.  Nothing here was measured on a kernel.
"""
import collections
import functools

import numpy as np
import torch

from tests import density_grad_model as D
from tests import ray_grad_model as R
from tests.density_grad_model import _OTHER, _PAIRS, _SIGN, _cells, _pos, _valid  # noqa: F401
from tests.ray_grad_model import (BAR, U, WAVE, _fma, _mul, _sub, _v, ambiguous,  # noqa: F401
                                  contract_bwd_model, contract_f32, corner_rows, gamma, ratio, ray_sums)

SEG_LENGTHS = D.SEG_LENGTHS          # (0, 1, 2, 63, 64, 65, 129, 200)
G_DECADES = (-12.0, -4.0)            # log10 of the per-sample scale of g (draw_g)
GRAD_SCALE = R.GRAD_SCALE


# ---- values ---------------------------------------------------------------------------------------------

def cells_at(fld, x32):
    """_cells for points that are contracted already (f2n_hash_pts_grad_exact's input): x = x32 as
    float64, E_x = 0 -> x, E_x, feat [n, L, 8, F]"""
    x32 = np.ascontiguousarray(x32, dtype=np.float32)
    L, F, stride = fld["L"], fld["F"], fld["stride"]
    rows = corner_rows(fld, x32)
    tab = fld["table16"].numpy().view(np.float16)
    feat = np.stack([tab[stride * l + rows[:, l, :, None] * F + np.arange(F)].astype(np.float64)
                     for l in range(L)], 1)
    x = x32.astype(np.float64)
    return x, np.zeros_like(x), feat


def _g3(fld, g):
    g = g.numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
    return g.astype(np.float64).reshape(g.shape[0], fld["L"], fld["F"])


def interpolant(fld, feat, x, g, dx=0.0):
    """density_grad_model.interpolant generalised to per-sample weights: sum_c g[p, c] enc[p, c] at the
    contracted points x + dx, the step added to the fractions -> [n]"""
    g = _g3(fld, g)
    out = np.zeros(x.shape[0])
    for l in range(fld["L"]):
        pos = _pos(fld, x, l)
        fr = (pos - np.floor(pos)) + dx * float(fld["mul"][l])
        for d in range(8):
            w = np.ones(x.shape[0])
            for ax, bit in enumerate((4, 2, 1)):
                w = w * (fr[:, ax] if d & bit else 1.0 - fr[:, ax])
            out += w * (feat[:, l, d, :] * g[:, l]).sum(1)
    return out


def f16_through_scale(g):
    """f16(128 g) / 128, what the Q5 kernels make of g"""
    with np.errstate(over="ignore"):
        return ((np.asarray(g, dtype=np.float32) * np.float32(GRAD_SCALE)).astype(np.float16)
                .astype(np.float64) / GRAD_SCALE)


def grad_values(fld, feat, x, g, mut=None):
    """the closed form in float64 -> G [n, 3] at the contracted point.  mut (values only): 'q5' the other
    two axes' weights dropped (the old kernels' form, without their f16 roundings), 'q5_quarter' that
    over 4, ('swap_w', axis) the two middle pair weights of one axis exchanged (the weights of its two
    other axes swapped), ('no_mul', l), 'swap_chan' channels 0 and 1 of g exchanged at every level,
    'g_f16' g rounded through f16(128 g) / 128."""
    L = fld["L"]
    g = _g3(fld, g)
    if mut == "swap_chan":
        g = g.copy()
        g[:, :, [0, 1]] = g[:, :, [1, 0]]
    if mut == "g_f16":
        g = f16_through_scale(g)
    G = np.zeros((x.shape[0], 3))
    for l in range(L):
        mul = 1.0 if mut == ("no_mul", l) else float(fld["mul"][l])
        s = (feat[:, l] * g[:, l, None, :]).sum(2)                      # [n, 8]
        pos = _pos(fld, x, l)
        fr = pos - np.floor(pos)
        for ax in range(3):
            if mut in ("q5", "q5_quarter"):
                G[:, ax] += mul * (s * _SIGN[:, ax]).sum(1) * (0.25 if mut == "q5_quarter" else 1.0)
                continue
            p, q = fr[:, _OTHER[ax][0]], fr[:, _OTHER[ax][1]]
            wg = [(1 - p) * (1 - q), (1 - p) * q, p * (1 - q), p * q]
            if mut == ("swap_w", ax):
                wg[1], wg[2] = wg[2], wg[1]
            G[:, ax] += mul * sum((s[:, hi] - s[:, lo]) * wg[j] for j, (hi, lo) in enumerate(_PAIRS[ax]))
    return G


def grad_bound(fld, feat, x, E_x, g):
    """density_grad_model.grad_bound with the sample's own g[p, lF + k] for w0[lF + k]
    -> (G, E_G) [n, 3]"""
    L, F = fld["L"], fld["F"]
    g = _g3(fld, g)
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
            sd = _mul(_v(g[:, l, 0]), _v(feat[:, l, d, 0]))
            for k in range(1, F):
                sd = _fma(_v(g[:, l, k]), _v(feat[:, l, d, k]), sd)
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


def contracted_input(pts):
    """the float32 contracted points handed to f2n_hash_pts_grad_exact: contract_f32, the |p| == 0 rows
    at 0 (any finite cell)"""
    x32 = contract_f32(pts)
    x32[np.isnan(x32).any(1)] = 0.0
    return x32


def pts_model(fld, x32, g, mut=None):
    """f2n_hash_pts_grad_exact at the contracted float32 points x32 -> dict G, E_G"""
    x, E_x, feat = cells_at(fld, x32)
    G, E_G = grad_bound(fld, feat, x, E_x, g)
    if mut is not None:
        G = grad_values(fld, feat, x, g, mut)
    return dict(G=G, E_G=E_G, x=x, feat=feat)


def sample_model(fld, pts, g, mut=None):
    """per sample of f2n_hash_rays_grad_exact, from the raw points -> dict G, E_G (contracted point),
    dp, E_dp (raw point), zero, x, feat.  mut: grad_values', or 'identity_jac'"""
    x, E_x, zero, _, feat = _cells(fld, pts)
    G, E_G = grad_bound(fld, feat, x, E_x, g)
    if mut is not None and mut != "identity_jac":
        G = grad_values(fld, feat, x, g, mut)
    dp, E_dp = contract_bwd_model(pts, G, E_G)
    if mut == "identity_jac":
        dp = np.where(zero[:, None], np.nan, G)
    return dict(G=G, E_G=E_G, dp=dp, E_dp=E_dp, zero=zero, x=x, feat=feat)


def rays_model(bounds, t, dp, E_dp, rays_d, mut=None):
    """ray_grad_model.ray_sums -> d_o, E_o, d_d, E_d [n_rays, 3].  mut: 'drop_last_stride' (the samples
    of a last, partial 64-sample stride), 'no_t' (t left out of m)"""
    if mut == "no_t":
        return ray_sums(bounds, torch.ones_like(t), dp, E_dp, rays_d)
    if mut == "drop_last_stride":
        b = bounds.numpy().astype(np.int64)
        length = b[:, 1] - b[:, 0]
        ray = np.repeat(np.arange(b.shape[0]), length)
        k = np.arange(dp.shape[0]) - b[ray, 0]
        lost = (length[ray] % WAVE != 0) & (k >= (length[ray] // WAVE) * WAVE)
        dp = np.where(lost[:, None], 0.0, dp)
    return ray_sums(bounds, t, dp, E_dp, rays_d)


# ---- cases ----------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "F L T disjoint chan_major n_rays origin")

SHAPES = D.SHAPES                    # F in (1, 2, 4, 8) x L in (4, 16), plus (2, 32)
TABLES = D.TABLES                    # (2^14, 12289): both POW2 instantiations
SMALL, WIDE = 8, 72                  # rays: one and nine rounds of SEG_LENGTHS (524 and 4716 samples)


def cases():
    """Every (F, L) once with the table size, the level stride and the layout of g taking turns; then
    (2, 16) at the combinations of table size and stride the turns leave out, in both layouts; the
    origin sample in two of them; one wide case whose rays are enough for the per-ray mutants."""
    out = []
    for i, (F, L) in enumerate(SHAPES):
        T, disjoint = TABLES[i % 2], bool((i // 2) % 2)
        out.append(Case(F, L, T, disjoint or not _valid(F, T, disjoint), bool(i % 3 == 1), SMALL, i == 3))
    for j, (T, disjoint) in enumerate([(1 << 14, False), (1 << 14, True), (12289, False), (12289, True)]):
        if _valid(2, T, disjoint):
            out.append(Case(2, 16, T, disjoint, bool(j % 2 == 0), SMALL, j == 1))
    out.append(Case(1, 16, 12289, False, True, SMALL, False))         # overlapping windows of an odd T
    out.append(Case(2, 16, 1 << 14, False, False, WIDE, False))
    return out


def case_id(c):
    return "F%d-L%d-T%d-%s-%s-r%d%s" % (c.F, c.L, c.T, "TF" if c.disjoint else "T",
                                         "cm" if c.chan_major else "rm", c.n_rays, "-origin" if c.origin else "")


Built = collections.namedtuple("Built", "case fld pts t bounds rays_d g x32 ms mp d_o E_o d_d E_d redrawn nan_at nan_ray")


def lengths_of(n_rays):
    return [SEG_LENGTHS[(r + r // 8) % 8] for r in range(n_rays)]


def draw_g(gen, bounds, n, C):
    """d(loss)/d(enc) [n, C]: normal draws times a scale per sample, log-uniform over G_DECADES.  In a
    render this gradient is a compositing weight times a colour gradient: of the order of 1e-4 at a
    surface, arbitrarily small behind it -- and f16(128 g), which Q5 is formed from, has a fixed spacing
    of 2^-24 / 128 = 4.7e-10 below |g| = 4.8e-7 and flushes to zero below 2.3e-10, so a kernel that
    rounds g that way is told apart only where g is small.  The last sample of every ray is its surface
    hit and takes the top of the range, so that a kernel which loses the last, partial stride cannot
    hide behind the larger samples of the rest (density_grad_model.build_case's weights)."""
    lo, hi = G_DECADES
    scale = 10.0 ** (torch.rand(n, 1, generator=gen, dtype=torch.float64) * (hi - lo) + lo)
    last = bounds[bounds[:, 1] > bounds[:, 0], 1].long() - 1
    scale[last] = 10.0 ** hi
    return (torch.randn(n, C, generator=gen, dtype=torch.float64) * scale).float().contiguous()


def ambiguous_at(fld, x32):
    """ray_grad_model.ambiguous for contracted float32 inputs (E_x = 0): [n] bool"""
    x = np.asarray(x32, dtype=np.float64)
    mul = fld["mul"].numpy().astype(np.float64)[None, :, None]
    pos = x[:, None, :] * mul + fld["bias"].numpy().astype(np.float64)[None]
    return (np.abs(pos - np.rint(pos)) <= 2.0 * U * np.abs(pos)).any((1, 2))


@functools.lru_cache(maxsize=None)
def build_case(c):
    """-> Built: inputs as CPU tensors (g row-major [n, L F] whatever the case's layout: the caller lays
    it out), ms = sample_model, mp = pts_model at x32, the per-ray values and bounds.  Fixed seeds;
    ambiguous samples are redrawn until the case holds none."""
    seed = 104729 * cases().index(c) + 17
    gen = torch.Generator().manual_seed(seed)
    fld = D.make_field(c.L, c.F, c.T, c.disjoint, seed)
    lengths = lengths_of(c.n_rays)
    bounds = R._bounds(lengths)
    n = sum(lengths)
    pts = R._anywhere(gen, n)
    redrawn = 0
    for _ in range(200):
        bad = ambiguous(fld, pts)
        if not bad.any():
            break
        k = int(bad.sum())
        redrawn += k
        pts[torch.from_numpy(bad)] = R._anywhere(gen, k)
    else:
        raise AssertionError("ambiguous samples left: " + case_id(c))
    nan_at = nan_ray = -1
    if c.origin:
        nan_ray = lengths.index(65)
        nan_at = int(bounds[nan_ray, 0]) + 1
        pts[nan_at] = 0.0
    pts = pts.contiguous()
    t = (torch.rand(n, generator=gen) * 3.0 + 0.01).contiguous()       # drawn independently of pts
    rays_d = R._rays_d(gen, c.n_rays)
    g = draw_g(gen, bounds, n, c.L * c.F)
    ms = sample_model(fld, pts, g)
    x32 = contracted_input(pts)
    assert not ambiguous_at(fld, x32).any(), "an ambiguous contracted input: " + case_id(c)
    mp = pts_model(fld, x32, g)
    d_o, E_o, d_d, E_d = rays_model(bounds, t, ms["dp"], ms["E_dp"], rays_d)
    return Built(c, fld, pts, t, bounds, rays_d, g, x32, ms, mp, d_o, E_o, d_d, E_d, redrawn / max(n, 1),
                 nan_at, nan_ray)
