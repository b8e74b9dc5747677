"""Inputs, a float64 restatement, per-ray rounding bounds and mutants for the one-pass inference render:
f2n_render_rays (render_rays.hip), f2n_render_rays_head and f2n_render_rays_tail (render_rays_head.hip),
all three around render_one_ray (render_rays.hiph).  No tests in here: tests/test_render_model_cpu.py
checks the restatement, the bound and its power on the CPU, tests/test_gpu_render_f64.py holds the HIP
kernels to it.

Inputs of the model, per sample: t, dt, the contracted point, the f16 encoding row; per ray: the unit
direction, the image id (or none), bg; per case: the field, the network, the optional occupancy bits,
t_thresh, density_shift, t_shift.  They are those of the op-by-op route: R.get_samples,
ray_grad_model.contract_f32 and K.hash_fwd on the CPU (cpu_samples), f2n_sample_rays, f2n_contract_fwd
and f2n_hash_fwd on the device (tests/test_gpu_render_f64.py).  The one-pass kernels claim to form the
same samples and encodings in bits whatever their stride width (sampler.hiph); the GPU test is a test of
that claim too.

Stages, in the kernels' order (render_rays.hiph:134-248, render_rays_head.hip:140-282):

  1. occupancy   the bit of the contracted point's cell, tests/util.py::_cells (the header's f32
                 cell expression); no grid = every sample occupied.
  2. chain       logit0 = b_h[0] + sum_c enc_c w_h[0, c]; sec = exp(logit0 - shift) dt, 0 where the
                 sample is unoccupied.
  3. keep        ragged_cases.keep_rule, the rule and the band of density_scan_ref: sample k is kept
                 while exp(-depth_k) > t_thresh with depth the exclusive sum of sec; the first sample
                 not kept ends the ray.  len = kept positions, kept = those that are occupied too.
                 band_k = u (k depth_k + sum_{j<k} sec_j e_j + 4), e_j = (C + 1) A_j + |x_j| + 4; a ray
                 with a depth inside the band of -ln(t_thresh) is ambiguous.
  4. network     shade_model.model(backward=False) on the kept, occupied samples: head logit, rgb and
                 their bounds E_logit, E_rgb.  Its counts hold for these kernels as they stand:
                   K_HEAD = C + 1   render_rays.hiph:166-173, render_rays_head.hip:175-182: C / 4
                                    products of 4 terms onto b_h
                   K_EMBED = 1      render_rays.hiph:183, render_rays_head.hip:195
                   K_PRE = 32 + 1   render_rays.hiph:119-122 then :195-201, render_rays_head.hip:206-221:
                                    b1, the SH half's 4 products, then the feature half's 4: the same 8
                                    products of 4 terms onto b1, the SH half first in both forms
                   K_OUT = 64 + 1   render_rays.hiph:188-207, render_rays_head.hip:199-227: 16 products
                                    of 4 terms onto b2
                   K_RGB = 6        render_rays.hiph:225-227, render_rays_head.hip:245-247: expf (2), +,
                                    /, the constant 1 + 2 eps, -
                 No form adds a rounding these constants do not allow: none was raised.
  5. composite   over that list with the head logit: sec2, T_k, alpha, w, last_trans, colors with bg,
                 depths = sum w (t + t_shift) / (1 - T_last + 1e-4f): the closed forms of
                 ragged_cases.composite_fwd_ref, with t_shift and 1e-4f as the float32 the kernels hold.

Bound per output, first order, u = 2^-24, |got - f64| <= BAR E with BAR = 2; E = (a) + (b):

  (a) the compositing's own roundings, u (kept M_sum + K_COMPOSITE M_op) with ragged_cases' conditioning
      numbers and its K = 4 (measured there on the f32 oracle, never on a kernel).  The sums are trees
      over the ray's kept terms in every form: per lane across strides, then the DPP tree
      (render_rays.hiph:225-238), or per lane, the 8-lane group scan (render_rays_head.hip:61-75,
      :245-258) and, for a ray handed over, lane 0 of the tail and its DPP tree (render_rays.hiph:131,
      :235-238).  A merge with a lane that holds 0 is exact, so a term passes at most kept - 1 roundings
      whatever the form: the any-order term covers the head's reduction followed by the tail's, and the
      hand-over adds nothing to M_op.  (The optical depths likewise: comp_carry + the scan inside the
      stride or group, render_rays.hiph:220-230, render_rays_head.hip:240-250; the state hands both on
      as they are, :273-275.)
  (b) the errors of the network's outputs through the float64 Jacobian of the closed form:
      sum_k w_k E_rgb_k + sum_k |d out / d logit_k| E_logit_k with d out / d logit_k =
      sec2_k (dw_k (T_k - w_k) - sum_{j>k} dw_j w_j - T_last d_tl), composite_bwd_ref's d_sec with d_out
      a unit vector (dw = rgb_c, d_tl = bg_c for a colour; dw = (t + t_shift) / den, d_tl = Nd / den^2
      for the depth; dw = 0, d_tl = 1 for last_trans).

A ray without a kept, occupied sample has E = 0: colors == bg, last_trans == 1, depths == 0 as numbers
(expf(-0.f) = 1, fmaf(1, bg, 0) = bg, 0 / 1e-4f = 0).  Nothing in the bound was measured on a kernel.

Ambiguous rays (stage 3) are left out of the value comparison only: their outputs must be finite and
their counts within one of the model's.  A case may hold at most MAX_AMBIGUOUS of them, a case of fewer
than 50 rays none; build_case walks seeds until that holds.  The forward is continuous across a ReLU:
shade_model's ambiguous neurons need no exclusion.

len = 1 cannot occur at S > 1: dt_0 = 0 (sampler.hiph:260), so the depth in front of sample 1 is 0 and
sample 1 is always kept.  The smallest length the cases ask for is 2.
"""
import collections
import functools
import math

import numpy as np
import torch

from oracle import kernels as K
from oracle import ref_render as R
from tests import ragged_cases as rc
from tests import shade_model as sm
from tests.ray_grad_model import contract_f32, contract_fwd_model
from tests.util import _cells, _raw_field

U = 2.0 ** -24
BAR = 2.0
MAX_AMBIGUOUS = 0.02
T_THRESH = 1e-4
DENSITY_SHIFT = 3.0
T_SHIFT = 1e-2
T_SHIFT32 = float(np.float32(T_SHIFT))
DEN_EPS32 = float(np.float32(1e-4))
G_OCC = 64
N_EMB = 8                # embedding rows: a different id for every ray of a group of eight
WHOLE = 1 << 30          # n_head >= S: the head takes the whole ray
ONE_RAY_LOOP = 512 * 8   # rays one pass of f2n_render_rays' / the tail's persistent grid covers
HEAD_LOOP = 256 * 96     # ... and of the head's (256 workgroups of 12 waves of 8 rays)
OUTPUTS = ("colors", "depths", "last_trans")
LIMIT = -math.log(float(np.float32(T_THRESH)))

WIDTHS = {32: (16, 2, 1 << 19), 8: (8, 1, 3001), 16: (8, 2, 1 << 14), 64: (8, 8, 1 << 12)}


# ---- cases ----------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "name C S noise n_rays mode img occ paired")
Case.__new__.__defaults__ = (0,)


def cases():
    """mode: 'lengths' (each ray's noise row scaled so that it ends at a required length), 'natural'
    (one bias, the rays end where they end), 'weight' (nothing ends: every link carries weight),
    'short' (the persistent loops: every ray but a few named ones ends within 16 samples)."""
    return [
        Case("len-C32-S64", 32, 64, True, 99, "lengths", "distinct", "none"),
        Case("len-C8-S100", 8, 100, True, 97, "lengths", "runs3", "none"),
        Case("len-C16-S192", 16, 192, True, 96, "lengths", "none", "none"),
        Case("len-C64-S192", 64, 192, True, 95, "lengths", "equal", "ones"),
        Case("nat-C32-S192-random", 32, 192, True, 96, "natural", "distinct", "random"),
        Case("nat-C32-S100-shell", 32, 100, False, 97, "natural", "runs3", "shell"),
        Case("nat-C16-S100-random", 16, 100, False, 99, "natural", "distinct", "random"),
        Case("nat-C64-S64-ones", 64, 64, False, 8, "natural", "distinct", "ones"),
        Case("nat-C8-S192-shell", 8, 192, False, 7, "natural", "equal", "shell"),
        Case("nat-C32-S192-one-ray", 32, 192, True, 1, "natural", "equal", "none"),
        Case("empty-C8-S100", 8, 100, True, 9, "natural", "distinct", "empty"),
        Case("weight-C32-S192", 32, 192, False, 96, "weight", "distinct", "none", 1),
        Case("weight-C8-S100", 8, 100, True, 9, "weight", "runs3", "none"),
        Case("weight-C64-S64", 64, 64, True, 8, "weight", "none", "none"),
        Case("weight-C16-S192", 16, 192, True, 7, "weight", "equal", "ones"),
        Case("loop-C8-S64", 8, 64, True, ONE_RAY_LOOP + 9, "short", "runs3", "none"),
        Case("loop-C8-S100", 8, 100, True, HEAD_LOOP + 9, "short", "runs3", "none"),
    ]


def case_id(c):
    return c.name


def heads(S):
    """the n_head values the head + tail route runs at; n_head >= S is the head alone"""
    return [WHOLE, 64] + ([128] if S == 192 else [])


def required_lengths(S):
    return sorted({m for m in (2, 7, 8, 9, 15, 16, 17, 63, 64, 65, S - 1, S) + (
        (127, 128, 129) if S == 192 else ()) if m <= S})


def long_rays(c):
    """'short' cases: the rays whose noise row is scaled down so that they outlive sample 64 -- some in
    the first pass of each persistent loop, and all nine of the last"""
    if c.mode != "short":
        return []
    return [3, 1030, ONE_RAY_LOOP + 2] + ([ONE_RAY_LOOP * 2 + 5, HEAD_LOOP - 6] + list(
        range(HEAD_LOOP, c.n_rays)) if c.n_rays > HEAD_LOOP else list(range(ONE_RAY_LOOP + 5, c.n_rays)))


def grids_bool(S, G=G_OCC):
    """The grids of tests/test_gpu_render_rays_head.py::_grids, as bool [G^3]"""
    out = {"ones": torch.ones(G ** 3, dtype=torch.bool), "empty": torch.zeros(G ** 3, dtype=torch.bool),
           "random": torch.rand(G ** 3, generator=torch.Generator().manual_seed(S + 1)) < 0.5}
    c = (torch.arange(G, dtype=torch.float32) + 0.5) * (4.0 / G) - 2.0
    cz, cy, cx = torch.meshgrid(c, c, c, indexing="ij")
    r = (cx * cx + cy * cy + cz * cz).sqrt()
    out["shell"] = ((r > 0.35) & (r < 1.2)).reshape(-1)
    return out


# ---- inputs ---------------------------------------------------------------------------------------------

Inputs = collections.namedtuple("Inputs", "case fld P o d noise img bg occ step seed")
# numpy f32: t, dt [n,S]; x (contracted) [n,S,3]; enc [n,S,C]; dirs [n,3]; pts (as sampled) [n,S,3]
Samples = collections.namedtuple("Samples", "t dt x enc dirs pts")


def network(fld, g):
    """tests/test_gpu_render_rays.py::_raw_network's layout (row 0 of w_h / b_h IS the field's density
    head) with the scales of shade_model._params and N_EMB embedding rows"""
    C = fld["L"] * fld["F"]
    P = sm._params(g, C, 1.0)
    P["emb"] = torch.randn(N_EMB, 16, generator=g) * 0.1
    P["w_h"][0] = fld["w0"]
    P["b_h"][0] = float(fld["b0"][0])
    return {k: v.contiguous() for k, v in P.items()}


def cpu_samples(fld, o, d, noise, S, step):
    """the op-by-op route's per-sample inputs from the CPU oracle"""
    n = o.shape[0]
    pts, dirs, dt, t, _ = R.get_samples(o, d, noise, S, step)
    x = contract_f32(pts)
    enc = K.hash_fwd(torch.from_numpy(x), fld["table16"], fld["primes"], fld["bias"], fld["mul"], fld["L"],
                     fld["F"], fld["T"], fld["stride"])
    return Samples(t.numpy().reshape(n, S), dt.numpy().reshape(n, S), x.reshape(n, S, 3),
                   enc.numpy().reshape(n, S, -1), dirs.numpy().reshape(n, S, 3)[:, 0].copy(),
                   pts.numpy().reshape(n, S, 3))


def _img(kind, n):
    r = np.arange(n)
    return {"none": None, "equal": np.full(n, 3), "distinct": (r + r // 8) % N_EMB,
            "runs3": r // 3 % N_EMB}[kind]


def _set_bias(fld, P, b):
    fld["b0"].fill_(b)
    P["b_h"][0] = b


def make_inputs(c, seed):
    L, F, T = WIDTHS[c.C]
    g = torch.Generator().manual_seed(seed)
    fld = _raw_field(L, F, T, 0.0, seed=seed + 1, dev="cpu")
    P = network(fld, g)
    n, S = c.n_rays, c.S
    step = 4.0 / S
    o = torch.randn(n, 3, generator=g) * 0.25
    d = torch.randn(n, 3, generator=g)
    noise = (torch.rand(n, S, generator=g) - 0.5 + 1.0) if c.noise else None
    bg = torch.rand(n, 3, generator=g)
    img = _img(c.img, n)
    occ = None if c.occ == "none" else grids_bool(S)[c.occ].numpy()
    # the field is a near-uniform fog: a ray ends where exp(b - 3) t reaches -ln(t_thresh), t_S = 4
    if c.mode == "weight":
        b = DENSITY_SHIFT + math.log(1.0 / 4.0)                   # tau of about 1 over the whole ray
    elif c.mode == "short":
        b = DENSITY_SHIFT + math.log(LIMIT / (5.0 * step))        # about six samples
    else:
        b = DENSITY_SHIFT + math.log(LIMIT / 2.0)                 # about the middle of the ray
    _set_bias(fld, P, b)
    inp = Inputs(c, fld, P, o, d, noise, img, bg, occ, step, seed)
    if c.mode == "short":
        noise[long_rays(c)] *= 1.0 / 14.0
    elif c.mode == "lengths":
        inp = inp._replace(noise=_solve_lengths(inp))
    return inp


def _chain(inp, smp):
    """stages 1-3 -> occ, sec, e_rel [n, S]"""
    n, S, C = smp.enc.shape
    P = inp.P
    prod = smp.enc.astype(np.float64) * P["w_h"][0].double().numpy()
    b0 = float(P["b_h"][0])
    logit0, A0 = b0 + prod.sum(-1), abs(b0) + np.abs(prod).sum(-1)
    if inp.occ is None:
        occ = np.ones((n, S), dtype=bool)
    else:
        occ = inp.occ[_cells(smp.x.reshape(-1, 3), G_OCC)].reshape(n, S)
    x0 = logit0 - DENSITY_SHIFT
    sec = np.where(occ, np.exp(x0) * smp.dt.astype(np.float64), 0.0)
    return occ, sec, (C + 1) * A0 + np.abs(x0) + 4.0


def _solve_lengths(inp):
    """Per-ray scales of the noise rows so that ray r ends at required_lengths(S)[r mod .]: its depth
    crosses -ln(t_thresh) in the middle of sample m - 1 (m = S: it reaches half of it).  Decided by the
    model's own chain on the CPU oracle's samples: a condition on the inputs."""
    c = inp.case
    n, S = c.n_rays, c.S
    req = required_lengths(S)
    m = np.array([req[r % len(req)] for r in range(n)])
    rows = np.arange(n)
    # uniform fog, sigma = LIMIT / 2 per unit t, unit noise: depth_k = sigma step k s
    s = LIMIT / (LIMIT / 2.0 * inp.step * np.maximum(m - 1.5, 0.5))
    s[m == S] = 0.5
    for _ in range(12):
        noise = (inp.noise.double() * torch.from_numpy(s)[:, None]).float()
        _, sec, _ = _chain(inp, cpu_samples(inp.fld, inp.o, inp.d, noise, S, inp.step))
        depth = np.cumsum(sec, 1) - sec
        D = np.where(m == S, 2.0 * sec.sum(1), depth[rows, m - 1] + 0.5 * sec[rows, m - 1])
        s = s * np.clip(LIMIT / np.maximum(D, 1e-30), 0.25, 4.0)
    return (inp.noise.double() * torch.from_numpy(s)[:, None]).float()


# ---- the model ------------------------------------------------------------------------------------------

MUTANTS = collections.OrderedDict([   # name: what one defect it carries
    ("carry8", "the compositing carry is dropped between 8-sample strides"),
    ("carry_handover", "the compositing carry is dropped at the hand-over"),
    ("sums_handover", "the head's partial sums are dropped at the hand-over"),
    ("tail_start", "the tail starts at n_head + 64"),
    ("resumed", "a ray that ended in the head is resumed"),
    ("sh_neighbour", "SH comes from the neighbouring ray of the group"),
    ("sh_2TT", "SH comes from ray 2 TT for both halves of a 16-column block"),
    ("emb_first", "the embedding row of the group's first ray is used for all eight"),
    ("emb_none", "the embedding is not added at all"),
    ("unocc", "kept but unoccupied samples are composited"),
    ("after_stop", "compositing goes on after the stop"),
    ("drop_last", "a ray's last sample is dropped"),
    ("k_ge_S", "a sample at k >= S is included"),
    ("chain_T_last", "the chain's optical depth (to the end of the stop's 64-sample stride) gives T_last"),
    ("no_t_shift", "t_shift is omitted"),
    ("no_den_eps", "the 1e-4 of the denominator is omitted"),
    ("no_kEps", "kEps is omitted"),
    ("f16_ulp", "one encoding value of one sample is moved by one f16 ulp"),
    ("prev_sh", "the previous group's SH row is used on the second iteration of the persistent loop"),
])
HANDOVER_MUTANTS = ("carry_handover", "sums_handover", "tail_start", "resumed")
# Not a test of the bound on the rays' outputs: one ulp of one value moves its sample's logit by |w| ulp16,
# 1.1-68 E_logit (above 2 E_logit at C <= 32), but a ray's outputs carry the bounds of all its samples and
# the flip stays inside them: below 0.5 E at the sample where the logit moves most, 0.66-2.86 E at the
# opaque second sample of a two-sample ray (the len-* cases), below 0.3 E at the most opaque sample of
# every other case.  tests/test_render_model_cpu.py holds it where it is visible, the sample's head logit
# against E_logit, and prints these ratios.
INFORMATIONAL = ("f16_ulp",)


def _network(inp, smp_enc, dirs, img, use, ray_dir, ray_emb):
    """shade_model.model on the samples of `use` -> hl, E_hl [n, S], rgb, E_rgb [n, S, 3] (0 elsewhere)"""
    n, S = use.shape
    hl, E_hl = np.zeros((n, S)), np.zeros((n, S))
    rgb, E_rgb = np.zeros((n, S, 3)), np.zeros((n, S, 3))
    ri, ki = np.nonzero(use)
    C = smp_enc.shape[2]
    for lo in range(0, ri.shape[0], 1 << 15):
        r, k = ri[lo:lo + (1 << 15)], ki[lo:lo + (1 << 15)]
        rows = torch.from_numpy(np.ascontiguousarray(smp_enc[r, k]))
        ids = None if img is None else torch.from_numpy(img[ray_emb[r]].astype(np.int32))
        sin = sm.Inputs(C, rows.shape[0], rows, torch.from_numpy(np.ascontiguousarray(dirs[ray_dir[r]])), ids,
                        inp.P, None, None, 0, 0, None)
        m = sm.model(sin, backward=False)
        hl[r, k], E_hl[r, k] = m["logit"].numpy(), m["E"]["logit"].numpy()
        rgb[r, k], E_rgb[r, k] = m["rgb"].numpy(), m["E"]["rgb"].numpy()
    return hl, E_hl, rgb, E_rgb


def _excl(a):
    return np.cumsum(a, 1) - a


def _later(a):
    """out[:, k] = sum_{j>k} a[:, j]"""
    return np.cumsum(a[:, ::-1], 1)[:, ::-1] - a


def model(inp, smp, mut=None, n_head=WHOLE, at=None, loop=HEAD_LOOP, t_shift=T_SHIFT32, den_eps=DEN_EPS32):
    """-> dict: colors [n,3], depths, last_trans [n] (float64), kept, len [n] int, ambiguous [n] bool,
    E: bound per output, and the intermediates the tests look at (w, use [n, S]).  mut: one of MUTANTS
    (n_head: where the hand-over lies, for the mutants that need one; at = (ray, sample, channel) for
    f16_ulp; loop: the rays one pass of the persistent grid covers, for prev_sh)."""
    assert mut is None or mut in MUTANTS
    c = inp.case
    n, S, C = smp.enc.shape
    enc, t, dt, dirs = smp.enc, smp.t.astype(np.float64), smp.dt.astype(np.float64), smp.dirs
    if mut == "f16_ulp":
        r, k, ch = at
        enc = enc.copy()
        v = np.float16(enc[r, k, ch])
        enc[r, k, ch] = np.float32(np.nextafter(v, np.float16(np.inf)))
        smp = smp._replace(enc=enc)
    occ, sec, e_rel = _chain(inp, smp)
    length, in_band = rc.keep_rule(sec, e_rel, T_THRESH)
    length = length.astype(np.int64)
    kk = np.arange(S)[None, :]
    pos = kk < length[:, None]
    use = pos & occ
    kept = use.sum(1)
    rays = np.arange(n)
    ray_dir, ray_emb, img = rays, rays, inp.img
    goes_on = (length > n_head)[:, None]
    if mut == "unocc":
        use = pos
    elif mut == "after_stop":
        use = occ
    elif mut == "drop_last":
        last = S - 1 - np.argmax(use[:, ::-1], 1)
        use = use.copy()
        use[rays, last] = False
    elif mut == "tail_start":
        use = use & ~(goes_on & (kk >= n_head) & (kk < n_head + 64))
    elif mut == "resumed":
        use = use | ((length <= n_head)[:, None] & occ & (kk >= n_head))
    elif mut == "sh_neighbour":
        ray_dir = np.where((rays ^ 1) < n, rays ^ 1, rays - 1 if n > 1 else rays)
    elif mut == "sh_2TT":
        ray_dir = rays & ~1
    elif mut == "emb_first":
        ray_emb = rays & ~7
    elif mut == "emb_none":
        img = None
    elif mut == "prev_sh":
        ray_dir = np.where(rays >= loop, rays - loop, rays)
    elif mut == "k_ge_S":        # sample S: sample S - 1 once more, one dt further on
        ext = (length == S) & occ[:, -1]
        enc = np.concatenate([enc, enc[:, -1:]], 1)
        t = np.concatenate([t, t[:, -1:] + dt[:, -1:]], 1)
        dt = np.concatenate([dt, dt[:, -1:]], 1)
        use = np.concatenate([use, ext[:, None]], 1)
        sec = np.concatenate([sec, sec[:, -1:]], 1)
        kk = np.arange(S + 1)[None, :]
    hl, E_hl, rgb, E_rgb = _network(inp, enc, dirs, img, use, ray_dir, ray_emb)
    if mut == "no_kEps":
        rgb = np.where(use[:, :, None], rgb + sm.EPS32, 0.0)

    # ---- compositing: the closed forms of ragged_cases.composite_fwd_ref over the list `use`
    x2 = hl - DENSITY_SHIFT
    ax = np.abs(x2)
    sec2 = np.where(use, np.exp(x2) * dt, 0.0)
    acc = _excl(sec2)
    if mut == "carry8":
        acc = acc - acc[:, (np.arange(acc.shape[1]) // 8) * 8]
    elif mut == "carry_handover" and n_head < S:
        acc = np.where(kk >= n_head, acc - acc[:, n_head:n_head + 1], acc)
    T = np.exp(-acc)
    w = np.where(use, T * -np.expm1(-sec2), 0.0)
    tau = sec2.sum(1)
    if mut == "chain_T_last":
        tau = np.where(kk < np.minimum(S, -(-length // 64) * 64)[:, None], sec, 0.0).sum(1)
    Tl = np.exp(-tau)
    tp = np.where(use, t + (0.0 if mut == "no_t_shift" else t_shift), 0.0)
    ws = w
    if mut == "sums_handover":
        ws = np.where(goes_on & (kk < n_head), 0.0, w)
    bg = inp.bg.double().numpy()
    colors = (ws[:, :, None] * rgb).sum(1) + Tl[:, None] * bg
    den = 1.0 - Tl + (0.0 if mut == "no_den_eps" else den_eps)
    Nd = (ws * tp).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        depths = np.where(den > 0, Nd / den, 0.0)
        den = np.where(den > 0, den, 1.0)

    # ---- (a) the compositing's own roundings: ragged_cases' conditioning numbers
    argb, abg = np.abs(rgb), np.abs(bg)
    accx, taux = _excl(sec2 * (2.0 + ax)), (sec2 * (2.0 + ax)).sum(1)
    m_w_sum = w * acc
    m_w_op = np.where(use, T * (1.0 + (2.0 + ax) * np.minimum(sec2, 1.0)) + w * (2.0 + accx), 0.0)
    m_Tl_sum, m_Tl_op = Tl * tau, Tl * (1.0 + taux)
    msum = {"last_trans": m_Tl_sum, "colors": ((m_w_sum + w)[:, :, None] * argb).sum(1) + (m_Tl_sum + Tl)[:, None] * abg}
    mop = {"last_trans": m_Tl_op, "colors": (m_w_op[:, :, None] * argb).sum(1) + (m_Tl_op + Tl)[:, None] * abg}
    m_Nd_sum, m_Nd_op = ((m_w_sum + w) * tp).sum(1), ((m_w_op + w) * tp).sum(1)
    dep = Nd / den
    msum["depths"] = m_Nd_sum / den + dep * m_Tl_sum / den
    mop["depths"] = m_Nd_op / den + dep * (m_Tl_op / den + 3.0)
    # ---- (b) E_rgb and E_logit through the Jacobian
    some = kept > 0
    E, Ea, Eb = {}, {}, {}
    Eb["last_trans"] = (Tl[:, None] * sec2 * E_hl).sum(1)
    dw = tp / den[:, None]
    J = sec2 * (dw * (T - w) - _later(dw * w) - (Tl * Nd / (den * den))[:, None])
    Eb["depths"] = (np.abs(J) * E_hl).sum(1)
    Jc = sec2[:, :, None] * (rgb * (T - w)[:, :, None] - _later(rgb * w[:, :, None]) - (Tl[:, None] * bg)[:, None, :])
    Eb["colors"] = (w[:, :, None] * E_rgb).sum(1) + (np.abs(Jc) * E_hl[:, :, None]).sum(1)
    for name in OUTPUTS:
        cnt = kept if msum[name].ndim == 1 else kept[:, None]
        Ea[name] = U * (cnt * msum[name] + rc.K_COMPOSITE * mop[name])
        E[name] = np.where(some if msum[name].ndim == 1 else some[:, None], Ea[name] + Eb[name], 0.0)
    return dict(colors=colors, depths=depths, last_trans=Tl, kept=kept.astype(np.int64), len=length,
                ambiguous=in_band, E=E, Ea=Ea, Eb=Eb, w=w, use=use, occ=occ, hl=hl, E_hl=E_hl, rgb=rgb,
                sec2=sec2,
                J_depths=J, J_colors=Jc)


# ---- comparison -----------------------------------------------------------------------------------------

def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def ratios(got, ref):
    """largest |got - f64| / E per output over the unambiguous rays (0 / 0 = 0, x / 0 = inf)"""
    rows = ~ref["ambiguous"]
    out = {}
    for name in OUTPUTS:
        r = sm.ratio(torch.from_numpy(_np(got[name]).astype(np.float64)), torch.from_numpy(ref[name]),
                     torch.from_numpy(ref["E"][name]), torch.from_numpy(rows))
        out[name] = float(r.max()) if r.numel() else 0.0
    return out


def failures(got, ref):
    """Every assertion tests/test_gpu_render_f64.py makes on one route's outputs (colors, depths,
    last_trans, kept, len: arrays or tensors) against a model, as a list of messages; empty = all
    hold."""
    fails = []
    amb = ref["ambiguous"]
    for name in ("kept", "len"):
        g = _np(got[name]).astype(np.int64)
        bad = np.flatnonzero(np.where(amb, np.abs(g - ref[name]) > 1, g != ref[name]))
        fails += ["%s[%d] = %d, model %d%s" % (name, r, g[r], ref[name][r], " (ambiguous)" if amb[r] else "")
                  for r in bad]
    for name in OUTPUTS:
        g = _np(got[name]).astype(np.float64)
        if not np.isfinite(g).all():
            fails.append("%s: not finite on rays %s" % (name, np.flatnonzero(~np.isfinite(g).reshape(g.shape[0], -1).all(1))[:8]))
            continue
        err, E = np.abs(g - ref[name]), ref["E"][name]
        bad = ~(err <= BAR * E)
        bad[amb] = False
        for r in np.flatnonzero(bad.reshape(bad.shape[0], -1).any(1)):
            fails.append("%s[%d]: got %s, f64 %s, |err| %s, E %s (kept %d, len %d)" % (
                name, r, g[r], ref[name][r], err[r], E[r], ref["kept"][r], ref["len"][r]))
    return fails


def old_bar_passes(got, ref):
    """The bar of the existing render tests, _close(a, b, 1e-4) = rtol 1e-4 + 1e-5 of the largest
    element, on colours, depths and the opacity 1 - last_trans, and their exact counts."""
    for name in ("kept", "len"):
        if not np.array_equal(_np(got[name]).astype(np.int64), ref[name]):
            return False
    for name in OUTPUTS:
        g, b = _np(got[name]).astype(np.float64), ref[name]
        if name == "last_trans":
            g, b = 1.0 - g, 1.0 - b
        if not (np.abs(g - b) <= 1e-4 * np.abs(b) + 1e-5 * np.abs(b).max() + 1e-12).all():
            return False
    return True


def sources_differ(fld, cpu, dev):
    """The device's samples (f2n_sample_rays, f2n_contract_fwd, f2n_hash_fwd) against the CPU oracle's;
    raises AssertionError where they differ by more than is allowed:
      t, dt, points, directions   as tests/test_gpu_ops.py::test_sample_rays allows;
      contracted points           within 2 E of ray_grad_model.contract_fwd_model at the device's points;
      encoding rows               the bits of K.hash_fwd at the device's OWN contracted points: the
                                  standing bar of test_hash_fwd_parity, and with the same points no
                                  discontinuity of the encoding is involved.
    Between the two sources' encodings themselves no bound is asserted: their points differ by an ulp or
    a few, and a scaled coordinate below zero reads cell 0 whatever its integer part (quirk Q1), so the
    encoding is not continuous there.  -> share of encoding values that differ between the sources at
    all, largest difference (reported)."""
    torch.testing.assert_close(torch.from_numpy(dev.t), torch.from_numpy(cpu.t), rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(torch.from_numpy(dev.pts), torch.from_numpy(cpu.pts), rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(torch.from_numpy(dev.dt), torch.from_numpy(cpu.dt), rtol=1e-3, atol=2e-6)
    assert (dev.dt[:, 0] == 0).all()
    torch.testing.assert_close(torch.from_numpy(dev.dirs), torch.from_numpy(cpu.dirs), rtol=1e-6, atol=1e-7)
    x64, E_x, zero = contract_fwd_model(torch.from_numpy(np.ascontiguousarray(dev.pts.reshape(-1, 3))))
    assert not zero.any()
    err = np.abs(dev.x.reshape(-1, 3).astype(np.float64) - x64)
    assert (err <= BAR * E_x).all(), float((err / np.maximum(E_x, 1e-300)).max())
    want = K.hash_fwd(torch.from_numpy(np.ascontiguousarray(dev.x.reshape(-1, 3))), fld["table16"], fld["primes"],
                      fld["bias"], fld["mul"], fld["L"], fld["F"], fld["T"], fld["stride"]).numpy()
    got = dev.enc.reshape(want.shape)
    assert np.array_equal(got, want), (int((got != want).sum()), want.size)
    diff = np.abs(dev.enc.astype(np.float64) - cpu.enc.astype(np.float64))
    return float((diff != 0).mean()), float(diff.max())


# ---- conditions on the inputs ---------------------------------------------------------------------------

def ambiguity_ok(c, m):
    n_amb = int(m["ambiguous"].sum())
    return n_amb == 0 if c.n_rays < 50 else n_amb <= MAX_AMBIGUOUS * c.n_rays


def check_conditions(c, m):
    """What a case has to show, from the model's counts and weights alone (conditions on the inputs,
    not on a kernel); raises AssertionError."""
    S, n = c.S, c.n_rays
    clear = ~m["ambiguous"]
    length, kept, Tl, w = m["len"], m["kept"], m["last_trans"], m["w"]
    assert ambiguity_ok(c, m), (c.name, int(m["ambiguous"].sum()))
    if c.mode == "lengths":
        seen = set(length[clear].tolist())
        assert set(required_lengths(S)) <= seen, (c.name, sorted(set(required_lengths(S)) - seen))
        groups = [len(set(length[g:g + 8].tolist())) for g in range(0, n - 7, 8)]
        assert max(groups) >= 5, (c.name, groups)
        if S > 64:       # the hand-over: rays that end exactly at sample 64, before it, and go on
            assert (length[clear] == 64).any() and (length[clear] < 64).any() and (length[clear] > 64).any()
    if c.mode == "weight":
        assert (length == S).all() and ((Tl > 0.05) & (Tl < 0.95)).all(), (c.name, Tl.min(), Tl.max())
        assert (w[:, 8:].sum(1) > 0.1 * w.sum(1)).all(), c.name
        if S > 64:
            assert (w[:, 64:].sum(1) > 0.1 * w.sum(1)).all(), c.name
    if c.mode == "short":
        far = np.zeros(n, dtype=bool)
        far[long_rays(c)] = True
        assert (length[~far] <= 16).all() and (length[far] > min(64, S - 1)).all(), c.name
        assert far[ONE_RAY_LOOP:].any() and (n <= HEAD_LOOP or far[HEAD_LOOP:].all())
    if c.occ == "random":
        assert (kept < length).any(), c.name
    if c.occ == "empty":
        assert (kept == 0).all() and (length == S).all()
    if c.occ in ("shell", "random"):
        assert (kept > 0).any(), c.name


@functools.lru_cache(maxsize=None)
def build_case(c):
    """-> (Inputs, Samples, model dict) from the CPU oracle's samples; seeds are walked until the
    ambiguity cap and the case's other conditions hold, the seed that did is inp.seed.  Built once and shared, read only."""
    why = []
    for bump in range(32):
        seed = 1009 * c.C + 7 * c.S + c.n_rays + 100000 * bump
        inp = make_inputs(c, seed)
        smp = cpu_samples(inp.fld, inp.o, inp.d, inp.noise, c.S, inp.step)
        m = model(inp, smp)
        try:
            check_conditions(c, m)
            break
        except AssertionError as e:      # (an unoccupied sample where a ray was to end, an ambiguous ray)
            why.append("seed %d: %r" % (seed, e))
    else:
        raise AssertionError("no seed meets the conditions of %s:\n%s" % (c.name, "\n".join(why)))
    return inp, smp, m


def ulp_site(inp, smp, m):
    """f16_ulp: the kept, occupied sample and the channel where one f16 ulp moves the head logit the most
    in units of its bound, |w_h[0, c]| ulp16(enc_c) / E_logit -> (ray, sample, channel), |moved| / E_logit"""
    enc16 = smp.enc.astype(np.float16)
    ulp = np.nextafter(enc16, np.float16(np.inf)).astype(np.float64) - enc16.astype(np.float64)
    moved = np.abs(inp.P["w_h"][0].double().numpy()) * ulp
    ch = moved.argmax(-1)
    best = np.where(m["use"] & ~m["ambiguous"][:, None], moved.max(-1) / np.maximum(m["E_hl"], 1e-300), 0.0)
    r, k = np.unravel_index(int(np.argmax(best)), best.shape)
    return (int(r), int(k), int(ch[r, k])), float(best[r, k])


def applies(mut, c, m, n_head=WHOLE):
    """whether mutant `mut` changes anything the case can show (from the model's counts alone)"""
    length, kept, clear = m["len"], m["kept"], ~m["ambiguous"]
    S = c.S
    if c.mode == "short":            # the loop cases exist for the loops alone
        return mut == "prev_sh"
    if mut == "prev_sh":
        return False
    some = bool((kept[clear] > 0).any())
    if mut in HANDOVER_MUTANTS:
        if n_head >= S:
            return False
        use = m["use"]
        before, behind = use[:, 1:n_head].any(1), use[:, n_head:].any(1)    # (sample 0 has dt = 0: no weight)
        if mut == "resumed":         # a ray that ended in the head, with occupied samples behind n_head
            return bool((clear & (length <= n_head) & m["occ"][:, n_head:].any(1)).any())
        if mut == "tail_start":
            return bool((clear & use[:, n_head:n_head + 64].any(1)).any())
        return bool((clear & before & behind).any())
    if mut == "carry8":
        return bool((clear & m["use"][:, 1:8].any(1) & m["use"][:, 8:].any(1)).any())
    if mut in ("sh_neighbour", "sh_2TT"):
        return some and c.n_rays > 1
    if mut in ("emb_first", "emb_none"):
        return some and c.img != "none" and (mut == "emb_none" or (c.img != "equal" and c.n_rays > 1))
    if mut == "unocc":
        return bool((clear & (kept < length)).any())
    if mut == "after_stop":
        return bool((clear & (length < S) & m["occ"][np.arange(c.n_rays), np.minimum(length, S - 1)]).any())
    if mut == "k_ge_S":
        return bool((clear & (length == S) & m["occ"][:, -1]).any())
    if mut == "chain_T_last":
        return bool((clear & (length < S) & (length % 64 != 0) & (kept > 0)).any())
    return some
