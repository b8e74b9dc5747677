"""Inputs, a CPU model and the assertions for the loss terms of f2n::train_step taken together: the
variance, distortion, three line-of-sight depth terms, the opacity term and the D-SSIM term on ONE
render, each alone and all at once, in four contexts.  No tests in here: tests/test_step_terms_cpu.py
checks the model and its mutants on the CPU, tests/test_gpu_step_terms.py makes the same assertions on
the HIP step on every route.

Scenes (tests/test_gpu_render._setup: L = 4, F = 2, T = 2^12, S = 128, 8 patches of 11 x 11 = 968 rays in
patch-major order): "thin" keeps every sample (123 904 >= 65 536: the table gradient takes the binned
integer sums); "terminating" stops rays and compacts.

The two assertions.
  1. sum of the parts:  g(all) - g(none) = sum_i [g(only i) - g(none)], exact in real arithmetic (the
     loss is a sum of terms on one render and no term changes the render).  k + 2 gradient evaluations
     meet in it: residual <= (k + 2) bar(key) max |g|.
  2. a route against the op-by-op route, term by term:  |D_i(route) - D_i(op by op)| <= bar(key) max |g|,
     D_i = g(only i) - g(none), and the same for g(all).
max |g| is the largest norm among the FULL gradients involved (the rounding of g(only i) scales with g,
not with D_i).  bar: 1e-4 for every parameter (the figure the suite holds a table gradient to between
two routes, and the float-atomic sums of the network and the embedding between two evaluations), 5e-3
for ray and pose gradients (tests/test_gpu_pose_grad.py between fused and op by op).
The precondition that gives the bars their teeth: |D_i| >= 0.1 |g(none)| in the table gradient, for
every term, asserted by every test.

The model.  Two stages.  Stage 1, `per_ray` and `step_grads`: the terms as the host code spells them, from the
render's colours [n, 3] and kept weights as leaves -- the divisors 1/n, 1/n_valid, 1/W, 1/M, the masked
rays' weights before each reduction, the composited target.  Stage 2: the oracle's Renderer (float32,
f16 table contributions; `render32`) or its float64 twin (`render64`: the same samples and the f16
roundings that define the encoding and its table gradient, everything else in float64) carries (d_colors, d_weights) to the parameters.  The
mutants (MUTANTS) live between the stages, where the host glue is.
"""
import collections
import functools

import numpy as np
import torch

from oracle import kernels as K
from oracle import ref_render as R

L, F, LOG2_T, S = 4, 2, 12, 128
STEP = 4.0 / S
N_PATCH, P = 8, 11
N = N_PATCH * P * P
E_IMG = 7
SCENES = collections.OrderedDict([("thin", (1.0, 61)), ("terminating", (4.0, 67))])   # bias0, seed
TERMS = ("var", "dist", "empty", "near", "expected", "opacity", "ssim")
CONTEXTS = ("plain", "masked", "sky", "pose")
DEPTH_EPS = 0.05
# chosen on the CPU model, per scene, so that every term alone moves the table gradient by about half of
# |g(none)|: well above MIN_SHARE, and no term so large that the others hide under a bar that scales
# with |g(all)| (tests/test_step_terms_cpu.py prints the shares)
WEIGHTS = dict(
    thin=dict(var=0.025, dist=0.05, empty=12.0, near=0.7, expected=0.02, opacity=0.2, ssim=0.06),
    terminating=dict(var=0.005, dist=0.012, empty=0.08, near=0.07, expected=0.005, opacity=3.3, ssim=0.03))
# An occupancy grid thins the kept lists: the render is another one, and so is every term's share.
# Factors on WEIGHTS for the *_grid routes, from the shares the routes showed at WEIGHTS (linear in
# the weight): again about a half, at least MIN_SHARE in every context.
GRID_FACTOR = dict(
    thin=dict(var=3.0, dist=15.0, empty=1.0, near=1.0, expected=2.0, opacity=0.3, ssim=6.0),
    terminating=dict(var=20.0, dist=25.0, empty=4.0, near=4.0, expected=12.0, opacity=0.02, ssim=1.0))
MIN_SHARE = 0.1


def weights(scene_name, route=""):
    w = dict(WEIGHTS[scene_name])
    if route.endswith("grid"):
        w = {k: v * GRID_FACTOR[scene_name][k] for k, v in w.items()}
    return w
BAR_PARAM, BAR_RAYS = 1e-4, 5e-3
U = 2.0 ** -24


def bar(key):
    return BAR_RAYS if key_class(key) == "rays" else BAR_PARAM


def key_class(key):
    if key in ("rays_o", "rays_d", "delta"):
        return "rays"
    return "table" if key.endswith("feat_pool") else "net"


# What the unmutated float32 model uses of a bar, as residual / bar, the largest over the contexts: the
# figures as measured, not rounded up (tests/test_step_terms_cpu.py::test_model_residuals_are_the_recorded_ones
# re-measures them):
#   a1  the model's own sum of the parts (in real arithmetic 0);
#   a2  the float32 model against its float64 twin, term by term and for g(all).
# A figure above a quarter widens that bar to four times the figure (the rule of ssim_cases.allowed); a
# figure at or below it leaves the bar alone, however close it comes.  NOTES section 36 says where the
# table's figures come from.  Never set from what the HIP step gives.
# The "table" and "rays" figures come from the f16 roundings of the encoding and its gradients and
# repeat to three digits from machine to machine; the "net" figures are reassociation noise of the
# CPU's BLAS and move with it (0.001 to 0.12 between two machines; the one above a quarter, 0.26, was
# 0.243 on another).
MODEL_RESIDUAL = {
    ("thin", "a1", "table"): 3.29, ("thin", "a1", "net"): 0.0012, ("thin", "a1", "rays"): 0.0486,
    ("thin", "a2", "table"): 0.2407, ("thin", "a2", "net"): 0.033, ("thin", "a2", "rays"): 0.0,
    ("terminating", "a1", "table"): 12.39, ("terminating", "a1", "net"): 0.0135,
    ("terminating", "a1", "rays"): 0.2383,
    ("terminating", "a2", "table"): 1.86, ("terminating", "a2", "net"): 0.26,
    ("terminating", "a2", "rays"): 0.0,                          # (the twin carries no ray gradient)
}


def allowed(scene_name, which, key):
    """the largest residual / bar an assertion accepts: 1, or 4 x the model's figure where that is
    above a quarter.  The model has no occupancy grid: the *_grid routes are held to the figures of
    the model without one (their weights differ, GRID_FACTOR; the bars do not)."""
    r = MODEL_RESIDUAL[(scene_name, which, key_class(key))]
    return 4.0 * r if r > 0.25 else 1.0


# ---- inputs ----------------------------------------------------------------------------------------

def setup(host, bias0, seed):
    """tests/test_gpu_render._setup; without a host only the oracle half of it (the same draws)"""
    if host is not None:
        from tests.test_gpu_render import _setup
        return _setup(host, L, F, LOG2_T, S, STEP, N, bias0, seed, E=E_IMG)
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    oracle = R.Renderer(E_IMG, L=L, F=F, log2_T=LOG2_T, S=S, step=STEP, gen=g, feat_init="trained")
    with torch.no_grad():
        oracle.scene_field.mlp.bias[0] = bias0
    o = torch.randn(N, 3, generator=g) * 0.25
    d = torch.randn(N, 3, generator=g)
    noise = torch.rand(N, S, generator=g) - 0.5 + 1.0
    bg = torch.rand(N, 3, generator=g)
    gt = torch.rand(N, 3, generator=g)
    emb = torch.randint(0, E_IMG, (N,), generator=g).to(torch.int32)
    return oracle, None, o, d, noise, bg, gt, emb


def extras(name, noise):
    """what the terms and the contexts need beside _setup's draws; all float32, on the CPU"""
    g = torch.Generator().manual_seed(1000 + SCENES[name][1])
    t = torch.cumsum(noise, 1) * STEP
    z = t[:, 0] + (0.05 + 0.6 * torch.rand(N, generator=g)) * (t[:, -1] - t[:, 0])
    bad = torch.tensor([0.0, float("inf"), float("nan")])
    z[::8] = bad[torch.arange(z[::8].numel()) % 3]
    alpha = torch.rand(N, generator=g)
    alpha[::7] = 0.0
    m = 2.0 * (1.0 - torch.rand(N, generator=g))                 # (0, 2]
    m[torch.randperm(N, generator=g)[:N // 5]] = 0.0            # a fifth of the rays at exactly 0
    patch_weight = torch.tensor([1.0, 0.0, 0.5, 2.0, 1.0, 1.5, 0.25, 1.0])
    sky_bg = torch.rand(N, 3, generator=g)                       # the model's stand-in for the sky's colours
    perm = torch.randperm(N, generator=g)
    return dict(z=z, alpha=alpha, ray_weight=m, patch_weight=patch_weight, sky_bg=sky_bg, perm=perm)


def depth_n_valid(z):
    return float((z.gt(0) & z.lt(float("inf"))).sum().clamp_min(1))


# ---- the render, twice -------------------------------------------------------------------------------

Render = collections.namedtuple("Render", "colors weights idx t dt rid pos params leaves")


def _params(oracle):
    return collections.OrderedDict([
        ("scene_field.feat_pool", oracle.scene_field.feat_pool),
        ("scene_field.mlp.weight", oracle.scene_field.mlp.weight),
        ("scene_field.mlp.bias", oracle.scene_field.mlp.bias),
        ("shader.mlp.0.weight", oracle.shader.mlp[0].weight),
        ("shader.mlp.0.bias", oracle.shader.mlp[0].bias),
        ("shader.mlp.2.weight", oracle.shader.mlp[2].weight),
        ("shader.mlp.2.bias", oracle.shader.mlp[2].bias),
        ("app_emb", oracle.app_emb),
    ])


def _ray_ids(idx):
    count = (idx[:, 1] - idx[:, 0]).long()
    rid = torch.repeat_interleave(torch.arange(idx.shape[0]), count)
    pos = torch.arange(int(count.sum())) - idx[:, 0].long()[rid]
    return rid, pos


def render32(oracle, o, d, emb, noise, bg, grad_rays=False):
    """R.Renderer.render (TRAIN) line for line, handing the kept t and dt on as well; bg and, when
    asked, the rays are leaves whose gradients join the compared set"""
    f = oracle.scene_field
    leaves = collections.OrderedDict(bg=bg.clone().requires_grad_(True))
    if grad_rays:
        o, d = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
        leaves["rays_o"], leaves["rays_d"] = o, d
    pts, dirs, dt, t, bounds = R.get_samples(o, d, noise, S, STEP)
    with torch.no_grad():
        sec = oracle.density_act(f.query(pts)[:, 0:1])[:, 0] * dt
        mask = torch.exp(-R.flex_accumulate_sum(sec, bounds, False)) > 1e-4
    mask_idx = torch.where(mask)[0]
    pts2, dirs2 = pts[mask_idx].contiguous(), dirs[mask_idx].contiguous()
    dt2, t2 = dt[mask_idx].contiguous(), t[mask_idx].contiguous()
    num = mask.reshape(N, S).sum(1)
    cum = torch.cumsum(num, 0)
    idx = torch.stack([cum - num, cum], -1).to(torch.int32).contiguous()
    feat = f.query(pts2)
    density = oracle.density_act(feat[:, 0:1])
    shading = torch.cat([torch.ones_like(feat[:, 0:1]), feat[:, 1:]], 1)
    shading = R.ScatterAddFunc.apply(oracle.app_emb, K.scatter_idx(pts2.shape[0], idx, emb), shading)
    rgb = oracle.shader.query(shading, dirs2)
    sec = density[:, 0] * dt2
    weights = torch.exp(-R.flex_accumulate_sum(sec, idx, False)) * (1.0 - torch.exp(-sec))
    last_trans = torch.exp(-R.flex_sum(sec, idx))
    colors = R.flex_sum(weights.unsqueeze(-1) * rgb, idx) + last_trans.unsqueeze(-1) * leaves["bg"]
    rid, pos = _ray_ids(idx)
    return Render(colors, weights, idx, t2.detach(), dt2.detach(), rid, pos, _params(oracle), leaves)


class _Encode64(torch.autograd.Function):
    """the trilinear hash encoding of f2no_hash_fwd / f2no_hash_bwd in float64 arithmetic, with the
    f16 roundings that belong to the operation's definition kept: the result is rounded to f16, and the
    table gradient is the sum of the contributions f16(f16(128 g) w) / 128"""

    @staticmethod
    def forward(ctx, x, feat, f):
        flat = feat.reshape(-1)
        mul = f.mul.to(x.dtype)
        out, rows, ws = [], [], []
        for l in range(f.L):
            # (the cell coordinate is the kernels' own float32 fmaf of the float32 position: data)
            pt = (x * mul[l] + f.bias_pool[l].detach().to(x.dtype)).float().to(x.dtype)
            fl = torch.floor(pt)
            a = pt - fl
            p = fl.clamp_min(0.0).long()                       # (sat_u32: a negative coordinate hashes as 0)
            prim = f.prim_pool[l].long()
            acc = 0
            for c in range(8):
                off = torch.tensor([(c >> 2) & 1, (c >> 1) & 1, c & 1])
                h = ((p + off) * prim) & 0xFFFFFFFF
                row = (h[:, 0] ^ h[:, 1] ^ h[:, 2]) % f.T
                w = torch.where(off.bool(), a, 1.0 - a).prod(1)
                base = f.level_stride * l + row * f.F
                acc = acc + w[:, None] * flat[base[:, None] + torch.arange(f.F)]
                rows.append(base)
                ws.append(w)
            out.append(acc)
        ctx.f, ctx.shape = f, feat.shape
        ctx.save_for_backward(torch.stack(rows), torch.stack(ws))
        return torch.cat(out, 1).half().to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        rows, ws = ctx.saved_tensors
        f = ctx.f
        grad = torch.zeros(int(np.prod(ctx.shape)), dtype=g.dtype)
        g16 = (128.0 * g).half().to(g.dtype)
        for l in range(f.L):
            for c in range(8):
                for k in range(f.F):
                    contrib = (g16[:, l * f.F + k] * ws[l * 8 + c]).half().to(g.dtype)
                    grad.index_add_(0, rows[l * 8 + c] + k, contrib)
        return None, (grad / 128.0).reshape(ctx.shape), None


def render64(oracle, o, d, emb, noise, bg, idx):
    """the float64 twin on the kept samples of render32 (`idx`): float32 samples and SH values as data,
    the table read at its f16 values with the gradient handed to the master copy; the f16 roundings of
    the encoding and of its table-gradient contributions are part of the operation and stay"""
    f, dt64 = oracle.scene_field, torch.float64
    params = collections.OrderedDict((k, v.detach().to(dt64).requires_grad_(True))
                                     for k, v in _params(oracle).items())
    leaves = collections.OrderedDict(bg=bg.to(dt64).requires_grad_(True))
    pts, dirs, dt, t, _ = R.get_samples(o, d, noise, S, STEP)
    rid, pos = _ray_ids(idx)
    flat = rid * S + pos                                         # kept prefixes
    pts2, dirs2, dt2, t2 = pts[flat], dirs[flat].contiguous(), dt[flat].to(dt64), t[flat].to(dt64)
    norm = pts2.norm(2, dim=1, keepdim=True)                     # Hash3DAnchored.query, in its float32
    inside = norm <= 1.0
    x = (pts2 * inside + ~inside * (1 + 1.0 - 1.0 / norm) * pts2 / norm).to(dt64)
    pool = params["scene_field.feat_pool"]
    pool16 = R.K.cast_f16(pool.detach().float().reshape(-1)).view(torch.float16).to(dt64).reshape(pool.shape)
    enc = _Encode64.apply(x.detach(), pool + (pool16 - pool).detach(), f)
    feat = enc @ params["scene_field.mlp.weight"].t() + params["scene_field.mlp.bias"]
    density = torch.exp(feat[:, 0] - 3.0)
    shading = torch.cat([torch.ones_like(feat[:, 0:1]), feat[:, 1:]], 1) + params["app_emb"][emb.long()[rid]]
    h = torch.cat([shading, K.sh_encode(dirs2, 4).to(dt64)], 1)
    h = torch.relu(h @ params["shader.mlp.0.weight"].t() + params["shader.mlp.0.bias"])
    out = h @ params["shader.mlp.2.weight"].t() + params["shader.mlp.2.bias"]
    rgb = (1.0 + 2e-3) / (1.0 + torch.exp(-out)) - 1e-3
    sec = density * dt2
    secp = torch.zeros(N, S, dtype=dt64).index_put((rid, pos), sec)
    acc = (torch.cumsum(secp, 1) - secp)[rid, pos]
    weights = torch.exp(-acc) * (1.0 - torch.exp(-sec))
    last_trans = torch.exp(-secp.sum(1))
    colors = torch.zeros(N, 3, dtype=dt64).index_add(0, rid, weights[:, None] * rgb) + \
        last_trans[:, None] * leaves["bg"]
    return Render(colors, weights, idx, t2, dt2, rid, pos, params, leaves)


# ---- stage 1: the terms as the host code spells them ---------------------------------------------------

class _WeightVar(torch.autograd.Function):
    """WeightVarLoss forward and backward as coded (oracle/f2n_oracle.c), in the dtype of w"""

    @staticmethod
    def forward(ctx, wp):                                        # [n, S], zeros behind the kept prefix
        x = torch.arange(wp.shape[1], dtype=wp.dtype) / 16.0
        wsum = wp.sum(1) + 1e-6
        mean = (wp * x).sum(1) / wsum
        b = x[None] - mean[:, None]
        ctx.save_for_backward(wp, b, wsum, x)
        return (wp * b * b).sum(1)

    @staticmethod
    def backward(ctx, g):
        wp, b, wsum, x = ctx.saved_tensors
        tmp = (2.0 * wp * b).sum(1)
        return g[:, None] * (b * b + (tmp / wsum)[:, None] * -x[None])


class _PermGrad(torch.autograd.Function):
    """identity whose gradient comes back through a permutation of the rays (a mutant's tool)"""

    @staticmethod
    def forward(ctx, x, perm):
        ctx.perm = perm
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return g[ctx.perm], None


def _padded(r, v):
    return torch.zeros(N, S, dtype=v.dtype).index_put((r.rid, r.pos), v)


def per_ray(r, weights, z):
    """var [n], dist [n], depth terms [n, 3], opacity [n] of the kept weights, in their dtype"""
    dt_ = weights.dtype
    kept = _padded(r, torch.ones_like(weights)).bool()
    wp = _padded(r, weights)
    var = torch.where(kept.any(1), _WeightVar.apply(wp), torch.zeros(N, dtype=dt_))
    t, dt = r.t.to(dt_), r.dt.to(dt_)
    mid = _padded(r, t - 0.5 * dt)
    x = torch.where(kept, mid - mid[:, :1], torch.zeros_like(mid))
    dtp = _padded(r, dt)
    Pp = torch.cumsum(wp, 1) - wp
    Qp = torch.cumsum(wp * x, 1) - wp * x
    dist = (2.0 * wp * (x * Pp - Qp)).sum(1) + (wp * wp * dtp).sum(1) / 3.0
    # membership by the kernels' own float32 comparisons
    m32 = _padded(r, (r.t.float() - 0.5 * r.dt.float()))
    lo, hi = (z - np.float32(DEPTH_EPS))[:, None], (z + np.float32(DEPTH_EPS))[:, None]
    valid = z.gt(0) & z.lt(float("inf"))
    front = (kept & (m32 < lo)).to(dt_)
    band = (kept & (m32 >= lo) & (m32 <= hi)).to(dt_)
    zz = torch.where(valid, z, torch.zeros_like(z)).to(dt_)
    terms = torch.stack([(front * wp * wp).sum(1), (1.0 - (band * wp).sum(1)) ** 2,
                         ((wp * mid).sum(1) - zz) ** 2], 1)
    terms = torch.where(valid[:, None], terms, torch.zeros_like(terms))
    return var, dist, terms, wp.sum(1)


def _ssim(x, y):
    """[n, P, P, 3] -> [n]: the unclamped SSIM of tests/ssim_model.ssim64 in ATen's conv form"""
    from tests import ssim_model as M
    f = torch.as_tensor(M.filter64()).to(x.dtype)
    k = (f[:, None] * f[None, :])[None, None]
    n = x.shape[0]
    cv = lambda v: torch.nn.functional.conv2d(v.permute(0, 3, 1, 2).reshape(n * 3, 1, P, P), k)
    mux, muy = cv(x), cv(y)
    sxx, syy, sxy = cv(x * x) - mux * mux, cv(y * y) - muy * muy, cv(x * y) - mux * muy
    s = ((2 * mux * muy + M.C1) * (2 * sxy + M.C2)) / ((mux * mux + muy * muy + M.C1) * (sxx + syy + M.C2))
    return s.reshape(n, -1).mean(1)


MUTANTS = collections.OrderedDict([   # name: the one defect it carries
    ("overwrite", "the last term to write d_weights replaces the others"),
    ("perm_opacity", "the opacity's per-ray factor comes back through another permutation"),
    ("perm_depth", "the depth terms' per-ray factors come back through another permutation"),
    ("perm_dist", "the distortion's per-ray factor comes back through another permutation"),
    ("n_for_n_valid", "with a mask on, the depth terms are divided by n where n_valid belongs"),
    ("mask_after_reduction", "the ray weight m is applied to the mean instead of to the rays"),
    ("term_lost_when_compacted", "the distortion's factor is dropped on rays that kept fewer than S"),
    ("ssim_target_plain", "the patch term reads gt where it should read the composited target"),
    ("var_attached_at_zero", "a zero variance weight leaves the variance backward running at VAR_STUCK"),
])
VAR_STUCK = 1e-2
D_WEIGHT_WRITERS = ("var", "dist", "depth", "opacity")


def applies(mut, scene, context):
    masked = context in ("masked", "sky")
    if mut in ("n_for_n_valid", "mask_after_reduction"):
        return masked
    if mut.startswith("perm_"):
        # without ray weights every ray's factor is the same lambda / n (and the opacity term needs an
        # alpha target): a permutation of equal factors is no defect
        return masked
    if mut == "ssim_target_plain":
        return context == "masked"             # composite_target
    if mut == "term_lost_when_compacted":
        return scene == "terminating"
    return True


def step_grads(r, inp, context, on, mut=None):
    """one step on the render r: -> (loss, {name: gradient}).  `on`: the set of terms switched on."""
    dt_ = r.colors.dtype
    C = r.colors.detach().requires_grad_(True)
    w = r.weights.detach().requires_grad_(True)
    gt, z = inp["gt"].to(dt_), inp["z"]
    masked = context in ("masked", "sky")
    m = inp["ray_weight"].to(dt_) if masked else None
    alpha = inp["alpha"].to(dt_) if masked else None
    composite = context == "masked"
    lam = {k: (weights(inp["name"])[k] if k in on else 0.0) for k in TERMS}
    if not masked:
        lam["opacity"] = 0.0                                      # no alpha target, no term
    var, dist, terms, opacity = per_ray(r, w, z)
    if mut == "perm_dist":
        dist = _PermGrad.apply(dist, inp["perm"])
    if mut == "perm_depth":
        terms = _PermGrad.apply(terms, inp["perm"])
    if mut == "perm_opacity":
        opacity = _PermGrad.apply(opacity, inp["perm"])
    if mut == "term_lost_when_compacted":
        full = ((r.idx[:, 1] - r.idx[:, 0]) == S).to(dt_)
        dist = dist * full + (dist * (1.0 - full)).detach()
    # colour (+ variance, + opacity where the target composites): f2n_loss_fwd / f2n_loss_sup_fwd
    target = gt
    if composite:
        target = alpha[:, None] * gt + (1.0 - alpha[:, None]) * r.leaves["bg"].detach().to(dt_)
    on_ray = torch.ones(N, dtype=torch.bool) if m is None else m.ne(0)
    mm = torch.ones(N, dtype=dt_) if m is None else m
    W = mm.sum() if float(mm.sum()) > 0 else torch.ones((), dtype=dt_)
    e = torch.where(on_ray[:, None], C - target, torch.zeros_like(C))
    pieces = collections.OrderedDict()
    pieces["colour"] = (mm * torch.sqrt(e * e + 1e-4).sum(1)).sum() / (3.0 * W)
    vw = lam["var"]
    var_in = var if vw != 0.0 else var.detach()
    pieces["var"] = vw * (mm * torch.sqrt(var_in + 1e-2)).sum() / W
    if mut == "var_attached_at_zero" and vw == 0.0:
        stuck = VAR_STUCK * (mm * torch.sqrt(var + 1e-2)).sum() / W
        pieces["var"] = pieces["var"] + stuck - stuck.detach()
    if lam["opacity"] != 0.0:
        do = torch.where(on_ray, opacity - alpha, torch.zeros_like(opacity))
        pieces["opacity"] = lam["opacity"] * (mm * do * do).sum() / W
    # the regularisers: weighted before their reductions, which keep their divisors
    if lam["dist"] != 0.0:
        if mut == "mask_after_reduction" and m is not None:
            pieces["dist"] = lam["dist"] * dist.mean() * m.mean()
        else:
            pieces["dist"] = lam["dist"] * (dist if m is None else dist * m).mean()
    if any(lam[k] != 0.0 for k in ("empty", "near", "expected")):
        n_valid = float(N) if (mut == "n_for_n_valid" and m is not None) else depth_n_valid(z)
        coef = torch.tensor([lam["empty"], lam["near"], lam["expected"]], dtype=dt_) / n_valid
        if mut == "mask_after_reduction" and m is not None:
            pieces["depth"] = torch.dot(terms.sum(0), coef) * m.mean()
        else:
            pieces["depth"] = torch.dot((terms if m is None else terms * m[:, None]).sum(0), coef)
    if lam["ssim"] != 0.0:
        tgt = gt if mut == "ssim_target_plain" else target
        pw = inp["patch_weight"].to(dt_)
        one_minus = 1.0 - _ssim(C.reshape(N_PATCH, P, P, 3), tgt.detach().reshape(N_PATCH, P, P, 3))
        pieces["ssim"] = lam["ssim"] * (pw * one_minus).sum() / pw.sum()
    loss = sum(pieces.values())
    # what each piece hands to the render's outputs; d_weights has four writers
    d_C = torch.zeros_like(C)
    d_w = collections.OrderedDict()
    for name, v in pieces.items():
        if not v.requires_grad:
            continue
        gC, gw = torch.autograd.grad(v, [C, w], retain_graph=True, allow_unused=True)
        if gC is not None:
            d_C = d_C + gC
        if gw is not None:
            d_w[name] = gw
    if mut == "overwrite" and d_w:
        d_w = {k: v for k, v in d_w.items() if k == list(d_w)[-1]}
    d_weights = sum(d_w.values()) if d_w else torch.zeros_like(w)
    wanted = list(r.params.values()) + list(r.leaves.values())
    grads = torch.autograd.grad([r.colors, r.weights], wanted, [d_C, d_weights], retain_graph=True,
                                allow_unused=True)
    names = list(r.params) + list(r.leaves)
    out = {k: g.detach().clone() for k, g in zip(names, grads) if g is not None}
    if context != "sky":
        out.pop("bg", None)
    return float(loss.detach()), out, {k: float(v.detach()) for k, v in pieces.items()}


STEPS = ("none",) + TERMS + ("all",)


def terms_on(step):
    return set() if step == "none" else set(TERMS) if step == "all" else {step}


def live_terms(context):
    """the terms that exist in a context: the opacity term needs an alpha target"""
    return tuple(t for t in TERMS if t != "opacity" or context in ("masked", "sky"))


# ---- the assertions --------------------------------------------------------------------------------------

def _norm(g):
    return float(g.double().norm())


def shares(grads, key="scene_field.feat_pool"):
    """|D_i| / |g(none)| per term: the precondition"""
    g0 = grads["none"][key].double()
    return {t: _norm(grads[t][key].double() - g0) / _norm(g0) for t in grads if t not in ("none", "all")}


def sum_of_parts(grads):
    """assertion 1 -> {key: residual / ((k + 2) bar max|g|)}; grads: {step: {key: tensor}}"""
    terms = [t for t in grads if t not in ("none", "all")]
    out = {}
    for key in grads["none"]:
        g0 = grads["none"][key].double()
        parts = sum(grads[t][key].double() - g0 for t in terms)
        resid = _norm(grads["all"][key].double() - g0 - parts)
        scale = max(_norm(grads[s][key]) for s in grads)
        out[key] = resid / ((len(terms) + 2) * bar(key) * scale) if scale > 0 else (0.0 if resid == 0 else np.inf)
    return out


def against(grads, ref):
    """assertion 2 -> {(step, key): residual / (bar max|g|)}, D_i for the terms, g itself for 'all'"""
    out = {}
    for step in grads:
        if step == "none":
            continue
        for key in grads["none"]:
            a0, b0 = grads["none"][key].double(), ref["none"][key].double()
            a, b = grads[step][key].double(), ref[step][key].double()
            resid = _norm(a - b) if step == "all" else _norm((a - a0) - (b - b0))
            scale = max(_norm(a), _norm(b), _norm(a0), _norm(b0))
            out[(step, key)] = resid / (bar(key) * scale) if scale > 0 else (0.0 if resid == 0 else np.inf)
    return out


def worst(ratios):
    k = max(ratios, key=ratios.get)
    return k, ratios[k]


# ---- the model's runs, shared ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scene(name):
    bias0, seed = SCENES[name]
    oracle, _, o, d, noise, bg, gt, emb = setup(None, bias0, seed)
    inp = dict(name=name, o=o, d=d, noise=noise, bg=bg, gt=gt, emb=emb, oracle=oracle)
    inp.update(extras(name, noise))
    return inp


@functools.lru_cache(maxsize=None)
def model_render(name, context, dtype):
    inp = scene(name)
    bg = inp["sky_bg"] if context == "sky" else inp["bg"]
    r32 = render32(inp["oracle"], inp["o"], inp["d"], inp["emb"], inp["noise"], bg, context == "pose")
    if dtype == "f32":
        return r32
    return render64(inp["oracle"], inp["o"], inp["d"], inp["emb"], inp["noise"], bg, r32.idx)


@functools.lru_cache(maxsize=None)
def model_step(name, context, dtype, step, mut=None):
    return step_grads(model_render(name, context, dtype), scene(name), context, terms_on(step), mut)


def affected(mut, step):
    """whether a mutant can change a step at all (the others are the unmutated model's, not run again)"""
    on = terms_on(step)
    if mut == "overwrite":
        return step == "all"
    if mut == "var_attached_at_zero":
        return "var" not in on
    touched = dict(perm_opacity={"opacity"}, perm_dist={"dist"}, term_lost_when_compacted={"dist"},
                   perm_depth={"empty", "near", "expected"}, n_for_n_valid={"empty", "near", "expected"},
                   mask_after_reduction={"dist", "empty", "near", "expected"}, ssim_target_plain={"ssim"})
    return bool(on & touched[mut])


def model_grads(name, context, dtype, mut=None):
    """{step: {key: gradient}} over 'none', the live terms and 'all'"""
    steps = ("none",) + live_terms(context) + ("all",)
    return {s: model_step(name, context, dtype, s, mut if mut and affected(mut, s) else None)[1]
            for s in steps}
