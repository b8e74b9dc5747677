"""Model of the learned background (f2n_envmap_fwd / f2n_envmap_bwd / f2n_envmap_grad_apply): the
evaluation order in the header comment of f2-nerf_amd/csrc/kernels/envmap.hip, line by line.

GEOMETRY, in float32 exactly as the kernel (fmaf through tests/mesh_model.fmaf32; every other
operation is one IEEE float32 operation of numpy): axis, face, the two in-face coordinates, the four
texel indices and the four weights.  A test compares nothing of it with a tolerance: the backward's
sums must be the kernel's to the bit, and they are products of these weights.

FORWARD, in float64 on those float32 weights, with a bound counted from the kernel's lines,
u = 2^-24:
    logit = fmaf(w11, T11, fmaf(w01, T01, fmaf(w10, T10, w00*T00)))     4 roundings of partial sums
            that are each at most A = sum |w T| in magnitude (to first order): |d logit| <= 4 u A
    e   = expf(-logit)       the argument carries d logit, expf counts 2 (tests/render_model.py):
                             relative  d logit + 2 u
    den = 1.f + e            one rounding
    bg  = 1.f / den          one rounding
  bg = 1 / (1 + e) has d bg / bg = -(e / (1 + e)) d e / e = -(1 - bg) d e / e, so
    |d bg| <= bg ((1 - bg) (4 u A + 2 u) + 2 u)
  times SLACK for the second-order terms, plus one float32 denormal.

BACKWARD in Python integers: per ray and channel gl = d_bg * (bg * (1 - bg)) in float32 (three
roundings, as the kernel), then per corner q = rint(gl * w * 2^48) with the product exact in float64
and rint rounding half to even, as llrint does.  The sums are Python integers of any size, and the
model asserts that the sum of |q| of every element stays below 2^63, so that no order of the int64
additions can wrap.  (At |d_bg| <= 1e3: gl <= 250, |q| <= 250 * 2^48 < 2^56 -- the cap at 2^62 is out
of reach, and a wrap needs 128 such rays on one texel, all of one sign.)

APPLY: float(acc) is the correctly rounded float64 of a Python integer, ldexp by -48 is exact, and
the cast to float32 rounds to nearest even -- the kernel's two conversions.
"""
import numpy as np

from tests.mesh_model import fmaf32

F32 = np.float32
U = 2.0 ** -24
SHIFT = 48
CAP = 1 << 62
SLACK = 1.0 + 2.0 ** -10
R_MIN, R_MAX = 2, 4096


def texels(R):
    return 6 * R * R if R_MIN <= R <= R_MAX else 0


def special_dirs():
    """float32 [k, 3]: the 6 axes, the 8 cube corners, the 12 edge midpoints (every tie of the axis
    choice), the same with -0.0 in place of 0, and scales 1e-20 and 1e20"""
    axes = [tuple(s * row) for row in np.eye(3) for s in (1.0, -1.0)]
    axes = [tuple(0.0 if c == 0 else c for c in v) for v in axes]          # +0.0 here, -0.0 below
    corners = [(x, y, z) for x in (1.0, -1.0) for y in (1.0, -1.0) for z in (1.0, -1.0)]
    edges = []
    for zero in range(3):
        for p in (1.0, -1.0):
            for q in (1.0, -1.0):
                v = [p, q]
                v.insert(zero, 0.0)
                edges.append(tuple(v))
    base = np.array(axes + corners + edges, dtype=F32)
    neg0 = base.copy()
    neg0[neg0 == 0] = F32(-0.0)
    tilt = np.array([(0.3, -0.7, 0.2), (-0.9, 0.1, 0.4), (0.25, 0.5, -1.0), (1.0, 0.999, -0.5)], dtype=F32)
    # a NaN in a component that is not the largest: the ray is live and the coordinate lands on 0
    odd = np.array([(np.nan, -2.0, 0.5), (0.5, np.nan, 3.0)], dtype=F32)
    return np.concatenate([base, neg0, base * F32(1e-20), base * F32(1e20), tilt * F32(1e-20),
                           tilt * F32(1e20), tilt, odd])


def degenerate_dirs():
    """float32 [k, 3]: rays whose largest |component| is not finite and positive"""
    nan, inf = np.nan, np.inf
    return np.array([(0, 0, 0), (-0.0, 0.0, -0.0), (nan, nan, nan), (inf, 0, 0), (1, -inf, 2),
                     (inf, inf, inf), (nan, 1, inf), (0, nan, 0)], dtype=F32)


def random_dirs(n, seed):
    rng = np.random.RandomState(seed)
    return (rng.randn(n, 3) * np.exp(rng.randn(n, 1))).astype(F32)


def _axis_coord(s, R):
    top = F32(R - 1)
    u = fmaf32(fmaf32(s, F32(0.5), F32(0.5)), F32(R), F32(-0.5))
    with np.errstate(invalid="ignore"):
        u = np.where(u > 0, u, F32(0)).astype(F32)
        u = np.where(u < top, u, top).astype(F32)
    i0 = np.floor(u).astype(np.int64)
    i1 = np.minimum(i0 + 1, R - 1)
    f = (u - i0.astype(F32)).astype(F32)
    return i0, i1, f


def geometry(dirs, R):
    """-> dict(live [n] bool, face [n], idx [n, 4] texel indices in the order 00, 10, 01, 11 (times
    3 plus the channel is the element), w [n, 4] float32).  Degenerate rays: idx 0, weights 0."""
    assert texels(R) > 0
    d = np.asarray(dirs, dtype=F32).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    with np.errstate(invalid="ignore"):
        axis = np.where((ax >= ay) & (ax >= az), 0, np.where(ay >= az, 1, 2))
        comp = np.where(axis == 0, x, np.where(axis == 1, y, z))
        m = np.where(axis == 0, ax, np.where(axis == 1, ay, az))
        live = (m > 0) & (m < np.inf)
        face = 2 * axis + (comp < 0)
    a = np.where(axis == 0, y, x)
    b = np.where(axis == 2, y, z)
    safe = np.where(live, m, F32(1)).astype(F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        s = (np.where(live, a, F32(0)).astype(F32) / safe).astype(F32)
        t = (np.where(live, b, F32(0)).astype(F32) / safe).astype(F32)
    x0, x1, fx = _axis_coord(s, R)
    y0, y1, fy = _axis_coord(t, R)
    gx, gy = (F32(1) - fx).astype(F32), (F32(1) - fy).astype(F32)
    w = np.stack([gx * gy, fx * gy, gx * fy, fx * fy], 1).astype(F32)
    row0, row1 = (face * R + y0) * R, (face * R + y1) * R
    idx = np.stack([row0 + x0, row0 + x1, row1 + x0, row1 + x1], 1)
    idx = np.where(live[:, None], idx, 0)
    w = np.where(live[:, None], w, F32(0)).astype(F32)
    assert idx.min() >= 0 and idx.max() < texels(R)
    return dict(live=live, face=np.where(live, face, 0), idx=idx, w=w, fx=fx, fy=fy)


def forward(dirs, tex, R, geo=None):
    """-> (bg [n, 3] float64, tol [n, 3]): the definition in float64 and the counted bound"""
    geo = geo or geometry(dirs, R)
    T = np.asarray(tex, dtype=F32).reshape(-1, 3).astype(np.float64)
    w = geo["w"].astype(np.float64)
    taps = T[geo["idx"]]                                     # [n, 4, 3]
    logit = (w[:, :, None] * taps).sum(1)
    A = (np.abs(w[:, :, None] * taps)).sum(1)
    bg = 1.0 / (1.0 + np.exp(-logit))
    tol = (bg * ((1.0 - bg) * (4.0 * U * A + 2.0 * U) + 2.0 * U)) * SLACK + 2.0 ** -149
    dead = ~geo["live"]
    bg[dead] = 0.5
    tol[dead] = 0.0
    return bg, tol


def backward(dirs, bg, d_bg, R, geo=None):
    """-> (acc: object array [6*R*R*3] of Python integers, flags).  bg: the forward's float32 output."""
    geo = geo or geometry(dirs, R)
    b = np.asarray(bg, dtype=F32).reshape(-1, 3)
    g = np.asarray(d_bg, dtype=F32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        om = (F32(1) - b).astype(F32)
        ds = (b * om).astype(F32)
        gl = (g * ds).astype(F32)
    gl = np.where(geo["live"][:, None], gl, F32(0))          # a degenerate ray contributes nothing
    flags = 0
    with np.errstate(invalid="ignore"):
        bad = (gl != 0) & ~np.isfinite(gl)
    if bad.any():
        flags |= 1
    gl64 = np.where(bad, 0.0, gl.astype(np.float64))
    v = np.ldexp(gl64[:, None, :] * geo["w"].astype(np.float64)[:, :, None], SHIFT)   # [n, 4, 3], exact
    over = np.abs(v) > float(CAP)
    if over.any():
        flags |= 2
        v = np.where(over, np.copysign(float(CAP), v), v)
    q = np.rint(v).astype(np.int64)                          # |v| <= 2^62: exact
    acc = np.zeros(texels(R) * 3, dtype=object)
    mag = np.zeros(texels(R) * 3, dtype=object)
    elem = geo["idx"][:, :, None] * 3 + np.arange(3)[None, None, :]
    nz = np.nonzero(q)
    for e, val in zip(elem[nz].tolist(), q[nz].tolist()):
        acc[e] += val
        mag[e] += abs(val)
    assert all(int(s) < (1 << 63) for s in mag), "a texel's sum can leave int64"
    return acc, flags


def acc_int64(acc):
    return np.array([int(a) for a in acc], dtype=np.int64)


def apply(acc, d_tex=None):
    """-> float32 [len(acc)]: (d_tex +) (float32) ldexp((float64) acc, -48)"""
    g = np.array([np.ldexp(float(int(a)), -SHIFT) for a in acc], dtype=np.float64).astype(F32)
    if d_tex is None:
        return g
    return (np.asarray(d_tex, dtype=F32).reshape(-1) + g).astype(F32)


def backward_float64(dirs, bg, d_bg, R, geo=None):
    """the gradient of the texture as plain float64 sums (what the fixed point is compared with)"""
    geo = geo or geometry(dirs, R)
    b = np.asarray(bg, dtype=np.float64).reshape(-1, 3)
    gl = np.asarray(d_bg, dtype=np.float64).reshape(-1, 3) * b * (1.0 - b)
    gl = np.where(geo["live"][:, None], gl, 0.0)
    out = np.zeros(texels(R) * 3)
    elem = geo["idx"][:, :, None] * 3 + np.arange(3)[None, None, :]
    np.add.at(out, elem.reshape(-1), (gl[:, None, :] * geo["w"].astype(np.float64)[:, :, None]).reshape(-1))
    return out


# ---- the fit of tests/test_gpu_envmap_routes.py (f) -------------------------------------------------

FIT_R, FIT_RAYS, FIT_STEPS, FIT_LR, FIT_SEED = 8, 1024, 200, 0.05, 77
FIT_BETAS, FIT_EPS = (0.9, 0.99), 1e-15


def fit_hidden_texture():
    return (np.random.RandomState(FIT_SEED).randn(6, FIT_R, FIT_R, 3) * 1.5).astype(F32)


def fit(dirs, A, T, steps=FIT_STEPS, lr=FIT_LR):
    """The optimisation of test (f) on the model: colours C = A + T bg(texture) with the field's own
    colours A [n, 3] and the transmittance behind it T [n], the target the same render of the hidden
    texture, loss = mean (C - gt)^2, Adam (torch's update, float32 state) on the texture alone from
    zeros; the forward in float64 rounded to float32, the backward in integers.
    -> (final mean |C - gt|, initial mean |C - gt|)"""
    R = FIT_R
    geo = geometry(dirs, R)
    A = np.asarray(A, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64).reshape(-1, 1)
    gt = (A + T * forward(dirs, fit_hidden_texture(), R, geo)[0]).astype(F32).astype(np.float64)
    tex = np.zeros(texels(R) * 3, dtype=F32)
    m = np.zeros_like(tex)
    v = np.zeros_like(tex)
    b1, b2 = FIT_BETAS
    errs = []
    n_values = A.size
    for step in range(1, steps + 2):
        bg = forward(dirs, tex, R, geo)[0].astype(F32)
        C = (A + T * bg.astype(np.float64)).astype(F32).astype(np.float64)
        errs.append(float(np.abs(C - gt).mean()))
        if step > steps:
            break
        d_C = (2.0 * (C - gt) / n_values).astype(F32)
        d_bg = (T * d_C.astype(np.float64)).astype(F32)
        acc, flags = backward(dirs, bg, d_bg, R, geo)
        assert flags == 0
        g = apply(acc)
        m = (b1 * m + (1.0 - b1) * g).astype(F32)
        v = (b2 * v + (1.0 - b2) * g * g).astype(F32)
        denom = (np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + FIT_EPS).astype(F32)
        tex = (tex - (lr / (1.0 - b1 ** step)) * (m / denom)).astype(F32)
    return errs[-1], errs[0]


# the final mean absolute error of fit(*fit_scene_cpu()), as run on the CPU (the initial one, with the
# texture at zero, is 0.1022); tests/test_envmap_model_cpu.py runs it again
FIT_MODEL_MAE = 0.0014091344152499612


def fit_scene_cpu():
    """The scene of test (f) from the CPU oracle: thin field (bias 1), FIT_RAYS rays, and the field's
    colours A (the render with bg = 0) and transmittance T = render(bg = 1) - A per ray.
    -> (dirs, A, T) as numpy arrays"""
    import torch

    from oracle import ref_render as RR

    oracle, o, d, emb = fit_scene(None)[:4]
    with torch.no_grad():
        zero = oracle.render(o, d, emb, RR.VALIDATE, None, torch.zeros(FIT_RAYS, 3)).colors
        one = oracle.render(o, d, emb, RR.VALIDATE, None, torch.ones(FIT_RAYS, 3)).colors
    return d.numpy(), zero.numpy(), (one - zero).mean(1).numpy()


def fit_scene(host):
    """(oracle, o, d, emb, hr): the field of tests/test_gpu_supervised_step.py's thin scene (L = 4,
    F = 2, T = 2^12, 128 samples, bias 1) with FIT_RAYS rays; hr is the host Renderer with the
    oracle's parameters, or None without a host module"""
    import torch

    from oracle import ref_render as RR

    S, E = 128, 7
    g = torch.Generator().manual_seed(FIT_SEED)
    torch.manual_seed(FIT_SEED)
    oracle = RR.Renderer(E, L=4, F=2, log2_T=12, S=S, step=4.0 / S, gen=g, feat_init="trained")
    with torch.no_grad():
        oracle.scene_field.mlp.bias[0] = 1.0
    o = torch.randn(FIT_RAYS, 3, generator=g) * 0.25
    d = torch.randn(FIT_RAYS, 3, generator=g)
    emb = torch.randint(0, E, (FIT_RAYS,), generator=g).to(torch.int32)
    hr = None
    if host is not None:
        from tests.test_gpu_render import _copy_params

        hr = host.Renderer(E, n_levels=4, n_channels=2, log2_table=12, max_samples=S, step=4.0 / S)
        _copy_params(oracle, hr)
    return oracle, o, d, emb, hr
