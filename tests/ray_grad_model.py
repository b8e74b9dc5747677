"""Inputs, a float64 restatement and per-element rounding bounds for the gradient of the hash encoding
with respect to the rays: f2n_hash_rays_grad (pose_grad.hip, the fused route) and the op-by-op route
f2n_hash_bwd with a point gradient + f2n_contract_bwd (hash_grid.hip), with f2n_contract_fwd beside
them.  No tests in here: tests/test_ray_grad_model_cpu.py checks the restatement and the bounds on the
CPU, tests/test_gpu_ray_grad_f64.py holds the HIP kernels to them.

Cells.  The eight table rows of a (sample, level) come from the float32 chain the kernels run --
contract_point, fmaf(x, mul, bias), floorf, the hash -- through oracle.kernels.hash_fwd(want_idx=True),
which tests/test_gpu_ops.py::test_hash_fwd_parity holds bit-exact to the device.  The contraction in
front of it is float32 numpy; it need not match the device's bit for bit, because a case holds no
sample whose cell could depend on it (below).

Terms (quirk Q5, pose_grad.hip:78-97, hash_grid.hip:244-279).  gk = f16(f32(g * grad_scale)),
term = f16(f32(f32(feature * mul) * gk)), added with the sign of the corner bit of each axis (d & 4,
d & 2, d & 1).  A term is an f16 value and the sums of at most 32 * 64 of them are exact in float64.

Outputs.  level_f32[n, L, 3]: the float32 sum of one level in the kernels' order (corner outer,
channel inner) times 1 / grad_scale -- what both kernels must return, as numbers, when only that level
carries a gradient and the point lies inside the unit ball.  G[n, 3]: the float64 sum of all terms over
grad_scale, A: the same of their magnitudes.  dp: the contraction's Jacobian-vector product in float64
at the float32 point, identity for |p| <= 1, a G + (a'/n)(p.G) p outside with a = 2/n - 1/n^2, NaN at
|p| == 0.  x: the contracted point.  Per ray d_o = sum dp, m = sum t dp, d_d = (m - n (n.m)) / |d|.

Bound, first order, per element, u = 2^-24, gamma(k) = k u / (1 - k u), propagated through the
absolute-value version of each formula.  Scalar expressions are followed operation by operation (the
helpers _add .. _sqrt: the propagated error plus u |result| per rounding; division and square root are
correctly rounded in the build, no fast-math flag); sums take gamma(k) of their absolute terms with k
the roundings on the longest path of one term.  The counts, each with the lines it was taken from:

  level sum      K_LEVEL(F) = 8 F - 1   pose_grad.hip:85-98 / hash_grid.hip:266-280: 8 F additions per
                                        axis, the first onto 0; 1 / grad_scale is a power of two
  level adds     K_LEVELS(L) = L - 1    pose_grad.hip:99-101: gx += in level order, the first onto 0;
                                        hash_grid.hip:281-283: L atomics in any order onto the zeroed
                                        buffer, the first of them onto 0
  norm           4: x x, fmaf, fmaf, sqrtf      hash_grid.hiph:44, pose_grad.hip:104-105, hash_grid.hip:409-410
  contract_fwd   + 4: 1 / n, 2 -, s x, / n      hash_grid.hiph:51-54
  Jacobian       1 / n; a: 2 -, x; a'/n: 2 inv (exact), - 2, x inv three times; p.G: x, fmaf, fmaf;
                 c = a'/n x p.G; dp = fmaf(c, p, a G): 2       pose_grad.hip:113-120, hash_grid.hip:418-425
  d_o            K_RAY_O(len) = ceil(len / 64) - 1 + 6         pose_grad.hip:123-125 (one add per stride
                 into the lane's partial, the first onto 0), :130-132 wave_sum: common.hiph:33-42, four
                 row_shr steps and two row broadcasts on the way to lane 63
  m              K_RAY_M(len) = ceil(len / 64) + 6             pose_grad.hip:126-128: fmaf, the first one
                 rounds too; :133-135
  epilogue       |d|: 4; n = d / |d|; n.m: x, fmaf, fmaf; n (n.m); m -; / |d|        pose_grad.hip:138-147

Where the float32 norm can fall on the other side of 1 than the float64 one (| |p| - 1 | within twice
the norm's bound) either branch is right: the bound there is the larger of the two plus their
difference.

Ambiguous cells.  A sample is ambiguous when for some (level, axis) the float64 value of x mul + bias
lies within twice its bound, E_x mul + u |x mul + bias|, of an integer: a correct kernel may then sit
in the neighbouring cell, and Q5's gradient jumps there.  build_case redraws such samples (cases of
fixed points walk the field's seed instead) until none is left: the cap is 0.  No term may be
non-finite.

Bar: |got - f64| <= BAR * E with BAR = 2 for the second-order terms the rule drops; where E = 0 the
value must be equal as a number; where the model is NaN the kernel's value must be NaN.  Nothing here
was measured on a kernel.
"""
import collections
import math

import numpy as np
import torch

from oracle import kernels as K
from oracle.ref_render import _is_prime

U = 2.0 ** -24
BAR = 2.0
WAVE = 64
WAVES_PER_BLOCK = 4      # F2N_WAVES_PER_BLOCK (common.hiph:13)
SCAN_DEPTH = 6           # wave_sum (common.hiph:33-42, :78)
GRAD_SCALE = 128.0
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 200, 1024)
RADII = (1e-3, 0.5, 1.5, 10.0, 1e3, 1e6)
D_NORMS = (1e-3, 1.0, 2.0, 1e3)


def gamma(k):
    return k * U / (1.0 - k * U)


def K_LEVEL(F):
    return 8 * F - 1


def K_LEVELS(L):
    return L - 1


def _strides(length):
    return (np.asarray(length) + WAVE - 1) // WAVE


def K_RAY_O(length):
    return np.maximum(_strides(length) - 1, 0) + SCAN_DEPTH


def K_RAY_M(length):
    return _strides(length) + SCAN_DEPTH


# ---- value-and-bound arithmetic: (v, e), one rounding u |v| per float32 operation ---------------------

def _v(x):
    x = np.asarray(x, dtype=np.float64)
    return x, np.zeros_like(x)


def _rnd(v, e):
    return v, e + U * np.abs(v)


def _add(a, b):
    return _rnd(a[0] + b[0], a[1] + b[1])


def _sub(a, b):
    return _rnd(a[0] - b[0], a[1] + b[1])


def _mul(a, b):
    return _rnd(a[0] * b[0], a[1] * np.abs(b[0]) + np.abs(a[0]) * b[1])


def _fma(a, b, c):
    return _rnd(a[0] * b[0] + c[0], a[1] * np.abs(b[0]) + np.abs(a[0]) * b[1] + c[1])


def _div(a, b):
    v = a[0] / b[0]
    return _rnd(v, (a[1] + np.abs(v) * b[1]) / np.abs(b[0]))


def _sqrt(a):
    v = np.sqrt(a[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(v > 0, a[1] / (2.0 * v), 0.0)
    return _rnd(v, e)


def _twice(a):            # 2.f * x: exact
    return 2.0 * a[0], 2.0 * a[1]


def _norm(cols):
    """sqrtf(fmaf(z, z, fmaf(y, y, x * x))) of three (v, e) columns"""
    x, y, z = cols
    return _sqrt(_fma(z, z, _fma(y, y, _mul(x, x))))


def _cols(p):
    p = np.asarray(p, dtype=np.float64)
    return [_v(p[:, a]) for a in range(3)]


def _either(inside, near, v_in, e_in, v_out, e_out):
    """the float64 branch's value; where the float32 norm may fall on the other side, both bounds"""
    v = np.where(inside, v_in, v_out)
    e = np.where(inside, e_in, e_out)
    return v, np.where(near, np.maximum(e_in, e_out) + np.abs(v_in - v_out), e)


# ---- the contraction ------------------------------------------------------------------------------------

def contract_f32(pts):
    """contract_point in float32 numpy -> float32 [n, 3] (NaN rows at |p| == 0)"""
    p = pts.numpy().astype(np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    n = np.sqrt(z * z + (y * y + x * x))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.float32(2.0) - np.float32(1.0) / n
        out = (s[:, None] * p) / n[:, None]
    out = np.where((n <= 1)[:, None], p, out)
    out[n == 0] = np.nan
    return out.astype(np.float32)


def contract_fwd_model(pts):
    """-> x [n, 3] float64, E [n, 3], zero [n] (rows with |p| == 0: x is NaN there)"""
    cols = _cols(pts.numpy())
    n = _norm(cols)
    zero = n[0] == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        s = _sub(_v(2.0), _div(_v(1.0), n))
        inside, near = n[0] <= 1.0, np.abs(n[0] - 1.0) <= 2.0 * n[1]
        xs, es = [], []
        for c in cols:
            v_out, e_out = _div(_mul(s, c), n)
            v, e = _either(inside, near, c[0], 0.0 * c[0], v_out, e_out)
            xs.append(np.where(zero, np.nan, v))
            es.append(np.where(zero, np.nan, e))
    return np.stack(xs, 1), np.stack(es, 1), zero


def contract_bwd_model(pts, G, E_G, mut=None):
    """dp = J^T G at the float32 point -> dp [n, 3], E [n, 3]; NaN rows at |p| == 0.
    mut: 'no_pg_term' drops (a'/n)(p.G) p, 'a_no_sq' takes a = 2 / n, 'jac_101' evaluates the Jacobian
    at 1.01 p."""
    cols = _cols(pts.numpy())
    g = [(np.asarray(G[:, a], dtype=np.float64), np.asarray(E_G[:, a], dtype=np.float64)) for a in range(3)]
    n = _norm(cols)
    zero = n[0] == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = _div(_v(1.0), n)
        a = _mul(_sub(_v(2.0), inv), inv)
        da = _mul(_mul(_mul(_sub(_twice(inv), _v(2.0)), inv), inv), inv)
        pg = _fma(cols[2], g[2], _fma(cols[1], g[1], _mul(cols[0], g[0])))
        cc = _mul(da, pg)
        # the values from the closed form the bound is not taken from
        nn, pv = n[0], [c[0] for c in cols]
        if mut == "jac_101":
            nn, pv = 1.01 * nn, [1.01 * v for v in pv]
        a_v = 2.0 / nn - (0.0 if mut == "a_no_sq" else 1.0 / (nn * nn))
        da_v = 0.0 * nn if mut == "no_pg_term" else (-2.0 / nn ** 2 + 2.0 / nn ** 3) / nn
        pg_v = sum(pv[i] * g[i][0] for i in range(3))
        inside, near = n[0] <= 1.0, np.abs(n[0] - 1.0) <= 2.0 * n[1]
        out, err = [], []
        for i in range(3):
            e_out = _fma(cc, cols[i], _mul(a, g[i]))[1]
            v_out = a_v * g[i][0] + da_v * pg_v * pv[i]
            v, e = _either(inside, near, g[i][0], g[i][1], v_out, e_out)
            out.append(np.where(zero, np.nan, v))
            err.append(np.where(zero, np.nan, e))
    return np.stack(out, 1), np.stack(err, 1)


# ---- fields ---------------------------------------------------------------------------------------------

FIELDS = collections.OrderedDict([     # name: (L, F, T, disjoint)
    ("ref", (16, 2, 1 << 19, False)),  # the reference's: overlapping level windows
    ("f8", (16, 8, 1 << 12, True)),
    ("l32", (32, 4, 1 << 12, True)),
    ("np2", (16, 1, 5000, False)),     # overlapping, T no power of two
    ("l1", (1, 2, 1000, True)),
])


def make_field(name, seed):
    """tests/test_gpu_pose_grad.py::_field with the shapes of FIELDS"""
    L, F, T, disjoint = FIELDS[name]
    g = torch.Generator().manual_seed(seed)
    stride = T * F if disjoint else T
    numel = max(T * L * F, stride * (L - 1) + T * F)
    table = torch.randn(numel, generator=g) * 0.1
    primes = []
    while len(primes) < 3 * L:
        v = int(torch.randint(1 << 28, 1 << 30, (1,), generator=g))
        if _is_prime(v):
            primes.append(v)
    return dict(name=name, L=L, F=F, T=T, stride=stride, numel=numel, table16=K.cast_f16(table),
                primes=torch.tensor(primes, dtype=torch.int32).reshape(L, 3),
                bias=torch.rand(L, 3, generator=g) * 1000.0 + 100.0, mul=K.level_mul(L))


def corner_rows(fld, x32):
    """table rows [n, L, 8] (int64) of float32 points through the oracle's float32 chain"""
    _, idx = K.hash_fwd(torch.from_numpy(np.ascontiguousarray(x32)), fld["table16"], fld["primes"],
                        fld["bias"], fld["mul"], fld["L"], fld["F"], fld["T"], fld["stride"], want_idx=True)
    return idx.numpy().astype(np.int64) & 0xFFFFFFFF


_SIGN = np.array([[1.0 if d & bit else -1.0 for bit in (4, 2, 1)] for d in range(8)])


def level_sums(fld, x32, g, mut=None, scale=GRAD_SCALE):
    """Q5 per level at the contracted float32 points x32 [n, 3] (finite) with the gradient g [n, L F]
    -> G [n, L, 3] float64, A [n, L], f32 [n, L, 3] float32, terms finite, share of subnormal terms.
    mut: ('flip', l, d, axis), ('no_chan', k), ('base_TF',), ('chan_098',) channel F - 1 of the finest
    level times 0.98."""
    L, F, T, stride = fld["L"], fld["F"], fld["T"], fld["stride"]
    n = x32.shape[0]
    rows = corner_rows(fld, x32)
    tab = fld["table16"].numpy().view(np.float16)
    mul = fld["mul"].numpy().astype(np.float32)
    with np.errstate(over="ignore"):
        gk = (g.numpy().astype(np.float32) * np.float32(scale)).astype(np.float16).astype(np.float32)
    gk = gk.reshape(n, L, F)
    Gl, Al = np.zeros((n, L, 3)), np.zeros((n, L))
    f32 = np.zeros((n, L, 3), dtype=np.float32)
    finite, subnormal, count = True, 0, 0
    for l in range(L):
        base = T * F * l if mut == ("base_TF",) else stride * l
        feat = tab[base + rows[:, l, :, None] * F + np.arange(F)].astype(np.float32)      # [n, 8, F]
        with np.errstate(over="ignore", invalid="ignore"):
            term = ((feat * mul[l]) * gk[:, l, None, :]).astype(np.float16)
        finite = finite and bool(np.isfinite(term).all())
        mag = np.abs(term.astype(np.float64))
        subnormal += int(((mag > 0) & (mag < 2.0 ** -14)).sum())
        count += int((mag > 0).sum())
        sign = _SIGN.copy()
        if mut is not None and mut[0] == "flip" and mut[1] == l:
            sign[mut[2], mut[3]] *= -1.0
        if mut is not None and mut[0] == "no_chan":
            term[:, :, mut[1]] = 0
        t64 = term.astype(np.float64)
        if mut == ("chan_098",) and l == L - 1:
            t64[:, :, F - 1] *= 0.98
        Gl[:, l] = np.einsum("ndk,da->na", t64, sign) / scale
        Al[:, l] = np.abs(t64).sum((1, 2)) / scale
        acc = np.zeros((n, 3), dtype=np.float32)
        t32, s32 = term.astype(np.float32), sign.astype(np.float32)
        for d in range(8):
            for k in range(F):
                acc = acc + t32[:, d, k, None] * s32[d]
        f32[:, l] = acc * np.float32(1.0 / scale)
    return dict(G=Gl, A=Al, f32=f32, finite=finite, subnormal=subnormal / max(count, 1))


def point_grad(fld, x32, g, mut=None, lev=None):
    """all levels -> G [n, 3], A [n, 3], E [n, 3] (the point gradient of either route), the levels
    (`lev`: those of the unchanged model, reused where `mut` leaves them alone)"""
    if isinstance(mut, tuple) and mut[0] != "no_level":
        lev = level_sums(fld, x32, g, mut)
    elif lev is None:
        lev = level_sums(fld, x32, g)
    Gl = lev["G"]
    if isinstance(mut, tuple) and mut[0] == "no_level":
        Gl = Gl.copy()
        Gl[:, mut[1]] = 0.0
    G = Gl.sum(1)
    A = np.repeat(lev["A"].sum(1)[:, None], 3, 1)
    E = (gamma(K_LEVEL(fld["F"])) + gamma(K_LEVELS(fld["L"]))) * A
    return G, A, E, lev


# ---- per ray --------------------------------------------------------------------------------------------

def ray_sums(bounds, t, dp, E_dp, rays_d, mut=None):
    """-> d_o, E_o, d_d, E_d [n_rays, 3].  mut: 'lose_127', 'lose_last', 't_next', 't_102' (t times 1.02), 'no_proj', 'no_inv_d'."""
    b = bounds.numpy().astype(np.int64)
    n_rays, n = b.shape[0], dp.shape[0]
    length = b[:, 1] - b[:, 0]
    ray = np.repeat(np.arange(n_rays), length)
    tt = t.numpy().astype(np.float64)
    live = np.ones(n)
    if mut == "lose_127":
        live[b[length > 127, 0] + 127] = 0.0
    if mut == "lose_last":
        live[b[length > 0, 1] - 1] = 0.0
    if mut == "t_next":
        tt = np.roll(tt, -1)
    if mut == "t_102":
        tt = 1.02 * tt

    def per_ray(v):      # [n, 3] -> [n_rays, 3]; a NaN sample makes its own ray NaN, no other
        out = np.zeros((n_rays, 3))
        np.add.at(out, ray, v)
        return out

    lost = dp * live[:, None]
    d_o, A_o, Ein_o = per_ray(lost), per_ray(np.abs(dp)), per_ray(E_dp)
    tm = tt[:, None] * lost
    m, A_m, Ein_m = per_ray(tm), per_ray(np.abs(tt[:, None] * dp)), per_ray(np.abs(tt)[:, None] * E_dp)
    E_o = Ein_o + gamma(K_RAY_O(length))[:, None] * A_o
    E_m = Ein_m + gamma(K_RAY_M(length))[:, None] * A_m
    q = _cols(rays_d.numpy())
    dn = _norm(q)
    nh = [_div(c, dn) for c in q]
    mm = [(m[:, a], E_m[:, a]) for a in range(3)]
    nm = _fma(nh[2], mm[2], _fma(nh[1], mm[1], _mul(nh[0], mm[0])))
    E_d = np.stack([_div(_sub(mm[a], _mul(nh[a], nm)), dn)[1] for a in range(3)], 1)
    nv = np.stack([c[0] for c in q], 1) / dn[0][:, None]
    proj = 0.0 if mut == "no_proj" else (nv * m).sum(1, keepdims=True) * nv
    d_d = (m - proj) / (1.0 if mut == "no_inv_d" else dn[0][:, None])
    return d_o, E_o, d_d, E_d


# ---- the whole chain ------------------------------------------------------------------------------------

Inputs = collections.namedtuple("Inputs", "fld pts t bounds rays_d g")


def ambiguous(fld, pts):
    """[n] bool: some (level, axis) of the sample lies within twice its position bound of a cell face"""
    x, E_x, zero = contract_fwd_model(pts)
    mul = fld["mul"].numpy().astype(np.float64)[None, :, None]
    bias = fld["bias"].numpy().astype(np.float64)[None]
    with np.errstate(invalid="ignore"):
        pos = x[:, None, :] * mul + bias
        E_pos = E_x[:, None, :] * mul + U * np.abs(pos)
        amb = (np.abs(pos - np.rint(pos)) <= 2.0 * E_pos).any((1, 2))
    return amb & ~zero


def model(inp, mut=None, base=None):
    """-> dict of float64 values (x, G, dp, d_o, d_d, level_f32), `E` per output, A, flags.
    mut: one change of tests/test_ray_grad_model_cpu.py::test_bound_rejects, applied to the values only
    (base: the unchanged model of the same inputs, whose level sums are reused)."""
    fld = inp.fld
    x, E_x, zero = contract_fwd_model(inp.pts)
    x32 = contract_f32(inp.pts)
    x32[zero] = 0.0          # any finite cell: the sample's gradient is NaN whatever it reads
    G, A, E_G, lev = point_grad(fld, x32, inp.g, mut, None if base is None else base["lev"])
    dp, E_dp = contract_bwd_model(inp.pts, G, E_G, mut)
    d_o, E_o, d_d, E_d = ray_sums(inp.bounds, inp.t, dp, E_dp, inp.rays_d, mut)
    return dict(x=x, x32=x32, zero=zero, G=G, A=A, dp=dp, d_o=d_o, d_d=d_d, level_f32=lev["f32"], lev=lev,
                finite=lev["finite"], subnormal=lev["subnormal"],
                E=dict(x=E_x, G=E_G, dp=E_dp, d_o=E_o, d_d=E_d))


def ratio(got, ref, E):
    """|got - ref| / E per element with 0 / 0 = 0, x / 0 = inf; where ref is NaN: 0 if got is NaN too,
    inf otherwise.  got: tensor or array."""
    got = np.asarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
    ref, E = np.asarray(ref, dtype=np.float64), np.asarray(E, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(got - ref)
        r = err / E
    r[(err == 0) & (E == 0)] = 0.0
    nan = np.isnan(ref)
    r[nan] = np.where(np.isnan(got[nan]), 0.0, np.inf)
    r[~nan & np.isnan(got)] = np.inf
    return r


# ---- cases ----------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "layer field tag n_rays")


def cases():
    """Every case tests/test_gpu_ray_grad_f64.py runs.  layer: 'level' single-sample rays inside the
    unit ball (one level at a time, exact), 'points' single-sample rays at fixed radii, 'hot' one live
    sample per ray, 'dense' every sample live, 'count' a few dense rays around the workgroup's four."""
    out = [Case("level", f, "", 500) for f in FIELDS]
    out.append(Case("level", "ref", "subnormal", 500))
    out.append(Case("level", "f8", "rows", 500))
    out += [Case("points", f, "", 0) for f in FIELDS]
    out += [Case("hot", f, "", 0) for f in ("ref", "f8", "np2")]
    out += [Case("dense", f, "", 0) for f in FIELDS]
    out += [Case("count", "l32", "", k) for k in (WAVES_PER_BLOCK - 1, WAVES_PER_BLOCK, WAVES_PER_BLOCK + 1, 1)]
    return out


def case_id(c):
    return "-".join(str(v) for v in (c.layer, c.field, c.tag, c.n_rays or "") if v != "")


def _unit(g, n):
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return d / d.norm(dim=1, keepdim=True)


def _ball(g, n):
    """raw points inside the unit ball, |p| <= 0.99"""
    r = torch.rand(n, 1, generator=g, dtype=torch.float64) ** (1.0 / 3.0) * 0.99
    return (_unit(g, n) * r).float().contiguous()


def _anywhere(g, n):
    """raw points with |p| log-uniform in [0.05, 20]: a third inside the unit ball"""
    r = torch.exp(torch.rand(n, 1, generator=g, dtype=torch.float64) * math.log(400.0) + math.log(0.05))
    return (_unit(g, n) * r).float().contiguous()


def _rays_d(g, n_rays):
    """directions with |d| in D_NORMS in turn, every fifth along an axis"""
    d = _unit(g, n_rays)
    for r in range(0, n_rays, 5):
        d[r] = 0.0
        d[r, (r // 5) % 3] = -1.0 if (r // 5) % 2 else 1.0
    scale = torch.tensor([D_NORMS[r % len(D_NORMS)] for r in range(n_rays)], dtype=torch.float64)
    return (d * scale[:, None]).float().contiguous()


def _bounds(lengths):
    lens = torch.tensor(lengths, dtype=torch.int64)
    end = torch.cumsum(lens, 0)
    return torch.stack([end - lens, end], 1).to(torch.int32).contiguous()


def fixed_points():
    """-> (points [n, 3] float32, index of the |p| == 0 point).  |p| == 1 on an axis, the float32
    neighbours of 1 on an axis and spread over a diagonal, the radii RADII along an axis, a diagonal and
    two oblique directions; the zero point sits second in the second workgroup's four rays."""
    up, down = np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0))
    rows = [[1, 0, 0], [0, -1, 0], [0, 0, 1]]
    for v in (up, down):
        rows += [[float(v), 0, 0], [0, 0, -float(v)]]
        rows.append([float(v) / math.sqrt(3.0)] * 3)
        rows.append([-float(v) / math.sqrt(3.0), float(v) / math.sqrt(3.0), float(v) / math.sqrt(3.0)])
    dirs = [[0, 1, 0], [1 / math.sqrt(3.0)] * 3, [0.6, -0.64, 0.48], [-0.28, 0.0, 0.96]]
    for r in RADII:
        rows += [[r * c for c in d] for d in dirs]
    rows.insert(5, [0, 0, 0])
    return torch.tensor(rows, dtype=torch.float64).float().contiguous(), 5


def _hot_lengths():
    """one ray per (length, hot position), empty rays in between, an empty first and last ray
    -> lengths, hot sample index within its ray (-1: empty)"""
    lengths, hot = [0], [-1]
    for n in LENGTHS:
        for pos in sorted({p for p in (0, 1, 62, 63, 64, 65, n - 2, n - 1) if 0 <= p < n}):
            lengths += [n, 0]
            hot += [pos, -1]
    return lengths, hot


def build_case(c):
    """-> (Inputs, model dict, share of samples redrawn).  Fixed seeds; ambiguous samples are redrawn
    (fixed points: the field's seed is walked) until the case holds none."""
    L, F, T, _ = FIELDS[c.field]
    seed = 1000 * list(FIELDS).index(c.field) + 97 * len(c.layer) + len(c.tag) + 13 * c.n_rays
    g = torch.Generator().manual_seed(seed)
    fld = make_field(c.field, seed)
    n_fixed = 0
    if c.layer == "level":
        lengths = [1] * c.n_rays
        draw = _ball
    elif c.layer == "points":
        fixed, _ = fixed_points()
        n_fixed = fixed.shape[0]
        lengths = [1] * (n_fixed + 100)
        draw = _anywhere
    elif c.layer == "hot":
        lengths, hot = _hot_lengths()
        draw = _anywhere
    elif c.layer == "dense":
        lengths = [0] + [v for n in LENGTHS for v in (n, 0)]
        draw = _anywhere
    else:
        lengths = [(65, 0, 129, 1, 64)[r % 5] for r in range(c.n_rays)]
        draw = _anywhere
    bounds = _bounds(lengths)
    n = int(bounds[-1, 1])
    pts = draw(g, n)
    if c.tag == "rows":      # points with a corner in row 0 and points with one in row T - 1
        pool = _ball(g, 40000)
        pool = pool[torch.from_numpy(~ambiguous(fld, pool))]
        rows = corner_rows(fld, pool.numpy())
        first, last = (rows == 0).any((1, 2)), (rows == T - 1).any((1, 2))
        pick = np.concatenate([np.nonzero(first)[0][: n // 2], np.nonzero(last)[0][: n // 2]])
        assert pick.shape[0] == n, "too few points with a corner at either end of a level"
        pts = pool[torch.from_numpy(pick)].contiguous()
    redrawn = 0
    if n_fixed:
        pts[:n_fixed] = fixed
        for bump in range(1, 200):
            if not ambiguous(fld, pts[:n_fixed]).any():
                break
            fld = make_field(c.field, seed + 100000 * bump)
        else:
            raise AssertionError("no field without an ambiguous fixed point: " + case_id(c))
    for _ in range(200):
        amb = ambiguous(fld, pts)
        if not amb.any():
            break
        assert not amb[:n_fixed].any()
        k = int(amb.sum())
        redrawn += k
        pts[torch.from_numpy(amb)] = draw(g, k)
    else:
        raise AssertionError("ambiguous samples left: " + case_id(c))
    t = (torch.rand(n, generator=g) * 3.0 + 0.01).contiguous()       # drawn independently of pts
    rays_d = _rays_d(g, bounds.shape[0])
    std = 2e-6 if c.tag == "subnormal" else 5e-3
    grad = torch.randn(n, L * F, generator=g) * std
    if c.layer == "hot":
        live = torch.zeros(n, dtype=torch.bool)
        for r, pos in enumerate(hot):
            if pos >= 0:
                live[int(bounds[r, 0]) + pos] = True
        grad[~live] = 0.0
    inp = Inputs(fld, pts.contiguous(), t, bounds, rays_d, grad.contiguous())
    m = model(inp)
    m["ambiguous"] = int(ambiguous(fld, pts).sum())
    return inp, m, redrawn / max(n, 1)
