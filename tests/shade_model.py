"""Inputs, a float64 restatement and per-element rounding bounds for the per-sample network kernels
(f2n_shade_fwd, f2n_shade_bwd, f2n_shade_fwd_rays, f2n_shade_bwd_rays).  No tests in here:
tests/test_shade_model_cpu.py checks the restatement and the bounds on the CPU, tests/
test_gpu_shade_f64.py holds every route of the HIP kernels to them.

Network (shade.hip): h = enc w_h^T + b_h; logit = h[0]; X = [1, h[1..15]] (+ emb[img]) ++ SH16(dir);
pre = X w1^T + b1; o = relu(pre) w2^T + b2; rgb = (1 + 2 eps) sigmoid(o) - eps.  The constants of
sh_basis.hiph, eps = 1e-3f and 1.f + 2.f * eps enter as the float32 values the kernels hold: they are
part of the definition.  Everything else is float64, gradients in closed form.

Bound, first order, per element, u = 2^-24, gamma(k) = k u / (1 - k u).  For y = x W (+ b):
    E_y = E_x |W| + gamma(k) (|x| |W| + |b|)
with k the most roundings one output element sees in any kernel form that computes it: 1 per fmaf,
1 per added bias or embedding row, and for a matrix-core product (v_mfma_f32_16x16x4_f32: the code
does not state how its four products are ordered or fused) T + 1 for T terms onto a bias, T onto
zero: one rounding of the term's own product and one per addition after it, which holds for an
unfused multiply-add in any order and for a fused chain.  (Two per term, the first count taken, holds
as well but let two of the changes of test_shade_model_cpu.py::test_bound_rejects through at every
shape -- d_enc in f16 at C >= 32 and kY31 -- and was tightened to the count above from the code.)
The counts, each with the line it was taken from:

  head    h, logit        K_HEAD(C) = C + 1     shade_mfma.hip:370-376 / :973-979: C / 4 products of
                          4 terms onto b_h.  (shade.hip:56-58, :245-253: C fmaf onto b_h, = C.)
  embed   X[i] += emb[i]  K_EMBED = 1           shade.hip:66, :262; shade_mfma.hip:422, :1011
  SH      X[16..31]       per expression, sh16  sh_basis.hiph:49-69, built with -ffp-contract=off
  hidden  pre             K_PRE = 32 + 1        shade_mfma.hip:459-470, :1047-1056: 8 products of 4
                          terms onto b1; the ray-uniform forms :436-450, :1035-1045 add the same 32
                          terms, the SH half first.  (shade.hip:71-73, :287-296: 32 fmaf, = 32.)
  output  o               K_OUT = 64 + 1        shade_mfma.hip:1027-1072: 16 products of 4 terms onto
                          b2.  (shade.hip:78-80, :299-302: 64 fmaf; the backward's vector form,
                          shade_mfma.hip:483-510: 16 fmaf, a 4-term product onto 0, + b2 = 21.)
  rgb                     K_RGB = 6             shade.hip:106, shade_mfma.hip:1078: expf (2), +, /, the
                          rounding of the constant 1 + 2 eps, -; each times u (|rgb| + eps).  expf is
                          counted as 2 ulp: the ROCm installation at hand states no error for it.
  sigmoid' (backward)     see _sigmoid_prime    shade.hip:310-312, shade_mfma.hip:511-513
  d_hid                   K_DHID = 3            shade.hip:339-341, shade_mfma.hip:539-541: multiply,
                          fmaf, fmaf
  d_X                     K_DX = 64             shade_mfma.hip:663-673: 16 products of 4 terms onto 0.
                          (shade.hip:348-351: 64 fmaf.)
  d_enc                   K_DENC = 16           shade_mfma.hip:718-726: 4 products of 4 terms onto 0.
                          (shade.hip:393-396: 16 fmaf.)

ReLU: 1-Lipschitz, E_hid = E_pre.  rgb: the sigmoid is monotone, so (1 + 2 eps) sigmoid(.) - eps at
o -+ E_o brackets the value, widened by the six roundings above.  sigmoid'(o) = s (1 - s): its largest
deviation over [o - E_o, o + E_o] (the peak 1/4 at 0 included where the interval straddles it), plus
the roundings of s = 1 / (1 + expf(-o)) (4 u s), of 1 - s (u (1 - s), on top of the absolute error of
s: near s = 1 the difference has lost its leading bits), and of the three products of
d_o = d_rgb (1 + 2 eps) s (1 - s).

Parameter gradients G = sum_s a_s b_s:
    E_G = sum_s (E_a |b| + |a| E_b) + gamma(D) sum_s |a| |b|,
D the roundings on the longest path of one term, grad_depth(n):
    n // 1024 + 64   samples one persistent wave adds up.  Matrix-core backward: 1024 waves of
                     64-sample strides or 2048 of 32-sample ones (shade_mfma.hip:301-303, :1152);
                     vector backward: 2048 waves, 1024 at C = 64 (shade.hip:147, :226-229, :538)
    + 64             the product and the sums inside one stride: k-steps, quarters, lanes
                     (shade_mfma.hip:625-643, :568-592, :832-845; the ray-uniform form's per-stride
                     sum of d_pre, :624-642, is at most 17 of these; shade.hip:470-476 wave_sum: 6)
    + 8              the waves of a workgroup meet in LDS (shade_mfma.hip:783-817)
    + atomics        one float atomic per workgroup (matrix-core, <= 256, shade_mfma.hip:820-861) or
                     per wave (vector, <= 2048, shade.hip:458-477), and never more than waves were
                     launched: min(2048, n // 64 + 8).  (The matrix-core count of
                     tests/test_gpu_shade_bwd_waves.py::_check is 256 here; the vector backward's
                     per-wave atomics make it the largest of the three forms.)
    emb: + n + 2048  one atomic per sample where ids change inside a stride, one per wave otherwise
                     (shade_mfma.hip:687-700, shade.hip:438-451)

Ambiguous ReLUs.  Neuron (s, j) is ambiguous when |pre| <= 2 E_pre: a correct kernel may have it on
or off.  Samples with an ambiguous neuron are left out of the d_enc comparison (`keep`), and only
there; a case may leave out at most MAX_AMBIGUOUS of its samples, cases of at most 65 samples none
(seeds are walked until that holds).  Parameter gradients leave nothing out: the term of an ambiguous
neuron, taken as switched on, is added in absolute value to the error of d_hid and so to the bound of
every element it feeds.

Bar: |got - f64| <= BAR * E with BAR = 2 for the second-order terms (E u, E E) the rule drops; where
E = 0 the value must be exactly 0.  Nothing here was measured on a kernel.
"""
import collections

import numpy as np
import torch

U = 2.0 ** -24
BAR = 2.0
MAX_AMBIGUOUS = 0.02
N_IMG = 5
IMG_RUNS = [0, 0, 2, 1, 1, 1, 0, 3, 3, 1]     # per-ray ids of tests/test_gpu_shade_rays.py
GRAD_KEYS = ("w_h", "b_h", "w1", "b1", "w2", "b2", "emb")

EPS32 = float(np.float32(1e-3))
C32 = float(np.float32(1.0) + np.float32(2.0) * np.float32(1e-3))     # 1.f + 2.f * kEps

# sh_basis.hiph, as the float32 the kernels hold
SH_CONSTS = {k: float(np.float32(v)) for k, v in dict(
    kY00=0.28209479177387814, kY1=0.48860251190291987, kY2a=1.0925484305920792,
    kY20s=0.94617469575755997, kY20o=0.31539156525251999, kY22=0.54627421529603959,
    kY33=0.59004358992664352, kY32=2.8906114426405538, kY31=0.45704579946446572,
    kY30=0.3731763325901154, kY32b=1.4453057213202769).items()}

K_EMBED = 1
K_PRE = 32 + 1
K_OUT = 64 + 1
K_RGB = 6
K_DHID = 3
K_DX = 64
K_DENC = 16


def K_HEAD(C):
    return C + 1


def gamma(k):
    return k * U / (1.0 - k * U)


def grad_depth(n, emb=False):
    d = (n // 1024 + 64) + 64 + 8 + min(2048, n // 64 + 8)
    return d + (n + 2048 if emb else 0)


# ---- inputs ---------------------------------------------------------------------------------------

Inputs = collections.namedtuple(
    "Inputs", "C n enc dirs img P d_logit d_rgb n_rays S ray_img")


def _params(g, C, w2_scale):
    return {"w_h": torch.randn(16, C, generator=g) * 0.3, "b_h": torch.randn(16, generator=g) * 0.1,
            "w1": torch.randn(64, 32, generator=g) * 0.3, "b1": torch.randn(64, generator=g) * 0.1,
            "w2": torch.randn(3, 64, generator=g) * 0.3 * w2_scale,
            "b2": torch.randn(3, generator=g) * 0.1, "emb": torch.randn(N_IMG, 16, generator=g) * 0.1}


def make_inputs(C, n, with_emb, img_run, seed, w2_scale=1.0, zero_rows=False):
    """The generator of tests/test_gpu_shade_bwd_waves.py::_inputs: f16-exact encodings, unit float32
    directions (used as given), weights scaled by 0.3, N_IMG embedding rows, image ids in runs of
    `img_run`.  zero_rows: every tenth encoding row zero, and every tenth d_rgb row with its d_logit."""
    g = torch.Generator().manual_seed(seed)
    enc = (torch.randn(n, C, generator=g) * 0.1).to(torch.float16).float()
    dirs = torch.randn(n, 3, generator=g)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    img = (torch.arange(n) // img_run % N_IMG).to(torch.int32) if with_emb else None
    P = _params(g, C, w2_scale)
    d_logit = torch.randn(n, generator=g)
    d_rgb = torch.randn(n, 3, generator=g)
    if zero_rows:
        s = torch.arange(n)
        enc[s % 10 == 3] = 0.0
        d_rgb[s % 10 == 7] = 0.0
        d_logit[s % 10 == 7] = 0.0
    return Inputs(C, n, enc, dirs, img, P, d_logit, d_rgb, 0, 0, None)


def make_ray_inputs(C, n_rays, S, seed):
    """The generator of tests/test_gpu_shade_rays.py::_inputs: a dense [n_rays, S] grid, every ray its
    own direction, image ids per ray in the pattern IMG_RUNS."""
    g = torch.Generator().manual_seed(seed)
    n = n_rays * S
    enc = (torch.randn(n, C, generator=g) * 0.1).to(torch.float16).float()
    ray_dirs = torch.randn(n_rays, 3, generator=g)
    ray_dirs = ray_dirs / ray_dirs.norm(dim=1, keepdim=True)
    dirs = ray_dirs.repeat_interleave(S, 0).contiguous()
    ray_img = torch.tensor([IMG_RUNS[i % len(IMG_RUNS)] for i in range(n_rays)], dtype=torch.int32)
    P = _params(g, C, 1.0)
    d_logit = torch.randn(n, generator=g)
    d_rgb = torch.randn(n, 3, generator=g)
    return Inputs(C, n, enc, dirs, ray_img.repeat_interleave(S).contiguous(), P, d_logit, d_rgb,
                  n_rays, S, ray_img)


# ---- float64 restatement --------------------------------------------------------------------------

def sh16(dirs, consts=SH_CONSTS):
    """Bands 0..3 with the expressions of sh_basis.hiph in float64 -> (value, E) [n, 16]: E is the
    number of roundings in the float32 expression times u times the sum of its absolute terms."""
    k = consts
    x, y, z = dirs[:, 0].double(), dirs[:, 1].double(), dirs[:, 2].double()
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    ax, ay, az = x.abs(), y.abs(), z.abs()
    one = torch.ones_like(x)
    rows = [   # (value, roundings, sum of absolute terms)
        (k["kY00"] * one, 0, k["kY00"] * one),
        (-k["kY1"] * y, 1, k["kY1"] * ay),
        (k["kY1"] * z, 1, k["kY1"] * az),
        (-k["kY1"] * x, 1, k["kY1"] * ax),
        (k["kY2a"] * xy, 2, k["kY2a"] * xy.abs()),
        (-k["kY2a"] * yz, 2, k["kY2a"] * yz.abs()),
        (k["kY20s"] * z2 - k["kY20o"], 2, k["kY20s"] * z2 + k["kY20o"]),
        (-k["kY2a"] * xz, 2, k["kY2a"] * xz.abs()),
        (k["kY22"] * x2 - k["kY22"] * y2, 4, k["kY22"] * (x2 + y2)),
        (k["kY33"] * y * (-3.0 * x2 + y2), 5, k["kY33"] * ay * (3.0 * x2 + y2)),
        (k["kY32"] * xy * z, 3, k["kY32"] * (xy * z).abs()),
        (k["kY31"] * y * (-5.0 * z2 + 1.0), 4, k["kY31"] * ay * (5.0 * z2 + 1.0)),
        (k["kY30"] * z * (5.0 * z2 - 3.0), 4, k["kY30"] * az * (5.0 * z2 + 3.0)),
        (k["kY31"] * x * (-5.0 * z2 + 1.0), 4, k["kY31"] * ax * (5.0 * z2 + 1.0)),
        (k["kY32b"] * z * (x2 - y2), 5, k["kY32b"] * az * (x2 + y2)),
        (k["kY33"] * x * (3.0 * y2 - x2), 5, k["kY33"] * ax * (3.0 * y2 + x2)),
    ]
    val = torch.stack([r[0] for r in rows], 1)
    err = torch.stack([r[1] * U * r[2] for r in rows], 1)
    return val, err


def _rgb_of(o):
    return C32 * torch.sigmoid(o) - EPS32


def _sigmoid_prime(o, E_o):
    """s (1 - s) and its error: the interval [o - E_o, o + E_o] (s (1 - s) rises to 1/4 at 0, then
    falls), and the float32 roundings of s = 1 / (1 + expf(-o)) and of 1 - s."""
    s = torch.sigmoid(o)
    sp = s * (1 - s)
    sp_of = lambda t: torch.sigmoid(t) * (1 - torch.sigmoid(t))
    dev = torch.maximum((sp_of(o - E_o) - sp).abs(), (sp_of(o + E_o) - sp).abs())
    dev = torch.where(E_o >= o.abs(), torch.maximum(dev, 0.25 - sp), dev)
    E_s = 4 * U * s                       # expf (2), +, /
    E_1ms = E_s + U * (1 - s)
    return sp, dev + E_s * (1 - s) + s * E_1ms


def _index_sum(img, rows):
    return torch.zeros(N_IMG, rows.shape[1], dtype=rows.dtype).index_add_(0, img.long(), rows)


def model(inp, backward=True, consts=SH_CONSTS):
    """-> dict: the float64 values, `E` (bound per output, same shapes), `A` (each element's sum of
    absolute path products: the scale its errors are measured in), `keep` (samples compared in d_enc)
    and intermediates the CPU tests change."""
    C, n = inp.C, inp.n
    P = {k: v.double() for k, v in inp.P.items()}
    aP = {k: v.abs() for k, v in P.items()}
    enc = inp.enc.double()
    out, E, A = {}, {}, {}

    h = enc @ P["w_h"].t() + P["b_h"]
    A_h = enc.abs() @ aP["w_h"].t() + aP["b_h"]
    E_h = gamma(K_HEAD(C)) * A_h
    out["logit"], E["logit"], A["logit"] = h[:, 0], E_h[:, 0], A_h[:, 0]
    one, zero = torch.ones(n, 1, dtype=torch.float64), torch.zeros(n, 1, dtype=torch.float64)
    X16, E_X16, A_X16 = torch.cat([one, h[:, 1:]], 1), torch.cat([zero, E_h[:, 1:]], 1), \
        torch.cat([one, A_h[:, 1:]], 1)
    if inp.img is not None:
        row = P["emb"][inp.img.long()]
        E_X16 = E_X16 + gamma(K_EMBED) * (X16.abs() + row.abs())
        A_X16 = A_X16 + row.abs()
        X16 = X16 + row
    sh, E_sh = sh16(inp.dirs, consts)
    X, E_X, A_X = torch.cat([X16, sh], 1), torch.cat([E_X16, E_sh], 1), torch.cat([A_X16, sh.abs()], 1)
    pre = X @ P["w1"].t() + P["b1"]
    A["pre"] = A_X @ aP["w1"].t() + aP["b1"]
    E["pre"] = E_X @ aP["w1"].t() + gamma(K_PRE) * (X.abs() @ aP["w1"].t() + aP["b1"])
    hid = torch.relu(pre)
    o = hid @ P["w2"].t() + P["b2"]
    E_o = E["pre"] @ aP["w2"].t() + gamma(K_OUT) * (hid @ aP["w2"].t() + aP["b2"])
    rgb = _rgb_of(o)
    E["rgb"] = torch.maximum(_rgb_of(o + E_o) - rgb, rgb - _rgb_of(o - E_o)) + \
        K_RGB * U * (rgb.abs() + EPS32)
    A["rgb"] = rgb.abs() + EPS32
    out.update(pre=pre, rgb=rgb, o=o, X=X, hid=hid, E_o=E_o)
    amb = pre.abs() <= 2 * E["pre"]
    out["ambiguous"] = amb
    out["keep"] = ~amb.any(1)
    out["ambiguous_share"] = 1.0 - float(out["keep"].double().mean())
    if not backward:
        return dict(out, E=E, A=A)

    d_rgb, d_logit = inp.d_rgb.double(), inp.d_logit.double()
    sp, E_sp = _sigmoid_prime(o, E_o)
    d_o = d_rgb * C32 * sp
    E_do = d_rgb.abs() * C32 * E_sp + 3 * U * d_o.abs()
    dh_on = d_o @ P["w2"]
    A_dh_on = d_o.abs() @ aP["w2"]
    on = pre > 0
    live = on | amb
    d_hid = dh_on * on
    a_dhid = dh_on.abs() * live
    E_dhid = live * (E_do @ aP["w2"] + gamma(K_DHID) * A_dh_on) + amb * dh_on.abs()
    w1h, aw1h = P["w1"][:, :16], aP["w1"][:, :16]
    d_X = d_hid @ w1h
    E_dX = E_dhid @ aw1h + gamma(K_DX) * (a_dhid @ aw1h)
    A_dX = (A_dh_on * live) @ aw1h
    d_h, E_dh, A_dh = d_X.clone(), E_dX.clone(), A_dX.clone()
    d_h[:, 0], E_dh[:, 0], A_dh[:, 0] = d_logit, 0.0, d_logit.abs()
    out["d_enc"] = d_h @ P["w_h"]
    E["d_enc"] = E_dh @ aP["w_h"] + gamma(K_DENC) * (d_h.abs() @ aP["w_h"])
    A["d_enc"] = A_dh @ aP["w_h"]
    out.update(d_o=d_o, d_hid=d_hid, d_X=d_X, d_h=d_h)

    D = gamma(grad_depth(n))

    def outer(a, E_a, abs_a, A_a, b, E_b, A_b):
        return a.t() @ b, E_a.t() @ b.abs() + abs_a.t() @ E_b + D * (abs_a.t() @ b.abs()), A_a.t() @ A_b

    ones, nil = torch.ones(n, 1, dtype=torch.float64), torch.zeros(n, 1, dtype=torch.float64)
    g, Eg, Ag = {}, {}, {}
    g["w2"], Eg["w2"], Ag["w2"] = outer(d_o, E_do, d_o.abs(), d_o.abs(), hid, E["pre"], A["pre"])
    g["b2"], Eg["b2"], Ag["b2"] = (t[:, 0] for t in outer(d_o, E_do, d_o.abs(), d_o.abs(), ones, nil, ones))
    g["w1"], Eg["w1"], Ag["w1"] = outer(d_hid, E_dhid, a_dhid, A_dh_on * live, X, E_X, A_X)
    g["b1"], Eg["b1"], Ag["b1"] = (t[:, 0] for t in outer(d_hid, E_dhid, a_dhid, A_dh_on * live, ones, nil, ones))
    g["w_h"], Eg["w_h"], Ag["w_h"] = outer(d_h, E_dh, d_h.abs(), A_dh, enc, torch.zeros_like(enc), enc.abs())
    g["b_h"], Eg["b_h"], Ag["b_h"] = (t[:, 0] for t in outer(d_h, E_dh, d_h.abs(), A_dh, ones, nil, ones))
    if inp.img is not None:
        g["emb"] = _index_sum(inp.img, d_X)
        Eg["emb"] = _index_sum(inp.img, E_dX) + gamma(grad_depth(n, True)) * _index_sum(inp.img, d_X.abs())
        Ag["emb"] = _index_sum(inp.img, A_dX)
    for k in g:
        out["g_" + k], E["g_" + k], A["g_" + k] = g[k], Eg[k], Ag[k]
    return dict(out, E=E, A=A)


def ratio(got, ref, E, rows=None):
    """|got - ref| / E per element, with 0 / 0 = 0 and x / 0 = inf; `rows` restricts the sample axis
    (axis 0) to the samples compared."""
    err = (got.double() - ref).abs()
    if rows is not None:
        err, E = err[rows], E[rows]
    r = err / E
    r[(err == 0) & (E == 0)] = 0.0
    return r


# ---- cases ----------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "kind C n with_emb img_run S tag")
N_RAYS = 37
EDGE_W2_SCALE = 6.0      # |o| reaches about 20: test_shade_model_cpu.py::test_edge_case_saturates


def cases():
    """Every case tests/test_gpu_shade_f64.py runs.  kind: 'both' forward and backward, 'fwd' / 'bwd'
    one of them (the wrap cases), 'edge', 'rays'."""
    out = []
    for C in (8, 16, 32, 64):
        for with_emb in (True, False):
            for n in (1, 31, 33, 63, 64, 65, 64 * 9 + 17):
                out.append(Case("both", C, n, with_emb, 37, 0, ""))
    for img_run in (1, 5, 13, 16, 31):
        out.append(Case("both", 32, 64 * 40 + 21, True, img_run, 0, "run%d" % img_run))
    out.append(Case("fwd", 32, 64 * 4500 + 5, True, 37, 0, "wrap"))
    out.append(Case("bwd", 32, 64 * 2100 + 5, True, 37, 0, "wrap"))
    out.append(Case("edge", 32, 64 * 9 + 17, True, 37, 0, "edge"))
    for C in (8, 32, 64):
        for S in (64, 128, 192):
            out.append(Case("rays", C, N_RAYS * S, True, 0, S, "rays"))
    return out


def case_id(c):
    return "%s-C%d-n%d-%s%s" % (c.kind, c.C, c.n, "emb" if c.with_emb else "noemb",
                                ("-" + c.tag) if c.tag and c.tag != c.kind else "")


def build_case(c):
    """-> (Inputs, model dict).  Seeds are walked as tests/test_gpu_shade_rays.py::_case walks them:
    cases of at most 65 samples until no sample is ambiguous; every case asserts MAX_AMBIGUOUS."""
    for bump in range(64):
        seed = 7919 * c.C + c.n + (7 if c.with_emb else 0) + 13 * c.img_run + c.S + 100000 * bump
        if c.kind == "rays":
            inp = make_ray_inputs(c.C, N_RAYS, c.S, seed)
        else:
            edge = c.kind == "edge"
            inp = make_inputs(c.C, c.n, c.with_emb, c.img_run, seed,
                              w2_scale=EDGE_W2_SCALE if edge else 1.0, zero_rows=edge)
        m = model(inp, backward=c.kind != "fwd")
        if c.n > 65 or m["ambiguous_share"] == 0.0:
            break
    else:
        raise AssertionError("no seed without an ambiguous sample: " + case_id(c))
    assert m["ambiguous_share"] <= MAX_AMBIGUOUS, (case_id(c), m["ambiguous_share"])
    return inp, m
