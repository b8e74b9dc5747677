"""Shared input builders for the parity tests (seeded; same tensors go to the oracle and the GPU)."""
import math

import numpy as np
import torch

from oracle import kernels as K


from oracle.ref_render import _is_prime as is_prime  # noqa: E402


def make_field(L=16, F=2, log2_T=19, level_stride=None, seed=0, init="trained"):
    """Hash-grid parameters as Hash3DAnchored's ctor draws them (reference
    src/hash_3d_anchored.cpp:19-58); T = rows per level, stride in elements (default T, quirk Q2)."""
    g = torch.Generator().manual_seed(seed)
    T = 1 << log2_T
    stride = T if level_stride is None else level_stride
    numel = max(T * L * F, stride * (L - 1) + T * F)
    if init == "reference":
        table = (torch.rand(numel, generator=g) * 0.2 - 1.0) * 1e-4
    else:
        table = torch.randn(numel, generator=g) * 0.1
    primes = []
    while len(primes) < 3 * L:
        v = int(torch.randint(1 << 28, 1 << 30, (1,), generator=g))
        if is_prime(v):
            primes.append(v)
    primes = torch.tensor(primes, dtype=torch.int32).reshape(L, 3)
    bias = torch.rand(L, 3, generator=g) * 1000.0 + 100.0
    return dict(L=L, F=F, T=T, stride=stride, table=table, table16=K.cast_f16(table),
                primes=primes, bias=bias, mul=K.level_mul(L))


def ball_points(n, seed=0, radius=2.0):
    """Points inside the radius-2 ball (the image of the scene contraction)."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    r = torch.rand(n, 1, generator=g) ** (1.0 / 3.0) * radius
    return (d * r).contiguous()


def ragged_bounds(n_rays, max_len, seed=0, empty_frac=0.1):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(0, max_len + 1, (n_rays,), generator=g)
    lens[torch.rand(n_rays, generator=g) < empty_frac] = 0
    end = torch.cumsum(lens, 0)
    start = end - lens
    return torch.stack([start, end], 1).to(torch.int32).contiguous(), int(end[-1])


def f16_ulp(x):
    """Size of one f16 ulp at magnitude |x| (f32 tensor in, f32 out)."""
    ax = x.abs().clamp_min(2.0 ** -14)
    e = torch.floor(torch.log2(ax))
    return torch.pow(2.0, e - 10)


# ------------------------------------------------------------------ exact table gradient ---------

_U = 2.0 ** -24          # unit of a contribution, and the unit roundoff of f32


def binned_path_inputs(L, F, log2_T, stride_mode, n):
    """Field, points and gradient of test_hash_bwd_binned_path (half the points in a tiny ball, a
    tenth of the gradient zero): shared so the CPU tests measure on what the GPU tests run."""
    T = 1 << log2_T
    fld = make_field(L, F, log2_T, None if stride_mode == "ref" else T * F, seed=5 + F)
    pts = ball_points(n, seed=21)
    pts[: n // 2] *= 0.02
    g = torch.Generator().manual_seed(15)
    grad = torch.randn(n, L * F, generator=g) * 1e-3
    grad[torch.rand(n, L * F, generator=g) < 0.1] = 0.0
    return fld, pts, grad


def _compose(per_level, stride, numel):
    """[L, T*F] per-level values -> table-element space: level l lands at stride*l (added)."""
    out = torch.zeros(numel, dtype=per_level.dtype)
    for l in range(per_level.shape[0]):
        out[stride * l: stride * l + per_level.shape[1]] += per_level[l]
    return out


def table_grad_expectation(S, A, N, L, F, T, level_stride, grad_scale, numel, base=None):
    """What a table gradient may be, from the exact integer sums of K.hash_bwd_exact.

    exact  float64: sum over the covering levels of S_l 2^-24 / grad_scale (+ base)
    rne    float32: each level's S_l 2^-24 / grad_scale rounded to f32 ONCE, the covering levels then
           f32-added in level order (onto base when given) -- what an exact-sum kernel that flushes
           each (level, slice) once must give, bit for bit, where at most two terms meet
    cover  how many levels with a non-zero count touch the element
    count  how many non-zero contributions reach it, all levels together
    bound  sum over those levels of N_l 2^-24 * A_l 2^-24 / grad_scale: the any-order bound
           gamma_N sum|x_i| for adding N f32 terms, valid for every summation tree (float atomics,
           LDS float atomics, per-round partial flushes); with a base, plus one f32 ulp of the result
           per addition onto it
    """
    assert S.shape == (L, T * F) and A.shape == S.shape and N.shape == S.shape
    assert int(A.sum(0).max()) < 2 ** 53          # int64 -> float64 below stays exact
    m, e = torch.frexp(torch.tensor(float(grad_scale)))
    assert float(m) == 0.5, "a power-of-two grad_scale keeps the division exact"
    unit = _U / float(grad_scale)
    exact = _compose(S, level_stride, numel).double() * unit
    cover = _compose((N != 0).to(torch.int32), level_stride, numel)
    count = _compose(N.to(torch.int64), level_stride, numel)
    bound = _compose(N.double() * _U * (A.double() * unit), level_stride, numel)
    rne = torch.zeros(numel, dtype=torch.float32) if base is None else base.clone().float()
    for l in range(L):
        win = slice(level_stride * l, level_stride * l + T * F)
        rne[win] = rne[win] + (S[l].double() * unit).float()
    if base is not None:
        exact = exact + base.double()
        bound = bound + cover.double() * torch.maximum(f32_ulp(rne), f32_ulp(base.float())).double()
    return dict(exact=exact, rne=rne, cover=cover, count=count, bound=bound,
                base=None if base is None else base.clone().float())


def f32_ulp(x):
    """Size of one f32 ulp at magnitude |x| (f32 in, f32 out; subnormals and zero: 2^-149)."""
    _, e = torch.frexp(x.float().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float32), e - 24)


def _bits(x):
    return x.contiguous().view(torch.int32)


def assert_table_grad(got, expectation, exact_elements=False, max_inexact=0, few_exact=True):
    """got: f32 table gradient (CPU).  Asserts
    (a) elements nobody contributes to are bit-identical to base (or +0),
    (b) |got - exact| <= bound everywhere,
    (c) where exact_elements (bool tensor, True or False) holds, got == rne bit for bit, with at
        most max_inexact exceptions -- which (d) still satisfy (b), being part of "everywhere",
    (e) few_exact: elements that one or two contributions reach (one, onto a base) equal rne bit
        for bit with NO exception, on any route.  A contribution over a power-of-two grad_scale has
        11 significant bits and is an f32; any kernel, atomics included, can only form x1 or
        fl(x1 + x2) there (fl(base + x1) onto a base), and that single rounding of the exact sum is
        what rne holds.  Most fine-level elements are of this kind.
    Returns dict(max_ratio = largest err/bound over touched elements, inexact = exceptions in (c))."""
    ex = expectation
    got = got.detach().cpu().float()
    assert got.shape == ex["rne"].shape
    untouched = ex["cover"] == 0
    want0 = torch.zeros_like(got) if ex["base"] is None else ex["base"]
    n_a = int((_bits(got)[untouched] != _bits(want0)[untouched]).sum())
    assert n_a == 0, "(a) %d untouched elements were written" % n_a
    assert bool(torch.isfinite(got).all()), "non-finite table gradient"
    err = (got.double() - ex["exact"]).abs()
    over = err > ex["bound"]
    if bool(over.any()):
        i = int(torch.nonzero(over)[0])
        raise AssertionError("(b) %d elements off by more than the bound; first: element %d got %r "
                             "exact %r bound %r cover %d" % (
                                 int(over.sum()), i, float(got[i]), float(ex["exact"][i]),
                                 float(ex["bound"][i]), int(ex["cover"][i])))
    touched = ~untouched
    ratio = err[touched] / ex["bound"][touched].clamp_min(1e-300)
    stats = dict(max_ratio=float(ratio.max()) if ratio.numel() else 0.0, inexact=0)
    if few_exact:
        few = (ex["count"] >= 1) & (ex["count"] <= (2 if ex["base"] is None else 1))
        bad = few & (_bits(got) != _bits(ex["rne"]))
        if bool(bad.any()):
            i = int(torch.nonzero(bad)[0])
            raise AssertionError("(e) %d elements with one or two contributions differ from their "
                                 "exact sum; first: element %d got %r rne %r count %d" % (
                                     int(bad.sum()), i, float(got[i]), float(ex["rne"][i]),
                                     int(ex["count"][i])))
    if exact_elements is not False:
        diff = _bits(got) != _bits(ex["rne"])
        if exact_elements is not True:
            diff = diff & exact_elements
        stats["inexact"] = int(diff.sum())
        if stats["inexact"] > max_inexact:
            i = int(torch.nonzero(diff)[0])
            raise AssertionError("(c) %d elements differ from the correctly rounded exact sum "
                                 "(allowed %d); first: element %d got %r rne %r cover %d" % (
                                     stats["inexact"], max_inexact, i, float(got[i]),
                                     float(ex["rne"][i]), int(ex["cover"][i])))
    return stats


def old_table_grad_criterion(got, ref, max_tol=2e-5, norm_tol=1e-5):
    """The two assertions test_hash_bwd_binned_path makes against the f32 oracle sum: a global
    absolute tolerance scaled by the largest element, and a relative norm."""
    scale = ref.abs().max().item()
    assert (got - ref).abs().max().item() <= max_tol * scale
    assert ((got - ref).norm() / ref.norm()).item() < norm_tol


# ---- the occupancy grid and the raw field of the C-ABI tests (tests/test_gpu_occupancy.py, the render
# tests and tests/render_model.py share them)

def _pack(bits_bool):
    """bool [G^3] (index i = (cz*G + cy)*G + cx) -> int32 words, bit (i & 31) of word (i >> 5)."""
    b = np.ascontiguousarray(bits_bool.reshape(-1).cpu().numpy().astype(np.uint8))
    return torch.from_numpy(np.packbits(b, bitorder="little").view(np.int32).copy())


def _cells(x, G):
    """The header's cell expression in numpy f32: x [n,3] contracted -> linear bit index [n]."""
    x = x.astype(np.float32)
    c = np.floor((x + np.float32(2.0)) * (np.float32(0.25) * np.float32(G)))
    c = np.clip(c, 0, G - 1).astype(np.int64)
    return (c[:, 2] * G + c[:, 1]) * G + c[:, 0]


def _raw_field(L, F, T, bias0, seed, dev):
    """A hash grid + density head as device tensors for the C ABI ("trained-like" table)."""
    g = torch.Generator().manual_seed(seed)
    numel = T * L * F
    table = torch.randn(numel, generator=g) * 0.1
    primes = []
    while len(primes) < 3 * L:
        v = int(torch.randint(1 << 28, 1 << 30, (1,), generator=g))
        if is_prime(v):
            primes.append(v)
    C = L * F
    w0 = (torch.rand(C, generator=g) * 2 - 1) / math.sqrt(C)
    return dict(L=L, F=F, T=T, stride=T,
                table16=K.cast_f16(table).to(dev),
                primes=torch.tensor(primes, dtype=torch.int32).reshape(L, 3).to(dev),
                bias=(torch.rand(L, 3, generator=g) * 1000.0 + 100.0).to(dev),
                mul=K.level_mul(L).to(dev), w0=w0.to(dev),
                b0=torch.tensor([bias0], dtype=torch.float32).to(dev))
