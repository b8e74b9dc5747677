"""Numpy models of ssim.hip: SSIM of an image pair, its gradient, and the patch draw.

Three forms:
  * float64 (ssim64, grad64): the definition of include/f2nerf_hip.h -- the reference's rgb_ssim
    (scripts/eval.py:29-75) with max_val = 1: an 11-tap Gaussian (sigma 1.5, centred, normalised),
    `valid` borders, c1 = 1e-4, c2 = 9e-4, the three clamps when clip is set -- and the gradient of
    the unclamped form by its first argument.
  * float32 (ssim32, bwd32): the kernels' evaluation order as the header comment of ssim.hip states
    it, operation for operation (fmaf through mesh_model.fmaf32, which rounds once), tile sums and
    the f64 trees included, so that the GPU's results can be held to equal bits.
  * integers (draw_patches): the patch draw, on the Philox4x32-10 of supervision_model.

Images are [h, w, 3] arrays; pred is x, gt is y.
"""
import numpy as np

from tests.mesh_model import fmaf32
from tests.supervision_model import MASK32, mulhi, philox4x32_10

F32 = np.float32
TAPS, HALO = 11, 10
TILE = 16                              # F2N_SSIM_TILE
BLOCK = TILE * TILE
C1, C2 = 1e-4, 9e-4                    # (0.01 max_val)^2, (0.03 max_val)^2 with max_val = 1
PATCH_DOMAIN = 2                       # word 2 of the draw's Philox counter


def filter64():
    z = (np.arange(TAPS, dtype=np.float64) - TAPS // 2) / 1.5
    g = np.exp(-0.5 * (z * z))
    return g / g.sum()


def filter32():
    return filter64().astype(F32)


# ------------------------------------------------------------------------------- float64 ----------


def _valid64(z, f):
    """separable `valid` correlation of [h, w, C] with the taps f -> [h-10, w-10, C]"""
    h, w = z.shape[:2]
    t = sum(f[k] * z[:, k:k + w - HALO] for k in range(TAPS))
    return sum(f[k] * t[k:k + h - HALO] for k in range(TAPS))


def _full64(g, f):
    """separable `full` convolution of [mh, mw, C] with the taps f -> [mh+10, mw+10, C]"""
    mh, mw = g.shape[:2]
    p = np.pad(g, ((HALO, HALO), (HALO, HALO), (0, 0)))
    t = sum(f[k] * p[:, HALO - k:HALO - k + mw + HALO] for k in range(TAPS))
    return sum(f[k] * t[HALO - k:HALO - k + mh + HALO] for k in range(TAPS))


def _moments64(x, y, clip, taps):
    f = filter64() if taps is None else np.asarray(taps, dtype=np.float64)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    mux, muy = _valid64(x, f), _valid64(y, f)
    sxx = _valid64(x * x, f) - mux * mux
    syy = _valid64(y * y, f) - muy * muy
    sxy = _valid64(x * y, f) - mux * muy
    if clip:
        sxx, syy = np.maximum(0.0, sxx), np.maximum(0.0, syy)
        sxy = np.sign(sxy) * np.minimum(np.sqrt(sxx * syy), np.abs(sxy))
    return f, x, y, mux, muy, sxx, syy, sxy


def ssim64(x, y, clip, taps=None):
    """-> (ssim, map [h-10, w-10, 3]) in float64"""
    _, _, _, mux, muy, sxx, syy, sxy = _moments64(x, y, clip, taps)
    S = ((2 * mux * muy + C1) * (2 * sxy + C2)) / ((mux * mux + muy * muy + C1) * (sxx + syy + C2))
    return float(S.mean()), S


def grad64(x, y, d_ssim=1.0, taps=None):
    """d (d_ssim * ssim of the unclamped form) / d x -> [h, w, 3] float64; y gets none"""
    f, x, y, mux, muy, sxx, syy, sxy = _moments64(x, y, False, taps)
    N1, N2 = 2 * mux * muy + C1, 2 * sxy + C2
    D1, D2 = mux * mux + muy * muy + C1, sxx + syy + C2
    S = N1 * N2 / (D1 * D2)
    gmu = 2 * muy * N2 / (D1 * D2) - 2 * muy * N1 / (D1 * D2) - 2 * mux * S / D1 + 2 * mux * S / D2
    gxx = -S / D2
    gxy = 2 * N1 / (D1 * D2)
    v = _full64(gmu, f) + 2 * x * _full64(gxx, f) + y * _full64(gxy, f)
    return d_ssim / S.size * v


# ------------------------------------------------------------------------------- float32 ----------


def _chain32(z, f, axis, n):
    """acc = f[0] z[0 ..]; acc = fmaf(f[k], z[k ..], acc), k ascending, along `axis`, n outputs"""
    def at(k):
        return z[:, k:k + n] if axis == 1 else z[k:k + n]
    acc = f[0] * at(0)
    for k in range(1, TAPS):
        acc = fmaf32(f[k], at(k), acc).reshape(acc.shape)
    return acc


def _tree(lanes):
    """[n, 256] f64 -> [n]: t[i] += t[i + half], half = 128 .. 1"""
    t = np.array(lanes, dtype=np.float64)
    half = BLOCK // 2
    while half > 0:
        t[:, :half] += t[:, half:2 * half]
        half //= 2
    return t[:, 0]


def ssim32(x, y, clip, want_gmaps=False):
    """the kernel's order -> dict(ssim f32, map f32 [mh, mw, 3], gmaps f32 [mh, mw, 9] | None)"""
    assert not (clip and want_gmaps)
    f = filter32()
    x, y = np.asarray(x, dtype=F32), np.asarray(y, dtype=F32)
    h, w = x.shape[:2]
    mh, mw = h - HALO, w - HALO
    mom = [_chain32(_chain32(z, f, 1, mw), f, 0, mh) for z in (x, y, x * x, y * y, x * y)]
    mux, muy, exx, eyy, exy = mom
    mxx, myy, mxy = mux * mux, muy * muy, mux * muy
    sxx, syy, sxy = exx - mxx, eyy - myy, exy - mxy
    if clip:
        sxx = np.where(sxx > 0, sxx, F32(0))
        syy = np.where(syy > 0, syy, F32(0))
        lim = np.sqrt(sxx * syy)
        a = np.where(np.abs(sxy) < lim, np.abs(sxy), lim)
        sxy = np.copysign(a, sxy)
    two, c1, c2 = F32(2), F32(C1), F32(C2)
    N1, N2 = two * mxy + c1, two * sxy + c2
    D1, D2 = (mxx + myy) + c1, (sxx + syy) + c2
    P = D1 * D2
    S = (N1 * N2) / P
    assert S.dtype == F32
    gmaps = None
    if want_gmaps:
        e = (two * mux) * S
        gmu = ((two * muy) * (N2 - N1)) / P + (e / D2 - e / D1)
        gmaps = np.stack([gmu, -(S / D2), (two * N1) / P], axis=-1).reshape(mh, mw, 9)
        assert gmaps.dtype == F32
    # sums: per lane in channel order, per tile by the tree, per image lanes in strides, the tree
    lane = (S[..., 0].astype(np.float64) + S[..., 1].astype(np.float64)) + S[..., 2].astype(np.float64)
    ty, tx = -(-mh // TILE), -(-mw // TILE)
    padded = np.zeros((ty * TILE, tx * TILE))
    padded[:mh, :mw] = lane
    tiles = padded.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3).reshape(ty * tx, BLOCK)
    partial = _tree(tiles)
    acc = np.zeros(BLOCK)
    for s in range(0, partial.size, BLOCK):
        chunk = partial[s:s + BLOCK]
        acc[:chunk.size] += chunk
    total = _tree(acc[None])[0]
    return dict(ssim=F32(total / (float(mh) * float(mw) * 3.0)), map=S, gmaps=gmaps)


def bwd32(x, y, gmaps, d_ssim):
    """the backward kernel's order on the forward's gmaps -> d_pred f32 [h, w, 3]"""
    f = filter32()
    x, y = np.asarray(x, dtype=F32), np.asarray(y, dtype=F32)
    h, w = x.shape[:2]
    mh, mw = h - HALO, w - HALO
    d_ssim = F32(d_ssim)
    if d_ssim == 0:
        return np.zeros((h, w, 3), dtype=F32)
    scale = F32(np.float64(d_ssim) / (float(mh) * float(mw) * 3.0))
    p = np.pad(np.asarray(gmaps, dtype=F32), ((HALO, HALO), (HALO, HALO), (0, 0)))

    def rev_chain(z, axis, n):       # acc = f[0] z[10 ..]; acc = fmaf(f[k], z[10 - k ..], acc)
        def at(k):
            return z[:, HALO - k:HALO - k + n] if axis == 1 else z[HALO - k:HALO - k + n]
        acc = f[0] * at(0)
        for k in range(1, TAPS):
            acc = fmaf32(f[k], at(k), acc).reshape(acc.shape)
        return acc

    filt = rev_chain(rev_chain(p, 1, w), 0, h).reshape(h, w, 3, 3)
    A, Bq, C = filt[..., 0], filt[..., 1], filt[..., 2]
    v = (A + (F32(2) * x) * Bq) + y * C
    out = scale * v
    assert out.dtype == F32
    return out


# ------------------------------------------------------------------------------- patch draw -------


def draw_patches(mask, E, h, w, n, P, seed, attempts=32):
    """mask: uint8 / bool [E, h, w] or None -> cam [n P^2] i32, ij [n P^2, 2] i32, tries [n] i32,
    patch_weight [n] f32 of f2n_draw_patches"""
    seed_lo, seed_hi = seed & MASK32, (seed >> 32) & MASK32
    valid = None if mask is None else (np.asarray(mask).reshape(E, h, w) != 0)
    b = np.arange(n, dtype=np.uint64)
    cam = np.zeros(n, dtype=np.int64)
    i0 = np.zeros(n, dtype=np.int64)
    j0 = np.zeros(n, dtype=np.int64)
    tries = np.zeros(n, dtype=np.int64)
    for a in range(attempts):
        open_ = tries == 0
        if not open_.any():
            break
        x0, x1, x2, _ = philox4x32_10(b, a, PATCH_DOMAIN, 0, seed_lo, seed_hi)
        c = mulhi(x0, E).astype(np.int64)
        i = mulhi(x1, h - P + 1).astype(np.int64)
        j = mulhi(x2, w - P + 1).astype(np.int64)
        cam[open_], i0[open_], j0[open_] = c[open_], i[open_], j[open_]
        if valid is None:
            hit = open_
        else:
            full = np.array([valid[c[r], i[r]:i[r] + P, j[r]:j[r] + P].all() for r in range(n)],
                            dtype=bool)
            hit = open_ & full
        tries[hit] = a + 1
    u, v = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
    rows = (i0[:, None, None] + u).reshape(-1)
    cols = (j0[:, None, None] + v).reshape(-1)
    ij = np.stack([rows, cols], axis=1).astype(np.int32)
    return (np.repeat(cam, P * P).astype(np.int32), ij, tries.astype(np.int32),
            (tries > 0).astype(F32))
