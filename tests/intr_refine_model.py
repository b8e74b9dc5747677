"""Float64 and float32 restatements for the calibration-refinement tests (f2n_cam_intr_grad,
f2n_intr_compose, f2n_intr_compose_bwd).  No tests in here: tests/test_intr_refine_model_cpu.py checks
the formulas and the bounds on the CPU, tests/test_gpu_intr_refine.py holds the HIP kernels to them.

The per-ray terms (include/f2nerf_hip.h, intr_refine.hip).  The forward solves F(x, y; k) = (xd, yd),
xd = (col + .5 - cx) / fx, yd = (row + .5 - cy) / fy, and dir = R (x, -y, -1).  With
    gx = sum_i d_d[i] R[i][0],  gy = -sum_i d_d[i] R[i][1],  J = [[a, b], [b, d]] = dF/d(x, y),
    lx = (d gx - b gy) / det,   ly = (a gy - b gx) / det,    det = a d - b b
the eight terms of a ray, for (fx, fy, cx, cy, k1, k2, p1, p2), are
    -lx xd / fx, -ly yd / fy, -lx / fx, -ly / fy, -r2 s, -r2^2 s             (s = lx x + ly y)
    -(2 x y lx + (r2 + 2 y^2) ly), -((r2 + 2 x^2) lx + 2 x y ly).
(x, y) is an INPUT: the point the forward returned, as float32 bits; `ray_terms` in float64 is the
reference at those bits, in float32 it follows the device code operation by operation.

mag, per term: the sum of the absolute values of the products that form it, written out to the
inputs -- |gx| becomes sum_i |d_d[i] R[i][0]|, |lx| becomes (|d| mgx + |b| mgy) / |det|, and so on
through the term -- so that cancellation in gx, gy and lx, ly does not count against the kernel.

TERM_TOL.  lens_model.TOL's recipe: the largest |f32 restatement - f64| / mag over
lens_model.pixels() x the five lens_model.SETS and the zero set, on the inputs of `term_case`, is
3.95e-7 (tests/test_intr_refine_model_cpu.py::test_term_tol_covers_f32_restatement recomputes it);
TERM_TOL = 4 * that, rounded up to a power of two = 2^-19.  The factor 4 absorbs the operation order
and contraction that numpy cannot reproduce.  Measured on the CPU restatement only, never on the
kernel.

The per-camera sums: f64 sums of the f64 terms are the reference; a float32 sum of cnt float32 terms
in any order is within
    TERM_TOL * sum mag  +  gamma(cnt + 2) * (sum |term| + TERM_TOL * sum mag)
of it, gamma(k) = k u / (1 - k u) as in tests/pose_refine_model.py (the terms' own error, then the
summation bound on terms that large).

The correction: fx' = fx exp(c0), fy' = fy exp(c1), cx' = cx + c2 fx, cy' = cy + c3 fy (base fx, fy),
k' = k + c[4:8], per group; a negative group is a fixed image.  The backward sums per group
(dfx' fx', dfy' fy', dcx' fx, dcy' fy, dk1', dk2', dp1', dp2') in float64.
"""
import numpy as np

from tests import lens_model as lm
from tests import pose_refine_model as pm

TERM_TOL = 2.0 ** -19
SETS6 = tuple(lm.SETS) + ((0.0, 0.0, 0.0, 0.0),)
NAMES = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")


# ---- the per-ray terms -----------------------------------------------------------------------------

def ray_terms(ij, K, k, x, y, R, d_d, dtype, jac_identity=False, flip_gy=False):
    """-> (terms [n,8], mag [n,8]) in `dtype`.  ij [n,2]; K [3,3] or [n,3,3]; k [4] or [n,4]; x, y [n]
    the forward's ideal point; R [n,3,3]; d_d [n,3].  The two flags are the mutants of the CPU test."""
    xd, yd = lm.normalised(ij, K, dtype)
    Kd = np.asarray(K, dtype=np.float32).astype(dtype)
    fx, fy = Kd[..., 0, 0], Kd[..., 1, 1]
    k1, k2, p1, p2 = lm._coeffs(k, dtype)
    x, y = np.asarray(x).astype(dtype), np.asarray(y).astype(dtype)
    R = np.asarray(R, dtype=np.float32).astype(dtype)
    g = np.asarray(d_d, dtype=np.float32).astype(dtype)
    one, two, six = dtype(1), dtype(2), dtype(6)
    gx = (g[:, 0] * R[:, 0, 0] + g[:, 1] * R[:, 1, 0]) + g[:, 2] * R[:, 2, 0]
    gy = -((g[:, 0] * R[:, 0, 1] + g[:, 1] * R[:, 1, 1]) + g[:, 2] * R[:, 2, 1])
    if flip_gy:
        gy = -gy
    mgx = np.abs(g[:, 0] * R[:, 0, 0]) + np.abs(g[:, 1] * R[:, 1, 0]) + np.abs(g[:, 2] * R[:, 2, 0])
    mgy = np.abs(g[:, 0] * R[:, 0, 1]) + np.abs(g[:, 1] * R[:, 1, 1]) + np.abs(g[:, 2] * R[:, 2, 1])
    xx, yy, xy = x * x, y * y, x * y
    r2 = xx + yy
    rad = one + r2 * (k1 + k2 * r2)
    dr = k1 + two * k2 * r2
    a = rad + two * xx * dr + two * p1 * y + six * p2 * x
    b = two * xy * dr + two * p1 * x + two * p2 * y
    d = rad + two * yy * dr + six * p1 * y + two * p2 * x
    pinhole = np.broadcast_to((k1 == 0) & (k2 == 0) & (p1 == 0) & (p2 == 0), x.shape)
    if jac_identity:
        pinhole = np.ones(x.shape, dtype=bool)
    a = np.where(pinhole, one, a).astype(dtype)
    b = np.where(pinhole, dtype(0), b).astype(dtype)
    d = np.where(pinhole, one, d).astype(dtype)
    big = np.finfo(dtype).max
    with np.errstate(all="ignore"):
        det = a * d - b * b
        lx = (d * gx - b * gy) / det
        ly = (a * gy - b * gx) / det
        ok = (np.abs(det) > dtype(np.float32(lm.MIN_DET))) & (np.abs(lx) <= big) & (np.abs(ly) <= big)
        mlx = (np.abs(d) * mgx + np.abs(b) * mgy) / np.abs(det)
        mly = (np.abs(a) * mgy + np.abs(b) * mgx) / np.abs(det)
        xy2 = two * xy
        s = lx * x + ly * y
        ms = mlx * np.abs(x) + mly * np.abs(y)
        t = np.stack([
            -((lx * xd) / fx),
            -((ly * yd) / fy),
            -(lx / fx),
            -(ly / fy),
            -(r2 * s),
            -((r2 * r2) * s),
            -(xy2 * lx + (r2 + two * yy) * ly),
            -((r2 + two * xx) * lx + xy2 * ly)], 1)
        m = np.stack([
            mlx * np.abs(xd) / fx,
            mly * np.abs(yd) / fy,
            mlx / fx,
            mly / fy,
            r2 * ms,
            (r2 * r2) * ms,
            np.abs(xy2) * mlx + (r2 + two * yy) * mly,
            (r2 + two * xx) * mlx + np.abs(xy2) * mly], 1)
    t = np.where(ok[:, None], t, dtype(0)).astype(dtype)
    m = np.where(ok[:, None], m, dtype(0)).astype(dtype)
    return t, m


def forward_xy32(k, ij, K):
    """The float32 restatement of the forward's ideal point (the kernel's 8 Newton steps; the pinhole
    expression for a zero set)."""
    xd, yd = lm.normalised(ij, K, np.float32)
    if not np.any(np.asarray(k, dtype=np.float32)):
        return xd, yd
    x, y, _ = lm.undistort(k, xd, yd, np.float32)
    return x, y


def term_case(which, seed=17):
    """Every pixel of the lens_model image under coefficient set SETS6[which], a random rotation per
    ray and d_rays_d of random sign and log-normal size.  -> dict(ij, K, k, R, d_d) float32 / int32."""
    rng = np.random.default_rng(seed + which)
    ij = lm.pixels()
    n = ij.shape[0]
    d_d = (rng.choice([-1.0, 1.0], (n, 3)) * rng.lognormal(0.0, 1.0, (n, 3))).astype(np.float32)
    return dict(ij=ij, K=lm.intrinsic(), k=np.asarray(SETS6[which], dtype=np.float32),
                R=lm.rotations(n, seed + which), d_d=d_d, n=n)


# ---- the per-camera sums ---------------------------------------------------------------------------

def sums_f64(t64, cam_start):
    """t64 [n,C] in list order -> ([E,C] sums, [E,C] sums of magnitudes), float64."""
    E = len(cam_start) - 1
    s, a = np.zeros((E, t64.shape[1])), np.zeros((E, t64.shape[1]))
    for c in range(E):
        seg = t64[cam_start[c]:cam_start[c + 1]]
        s[c] = seg.sum(0)
        a[c] = np.abs(seg).sum(0)
    return s, a


def sum_tol(cam_start, abs_sums, mag_sums):
    cnt = np.diff(np.asarray(cam_start, dtype=np.int64))
    own = TERM_TOL * mag_sums
    return own + pm.gamma(cnt + 2)[:, None] * (abs_sums + own)


# ---- the correction --------------------------------------------------------------------------------

def compose64(base_K, base_dist, gamma, group, cx_by_new_fx=False):
    """-> (K' [E,3,3], dist' [E,4]) float64; float32 inputs are taken exactly.  The flag is the
    mutant of the CPU test: the centre shifted in units of fx' instead of the base fx."""
    K = np.asarray(base_K, dtype=np.float64).copy()
    E = K.shape[0]
    D = np.zeros((E, 4)) if base_dist is None else np.asarray(base_dist, dtype=np.float64).copy()
    c = np.asarray(gamma, dtype=np.float64)
    group = np.asarray(group)
    for e in range(E):
        g = int(group[e])
        if g < 0 or g >= c.shape[0]:
            continue
        fx, fy = K[e, 0, 0], K[e, 1, 1]
        K[e, 0, 0] = fx * np.exp(c[g, 0])
        K[e, 1, 1] = fy * np.exp(c[g, 1])
        K[e, 0, 2] += c[g, 2] * (K[e, 0, 0] if cx_by_new_fx else fx)
        K[e, 1, 2] += c[g, 3] * (K[e, 1, 1] if cx_by_new_fx else fy)
        D[e] += c[g, 4:]
    return K, D


def compose_bwd64(base_K, gamma, group, learn, d_K, d_dist):
    """-> (d_gamma [G,8], sums of magnitudes [G,8], images per group [G]) float64."""
    K = np.asarray(base_K, dtype=np.float64)
    c = np.asarray(gamma, dtype=np.float64)
    G, E = c.shape[0], K.shape[0]
    dK = np.zeros((E, 3, 3)) if d_K is None else np.asarray(d_K, dtype=np.float64)
    dD = np.zeros((E, 4)) if d_dist is None else np.asarray(d_dist, dtype=np.float64)
    out, mag, cnt = np.zeros((G, 8)), np.zeros((G, 8)), np.zeros(G, dtype=np.int64)
    for e in range(E):
        g = int(group[e])
        if g < 0 or g >= G:
            continue
        row = np.array([dK[e, 0, 0] * K[e, 0, 0] * np.exp(c[g, 0]), dK[e, 1, 1] * K[e, 1, 1] * np.exp(c[g, 1]),
                        dK[e, 0, 2] * K[e, 0, 0], dK[e, 1, 2] * K[e, 1, 1], *dD[e]])
        out[g] += row
        mag[g] += np.abs(row)
        cnt[g] += 1
    if learn is not None:
        keep = (np.asarray(learn) != 0).astype(np.float64)
        out, mag = out * keep, mag * keep
    return out, mag, cnt


def compose_bwd_tol(ref, mag, cnt):
    """f64 inside, rounded once: one float32 ulp of the result, and the f64 sum's own error with room
    for exp (a few f64 ulps): (cnt + 8) 2^-52 sum |term|."""
    return pm.ulp32(ref) + (cnt[:, None] + 8) * 2.0 ** -52 * mag


# ---- calibration recovery on rays alone ------------------------------------------------------------

REC_H, REC_W = 47, 65
REC_K = np.array([[40.0, 0.0, lm.CX], [0.0, 40.0, lm.CY], [0.0, 0.0, 1.0]], dtype=np.float32)
REC_DIST = np.array([-0.1, 0.02, 1e-3, -2e-3], dtype=np.float32)
REC_GAMMA = np.array([0.03, -0.02, 0.05, -0.04, 0.03, -0.01, 2e-3, 1e-3])
REC_STEPS, REC_BATCH, REC_LR = 300, 512, 1e-3


def recovery_pixels(step, seed=23):
    rng = np.random.default_rng(seed + step)
    return np.stack([rng.integers(0, REC_H, REC_BATCH), rng.integers(0, REC_W, REC_BATCH)],
                    1).astype(np.int32)


def recovery_dirs64(gamma, ij):
    """Camera-frame directions [n,3] under the correction `gamma` [8], float64 (30 Newton steps).
    lens_model reads the calibration as float32, so K' and k' are rounded to it as the device's are."""
    K, D = compose64(REC_K[None], REC_DIST[None], np.asarray(gamma)[None], [0])
    K32, D32 = K[0].astype(np.float32), D[0].astype(np.float32)
    return lm.camera_dirs(D32, ij, K32, np.float64, steps=30), K32, D32


def recovery_loss_and_grad(gamma, ij, target):
    """mean over the rays of |dirs(gamma) - target|^2 and its gradient in gamma [8], through
    ray_terms (R = I) and compose_bwd64."""
    dirs, K32, D32 = recovery_dirs64(gamma, ij)
    n = ij.shape[0]
    diff = dirs - target
    loss = float((diff * diff).sum(1).mean())
    d_d = 2.0 * diff / n
    # (ray_terms takes float32 gradients; this experiment wants them exact)
    hi = d_d.astype(np.float32)
    lo = (d_d - hi.astype(np.float64)).astype(np.float32)
    eye = np.tile(np.eye(3, dtype=np.float32)[None], (n, 1, 1))
    t = sum(ray_terms(ij, K32, D32, dirs[:, 0], -dirs[:, 1], eye, part, np.float64)[0] for part in (hi, lo))
    d_intr = t.sum(0)
    d_K = np.zeros((1, 3, 3))
    d_K[0, 0, 0], d_K[0, 1, 1], d_K[0, 0, 2], d_K[0, 1, 2] = d_intr[:4]
    g, _, _ = compose_bwd64(REC_K[None], np.asarray(gamma)[None], [0], None, d_K, d_intr[None, 4:])
    return loss, g[0]
