"""Inputs, numpy restatements and tolerances for the lens-distortion tests (f2n_gen_rays_dist,
f2n_gen_rays_dist_bwd, f2n_project_points).  No tests in here: tests/test_lens_cpu.py re-measures the
two tolerances on the CPU, tests/test_gpu_lens.py holds the HIP kernels to them.

Model (include/f2nerf_hip.h, camera.hiph): OpenCV's k1, k2, p1, p2 on the normalised image point, y
down.  `distort` is the forward model; `undistort` is the kernel's inverse, Newton on the 2x2 system
from (xd, yd), written operation by operation as the device code is (no fused multiply-add), in the
dtype it is given: float32 with 8 steps is the restatement of the kernel, float64 with 30 steps is
the reference.

TOL, for an undistorted coordinate: the largest |f32 restatement - f64 reference| over the image and
the five coefficient sets below is E32 = 2.16e-7 (test_lens_cpu.py::test_tol_covers_f32_restatement
recomputes it); TOL = 4 * E32 rounded up to a power of two = 2^-20.  The factor 4 absorbs the
operation order and contraction that numpy cannot reproduce.  Never measured on the kernel.

PIX_TOL, for a projected pixel coordinate: the same recipe on `project`, on the points of
`projection_case()`: the largest |f32 - f64| there is 7.71e-6 of a pixel (pixel coordinates reach 65,
where half a float32 ulp is 3.8e-6), PIX_TOL = 2^-14 (test_lens_cpu.py::
test_pix_tol_covers_f32_restatement).  The float64 projection of those float32 points lies within
4.4e-6 of the pixel centres they were built from.
"""
import numpy as np

H, W = 47, 65                      # 3055 rays: ends inside a 256-thread block
FX, FY, CX, CY = 40.0, 42.0, 32.3, 23.1
SETS = (
    (-0.3, 0.1, 1e-3, -5e-4),
    (0.2, -0.05, -2e-3, 1e-3),
    (-0.1, 0.01, 0.0, 0.0),
    (0.0, 0.0, 5e-3, 5e-3),
    (-0.35, 0.15, 2e-3, 2e-3),
)
TOL = 2.0 ** -20
PIX_TOL = 2.0 ** -14
U = 2.0 ** -24
NEWTON_STEPS = 8
MIN_DET = 1e-8


def intrinsic():
    """[3,3] float32: the values the kernels are given."""
    return np.array([[FX, 0.0, CX], [0.0, FY, CY], [0.0, 0.0, 1.0]], dtype=np.float32)


def pixels():
    """(row, col) of every pixel, row-major: [H*W, 2] int32."""
    px = np.arange(H * W)
    return np.stack([px // W, px % W], 1).astype(np.int32)


def _coeffs(k, dtype):
    k = np.asarray(k, dtype=np.float32).astype(dtype)  # the kernels read float32 coefficients
    return k[..., 0], k[..., 1], k[..., 2], k[..., 3]


def normalised(ij, K, dtype):
    """Pixel -> distorted normalised point with the kernel's expression, in `dtype`."""
    K = np.asarray(K, dtype=np.float32).astype(dtype)
    row, col = ij[:, 0].astype(dtype), ij[:, 1].astype(dtype)
    half = dtype(0.5)
    xd = ((col + half) - K[..., 0, 2]) / K[..., 0, 0]
    yd = ((row + half) - K[..., 1, 2]) / K[..., 1, 1]
    return xd, yd


def distort(k, x, y, dtype):
    k1, k2, p1, p2 = _coeffs(k, dtype)
    one, two = dtype(1), dtype(2)
    xx, yy, xy = x * x, y * y, x * y
    r2 = xx + yy
    rad = one + r2 * (k1 + k2 * r2)
    xd = x * rad + two * p1 * xy + p2 * (r2 + two * xx)
    yd = y * rad + p1 * (r2 + two * yy) + two * p2 * xy
    return xd, yd


def undistort(k, xd, yd, dtype, steps=NEWTON_STEPS):
    k1, k2, p1, p2 = _coeffs(k, dtype)
    one, two, six = dtype(1), dtype(2), dtype(6)
    big = np.finfo(dtype).max
    x, y = xd.astype(dtype).copy(), yd.astype(dtype).copy()
    with np.errstate(all="ignore"):
        for _ in range(steps):
            xx, yy, xy = x * x, y * y, x * y
            r2 = xx + yy
            rad = one + r2 * (k1 + k2 * r2)
            ex = (x * rad + two * p1 * xy + p2 * (r2 + two * xx)) - xd
            ey = (y * rad + p1 * (r2 + two * yy) + two * p2 * xy) - yd
            dr = k1 + two * k2 * r2
            a = rad + two * xx * dr + two * p1 * y + six * p2 * x
            b = two * xy * dr + two * p1 * x + two * p2 * y
            d = rad + two * yy * dr + six * p1 * y + two * p2 * x
            det = a * d - b * b
            nx = x - (d * ex - b * ey) / det
            ny = y - (a * ey - b * ex) / det
            ok = (np.abs(det) > dtype(MIN_DET)) & (np.abs(nx) <= big) & (np.abs(ny) <= big)
            x = np.where(ok, nx, x)
            y = np.where(ok, ny, y)
    return x, y, det


def camera_dirs(k, ij, K, dtype, steps=NEWTON_STEPS):
    """Camera-frame directions (x, -y, -1): [n,3]."""
    xd, yd = normalised(ij, K, dtype)
    x, y, _ = undistort(k, xd, yd, dtype, steps)
    return np.stack([x, -y, -np.ones_like(x)], 1)


def reference_dirs(k, ij, K):
    return camera_dirs(k, ij, K, np.float64, steps=30)


def project(points, poses, K, k, dtype):
    """World points -> (pix [n,2] (row, col), valid [n]).  poses [n,3|4,4] or [3|4,4], K and k per
    point or shared; operation order of project_points_kernel."""
    P = np.asarray(poses, dtype=np.float32).astype(dtype)
    Kd = np.asarray(K, dtype=np.float32).astype(dtype)
    p = np.asarray(points, dtype=np.float32).astype(dtype)
    dx, dy, dz = p[:, 0] - P[..., 0, 3], p[:, 1] - P[..., 1, 3], p[:, 2] - P[..., 2, 3]
    cx = P[..., 0, 0] * dx + P[..., 1, 0] * dy + P[..., 2, 0] * dz
    cy = P[..., 0, 1] * dx + P[..., 1, 1] * dy + P[..., 2, 1] * dz
    cz = P[..., 0, 2] * dx + P[..., 1, 2] * dy + P[..., 2, 2] * dz
    valid = cz < 0
    with np.errstate(all="ignore"):
        depth = -cz
        xd, yd = distort(k, cx / depth, -cy / depth, dtype)
        col = xd * Kd[..., 0, 0] + Kd[..., 0, 2]
        row = yd * Kd[..., 1, 1] + Kd[..., 1, 2]
    pix = np.where(valid[:, None], np.stack([row, col], 1), dtype(0))
    return pix, valid.astype(np.int32)


def rotations(n, seed):
    """n proper rotations (QR of a Gaussian), float32."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        q, r = np.linalg.qr(rng.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out.append(q)
    return np.stack(out).astype(np.float32)


def general_case(rows=3, seed=7):
    """Five cameras carrying the five sets, each with its own pose, and a random camera per ray over
    the full pixel list.  -> dict of float32 / int32 arrays and the float64 world rays."""
    rng = np.random.default_rng(seed)
    E = len(SETS)
    R = rotations(E, seed)
    t = (rng.standard_normal((E, 3)) * 0.2).astype(np.float32)
    poses = np.concatenate([R, t[:, :, None]], 2)
    if rows == 4:
        last = np.tile(np.array([[[0.0, 0.0, 0.0, 1.0]]], dtype=np.float32), (E, 1, 1))
        poses = np.concatenate([poses, last], 1)
    ij = pixels()
    cam = rng.integers(0, E, ij.shape[0]).astype(np.int32)
    K = np.tile(intrinsic()[None], (E, 1, 1))
    dist = np.asarray(SETS, dtype=np.float32)
    v = np.zeros((ij.shape[0], 3))
    for c in range(E):
        m = cam == c
        v[m] = reference_dirs(SETS[c], ij[m], K[c])
    Rr = poses[cam][:, :3, :3].astype(np.float64)
    dirs = np.einsum("nab,nb->na", Rr, v)
    return dict(poses=poses, K=K, dist=dist, cam=cam, ij=ij, v=v, R=Rr, dirs=dirs,
                origins=poses[cam][:, :3, 3].astype(np.float64))


def projection_case():
    """Points o + s d, s in {0.5, 2}, on the float64 rays of general_case(), as the float32 the
    kernel is given; each with its pixel centre (i + .5, j + .5) and its camera."""
    c = general_case()
    pts, centre, cam = [], [], []
    for s in (0.5, 2.0):
        pts.append((c["origins"] + s * c["dirs"]).astype(np.float32))
        centre.append(c["ij"].astype(np.float64) + 0.5)
        cam.append(c["cam"])
    return dict(points=np.concatenate(pts), centre=np.concatenate(centre),
                cam=np.concatenate(cam), poses=c["poses"], K=c["K"], dist=c["dist"])


def pow2_ceil(v):
    return 2.0 ** int(np.ceil(np.log2(v)))
