"""The camera-visibility carve of the occupancy bitfield (include/f2nerf_hip.h: f2n_occ_mark_rays,
f2n_occ_dilate, f2n_occ_count_add, f2n_occ_count_bits; host/occ_visibility.hpp) restated in numpy.  No
tests in here: tests/test_occ_visibility_model_cpu.py checks the model on the CPU,
tests/test_gpu_occ_visibility.py holds the kernels and the host functions to it.

Definition.  Camera c marks cell i when a walked pixel (row, col) of c and a k < n_steps exist such that
VALIDATE sample k of the pixel's ray contracts into cell i:

    (u, v)  = camera.hiph's pixel -> direction (tests/lens_model.py: pixel centre at +0.5, eight Newton
              steps when the camera's coefficients are not all zero, the pinhole expression otherwise)
    d_a     = fmaf(P[a][2], -1, fmaf(P[a][1], v, P[a][0] u)),  o = P[:, 3]
    p_k     = o + d^ ((k + 1) step)        (tests/ray_walk_model.py: load_ray, make_stride, no noise)
    x_k     = contract(p_k)                (hash_grid.hiph: contract_point)
    cell    = tests/util.py::_cells(x_k)   (a non-finite x_k marks nothing)

Walked rows at pixel stride s: min(a s, h - 1) for a = 0 .. ceil((h - 1) / s); columns likewise.  With
a mask [E, h, w] a pixel whose entry is 0 is skipped.

    dilate(B)  bit (x, y, z) = OR of B over |dx|, |dy|, |dz| <= 1 inside [0, G)^3 (no wrap-around)
    seen_c = dilate^d(marks of c),  count = min(255, sum_c seen_c),  visible = count >= min_views

What is expected in bits and what is not.  The float32 restatement (dtype = float32) follows the device
code operation by operation, but numpy has no fused multiply-add: the three fmaf of the rotation and the
two under each square root are emulated through float64 (a double rounding that can differ in the last
bit), and the device's sqrtf / division are correctly rounded only to within an ulp.  A contracted
coordinate lies in (-2, 2), so such differences move it by a few 2^-23; they can change the cell only of
a sample that close to a cell face.  Hence two sets per camera (camera_mark_bounds):

    sure   cells marked by a sample farther than FACE_TOL from every face of its cell
    maybe  every cell within FACE_TOL of a sample (the sample's own cell and the neighbours across the
           faces it is close to)

and the claim sure <= marks of the kernel <= maybe.  FACE_TOL = 1e-4 is the figure of the feature's
definition; it is 400 times the 2^-22 spacing of float32 just below 2, chosen from the number format and
never measured on a kernel.  Bit-exact agreement is asserted elsewhere, against the chain of kernels
that already produce these samples (f2n_gen_rays_dist, f2n_sample_rays, f2n_contract_fwd).
Dilation is monotone, so the bounds carry over: dilate^d(sure) <= seen_c <= dilate^d(maybe).
"""
import numpy as np

from tests import lens_model as LM
from tests import ray_walk_model as RW
from tests.util import _cells

F32 = np.float32
FACE_TOL = 1e-4

# the shapes of the tests: three cameras of 12 x 20 pixels, G = 32, step = 1/32
H, W, G = 12, 20, 32
STEP = 1.0 / 32
S_TRAIN, N_STEPS = 64, 96            # n_steps = ceil(1.5 S)


def walked(n, s):
    """rows (or columns) walked at pixel stride s: the last one always"""
    return np.minimum(np.arange((n - 1 + s - 1) // s + 1) * s, n - 1).astype(np.int64)


def walked_pixels(h, w, s, mask=None):
    """(row, col) int32 [n, 2] in row-major order of the walked grid, masked pixels dropped"""
    rr, cc = np.meshgrid(walked(h, s), walked(w, s), indexing="ij")
    ij = np.stack([rr.reshape(-1), cc.reshape(-1)], 1).astype(np.int32)
    if mask is not None:
        ij = ij[np.asarray(mask)[ij[:, 0], ij[:, 1]] != 0]
    return ij


def scene(seed=0, outside=True):
    """Three cameras: poses [3,3,4], K [3,3,3], dist [3,4] float32.  Camera 0 is a pinhole inside the
    unit ball, camera 1 has non-zero k1, k2, p1, p2, camera 2 lies outside the unit ball (|t| > 1)
    when `outside`.  seed 0 is the GPU tests' scene; other seeds are the random scenes of the
    soundness test."""
    rng = np.random.default_rng(1000 + seed)
    t = rng.uniform(-0.5, 0.5, (3, 3))
    if outside:
        t[2] = np.array([1.2, 0.9, -0.8]) + rng.uniform(-0.1, 0.1, 3)
    # every camera looks (down its -z axis) at a point near the origin, so the frusta overlap
    R = np.zeros((3, 3, 3))
    for c in range(3):
        z = t[c] - rng.uniform(-0.15, 0.15, 3)
        z /= np.linalg.norm(z)
        x = np.cross(rng.standard_normal(3), z)
        x /= np.linalg.norm(x)
        R[c] = np.stack([x, np.cross(z, x), z], 1)
    poses = np.concatenate([R, t.astype(F32)[:, :, None]], 2).astype(F32)
    K = np.zeros((3, 3, 3), dtype=F32)
    for c in range(3):
        f = 14.0 + 3.0 * c + rng.uniform(0.0, 1.0)
        K[c] = np.array([[f, 0, W / 2 + rng.uniform(-0.7, 0.7)],
                         [0, f * 1.05, H / 2 + rng.uniform(-0.7, 0.7)], [0, 0, 1]], dtype=F32)
    dist = np.zeros((3, 4), dtype=F32)
    dist[1] = LM.SETS[0]
    return dict(poses=poses, K=K, dist=dist)


def poses44(poses):
    """[n,3,4] -> [n,4,4]"""
    last = np.tile(np.array([[[0, 0, 0, 1]]], dtype=F32), (poses.shape[0], 1, 1))
    return np.concatenate([poses, last], 1)


def _fma(a, b, c, dtype):
    if dtype == F32:
        return RW._fma32(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    return a * b + c


def ray_dirs(pose, K, k, ij, dtype):
    """world directions [n,3] (not normalised) of pixels ij of one camera, in `dtype`"""
    if not np.any(np.asarray(k, dtype=F32) != 0):
        xd, yd = LM.normalised(ij, K, dtype)       # the pinhole expression: u = xd, v = -yd
        u, v = xd, -yd
    else:
        cd = LM.camera_dirs(k, ij, K, dtype, steps=LM.NEWTON_STEPS if dtype == F32 else 30)
        u, v = cd[:, 0], cd[:, 1]
    P = np.asarray(pose, dtype=F32).astype(dtype)
    return np.stack([_fma(P[a, 2], dtype(-1) * np.ones_like(u), _fma(P[a, 1], v, P[a, 0] * u, dtype),
                          dtype) for a in range(3)], 1).astype(dtype)


def contract(p, dtype):
    """contract_point on [..., 3]: the identity inside the unit ball (NaN at the origin), else
    ((2 - 1/|p|) p) / |p|"""
    p = np.asarray(p, dtype=dtype)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(all="ignore"):
        if dtype == F32:
            nrm = np.sqrt(RW._fma32(z, z, RW._fma32(y, y, x * x)))
        else:
            nrm = np.sqrt(z * z + (y * y + x * x))
        s = dtype(2) - dtype(1) / nrm
        out = np.where((nrm <= 1)[..., None], p, (s[..., None] * p) / nrm[..., None])
        out = np.where((nrm == 0)[..., None], dtype(np.nan), out)
    return out.astype(dtype)


def validate_points(pose, K, k, ij, n_steps, step):
    """contracted VALIDATE samples [n_pixels, n_steps, 3] of pixels ij of one camera, float32"""
    d = ray_dirs(pose, K, k, ij, F32)
    o = np.broadcast_to(np.asarray(pose, dtype=F32)[:3, 3], d.shape)
    return contract(RW.walk_f32(o, d, None, n_steps, step)["pts"], F32)


def validate_points64(pose, K, k, ij, n_steps, step):
    """the same in float64 from the same float32 inputs (30 Newton steps; the direction stays float64,
    which ray_walk_model.walk_f64 would round to float32 first)"""
    d = ray_dirs(pose, K, k, ij, np.float64)
    o = np.asarray(pose, dtype=F32)[:3, 3].astype(np.float64)
    dn = d / np.sqrt((d * d).sum(1))[:, None]
    t = np.arange(1, n_steps + 1, dtype=np.float64) * float(F32(step))
    return contract(o[None, None, :] + dn[:, None, :] * t[None, :, None], np.float64)


def marks_of_points(x, G):
    """bool [G^3]: the cells of the finite rows of x [n, 3]"""
    x = np.asarray(x).reshape(-1, 3)
    fin = np.isfinite(x).all(1)
    out = np.zeros(G ** 3, dtype=bool)
    out[_cells(x[fin].astype(F32), G)] = True
    return out


def face_distance(x, G):
    """distance of each coordinate of x to the nearest face of its cell, [..., 3] (float64)"""
    g = (np.asarray(x, dtype=np.float64) + 2.0) * (G / 4.0)
    fr = g - np.floor(g)
    return np.minimum(fr, 1.0 - fr) * (4.0 / G)


def camera_marks(sc, cam, G, n_steps, step, pixel_stride=1, mask=None, h=H, w=W):
    """bool [G^3]: the float32 restatement's marks of camera `cam` (mask: [h, w] of that camera)"""
    ij = walked_pixels(h, w, pixel_stride, mask)
    if ij.shape[0] == 0:
        return np.zeros(G ** 3, dtype=bool)
    return marks_of_points(
        validate_points(sc["poses"][cam], sc["K"][cam], sc["dist"][cam], ij, n_steps, step), G)


def camera_mark_bounds(sc, cam, G, n_steps, step, pixel_stride=1, mask=None, h=H, w=W,
                       tol=FACE_TOL):
    """(sure, maybe) bool [G^3] of the module docstring, from the float32 restatement's samples"""
    sure, maybe = np.zeros(G ** 3, dtype=bool), np.zeros(G ** 3, dtype=bool)
    ij = walked_pixels(h, w, pixel_stride, mask)
    if ij.shape[0] == 0:
        return sure, maybe
    x = validate_points(sc["poses"][cam], sc["K"][cam], sc["dist"][cam], ij, n_steps, step)
    x = x.reshape(-1, 3)
    x = x[np.isfinite(x).all(1)].astype(np.float64)
    far = (face_distance(x, G) > tol).all(1)
    sure[_cells(x[far].astype(F32), G)] = True
    for sx in (-tol, 0.0, tol):
        for sy in (-tol, 0.0, tol):
            for sz in (-tol, 0.0, tol):
                maybe[_cells((x + np.array([sx, sy, sz])).astype(F32), G)] = True
    return sure, maybe


def dilate(bits, G, d=1):
    """bool [G^3] -> bool [G^3], d passes; nothing wraps around"""
    b = np.asarray(bits, dtype=bool).reshape(G, G, G)
    for _ in range(d):
        p = np.zeros((G + 2, G + 2, G + 2), dtype=bool)
        p[1:-1, 1:-1, 1:-1] = b
        out = np.zeros_like(b)
        for dz in range(3):
            for dy in range(3):
                for dx in range(3):
                    out |= p[dz:dz + G, dy:dy + G, dx:dx + G]
        b = out
    return b.reshape(-1)


def count_add(count, bits):
    """uint8 [G^3]: min(255, count + bit)"""
    return np.minimum(count.astype(np.int64) + np.asarray(bits, dtype=np.int64), 255).astype(np.uint8)


def view_counts(per_camera_marks, G, d):
    count = np.zeros(G ** 3, dtype=np.uint8)
    for m in per_camera_marks:
        count = count_add(count, dilate(m, G, d))
    return count


def visible(per_camera_marks, G, d, min_views):
    return view_counts(per_camera_marks, G, d) >= min_views


def train_points(sc, cam, S, step, seed, h=H, w=W):
    """contracted TRAIN samples [h w, S, 3] (float32) of every pixel of one camera: multipliers
    U[0,1) + 0.5, one row per ray; returns (x, noise) so that a GPU test can replay the draw"""
    ij = walked_pixels(h, w, 1)
    rng = np.random.default_rng(seed)
    noise = (rng.random((ij.shape[0], S), dtype=F32) + F32(0.5)).astype(F32)
    d = ray_dirs(sc["poses"][cam], sc["K"][cam], sc["dist"][cam], ij, F32)
    o = np.broadcast_to(sc["poses"][cam][:3, 3], d.shape)
    pts = RW.walk_f32(o, d, noise, S, step)["pts"]
    return contract(pts, F32), noise


def outside_fraction(x, bits, G):
    """share of the finite samples x [..., 3] whose cell is not in bits"""
    x = np.asarray(x).reshape(-1, 3)
    x = x[np.isfinite(x).all(1)]
    return float((~np.asarray(bits, dtype=bool)[_cells(x.astype(F32), G)]).mean()), x.shape[0]
