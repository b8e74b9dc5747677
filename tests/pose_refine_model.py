"""Float64 and float32 restatements for the pose-refinement tests (f2n_cam_pose_grad, f2n_pose_compose,
f2n_pose_compose_bwd).  No tests in here: tests/test_pose_refine_cpu.py checks the bound on the CPU,
tests/test_gpu_pose_refine.py holds the HIP kernels to it.

The per-camera sums.  Ray r contributes twelve terms, row-major [3,4]:
    term[r, 4 i + j] = d_rays_d[r, i] * v_r[j]  (j < 3),    term[r, 4 i + 3] = d_rays_o[r, i]
and d_pose_c is the sum of the terms of camera c's rays.

The bound, per element:  tol_c = gamma(cnt_c + 2) * sum_r |term_r|,  gamma(k) = k u / (1 - k u),
u = 2^-24, the magnitudes summed in float64.  A float32 sum of cnt terms in ANY order (serial, lane
partials then a tree, partials of pieces) has at most cnt - 1 roundings on the path of any term, the
product adds one, and one is kept in hand: (1 + u)^(cnt + 1) - 1 <= gamma(cnt + 2) (Higham, Accuracy
and Stability of Numerical Algorithms, lemma 3.1).  Derived, never measured on the kernel.

The partition of f2n_cam_pose_grad (pose_refine.hip): the camera-sorted list is cut into pieces of
PIECE positions counted from the start of the list; camera c meets a piece in a run; a run shorter than
LANE_RUN is summed serially, a longer one in 64-position strides from its start into 64 lane
accumulators that the DPP tree of wave_incl_scan then adds; a camera that spans pieces adds its runs'
partials in piece order.
"""
import numpy as np
import torch

U = 2.0 ** -24
PIECE = 1024
LANE_RUN = 32
WAVE = 64


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


# ---- the per-camera sums ---------------------------------------------------------------------------

def terms(d_o, d_d, v, dtype):
    """[n,12] in `dtype`, each product rounded once to it."""
    d_o, d_d, v = (np.asarray(a, dtype=np.float32).astype(dtype) for a in (d_o, d_d, v))
    t = np.empty((d_o.shape[0], 12), dtype=dtype)
    for i in range(3):
        for j in range(3):
            t[:, 4 * i + j] = d_d[:, i] * v[:, j]
        t[:, 4 * i + 3] = d_o[:, i]
    return t


def cam_bounds(cam_sorted, E):
    """cam_start [E+1] of non-decreasing camera ids."""
    return np.searchsorted(cam_sorted, np.arange(E + 1), side="left").astype(np.int64)


def sums_f64(t64, cam_start):
    """t64 [n,12] in list order -> ([E,12] sums, [E,12] sums of magnitudes), float64."""
    E = len(cam_start) - 1
    s, a = np.zeros((E, 12)), np.zeros((E, 12))
    for c in range(E):
        seg = t64[cam_start[c]:cam_start[c + 1]]
        s[c] = seg.sum(0)
        a[c] = np.abs(seg).sum(0)
    return s, a


def tol(cam_start, abs_sums):
    cnt = np.diff(np.asarray(cam_start, dtype=np.int64))
    return gamma(cnt + 2)[:, None] * abs_sums


def runs_of(cam_start, c):
    """The runs of camera c: [(s, e)] in piece order."""
    s, e = int(cam_start[c]), int(cam_start[c + 1])
    out = []
    while s < e:
        stop = min(e, (s // PIECE + 1) * PIECE)
        out.append((s, stop))
        s = stop
    return out


def serial_sum32(t32):
    acc = np.zeros(12, dtype=np.float32)
    for row in t32:
        acc = acc + row
    return acc


def wave_sum32(v):
    """Lane 63 of wave_incl_scan (common.hiph) over v [64,12] float32."""
    v = v.astype(np.float32).copy()
    lane = np.arange(WAVE)
    for k in (1, 2, 4, 8):  # row_shr:k inside each row of 16
        src = np.zeros_like(v)
        src[k:] = v[:-k]
        src[(lane % 16) < k] = 0.0
        v = v + src
    add = np.zeros_like(v)  # row_bcast15, rows 1 and 3
    add[16:32] = v[15]
    add[48:64] = v[47]
    v = v + add
    add = np.zeros_like(v)  # row_bcast31, rows 2 and 3
    add[32:64] = v[31]
    v = v + add
    return v[63]


def run_sum32(t32):
    """One run as the piece kernel adds it."""
    if len(t32) < LANE_RUN:
        return serial_sum32(t32)
    lanes = np.zeros((WAVE, 12), dtype=np.float32)
    for p0 in range(0, len(t32), WAVE):
        blk = t32[p0:p0 + WAVE]
        lanes[:len(blk)] = lanes[:len(blk)] + blk
    return wave_sum32(lanes)


def sums32_serial(t32, cam_start):
    E = len(cam_start) - 1
    return np.stack([serial_sum32(t32[cam_start[c]:cam_start[c + 1]]) for c in range(E)])


def sums32_pieces(t32, cam_start):
    E = len(cam_start) - 1
    out = np.zeros((E, 12), dtype=np.float32)
    for c in range(E):
        parts = [run_sum32(t32[s:e]) for s, e in runs_of(cam_start, c)]
        if parts:
            acc = parts[0]
            for p in parts[1:]:
                acc = acc + p
            out[c] = acc
    return out


# ---- float64 mutants: what a wrong partition would compute -----------------------------------------

def mutant_dropped_piece(t64, cam_start):
    """The partial of a spanning camera's second run is never added.  -> (sums, eligible cameras)"""
    s, _ = sums_f64(t64, cam_start)
    elig = []
    for c in range(len(cam_start) - 1):
        runs = runs_of(cam_start, c)
        if len(runs) >= 2:
            a, b = runs[1]
            s[c] -= t64[a:b].sum(0)
            elig.append(c)
    return s, elig


def mutant_full_last_stride(t64, cam_start):
    """The last, partial stride of a wavefront-summed run reads all 64 positions."""
    s, _ = sums_f64(t64, cam_start)
    n = len(t64)
    elig = []
    for c in range(len(cam_start) - 1):
        hit = False
        for a, b in runs_of(cam_start, c):
            if b - a >= LANE_RUN and (b - a) % WAVE and b < n:
                stop = min(n, a + -(-(b - a) // WAVE) * WAVE)
                s[c] += t64[b:stop].sum(0)
                hit = True
        if hit:
            elig.append(c)
    return s, elig


def mutant_boundary_ray(t64, cam_start):
    """Every inner boundary one position early: a camera's last ray goes to the next camera."""
    cs = np.asarray(cam_start).copy()
    inner = cs[1:-1]
    cs[1:-1] = np.where(inner > 0, inner - 1, inner)
    cs = np.maximum.accumulate(cs)
    s, _ = sums_f64(t64, cs)
    # eligible: the camera's set of positions changed (an empty camera that stays empty did not)
    elig = [c for c in range(len(cs) - 1)
            if (cs[c], cs[c + 1]) != (cam_start[c], cam_start[c + 1])
            and (cs[c + 1] > cs[c] or cam_start[c + 1] > cam_start[c])]
    return s, elig


# ---- the 40-camera case ----------------------------------------------------------------------------

COUNTS = (0, 1, 2, 63, 64, 65, 3, 127, 128, 129, 5, 1023, 1024, 1025, 7, 2047, 2048, 2049, 31, 3000,
          32, 33, 0, 9, 100, 500, 17, 1, 64, 96, 200, 11, 0, 640, 4, 50, 300, 2, 77, 0)
ZERO_CAM = 24  # its gradients are all zero


def counts_case(seed=3, heavy=True):
    """40 cameras with COUNTS rays each, pixels of the lens_model image, d_rays = randn * exp(3 randn)
    (heavy) or of one sign within a factor of two (the mutants' data: see test_pose_refine_cpu.py).
    -> dict(cam [n] sorted, ij [n,2], d_o, d_d [n,3] float32, E)."""
    from tests import lens_model as lm
    rng = np.random.default_rng(seed)
    E = len(COUNTS)
    cam = np.repeat(np.arange(E), COUNTS).astype(np.int32)
    n = cam.shape[0]
    ij = np.stack([rng.integers(0, lm.H, n), rng.integers(0, lm.W, n)], 1).astype(np.int32)
    if heavy:
        d = rng.standard_normal((n, 6)) * np.exp(3.0 * rng.standard_normal((n, 6)))
    else:
        d = 1.0 + rng.random((n, 6))
    d = d.astype(np.float32)
    d[cam == ZERO_CAM] = 0.0
    return dict(cam=cam, ij=ij, d_o=np.ascontiguousarray(d[:, :3]),
                d_d=np.ascontiguousarray(d[:, 3:]), E=E, n=n)


def pinhole_dirs32(ij, K):
    """v_r [n,3] float32 with gen_rays_kernel's operations (no contraction: the kernel's bits)."""
    K = np.asarray(K, dtype=np.float32)
    row, col = ij[:, 0].astype(np.float32), ij[:, 1].astype(np.float32)
    half = np.float32(0.5)
    u = ((col + half) - K[..., 0, 2]) / K[..., 0, 0]
    v = -(((row + half) - K[..., 1, 2]) / K[..., 1, 1])
    return np.stack([u, v, -np.ones_like(u)], 1).astype(np.float32)


# ---- the correction ------------------------------------------------------------------------------

def hat(w):
    """torch [..., 3] -> [..., 3, 3]"""
    z = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1),
                        torch.stack([w[..., 2], z, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def compose_ref(base, delta, fixed=None):
    """The reference: float64, Exp = torch.linalg.matrix_exp of the hat matrix, differentiable in
    delta.  base [E,3|4,4], delta [E,6] (float32 values are taken exactly) -> [E,3,4] float64."""
    b = base.detach().to(torch.float64)[:, :3, :]
    d = delta.to(torch.float64)
    if fixed is not None:
        d = d * (fixed.reshape(-1, 1) == 0).to(torch.float64)
    Rn = torch.linalg.matrix_exp(hat(d[:, :3])) @ b[:, :, :3]
    tn = b[:, :, 3] + d[:, 3:]
    return torch.cat([Rn, tn[:, :, None]], 2)


def rodrigues(w):
    """Closed-form Exp for numpy [3] float64 (|w| > 0)."""
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) / th * Kx + 2.0 * np.sin(th / 2) ** 2 / th ** 2 * (Kx @ Kx)


def ulp32(x):
    """One float32 ulp at |x| (numpy float64 in, float64 out)."""
    a = np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


def compose_case(rows=3, seed=5):
    """Cameras with |omega| in {0, 1e-9, 1e-6, 1e-4, 1e-3, 0.1, 1, 3.1} in random directions, three of
    each, tau up to 0.5; the first of each triple with tau = 0 (so that one camera is all zeros), the
    last of each triple fixed.  -> base [E,rows,4], delta [E,6] float32, fixed [E] int32, d_out."""
    from tests import lens_model as lm
    rng = np.random.default_rng(seed)
    mags = (0.0, 1e-9, 1e-6, 1e-4, 1e-3, 0.1, 1.0, 3.1)
    E = 3 * len(mags)
    R = lm.rotations(E, seed)
    t = (rng.standard_normal((E, 3)) * 0.3).astype(np.float32)
    base = np.concatenate([R, t[:, :, None]], 2)
    if rows == 4:
        last = np.tile(np.array([[[0.0, 0.0, 0.0, 1.0]]], dtype=np.float32), (E, 1, 1))
        base = np.concatenate([base, last], 1)
    delta = np.zeros((E, 6), dtype=np.float32)
    fixed = np.zeros(E, dtype=np.int32)
    for k, m in enumerate(mags):
        for q in range(3):
            e = 3 * k + q
            axis = rng.standard_normal(3)
            delta[e, :3] = (m * axis / np.linalg.norm(axis)).astype(np.float32)
            if q > 0:
                delta[e, 3:] = (rng.random(3) - 0.5).astype(np.float32)
            fixed[e] = 1 if q == 2 else 0
    d_out = rng.standard_normal((E, 3, 4)).astype(np.float32)
    return dict(base=np.ascontiguousarray(base), delta=delta, fixed=fixed, d_out=d_out, E=E)
