"""Numpy model of f2n_robust_weights (robust_mask.hip): the weights of a trimmed colour loss with
patch-smoothed inlier masks.  No tests in here: tests/test_robust_model_cpu.py checks the model on the
CPU, tests/test_gpu_robust_weights.py holds the HIP kernels to it with array_equal.  Written from the
seven steps of the rule in include/f2nerf_hip.h and the header comment of robust_mask.hip, not from the
kernels: the residual is formed in float32 in the order of step 2, the k-th smallest is read off
np.sort, and steps 5 to 7 are integer counts against the float32 threshold products.

  1. considered iff m != 0 (no m: every ray); others get weight +0, label 0 and are not read
  2. eps = (d0*d0 + d1*d1) + d2*d2 in float32, d = colors - target; non-finite -> +inf
  3. N_c considered rays, k = min(N_c, max(1, ceil(float64(quantile) * N_c))), T = k-th smallest eps
     (N_c == 0: T = 0)
  4. w0 = isfinite(eps) & (eps <= T)
  5. W = cnt > 0 and float32(s) >= box_thresh * float32(cnt) over the considered pixels of the clipped
     3 x 3 window, s of them with w0
  6. R = cnt > 0 and float32(s) >= nbhd_thresh * float32(cnt) over the considered pixels of a block
     of nbhd x nbhd (edge blocks: what is left), s of them with W
  7. omega = considered & (w0 | W | R); weight = m (1 without m) where omega, else +0
stats = float32 {T, N_c, sum w0, sum omega}.
"""
import math

import numpy as np

F32 = np.float32
DEFAULTS = dict(quantile=0.5, box_thresh=0.5, nbhd_thresh=0.6, nbhd=8)


def residuals(colors, target, considered):
    """step 2 -> eps [n] float32; rays that are not considered hold +inf and are never looked at"""
    c = np.asarray(colors, dtype=F32)
    t = np.asarray(target, dtype=F32)
    eps = np.full(c.shape[0], np.inf, dtype=F32)
    with np.errstate(all="ignore"):
        d = (c[considered] - t[considered]).astype(F32)
        e = ((d[:, 0] * d[:, 0]).astype(F32) + (d[:, 1] * d[:, 1]).astype(F32)).astype(F32)
        e = (e + (d[:, 2] * d[:, 2]).astype(F32)).astype(F32)
    e[~np.isfinite(e)] = np.inf
    eps[considered] = e
    return eps


def rank(quantile, n_c):
    """step 3's k"""
    return min(n_c, max(1, int(math.ceil(float(np.float64(F32(quantile)) * np.float64(n_c))))))


def threshold(eps, considered, quantile):
    """step 3 -> (T float32, N_c, k)"""
    n_c = int(considered.sum())
    if n_c == 0:
        return F32(0), 0, 0
    k = rank(quantile, n_c)
    return np.sort(eps[considered])[k - 1], n_c, k


def box(w0, cons, P, box_thresh):
    """step 5 on [n_patches, P, P] bool arrays -> W"""
    n = w0.shape[0]
    cnt = np.zeros((n, P, P), dtype=np.int64)
    s = np.zeros((n, P, P), dtype=np.int64)
    pc = np.zeros((n, P + 2, P + 2), dtype=np.int64)
    pw = np.zeros((n, P + 2, P + 2), dtype=np.int64)
    pc[:, 1:-1, 1:-1] = cons
    pw[:, 1:-1, 1:-1] = w0 & cons
    for du in range(3):
        for dv in range(3):
            cnt += pc[:, du:du + P, dv:dv + P]
            s += pw[:, du:du + P, dv:dv + P]
    return (cnt > 0) & (s.astype(F32) >= (F32(box_thresh) * cnt.astype(F32)).astype(F32))


def vote(W, cons, P, nbhd, nbhd_thresh):
    """step 6 -> R spread over the pixels of its block, [n_patches, P, P] bool"""
    R = np.zeros_like(W)
    for u0 in range(0, P, nbhd):
        for v0 in range(0, P, nbhd):
            blk = (slice(None), slice(u0, min(u0 + nbhd, P)), slice(v0, min(v0 + nbhd, P)))
            cnt = cons[blk].sum(axis=(1, 2))
            s = (W[blk] & cons[blk]).sum(axis=(1, 2))
            r = (cnt > 0) & (s.astype(F32) >= (F32(nbhd_thresh) * cnt.astype(F32)).astype(F32))
            R[blk] = r[:, None, None]
    return R


def robust_weights(colors, target, ray_weight=None, P=0, nbhd=8, quantile=0.5, box_thresh=0.5,
                   nbhd_thresh=0.6):
    """-> dict(weight [n] f32, omega [n] u8, stats [4] f32, w0, W, R [n] bool, T, n_c, k)"""
    n = np.asarray(colors).shape[0]
    m = np.ones(n, dtype=F32) if ray_weight is None else np.asarray(ray_weight, dtype=F32)
    cons = m != 0
    eps = residuals(colors, target, cons)
    T, n_c, k = threshold(eps, cons, quantile)
    w0 = cons & np.isfinite(eps) & (eps <= T)
    W = np.zeros(n, dtype=bool)
    R = np.zeros(n, dtype=bool)
    if P > 0:
        assert n % (P * P) == 0 and 1 <= nbhd <= P
        shape = (n // (P * P), P, P)
        W3 = box(w0.reshape(shape), cons.reshape(shape), P, box_thresh)
        R = vote(W3, cons.reshape(shape), P, nbhd, nbhd_thresh).reshape(n)
        W = W3.reshape(n)
    omega = cons & (w0 | W | R)
    weight = np.where(omega, m, F32(0)).astype(F32)
    stats = np.array([T, n_c, w0.sum(), omega.sum()], dtype=F32)
    return dict(weight=weight, omega=omega.astype(np.uint8), stats=stats, w0=w0, W=W, R=R, T=F32(T),
                n_c=n_c, k=k, eps=eps)
