"""Level weights restated in numpy float64: the coarse-to-fine weights of a progress alpha, the number
of active levels, the schedule and the fold into the field head.  Written from the definitions in
include/f2nerf_hip.h (f2n_level_weights) and hash_3d_anchored.hpp, not from their code.  No tests."""
import math

import numpy as np


def weights(alpha, L):
    """w_l for l = 0 .. L-1, float64 (alpha > L is taken as L):
    0 for alpha - l <= 0, (1 - cos(pi (alpha - l))) / 2 inside the ramp, 1 from alpha - l >= 1 on."""
    alpha = min(float(alpha), float(L))
    d = alpha - np.arange(L, dtype=np.float64)
    ramp = (1.0 - np.cos(np.pi * np.clip(d, 0.0, 1.0))) / 2.0
    return np.where(d <= 0.0, 0.0, np.where(d >= 1.0, 1.0, ramp))


def active_levels(w):
    """1 + the index of the last non-zero weight"""
    nz = np.nonzero(np.asarray(w))[0]
    if nz.size == 0:
        raise ValueError("no active level")
    return int(nz[-1]) + 1


def alpha_at(it, L, start, end, base):
    u = (it - start) / (end - start) if end > start else (1.0 if it >= start else 0.0)
    return base + (L - base) * min(1.0, max(0.0, u))


def cols(lw, F):
    """lw (x) 1_F: the factor of each of the head's L * F columns"""
    return np.repeat(np.asarray(lw, dtype=np.float64), F)


def fold(W_h, lw, F):
    """W_eff = W_h diag(lw (x) 1_F)"""
    return np.asarray(W_h, dtype=np.float64) * cols(lw, F)[None, :]


def ulp32(x):
    """the spacing of float32 at |x| (the smallest normal's for tiny values)"""
    x = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), float(np.finfo(np.float32).tiny))
    return 2.0 ** (np.floor(np.log2(x)) - 23)


def ceil_alpha(alpha, L):
    return min(L, int(math.ceil(alpha)))
