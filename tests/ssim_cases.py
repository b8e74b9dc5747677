"""The image pairs the SSIM tests share, and their model results computed once (read-only).

  * the pairs of tests/golden/ssim/ssim_reference.npz with the reference's own results (a folder of
    its own: tests/test_oracle_cpu.py regenerates every .npz directly under tests/golden from the
    oracle, and this one is a recording of the reference);
  * stacks of B = 1, 2, 3 pairs of one size;
  * map sides T-1, T, T+1, 2T+1 around the kernel's tile T = 16 in either direction, and h or w of
    exactly 11 (one map row or column).
"""
import functools
import os

import numpy as np

from tests import ssim_model as M

_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim", "ssim_reference.npz")

FIXTURE_NAMES = (
    "noise_11x11", "noise_11x12", "noise_12x11", "noise_16x16", "noise_26x43", "noise_33x70",
    "ramp_noise", "black_self", "flat07_self", "flat02_flat08", "flat_noise", "ramp_negative",
    "quantised")
STACKS = (("noise_26x43",), ("ramp_noise", "flat02_flat08"), ("quantised", "flat_noise", "ramp_negative"))
T = M.TILE
# (h, w): map sides h - 10, w - 10
EDGE_SHAPES = tuple((m + 10, 21) for m in (T - 1, T, T + 1, 2 * T + 1)) + \
              tuple((21, m + 10) for m in (T - 1, T, T + 1, 2 * T + 1)) + ((11, 29), (29, 11), (43, 43))
BWD_SHAPES = ((11, 11), (12, 17)) + EDGE_SHAPES


@functools.lru_cache(maxsize=None)
def _npz():
    z = np.load(_NPZ)
    return {k: z[k] for k in z.files}


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def fixture_pair(name):
    z = _npz()
    return _frozen(z[name + ".pred"]), _frozen(z[name + ".gt"])


def fixture_ref(name):
    z = _npz()
    return float(z[name + ".ssim"]), z[name + ".map"]


@functools.lru_cache(maxsize=None)
def noise_pair(h, w):
    """a correlated pair: gt, and gt plus noise, in float32"""
    g = np.random.default_rng(7919 * h + w)
    y = g.random((h, w, 3))
    x = np.clip(y + 0.1 * g.standard_normal((h, w, 3)), 0.0, 1.0)
    return _frozen(x.astype(np.float32)), _frozen(y.astype(np.float32))


@functools.lru_cache(maxsize=None)
def forward_models(key, clip):
    """key: a fixture name or an (h, w) -> dict of the f64 and f32 models' results for one pair"""
    x, y = fixture_pair(key) if isinstance(key, str) else noise_pair(*key)
    s64, m64 = M.ssim64(x, y, clip)
    r32 = M.ssim32(x, y, clip, want_gmaps=not clip)
    return dict(x=x, y=y, ssim64=s64, map64=_frozen(m64), ssim32=r32["ssim"],
                map32=_frozen(r32["map"]), gmaps32=None if clip else _frozen(r32["gmaps"]))


@functools.lru_cache(maxsize=None)
def backward_models(key, d_ssim):
    f = forward_models(key, False)
    return dict(g64=_frozen(M.grad64(f["x"], f["y"], d_ssim)),
                g32=_frozen(M.bwd32(f["x"], f["y"], f["gmaps32"], d_ssim)))


def allowed(err32, scale=1.0):
    """the bound of the GPU tests: four times the float32 model's own error against the float64
    model on the same case, plus 4 * 2^-24 (of `scale`)"""
    return 4.0 * err32 + 4.0 * 2.0 ** -24 * scale
