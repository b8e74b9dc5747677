"""Argument validation of f2n_ssim_fwd, f2n_ssim_bwd and f2n_draw_patches, their size query and
the filter taps: every call here has a fault or no work, so nothing is launched and no GPU is needed."""
import ctypes
import re

import numpy as np

from tests import ssim_model as M

INVALID, OK = -1, 0
FAKE = 0x1000


def _sweep(fn, good, cases):
    for faults, want in cases:
        args = list(good)
        for i, bad in faults.items():
            args[i] = bad
        assert fn(*args) == want, faults


def test_tile_and_workspace(capi):
    c = capi.lib().cdll
    text = open(capi.HEADER).read()
    assert int(re.search(r"#define\s+F2N_SSIM_TILE\s+(\d+)", text).group(1)) == M.TILE == 16
    ws = c.f2n_ssim_workspace_doubles
    assert ws(1, 11, 11) == 1 and ws(1, 26, 26) == 1 and ws(1, 27, 26) == 2 and ws(3, 27, 27) == 12
    assert ws(8, 1080, 1920) == 8 * 67 * 120 and ws(0, 11, 11) == 0
    for bad in ((1, 10, 11), (1, 11, 10), (-1, 11, 11), (65536, 11, 11), (1, 0, 0), (1, -11, 11)):
        assert ws(*bad) == 0


def test_filter_taps_are_the_models(capi):
    c = capi.lib().cdll
    taps = (ctypes.c_float * 11)()
    assert c.f2n_ssim_filter(taps) == OK and c.f2n_ssim_filter(None) == INVALID
    assert np.array_equal(np.array(taps[:], dtype=np.float32), M.filter32())


def test_ssim_fwd_validates_before_any_hip_work(capi):
    fn = capi.lib().cdll.f2n_ssim_fwd
    # (pred, gt, B, h, w, clip, ssim, map, gmaps, partial, stream)
    good = [FAKE, FAKE, 0, 11, 11, 0, FAKE, None, None, FAKE, None]
    assert fn(*good) == OK                                   # no images: nothing launched
    _sweep(fn, good, (
        ({5: 1}, OK), ({7: FAKE}, OK), ({8: FAKE}, OK), ({3: 1080, 4: 1920}, OK),
        ({0: None}, INVALID), ({1: None}, INVALID), ({6: None}, INVALID), ({9: None}, INVALID),
        ({2: -1}, INVALID), ({2: 65536}, INVALID), ({3: 10}, INVALID), ({4: 10}, INVALID),
        ({3: 0}, INVALID), ({4: -11}, INVALID), ({5: 2}, INVALID), ({5: -1}, INVALID),
        ({5: 1, 8: FAKE}, INVALID),                          # the partial maps are the plain form's
        # ... and a fault is answered before the launch whatever the image count
        ({2: 4, 0: None}, INVALID), ({2: 4, 1: None}, INVALID), ({2: 4, 6: None}, INVALID),
        ({2: 4, 9: None}, INVALID), ({2: 4, 3: 10}, INVALID), ({2: 4, 4: 10}, INVALID),
        ({2: 4, 5: 2}, INVALID), ({2: 4, 5: 1, 8: FAKE}, INVALID)))


def test_ssim_bwd_validates_before_any_hip_work(capi):
    fn = capi.lib().cdll.f2n_ssim_bwd
    # (pred, gt, gmaps, d_ssim, B, h, w, d_pred, stream)
    good = [FAKE, FAKE, FAKE, FAKE, 0, 11, 11, FAKE, None]
    assert fn(*good) == OK
    _sweep(fn, good, (
        ({5: 1080, 6: 1920}, OK),
        ({0: None}, INVALID), ({1: None}, INVALID), ({2: None}, INVALID), ({3: None}, INVALID),
        ({7: None}, INVALID), ({4: -1}, INVALID), ({4: 65536}, INVALID), ({5: 10}, INVALID),
        ({6: 10}, INVALID), ({5: -1}, INVALID),
        ({4: 2, 0: None}, INVALID), ({4: 2, 1: None}, INVALID), ({4: 2, 2: None}, INVALID),
        ({4: 2, 3: None}, INVALID), ({4: 2, 7: None}, INVALID), ({4: 2, 5: 10}, INVALID),
        ({4: 2, 6: 10}, INVALID)))


def test_draw_patches_validates_before_any_hip_work(capi):
    fn = capi.lib().cdll.f2n_draw_patches
    # (bits, E, h, w, n_patches, P, seed_lo, seed_hi, attempts, cam, ij, tries, patch_weight, stream)
    good = [FAKE, 3, 40, 53, 0, 16, 1, 2, 32, FAKE, FAKE, FAKE, FAKE, None]
    assert fn(*good) == OK
    _sweep(fn, good, (
        ({0: None}, OK),                                     # no mask is a valid call
        ({5: 11}, OK), ({5: 40}, OK), ({8: 1}, OK), ({8: 64}, OK), ({2: 11, 3: 11, 5: 11}, OK),
        ({9: None}, INVALID), ({10: None}, INVALID), ({11: None}, INVALID), ({12: None}, INVALID),
        ({4: -1}, INVALID), ({1: 0}, INVALID), ({1: -3}, INVALID),
        ({2: 10, 5: 10}, INVALID), ({3: 10, 5: 10}, INVALID), ({5: 10}, INVALID), ({5: 41}, INVALID),
        ({5: 0}, INVALID), ({5: -16}, INVALID), ({8: 0}, INVALID), ({8: 65}, INVALID),
        ({1: 1 << 20, 2: 1 << 10, 3: 1 << 10, 5: 11}, INVALID),     # E*h*w = 2^40
        ({4: 1 << 24, 5: 16}, INVALID),                              # 2^32 rays
        ({4: 8, 9: None}, INVALID), ({4: 8, 12: None}, INVALID), ({4: 8, 5: 10}, INVALID),
        ({4: 8, 5: 41}, INVALID), ({4: 8, 8: 0}, INVALID), ({4: 8, 8: 65}, INVALID),
        ({4: 8, 2: 10, 5: 10}, INVALID)))
