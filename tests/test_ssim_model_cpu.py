"""The numpy models of ssim.hip (tests/ssim_model.py) against what they stand for: the reference's own
rgb_ssim as recorded in tests/golden/ssim/ssim_reference.npz, torch.autograd on the float64 conv2d spelling,
and the stated properties of the patch draw.  No GPU."""
import numpy as np
import pytest
import torch

from tests import ssim_model as M
from tests import supervision_model as sm
from tests.ssim_cases import FIXTURE_NAMES, fixture_pair, fixture_ref


def test_fixture_holds_the_listed_pairs():
    shapes = {n: fixture_pair(n)[0].shape[:2] for n in FIXTURE_NAMES}
    for hw in ((11, 11), (11, 12), (12, 11), (16, 16), (26, 43), (33, 70)):
        assert shapes["noise_%dx%d" % hw] == hw
    values = [fixture_ref(n)[0] for n in FIXTURE_NAMES]
    assert min(values) < -0.1 and max(values) == 1.0
    # the badly conditioned pair: two flat images, S = (2 * .16 + c1) / (.04 + .64 + c1)
    assert abs(fixture_ref("flat02_flat08")[0] - 0.4707) < 1e-4


@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_f64_model_with_clamps_is_the_reference(name):
    """1e-10: f64 rounding of about 1e-16 per operation over about 50 operations, amplified by at
    most 1 / sqrt(c1 c2) = 3e3 on flat regions"""
    x, y = fixture_pair(name)
    ref_ssim, ref_map = fixture_ref(name)
    got_ssim, got_map = M.ssim64(x, y, True)
    assert got_map.shape == ref_map.shape == (x.shape[0] - 10, x.shape[1] - 10, 3)
    assert abs(got_ssim - ref_ssim) <= 1e-10
    assert np.abs(got_map - ref_map).max() <= 1e-10


@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_clamps_only_act_on_rounding_error(name):
    x, y = fixture_pair(name)
    assert abs(M.ssim64(x, y, True)[0] - M.ssim64(x, y, False)[0]) <= 1e-10


def _autograd(x, y, d_ssim):
    """the same formula as grouped-free conv2d in float64, differentiated by torch"""
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yt = torch.tensor(y, dtype=torch.float64, requires_grad=True)
    f = torch.tensor(M.filter64())

    def blur(t):
        t = t.permute(2, 0, 1)[:, None]
        t = torch.nn.functional.conv2d(t, f.view(1, 1, 1, M.TAPS))
        return torch.nn.functional.conv2d(t, f.view(1, 1, M.TAPS, 1))

    mx, my = blur(xt), blur(yt)
    sxx, syy, sxy = blur(xt * xt) - mx * mx, blur(yt * yt) - my * my, blur(xt * yt) - mx * my
    S = ((2 * mx * my + M.C1) * (2 * sxy + M.C2)) / ((mx * mx + my * my + M.C1) * (sxx + syy + M.C2))
    (d_ssim * S.mean()).backward()
    return S.mean().item(), xt.grad.numpy()


@pytest.mark.parametrize("h,w", [(11, 11), (13, 17), (26, 43)])
def test_f64_gradient_is_autograds(h, w):
    g = np.random.default_rng(1000 * h + w)
    x, y = g.random((h, w, 3)), g.random((h, w, 3))
    for d_ssim in (1.0, -0.3):
        value, grad = _autograd(x, y, d_ssim)
        assert abs(M.ssim64(x, y, False)[0] - value) <= 1e-12
        assert np.abs(M.grad64(x, y, d_ssim) - grad).max() <= 1e-12


def test_f32_model_follows_the_f64_model():
    """the float32 spelling is the same function: a few ulp of its largest intermediate"""
    for name in FIXTURE_NAMES:
        x, y = fixture_pair(name)
        for clip in (True, False):
            got = M.ssim32(x, y, clip, want_gmaps=not clip)
            want_ssim, want_map = M.ssim64(x, y, clip)
            assert abs(float(got["ssim"]) - want_ssim) <= 2e-6
            assert np.abs(got["map"] - want_map).max() <= 2e-4
        g64 = M.grad64(x, y, -0.7)
        g32 = M.bwd32(x, y, got["gmaps"], -0.7)
        # (1e-6: a pair of equal flat images has gradient 0, the sum of terms of size 2 x / (c2 n)
        # = 4 that cancel; float32 leaves a few 1e-7 of them)
        assert np.abs(g32 - g64).max() <= 1e-4 * np.abs(g64).max() + 1e-6
    assert np.array_equal(M.bwd32(x, y, got["gmaps"], 0.0), np.zeros_like(x))


def test_filter_is_normalised_and_symmetric():
    f = M.filter64()
    assert abs(f.sum() - 1.0) < 1e-15 and np.array_equal(f, f[::-1]) and f.argmax() == 5
    assert M.filter32().dtype == np.float32


# ---- the patch draw -----------------------------------------------------------------------------

SEED = 0x51A7C0DE9B1D5EED


@pytest.mark.parametrize("P", [11, 16, 32])
@pytest.mark.parametrize("E", [1, 3])
def test_patches_lie_inside_the_image(E, P):
    h, w, n = 40, 53, 37
    cam, ij, tries, weight = M.draw_patches(None, E, h, w, n, P, SEED)
    assert cam.shape == (n * P * P,) and ij.shape == (n * P * P, 2)
    assert cam.min() >= 0 and cam.max() < E
    assert ij.min() >= 0 and ij[:, 0].max() < h and ij[:, 1].max() < w
    assert np.array_equal(tries, np.ones(n, np.int32)) and np.array_equal(weight, np.ones(n, np.float32))
    # patch-major, row-major inside the patch: ray b P^2 + u P + v is pixel (i0 + u, j0 + v)
    p = ij.reshape(n, P, P, 2)
    u, v = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
    assert np.array_equal(p[..., 0], p[:, :1, :1, 0] + u) and np.array_equal(p[..., 1], p[:, :1, :1, 1] + v)
    assert np.array_equal(cam.reshape(n, P * P), np.repeat(cam[::P * P, None], P * P, axis=1))
    if E == 3:
        assert len(set(cam.tolist())) == 3


def test_single_possible_row():
    cam, ij, _, _ = M.draw_patches(None, 2, 11, 30, 9, 11, SEED)
    assert np.array_equal(ij.reshape(9, 11, 11, 2)[:, 0, 0, 0], np.zeros(9, np.int32))


def test_draw_is_its_own_philox_domain():
    """counter word 2 is 2: neither the masked draw's stream (0) nor the guided draw's (1)"""
    x = sm.philox_scalar((5, 0, M.PATCH_DOMAIN, 0), (SEED & sm.MASK32, SEED >> 32))
    cam, ij, _, _ = M.draw_patches(None, 3, 40, 53, 6, 11, SEED)
    assert cam[5 * 121] == (x[0] * 3) >> 32
    assert ij[5 * 121, 0] == (x[1] * 30) >> 32 and ij[5 * 121, 1] == (x[2] * 43) >> 32
    assert x != sm.philox_scalar((5, 0, 0, 0), (SEED & sm.MASK32, SEED >> 32))


def test_a_patch_is_accepted_only_if_fully_valid():
    E, h, w, P, n = 2, 30, 36, 11, 48
    g = np.random.default_rng(3)
    mask = np.ones((E, h, w), np.uint8)
    mask[g.integers(0, E, 12), g.integers(0, h, 12), g.integers(0, w, 12)] = 0   # twelve holes
    cam, ij, tries, weight = M.draw_patches(mask, E, h, w, n, P, SEED, attempts=4)
    valid = mask[cam, ij[:, 0], ij[:, 1]].reshape(n, P * P).all(axis=1)
    assert np.array_equal(valid, tries > 0) and np.array_equal(weight, (tries > 0).astype(np.float32))
    assert 0 < int((tries == 0).sum()) < n and int(tries.max()) > 1              # every branch is taken


def test_no_window_fits():
    """every 11 x 11 window holds an invalid pixel: tries 0 and weight 0 everywhere"""
    E, h, w = 2, 24, 31
    mask = np.ones((E, h, w), np.uint8)
    mask[:, 10::11, :] = 0
    cam, ij, tries, weight = M.draw_patches(mask, E, h, w, 16, 11, SEED, attempts=8)
    assert not tries.any() and not weight.any()
    assert ij.min() >= 0 and ij[:, 0].max() < h and ij[:, 1].max() < w          # the last attempt stays


def test_one_invalid_band_accepts_all_64():
    """h = 64, P = 11, rows 0 .. 7 invalid: of the 54 possible first rows 46 give a valid patch, so
    one attempt succeeds with probability 46 / 54 > 1 / 4 and 32 attempts miss with 1e-27"""
    E, h, w, P = 2, 64, 48, 11
    mask = np.ones((E, h, w), np.uint8)
    mask[:, :8, :] = 0
    assert (h - P + 1 - 8) / (h - P + 1) >= 0.25
    cam, ij, tries, weight = M.draw_patches(mask, E, h, w, 64, P, SEED)
    assert (tries > 0).all() and (weight == 1).all() and ij[:, 0].min() >= 8
    assert int(tries.max()) > 1                                                  # some patch redrew
