"""f2n_mask_pack and f2n_draw_pixels_masked (pixel_mask.hip) against the integer model of
tests/supervision_model.py, bit for bit, on a 3 x 5 x 70 set (1050 pixels: no multiple of 32 or 64,
rows straddle words), and f2n::sample_masked_rays on top of them."""
import importlib

import numpy as np
import pytest
import torch

from tests import supervision_model as sm

pytestmark = pytest.mark.gpu

GUARD = 8
SENT_I32 = -7777


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def _packed(capi, dev, name):
    """f2n_mask_pack through the C ABI with guard words behind every output"""
    m = torch.from_numpy(sm.mask(name).copy()).to(dev)
    c = capi.lib().cdll
    n_words, n_part = c.f2n_mask_words(sm.E, sm.H, sm.W), c.f2n_mask_pack_workspace_words(sm.E, sm.H, sm.W)
    words = torch.full((n_words + GUARD,), SENT_I32, dtype=torch.int32, device=dev)
    partial = torch.full((n_part + GUARD,), SENT_I32, dtype=torch.int32, device=dev)
    count = torch.full((1 + GUARD,), SENT_I32, dtype=torch.int64, device=dev)
    capi.call("mask_pack", m, sm.E, sm.H, sm.W, words, count, partial)
    torch.cuda.synchronize()
    for buf, used in ((words, n_words), (partial, n_part), (count, 1)):
        assert bool((buf[used:] == SENT_I32).all()), "guard overwritten"
    return words[:n_words].clone(), count[:1].clone()


@pytest.mark.parametrize("name", sm.MASKS)
def test_pack_equals_model(capi, dev, host, name):
    want_words, want_count = sm.pack(sm.mask(name))
    words, count = _packed(capi, dev, name)
    assert torch.equal(words.cpu(), torch.from_numpy(want_words.view(np.int32).copy()))   # tail bits too
    assert torch.equal(count.cpu(), torch.tensor([want_count], dtype=torch.int64))
    # ... and the host's PixelMask holds the same, from uint8 and from bool
    for m in (torch.from_numpy(sm.mask(name).copy()).to(dev), torch.from_numpy(sm.mask(name) != 0).to(dev)):
        pm = host.PixelMask.from_mask(m)
        assert (pm.E, pm.h, pm.w) == (sm.E, sm.H, sm.W)
        assert torch.equal(pm.bits, words) and torch.equal(pm.count, count)


def test_pack_past_the_grid_cap(host, dev):
    """more than 2^28 pixels: the pack launches 2^20 workgroups and each walks on in strides of the
    grid (the size at which that path exists); words and count against integer arithmetic in ATen"""
    h, w = 16401, 16399                                      # 268 959 999 pixels, 2^28 = 268 435 456
    n = h * w
    assert n > 1 << 28 and n % 64 != 0
    g = torch.Generator(device=dev).manual_seed(17)
    mask = torch.randint(0, 3, (1, h, w), device=dev, generator=g, dtype=torch.uint8)    # 0, 1, 2
    pm = host.PixelMask.from_mask(mask)
    n_words = (n + 31) // 32
    flat = torch.zeros(n_words * 32, dtype=torch.bool, device=dev)
    flat[:n] = mask.reshape(-1) != 0
    place = torch.ones(32, dtype=torch.int64, device=dev) << torch.arange(32, device=dev)
    want = (flat.reshape(n_words, 32).to(torch.int64) * place).sum(1)                    # 0 .. 2^32 - 1
    want = torch.where(want >= 1 << 31, want - (1 << 32), want).to(torch.int32)
    assert pm.bits.shape == (n_words,) and torch.equal(pm.bits, want)
    assert torch.equal(pm.count, flat.sum().reshape(1))
    # the draw reads the far end of the words as well: every kept pixel is valid
    cam, ij, tries = host.draw_pixels_masked(pm, 4096, 99, 32)
    kept = tries > 0
    assert int(kept.sum()) == 4096 and int(cam.max()) == 0 and int(ij[:, 0].max()) > h - 64
    assert bool((mask[0][ij[:, 0].long(), ij[:, 1].long()] != 0).all())


@pytest.mark.parametrize("A", sm.DRAW_A)
@pytest.mark.parametrize("n", sm.DRAW_N)
@pytest.mark.parametrize("name", sm.MASKS)
def test_draw_equals_model(capi, dev, name, n, A):
    words, _ = _packed(capi, dev, name)
    cam = torch.full((n + GUARD,), SENT_I32, dtype=torch.int32, device=dev)
    ij = torch.full((2 * n + GUARD,), SENT_I32, dtype=torch.int32, device=dev)
    tries = torch.full((n + GUARD,), SENT_I32, dtype=torch.int32, device=dev)
    capi.call("draw_pixels_masked", words, sm.E, sm.H, sm.W, sm.DRAW_SEED & sm.MASK32,
              sm.DRAW_SEED >> 32, A, cam, ij, tries, n)
    torch.cuda.synchronize()
    for buf, used in ((cam, n), (ij, 2 * n), (tries, n)):
        assert bool((buf[used:] == SENT_I32).all()), "guard overwritten"
    want_cam, want_ij, want_tries = sm.shared_draw(name, n, A)
    assert torch.equal(tries[:n].cpu(), torch.from_numpy(want_tries.copy()))
    assert torch.equal(cam[:n].cpu(), torch.from_numpy(want_cam.copy()))
    assert torch.equal(ij[:2 * n].reshape(n, 2).cpu(), torch.from_numpy(want_ij.copy()))
    if name == "one_pixel":
        assert int((tries[:n] == 0).sum()) >= 1          # the miss branch ran (the model's count
                                                         # is asserted in the CPU tests)


def _cameras(dev):
    g = torch.Generator().manual_seed(5)
    poses = torch.eye(4)[:3].repeat(sm.E, 1, 1)
    poses[:, :, 3] = torch.randn(sm.E, 3, generator=g)
    intr = torch.tensor([[60.0, 0, sm.W / 2], [0, 60.0, sm.H / 2], [0, 0, 1]]).repeat(sm.E, 1, 1)
    return poses.to(dev), intr.to(dev)


@pytest.mark.parametrize("channels", [0, 3, 4])
@pytest.mark.parametrize("name,A", [("checker", 32), ("one_pixel", 32), ("image1_off", 1)])
def test_sample_masked_rays(host, dev, name, A, channels):
    n = 257
    poses, intr = _cameras(dev)
    pm = host.PixelMask.from_mask(torch.from_numpy(sm.mask(name).copy()).to(dev))
    images = None
    if channels:
        images = torch.rand(sm.E, sm.H, sm.W, channels, generator=torch.Generator().manual_seed(9)).to(dev)
    b = host.sample_masked_rays(poses, intr, pm, n, sm.DRAW_SEED, images=images, attempts=A)
    want_cam, want_ij, want_tries = (torch.from_numpy(a.copy()).to(dev) for a in sm.shared_draw(name, n, A))
    assert torch.equal(b["cam"], want_cam) and torch.equal(b["ij"], want_ij)
    assert torch.equal(b["tries"], want_tries)
    cam2, ij2, tries2 = host.draw_pixels_masked(pm, n, sm.DRAW_SEED, A)
    assert torch.equal(cam2, want_cam) and torch.equal(ij2, want_ij) and torch.equal(tries2, want_tries)
    o, d = host.get_rays_from_cameras(poses, intr, b["cam"], b["ij"])
    assert torch.equal(b["rays_o"], o) and torch.equal(b["rays_d"], d)       # the same launch: same bits
    assert b["ray_weight"].dtype == torch.float32
    assert torch.equal(b["ray_weight"], (want_tries > 0).float())
    if name == "one_pixel":
        assert 0 < int((b["ray_weight"] == 0).sum()) < n
    if not channels:
        assert b["gt"] is None and b["alpha"] is None
        return
    px = images[b["cam"].long(), b["ij"][:, 0].long(), b["ij"][:, 1].long()]
    assert torch.equal(b["gt"], px[:, :3])
    if channels == 4:
        assert torch.equal(b["alpha"], px[:, 3])
    else:
        assert b["alpha"] is None


def test_sample_masked_rays_with_lens_distortion(host, dev):
    n = 63
    poses, intr = _cameras(dev)
    dist = torch.tensor([[0.05, -0.01, 1e-3, -2e-3]]).repeat(sm.E, 1).to(dev)
    pm = host.PixelMask.from_mask(torch.from_numpy(sm.mask("checker").copy()).to(dev))
    b = host.sample_masked_rays(poses, intr, pm, n, sm.DRAW_SEED, dist=dist)
    o, d = host.get_rays_from_cameras(poses, intr, b["cam"], b["ij"], dist=dist)
    assert torch.equal(b["rays_o"], o) and torch.equal(b["rays_d"], d)
    o0, d0 = host.get_rays_from_cameras(poses, intr, b["cam"], b["ij"])
    assert not torch.equal(d, d0)
