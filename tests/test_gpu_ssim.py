"""ssim.hip on the GPU against tests/ssim_model.py: the forward (fixture pairs, stacks, tile edges), the
backward, determinism, the patch draw, sample_patch_rays and image_scores.

THE BOUND (tests/ssim_cases.allowed).  A result may differ from the float64 model by four times the
float32 model's own error against the float64 model on the same case (for a map or a gradient: its
largest error over the case), plus 4 * 2^-24 of the scale (1 for SSIM values, max |g| for a
gradient).  The factor 4 leaves room for another legitimate summation order; it is measured on the
model, never on the kernel.  The float32 model repeats the kernel's stated order, so equal bits are
asserted as well.
"""
import importlib

import numpy as np
import pytest
import torch

from tests import ssim_cases as C
from tests import ssim_model as M

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x51A7C0DE9B1D5EED


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def _dev(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)     # (a copy: the shared cases are read-only)


def _check_forward(host, dev, keys, clip):
    cases = [C.forward_models(k, clip) for k in keys]
    pred = _dev(np.stack([c["x"] for c in cases]), dev)
    gt = _dev(np.stack([c["y"] for c in cases]), dev)
    ssim, smap = host.ssim(pred, gt, clip, True)
    assert ssim.shape == (len(keys),) and smap.shape[1:] == cases[0]["map64"].shape
    ssim, smap = ssim.cpu().numpy(), smap.cpu().numpy()
    for b, c in enumerate(cases):
        err, err32 = abs(float(ssim[b]) - c["ssim64"]), abs(float(c["ssim32"]) - c["ssim64"])
        merr = np.abs(smap[b] - c["map64"]).max()
        merr32 = np.abs(c["map32"] - c["map64"]).max()
        print("ssim fwd %s clip=%d: ssim err %.3e (model %.3e), map err %.3e (model %.3e)"
              % (keys[b], clip, err, err32, merr, merr32))
        assert err <= C.allowed(err32) and merr <= C.allowed(merr32)
        assert np.array_equal(smap[b], c["map32"]) and ssim[b] == c["ssim32"]
    # without the map: the same value
    assert torch.equal(host.ssim(pred, gt, clip, False)[0].cpu(), torch.from_numpy(ssim))


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("name", C.FIXTURE_NAMES)
def test_forward_fixture_pairs(host, dev, name, clip):
    _check_forward(host, dev, (name,), clip)
    if clip:
        # ... and the reference's own number, through the float64 model's 1e-10
        c = C.forward_models(name, True)
        got = float(host.ssim(_dev(c["x"], dev), _dev(c["y"], dev))[0][0])
        bound = C.allowed(abs(float(c["ssim32"]) - c["ssim64"])) + 1e-10
        assert abs(got - C.fixture_ref(name)[0]) <= bound


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("names", C.STACKS, ids=lambda n: "B%d" % len(n))
def test_forward_stacks(host, dev, names, clip):
    _check_forward(host, dev, names, clip)


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("hw", C.EDGE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_forward_tile_edges(host, dev, hw, clip):
    _check_forward(host, dev, (hw,), clip)


def test_forward_accepts_one_image_and_refuses_bad_shapes(host, dev):
    c = C.forward_models("noise_16x16", True)
    one = host.ssim(_dev(c["x"], dev), _dev(c["y"], dev))
    assert one[0].shape == (1,) and one[1] is None and float(one[0][0]) == float(c["ssim32"])
    x = torch.zeros(1, 10, 11, 3, device=dev)
    for bad in ((x, x), (x.cpu(), x.cpu()), (torch.zeros(11, 11, 3, device=dev), torch.zeros(11, 12, 3, device=dev)),
                (torch.zeros(11, 11, 4, device=dev),) * 2, (torch.zeros(11, 11, 3, device=dev).double(),) * 2):
        with pytest.raises(RuntimeError):
            host.ssim(*bad)


# ---- backward -----------------------------------------------------------------------------------

D_SSIM = (-0.7, 0.0, 1.3)


def _grad(host, dev, keys, d_ssim):
    cases = [C.forward_models(k, False) for k in keys]
    pred = _dev(np.stack([c["x"] for c in cases]), dev).requires_grad_(True)
    gt = _dev(np.stack([c["y"] for c in cases]), dev).requires_grad_(True)
    out = host.ssim_loss(pred, gt)
    out.backward(_dev(np.asarray(d_ssim, dtype=F32), dev))
    assert gt.grad is None                                    # gt receives no gradient
    return out.detach().cpu().numpy(), pred.grad.cpu().numpy()


@pytest.mark.parametrize("hw", C.BWD_SHAPES, ids=lambda s: "%dx%d" % s)
def test_backward(host, dev, hw):
    """three images of one size: d_ssim negative, zero and positive"""
    value, grad = _grad(host, dev, (hw,) * 3, D_SSIM)
    f = C.forward_models(hw, False)
    assert (value == f["ssim32"]).all()                       # the differentiable form's forward
    for b, d in enumerate(D_SSIM):
        m = C.backward_models(hw, d)
        scale = np.abs(m["g64"]).max()
        err, err32 = np.abs(grad[b] - m["g64"]).max(), np.abs(m["g32"] - m["g64"]).max()
        print("ssim bwd %dx%d d_ssim=%+.1f: err / max|g| %.3e (model %.3e)"
              % (hw + (d, err / max(scale, 1e-30), err32 / max(scale, 1e-30))))
        assert (np.abs(grad[b] - m["g64"]) <= C.allowed(err32, scale)).all()
        assert np.array_equal(grad[b], m["g32"])
        if d == 0.0:
            assert not grad[b].any()
    if hw == (11, 11):
        # one map pixel: every input pixel is touched exactly once, through f[i] f[j]
        assert (grad[0] != 0).all()


def test_backward_of_a_single_image_keeps_its_shape(host, dev):
    f = C.forward_models((12, 17), False)
    pred = _dev(f["x"], dev).requires_grad_(True)
    out = host.ssim_loss(pred, _dev(f["y"], dev))
    out.sum().backward()
    assert out.shape == (1,) and pred.grad.shape == (12, 17, 3)
    assert np.array_equal(pred.grad.cpu().numpy(), C.backward_models((12, 17), 1.0)["g32"])


def test_two_runs_give_equal_bits(host, dev):
    g = torch.Generator().manual_seed(5)
    pred = torch.rand(3, 75, 58, 3, generator=g).to(dev)
    gt = torch.rand(3, 75, 58, 3, generator=g).to(dev)
    d = torch.tensor([0.5, -1.0, 2.0], device=dev)
    runs = []
    for _ in range(2):
        p = pred.clone().requires_grad_(True)
        out = host.ssim_loss(p, gt)
        out.backward(d)
        runs.append((out.detach().clone(), p.grad.clone(), host.ssim(pred, gt)[0]))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- the patch draw -----------------------------------------------------------------------------

def _mask(E, h, w):
    m = np.ones((E, h, w), np.uint8)
    m[:, :, ::17] = 0                                          # bands 16 apart: P = 32 never fits
    m[:, 3, :] = 0
    m[0, h // 2:, : w // 2] = 0
    return m


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("P", [11, 16, 32])
@pytest.mark.parametrize("E", [1, 3])
def test_draw_is_the_integer_model(host, dev, E, P, masked):
    h, w, n = 47, 70, 37
    mask = _mask(E, h, w) if masked else None
    pm = host.PixelMask.from_mask(_dev(mask, dev)) if masked else None
    for attempts in (32, 3):
        got = host.draw_patches(E, h, w, n, P, SEED, pm, attempts)
        want = M.draw_patches(mask, E, h, w, n, P, SEED, attempts)
        for a, b in zip(got, want):
            assert np.array_equal(a.cpu().numpy(), b)
        if masked and attempts == 32:
            tries = want[2]
            assert (tries == 0).all() if P == 32 else (tries > 1).any()     # both ends are reached


def test_draw_single_possible_row(host, dev):
    got = host.draw_patches(2, 11, 30, 9, 11, SEED)
    want = M.draw_patches(None, 2, 11, 30, 9, 11, SEED)
    for a, b in zip(got, want):
        assert np.array_equal(a.cpu().numpy(), b)
    assert not got[1][:, 0].reshape(9, 121)[:, 0].any()


def test_sample_patch_rays(host, dev):
    E, h, w, n, P = 3, 47, 70, 5, 16
    g = torch.Generator().manual_seed(11)
    poses = torch.eye(4)[:3].repeat(E, 1, 1)
    poses[:, :, 3] = torch.randn(E, 3, generator=g)
    intr = torch.tensor([[60.0, 0, w / 2], [0, 60.0, h / 2], [0, 0, 1]]).repeat(E, 1, 1)
    images = torch.rand(E, h, w, 4, generator=g)
    dist = torch.tensor([[0.05, -0.01, 1e-3, -1e-3]]).repeat(E, 1)
    poses, intr, images, dist = (t.to(dev) for t in (poses, intr, images, dist))
    mask = _mask(E, h, w)
    pm = host.PixelMask.from_mask(_dev(mask, dev))
    for d_arg in (None, dist):
        b = host.sample_patch_rays(poses, intr, h, w, n, P, SEED, images, pm, d_arg)
        want = M.draw_patches(mask, E, h, w, n, P, SEED)
        assert np.array_equal(b["cam"].cpu().numpy(), want[0]) and np.array_equal(b["ij"].cpu().numpy(), want[1])
        assert np.array_equal(b["patch_weight"].cpu().numpy(), want[3])
        assert torch.equal(b["ray_weight"], b["patch_weight"].repeat_interleave(P * P))
        ro, rd = host.get_rays_from_cameras(poses, intr, b["cam"], b["ij"], d_arg)
        assert torch.equal(b["rays_o"], ro) and torch.equal(b["rays_d"], rd)
        px = images[b["cam"].long(), b["ij"][:, 0].long(), b["ij"][:, 1].long()]
        assert torch.equal(b["gt"], px[:, :3]) and torch.equal(b["alpha"], px[:, 3])
    plain = host.sample_patch_rays(poses, intr, h, w, n, P, SEED)
    assert plain["gt"] is None and plain["alpha"] is None and bool((plain["patch_weight"] == 1).all())


# ---- scores -------------------------------------------------------------------------------------

def test_image_scores(host, dev):
    h, w = 48, 64
    g = np.random.default_rng(17)
    gt = g.random((2, h, w, 3)).astype(F32)
    pred = (gt + 0.08 * g.standard_normal((2, h, w, 3))).astype(F32)      # leaves [0, 1] in places
    sc = host.image_scores(_dev(pred, dev), _dev(gt, dev))
    d = pred.astype(np.float64) - gt
    mse = (d * d).mean(axis=(1, 2, 3))
    for b in range(2):
        assert abs(float(sc["mse"][b]) - mse[b]) <= 1e-6 * mse[b]
        got_mse = float(sc["mse"][b])
        assert abs(float(sc["psnr"][b]) + 10.0 * np.log10(got_mse)) <= 1e-4
        assert abs(float(sc["score"][b]) - h * w / (got_mse * h * w + 1e-6)) <= 1e-5 * float(sc["score"][b])
        x, y = np.clip(pred[b], 0, 1), np.clip(gt[b], 0, 1)
        s64 = M.ssim64(x, y, True)[0]
        s32 = M.ssim32(x, y, True)["ssim"]
        assert abs(float(sc["ssim"][b]) - s64) <= C.allowed(abs(float(s32) - s64))
        assert float(sc["ssim"][b]) == float(s32)
    for v in sc.values():
        assert v.shape == (2,) and v.is_cuda
