"""The D-SSIM term of f2n::train_step (PatchLoss) on the field and the routes of
tests/test_gpu_supervised_step.py (L = 4, F = 2, T = 2^12, 128 samples per ray): 4 patches of 11 x 11
(484 rays) and 2 of 16 x 16 (512 rays).

The loss identity.  With lambda = 0.2 the step's loss is the loss without the term plus
lambda sum_b m_b (1 - SSIM_b) / M of the colours the step returned.  SSIM_b is held to the forward
rule of tests/test_gpu_ssim.py (four times the float32 model's error against the float64 model, plus
4 * 2^-24), so the term may be off by lambda times the largest such bound over the patches; forming
1 - s, the weighted mean and the sum with the loss adds at most four more float32 roundings of
numbers below max(1, loss): 4 * 2^-24 max(1, loss).
"""
import importlib

import numpy as np
import pytest
import torch

from tests import ssim_cases as C
from tests import ssim_model as M
from tests.test_gpu_render import _setup
from tests.test_gpu_weight_dist import _route

pytestmark = pytest.mark.gpu

S = 128
VW = 1e-2
LAMBDA = 0.2
SHAPES = ((4, 11), (2, 16))                   # (patches, side)
STEP_ROUTES = ("march", "dense", "march_grid")


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


@pytest.fixture(scope="module")
def scenes(host, dev):
    """bias 1: a thin medium, the colours vary from ray to ray; one scene per patch shape"""
    out = {}
    for n, P in SHAPES:
        N = n * P * P
        _, hr, o, d, noise, bg, gt, emb = _setup(host, 4, 2, 12, S, 4.0 / S, N, 1.0, 50 + P)
        g = torch.Generator().manual_seed(P)
        alpha = torch.rand(N, generator=g)
        out[(n, P)] = dict(hr=hr, N=N, **{k: v.to(dev) for k, v in dict(
            o=o, d=d, noise=noise, bg=bg, gt=gt, emb=emb, alpha=alpha).items()})
    return out


def _step(host, sc, patch=None, sup=None):
    hr = sc["hr"]
    hr.zero_grad()
    a = (sc["o"], sc["d"], sc["emb"], sc["gt"])
    if patch is not None:
        out = hr.train_step_patches(*a, patch, sup if sup is not None else host.RaySupervision(),
                                    VW, sc["noise"], sc["bg"], True)
    elif sup is not None:
        out = hr.train_step_supervised(*a, sup, VW, sc["noise"], sc["bg"], True)
    else:
        out = hr.train_step(*a, VW, sc["noise"], sc["bg"], True)
    torch.cuda.synchronize()
    return out, {k: v.clone() for k, v in hr.grads().items() if v is not None}


def _same_step(a, b):
    (out_a, g_a), (out_b, g_b) = a, b
    assert torch.equal(out_a[0], out_b[0]) and torch.equal(out_a[1], out_b[1]) and out_a[3] == out_b[3]
    assert g_a.keys() == g_b.keys() and len(g_a) > 0
    # The table gradient is summed in integers: equal bits (under BWD_PHASES = 1, as in
    # tests/test_gpu_supervised_step.py).  The network's and the embedding's gradients are summed by
    # float atomics in the order the hardware picks, so two calls of the same step differ in their
    # last bits as well: those are held to 1e-4 of their norm, the figure this suite uses wherever
    # two such sums are compared (tests/test_gpu_depth_routes.py).
    for k in g_a:
        if k == "scene_field.feat_pool":
            assert torch.equal(g_a[k], g_b[k]), k
        else:
            assert float((g_a[k] - g_b[k]).norm()) <= 1e-4 * float(g_b[k].norm()), k
    assert float(g_a["scene_field.feat_pool"].abs().max()) > 0


def _term_model(colors, target, n, P, m):
    """-> (sum_b m_b (1 - ssim64_b) / M, the largest forward bound over the patches)"""
    x = colors.reshape(n, P, P, 3)
    y = np.asarray(target, dtype=np.float32).reshape(n, P, P, 3)
    m = np.ones(n) if m is None else np.asarray(m, dtype=np.float64)
    s64 = np.array([M.ssim64(x[b], y[b], False)[0] for b in range(n)])
    s32 = np.array([float(M.ssim32(x[b], y[b], False)["ssim"]) for b in range(n)])
    M_ = m.sum() if m.sum() > 0 else 1.0
    return float((m * (1.0 - s64)).sum() / M_), max(C.allowed(abs(a - b)) for a, b in zip(s32, s64)), s64


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("route", STEP_ROUTES)
def test_no_term_is_the_existing_step(host, capi, dev, scenes, route, shape):
    sc = scenes[shape]
    n, P = shape
    _route(sc["hr"], host, dev, route, sc["N"])
    capi.set_option("BWD_PHASES", 1)
    try:
        base = _step(host, sc)
        for patch in (host.PatchLoss(), host.PatchLoss(0, LAMBDA), host.PatchLoss(P, 0.0),
                      host.PatchLoss(P, 0.0, torch.ones(n, device=dev))):
            _same_step(_step(host, sc, patch), base)
            assert sc["hr"].last_ssim_loss is None
        sup = host.RaySupervision(ray_weight=torch.rand(sc["N"], device=dev), alpha=sc["alpha"],
                                  opacity_weight=0.3)
        _same_step(_step(host, sc, host.PatchLoss(P, 0.0), sup), _step(host, sc, None, sup))
        # every patch dropped: exact zeros join the colours' gradient, the loss gains 0 / 1
        dropped = _step(host, sc, host.PatchLoss(P, LAMBDA, torch.zeros(n, device=dev)))
        _same_step(dropped, base)
        assert sc["hr"].last_ssim_loss is not None
    finally:
        sc["hr"].set_occupancy(None)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("route", STEP_ROUTES)
def test_loss_gains_the_weighted_term(host, capi, dev, scenes, route, shape):
    sc = scenes[shape]
    n, P = shape
    hr = sc["hr"]
    _route(hr, host, dev, route, sc["N"])
    capi.set_option("BWD_PHASES", 1)
    want_colors = host.RaySupervision(want_colors=True)
    try:
        plain, _ = _step(host, sc, host.PatchLoss(), want_colors)
        colors = plain[5].cpu().numpy()
        gt = sc["gt"].cpu().numpy()
        for m in (None, [1.0, 0.0, 0.5, 2.0][:n]):
            pw = None if m is None else torch.tensor(m, device=dev)
            out, grads = _step(host, sc, host.PatchLoss(P, LAMBDA, pw), want_colors)
            assert torch.equal(out[5], plain[5]) and torch.equal(out[1], plain[1])
            term, bound, s64 = _term_model(colors, gt, n, P, m)
            loss, loss0 = float(out[0]), float(plain[0])
            err = abs(loss - (loss0 + LAMBDA * term))
            allowed = LAMBDA * bound + 4 * 2.0 ** -24 * max(1.0, abs(loss))
            print("step %s %dx%d m=%s: loss %.6f = %.6f + %.1f * %.6f, err %.2e of %.2e"
                  % (route, n, P, m, loss, loss0, LAMBDA, term, err, allowed))
            assert err <= allowed and term > 0.1
            # the unweighted mean, whatever the weights
            assert abs(float(hr.last_ssim_loss) - float((1 - s64).mean())) <= bound + 4 * 2.0 ** -24
            assert all(bool(torch.isfinite(g).all()) for g in grads.values())
            assert not torch.equal(grads["scene_field.feat_pool"], _step(host, sc)[1]["scene_field.feat_pool"])
    finally:
        hr.set_occupancy(None)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_with_ray_supervision_the_target_is_the_composited_one(host, capi, dev, scenes, shape):
    sc = scenes[shape]
    n, P = shape
    hr = sc["hr"]
    _route(hr, host, dev, "march", sc["N"])
    m = torch.tensor([1.0, 0.0, 1.0, 1.0][:n], device=dev)
    for composite in (True, False):
        sup = host.RaySupervision(ray_weight=m.repeat_interleave(P * P), alpha=sc["alpha"],
                                  opacity_weight=0.3, want_colors=True, composite_target=composite)
        plain, _ = _step(host, sc, host.PatchLoss(), sup)
        out, _ = _step(host, sc, host.PatchLoss(P, LAMBDA, m), sup)
        assert torch.equal(out[5], plain[5]) and torch.equal(out[4], plain[4])
        a = sc["alpha"].cpu().numpy()[:, None]
        gt, bg = sc["gt"].cpu().numpy(), sc["bg"].cpu().numpy()
        target = a * gt + (np.float32(1) - a) * bg if composite else gt
        term, bound, _ = _term_model(plain[5].cpu().numpy(), target, n, P, m.cpu().numpy())
        loss, loss0 = float(out[0]), float(plain[0])
        assert abs(loss - (loss0 + LAMBDA * term)) <= LAMBDA * bound + 4 * 2.0 ** -24 * max(1.0, abs(loss))


def test_a_dropped_patch_gets_exact_zeros(host, dev):
    """the term as train_step forms it, on a leaf: d_colors of the rays of a patch with m_b = 0"""
    n, P = 3, 11
    g = torch.Generator().manual_seed(3)
    colors = torch.rand(n * P * P, 3, generator=g).to(dev).requires_grad_(True)
    gt = torch.rand(n * P * P, 3, generator=g).to(dev)
    m = torch.tensor([1.0, 0.0, 0.5], device=dev)
    s = host.ssim_loss(colors.reshape(n, P, P, 3), gt.reshape(n, P, P, 3))
    (LAMBDA * (m * (1 - s)).sum() / m.sum()).backward()
    grad = colors.grad.reshape(n, P * P * 3)
    assert not grad[1].any() and bool(grad[0].ne(0).all()) and bool(grad[2].ne(0).all())
    want = np.stack([M.grad64(colors.detach().cpu().numpy().reshape(n, P, P, 3)[b],
                              gt.cpu().numpy().reshape(n, P, P, 3)[b],
                              -LAMBDA * float(m[b]) / 1.5).reshape(-1) for b in range(n)])
    assert np.abs(grad.cpu().numpy() - want).max() <= 1e-4 * np.abs(want).max()


def test_bad_patch_batches_throw(host, dev, scenes):
    sc = scenes[(4, 11)]
    _route(sc["hr"], host, dev, "march", sc["N"])
    for patch in (host.PatchLoss(16, LAMBDA),                                  # 484 is no multiple of 256
                  host.PatchLoss(2, LAMBDA),                                   # below the filter's 11 taps
                  host.PatchLoss(11, LAMBDA, torch.ones(3, device=dev))):      # four patches, three weights
        with pytest.raises(RuntimeError):
            _step(host, sc, patch)
