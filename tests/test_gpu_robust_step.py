"""The robust loss of f2n::train_step (RobustLoss) on the scene and the routes of
tests/test_gpu_ssim_step.py: L = 4, F = 2, T = 2^12, 128 samples per ray, 2 patches of 16 x 16 (512
rays), BWD_PHASES = 1 so that the table gradient is summed in integers.

Nothing here has a tolerance of its own.  Off, the step is today's (that file's _same_step).  On, the
step equals the supervised step handed the weights it returned: the wiring is pinned by an identity, and
the weights themselves are held to tests/robust_model.py, exactly."""
import importlib

import numpy as np
import pytest
import torch

from tests import robust_model as M
from tests.test_gpu_render import _setup
from tests.test_gpu_ssim_step import LAMBDA, S, VW, _same_step
from tests.test_gpu_weight_dist import _route

pytestmark = pytest.mark.gpu

N_PATCHES, P = 2, 16
N = N_PATCHES * P * P
STEP_ROUTES = ("march", "dense", "march_grid")


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


@pytest.fixture(scope="module")
def scene(host, dev):
    _, hr, o, d, noise, bg, gt, emb = _setup(host, 4, 2, 12, S, 4.0 / S, N, 1.0, 50 + P)
    g = torch.Generator().manual_seed(P)
    alpha = torch.rand(N, generator=g)
    m = torch.rand(N, generator=g)
    m[::5] = 0
    return dict(hr=hr, **{k: v.to(dev) for k, v in dict(
        o=o, d=d, noise=noise, bg=bg, gt=gt, emb=emb, alpha=alpha, m=m).items()})


def _step(host, sc, robust=None, patch=None, sup=None, gt=None, backward=True):
    hr = sc["hr"]
    hr.zero_grad()
    a = (sc["o"], sc["d"], sc["emb"], sc["gt"] if gt is None else gt)
    tail = (VW, sc["noise"], sc["bg"], backward)
    if robust is not None:
        out = hr.train_step_robust(*a, robust, patch if patch is not None else host.PatchLoss(),
                                   sup if sup is not None else host.RaySupervision(), *tail)
    elif patch is not None:
        out = hr.train_step_patches(*a, patch, sup if sup is not None else host.RaySupervision(), *tail)
    elif sup is not None:
        out = hr.train_step_supervised(*a, sup, *tail)
    else:
        out = hr.train_step(*a, *tail)
    torch.cuda.synchronize()
    return out, {k: v.clone() for k, v in hr.grads().items() if v is not None}


def _sup(host, sc, **kw):
    return host.RaySupervision(ray_weight=sc["m"], alpha=sc["alpha"], opacity_weight=0.3, **kw)


@pytest.mark.parametrize("route", STEP_ROUTES)
def test_off_is_todays_step(host, capi, dev, scene, route):
    sc = scene
    _route(sc["hr"], host, dev, route, N)
    capi.set_option("BWD_PHASES", 1)
    try:
        plain = _step(host, sc)
        supervised = _step(host, sc, sup=_sup(host, sc))
        patches = _step(host, sc, patch=host.PatchLoss(P, LAMBDA), sup=_sup(host, sc))
        for off in (host.RobustLoss(), host.RobustLoss(quantile=1.0, patch=P),
                    host.RobustLoss(quantile=1.5, patch=P, nbhd=4)):
            for got, want in ((_step(host, sc, off), plain),
                              (_step(host, sc, off, sup=_sup(host, sc)), supervised),
                              (_step(host, sc, off, host.PatchLoss(P, LAMBDA), _sup(host, sc)), patches)):
                _same_step(got, want)
                assert len(got[0]) == 8 and got[0][6] is None and got[0][7] is None
    finally:
        sc["hr"].set_occupancy(None)


@pytest.mark.parametrize("route", STEP_ROUTES)
def test_the_step_is_the_supervised_step_with_its_own_weights(host, capi, dev, scene, route):
    sc = scene
    _route(sc["hr"], host, dev, route, N)
    capi.set_option("BWD_PHASES", 1)
    robust = host.RobustLoss(quantile=0.5, patch=P)
    want_colors = dict(want_colors=True)
    try:
        # without supervision of the caller's: the body of the supervised step runs all the same
        got = _step(host, sc, robust, sup=host.RaySupervision(**want_colors))
        rw, stats = got[0][6], got[0][7]
        model = M.robust_weights(got[0][5].cpu().numpy(), sc["gt"].cpu().numpy(), None, P=P,
                                 **M.DEFAULTS)
        assert np.array_equal(rw.cpu().numpy(), model["weight"])
        assert np.array_equal(stats.cpu().numpy(), model["stats"])
        assert 0 < model["omega"].sum() < N
        ref = _step(host, sc, sup=host.RaySupervision(ray_weight=rw))
        _same_step(got, ref)
        assert torch.equal(got[0][4], ref[0][4])
        # with the caller's weights, an alpha target and the opacity term; composited and plain target
        for composite in (True, False):
            sup = _sup(host, sc, composite_target=composite, **want_colors)
            got = _step(host, sc, robust, sup=sup)
            rw = got[0][6]
            a = sc["alpha"].unsqueeze(1)
            target = a * sc["gt"] + (1.0 - a) * sc["bg"] if composite else sc["gt"]
            model = M.robust_weights(got[0][5].cpu().numpy(), target.cpu().numpy(),
                                     sc["m"].cpu().numpy(), P=P, **M.DEFAULTS)
            assert np.array_equal(rw.cpu().numpy(), model["weight"])
            assert not rw[::5].any() and torch.equal(rw[rw != 0], sc["m"][rw != 0])
            again = host.RaySupervision(ray_weight=rw, alpha=sc["alpha"], opacity_weight=0.3,
                                        composite_target=composite)
            ref = _step(host, sc, sup=again)
            _same_step(got, ref)
            assert torch.equal(got[0][4], ref[0][4])
        # the D-SSIM term keeps the caller's patch weight
        pl = host.PatchLoss(P, LAMBDA, torch.tensor([1.0, 0.5], device=dev))
        got = _step(host, sc, robust, pl, _sup(host, sc))
        again = host.RaySupervision(ray_weight=got[0][6], alpha=sc["alpha"], opacity_weight=0.3)
        _same_step(got, _step(host, sc, patch=pl, sup=again))
        assert sc["hr"].last_ssim_loss is not None
    finally:
        sc["hr"].set_occupancy(None)


def _distractor(host, sc):
    """gt = the render's own colours, plus noise of 1e-3 on patch 0 and plus 0.5 on patch 1"""
    with torch.no_grad():
        colors = _step(host, sc, sup=host.RaySupervision(want_colors=True), backward=False)[0][5]
    g = torch.Generator().manual_seed(77)
    gt = colors.clone()
    gt[:P * P] += (1e-3 * torch.randn(P * P, 3, generator=g)).to(colors.device)
    gt[P * P:] += 0.5
    return colors, gt


@pytest.mark.parametrize("route", STEP_ROUTES)
def test_a_whole_patch_distractor_contributes_exact_zeros(host, capi, dev, scene, route):
    sc = scene
    _route(sc["hr"], host, dev, route, N)
    capi.set_option("BWD_PHASES", 1)
    robust = host.RobustLoss(quantile=0.5, patch=P)
    want = np.repeat(np.array([1, 0], dtype=np.float32), P * P)
    try:
        colors, gt = _distractor(host, sc)
        # the model alone says so for these colours
        assert np.array_equal(M.robust_weights(colors.cpu().numpy(), gt.cpu().numpy(), None, P=P,
                                               **M.DEFAULTS)["weight"], want)
        got = _step(host, sc, robust, gt=gt)
        assert np.array_equal(got[0][6].cpu().numpy(), want)
        assert np.array_equal(got[0][7].cpu().numpy()[1:], np.array([N, P * P, P * P], dtype=np.float32))
        # another far colour on patch 1: a rejected ray contributes exact zeros
        other = gt.clone()
        other[P * P:] = colors[P * P:] - 0.7
        again = _step(host, sc, robust, gt=other)
        assert np.array_equal(again[0][6].cpu().numpy(), want)
        assert torch.equal(got[0][0], again[0][0]) and torch.equal(got[0][1], again[0][1])
        assert torch.equal(got[1]["scene_field.feat_pool"], again[1]["scene_field.feat_pool"])
        assert float(got[1]["scene_field.feat_pool"].abs().max()) > 0
        # ... which the plain step does not
        assert not torch.equal(_step(host, sc, gt=gt)[0][0], _step(host, sc, gt=other)[0][0])
    finally:
        sc["hr"].set_occupancy(None)


def test_with_the_error_map_rejected_rays_leave_no_trace(host, capi, dev, scene):
    """patch b is image b of a set of two 16 x 16 images, 4 x 4 cells each: cells 16 .. 31 are hit by
    patch 1's pixels only"""
    sc = scene
    _route(sc["hr"], host, dev, "march", N)
    colors, gt = _distractor(host, sc)
    got = _step(host, sc, host.RobustLoss(quantile=0.5, patch=P), gt=gt,
                sup=host.RaySupervision(want_colors=True))[0]
    cam = torch.arange(N_PATCHES, dtype=torch.int32, device=dev).repeat_interleave(P * P)
    u = torch.arange(P, dtype=torch.int32, device=dev)
    ij = torch.stack(torch.meshgrid(u, u, indexing="ij"), -1).reshape(-1, 2).repeat(N_PATCHES, 1).contiguous()
    emap = host.ErrorMap(N_PATCHES, P, P, host.ErrorMapOptions(gh=4, gw=4))
    before = emap.acc_cnt.clone()
    emap.accumulate(got[5], gt, cam, ij, ray_weight=got[6])
    torch.cuda.synchronize()
    assert torch.equal(emap.acc_cnt[16:], before[16:]) and torch.equal(emap.acc_sum[16:], torch.zeros_like(emap.acc_sum[16:]))
    assert bool((emap.acc_cnt[:16] == 16).all())
    # without the weights the distractor is exactly what the map would chase
    emap.accumulate(got[5], gt, cam, ij)
    torch.cuda.synchronize()
    assert bool((emap.acc_cnt[16:] == 16).all()) and bool((emap.acc_sum[16:] > emap.acc_sum[:16].max()).all())
