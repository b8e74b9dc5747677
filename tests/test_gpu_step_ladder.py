"""The ladder of training entries -- train_step, train_step_supervised, train_step_patches,
train_step_robust -- launch for launch: an entry handed nothing but defaults for what it adds is the
entry below it, and a term whose weight is zero is a term that was never passed.  What is compared is
the ordered list of device kernel names of one step under the torch profiler, element by element, on
the scene of tests/test_gpu_robust_step.py (L = 4, F = 2, T = 2^12, S = 128, 2 patches of 16 x 16,
noise and bg_color passed) and on five render routes.

Each profiled step follows one identical, unprofiled step, so that whatever a route remembers of the
previous call (the adaptive first pass, the dense route's guess) is the same for every list.  Equal
lists could be empty lists: the controls at the end of the test see the shade kernel in every list
and see a term that is on add launches."""
import importlib

import pytest
import torch

from tests.test_gpu_render import _setup
from tests.test_gpu_ssim_step import S, VW
from tests.test_gpu_weight_dist import _route

pytestmark = pytest.mark.gpu

N_PATCHES, P = 2, 16
N = N_PATCHES * P * P
ROUTES = ("op_by_op", "march", "dense", "lean_bucketed", "march_grid")


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
    z = 0.5 + 2.0 * torch.rand(N, generator=g)      # depth targets along the ray; every 7th ray has none
    z[::7] = 0
    return dict(hr=hr, **{k: v.to(dev) for k, v in dict(
        o=o, d=d, noise=noise, bg=bg, gt=gt, emb=emb, alpha=alpha, m=m, z=z).items()})


def _kernels(sc, entry, *head, **terms):
    """the device kernel names of hr.<entry>(rays, emb, gt, *head, VW, noise, bg, True, **terms), in
    the order they started"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile

    hr = sc["hr"]

    def step():
        hr.zero_grad()
        getattr(hr, entry)(sc["o"], sc["d"], sc["emb"], sc["gt"], *head, VW, sc["noise"], sc["bg"],
                           True, **terms)
        torch.cuda.synchronize()

    step()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
    events = [e for e in prof.events() if e.device_type == DeviceType.CUDA]
    return [e.name for e in sorted(events, key=lambda e: e.time_range.start)]


def _same(lists):
    first = lists[0]
    for other in lists[1:]:
        assert len(other) == len(first), (len(first), len(other))
        for i, (a, b) in enumerate(zip(first, other)):
            assert a == b, (i, a, b)


@pytest.mark.parametrize("route", ROUTES)
def test_the_ladder_launch_for_launch(host, dev, scene, route):
    sc = scene
    _route(sc["hr"], host, dev, route, N)
    # what shades a sample: the fused per-sample network on the fused routes, the SH encoding in front
    # of the ATen network on the op-by-op route
    shade = "sh_encode" if route == "op_by_op" else "shade"
    no_sup, no_patch, no_robust = host.RaySupervision(), host.PatchLoss(), host.RobustLoss()
    try:
        lists = []

        # the unweighted ladder, every term off and with the distortion and depth terms on
        loaded = dict(dist_loss_weight=0.01, depth_target=sc["z"],
                      depth_loss=host.DepthLossOptions(empty=0.1, near=0.2, expected=0.3, eps=0.05))
        for terms in ({}, loaded):
            rungs = [_kernels(sc, "train_step", **terms),
                     _kernels(sc, "train_step_supervised", no_sup, **terms),
                     _kernels(sc, "train_step_patches", no_patch, no_sup, **terms),
                     _kernels(sc, "train_step_robust", no_robust, no_patch, no_sup, **terms)]
            _same(rungs)
            lists += rungs
        plain, plain_loaded = lists[0], lists[4]

        # the weighted ladder: a ray_weight with zeros and an alpha target
        sup = host.RaySupervision(ray_weight=sc["m"], alpha=sc["alpha"], opacity_weight=0.3)
        weighted = [_kernels(sc, "train_step_supervised", sup),
                    _kernels(sc, "train_step_patches", no_patch, sup),
                    _kernels(sc, "train_step_robust", no_robust, no_patch, sup)]
        _same(weighted)
        lists += weighted

        # a zero weight is absence
        zeros = _kernels(sc, "train_step", dist_loss_weight=0.0, depth_target=sc["z"],
                         depth_loss=host.DepthLossOptions())
        _same([plain, zeros])
        sup0 = host.RaySupervision(ray_weight=sc["m"], alpha=sc["alpha"], opacity_weight=0.0)
        opacity_off = [_kernels(sc, "train_step_supervised", sup0),
                       _kernels(sc, "train_step_patches", no_patch, sup0)]
        _same(opacity_off)
        lists += [zeros] + opacity_off

        # the controls: equal lists are not empty lists, and a term that is on is seen
        for names in lists:
            assert len(names) > 0 and any(shade in n for n in names), sorted(set(names))
        with_dist = _kernels(sc, "train_step", dist_loss_weight=0.01)
        assert len(with_dist) > len(plain) and any("weight_dist" in n for n in with_dist)
        assert not any("weight_dist" in n for n in plain)
        assert len(plain_loaded) > len(with_dist)
        assert len(weighted[0]) > len(opacity_off[0])           # the opacity term's launches
        robust = _kernels(sc, "train_step_robust", host.RobustLoss(quantile=0.5, patch=P), no_patch,
                          no_sup)
        assert any("robust_" in n for n in robust) and not any("robust_" in n for n in plain)
    finally:
        sc["hr"].set_occupancy(None)
