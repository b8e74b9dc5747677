"""Depth supervision through the Renderer, on the small scenes of tests/test_gpu_weight_dist.py:
render_for_loss with a depth target on every route (op by op, march, dense, lean bucketed, and with an
occupancy grid) and train_step with DepthLossOptions -- the terms against the float64 model of
tests/depth_sight_model.py within its bound tol = u (len_r M_sum + K_SIGHT M_op), everything that
exists today against itself with torch.equal."""
import importlib
import math

import numpy as np
import pytest
import torch

from tests import depth_sight_model as dm
from tests import ragged_cases as rc
from tests.test_gpu_weight_dist import (N_RAYS, N_TRAIN, ROUTES, S, _route, _scene, _step,
                                        _term_against_op_by_op, hr_occupied)

pytestmark = pytest.mark.gpu

EPS = 0.05


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


@pytest.fixture(scope="module")
def scene(host, dev):
    return _scene(host, dev, N_RAYS, 4.0, 31)


@pytest.fixture(scope="module")
def thin_scene(host, dev):
    return _scene(host, dev, N_TRAIN, 1.0, 37)


def _targets(scene, seed):
    """a distinct target for every ray, somewhere along its samples (t is Euclidean distance along the
    unit direction); every eighth ray has no return: 0, negative, NaN, +inf in turn"""
    g = torch.Generator().manual_seed(seed)
    t = scene["t"]
    n = t.shape[0]
    frac = 0.02 + 0.9 * torch.rand(n, generator=g)
    z = t[:, 0] + frac * (t[:, -1] - t[:, 0])
    bad = torch.tensor([0.0, -2.0, float("nan"), float("inf")])
    z[::8] = bad[torch.arange(z[::8].numel()) % 4]
    valid = torch.isfinite(z) & (z > 0)
    assert len(set(z[valid].tolist())) == int(valid.sum()) and int(valid.sum()) == n - n // 8
    return z


def _kept_mask(route, host, dev, scene, count):
    if route.endswith("grid"):
        occ = hr_occupied(host, dev, scene).reshape(scene["n_rays"], S).cpu()
        return occ & (torch.cumsum(occ.long(), 1) <= count[:, None])
    return torch.arange(S)[None, :] < count[:, None]


@pytest.mark.parametrize("route", ROUTES)
def test_render_for_loss_depth_terms(host, capi, dev, scene, route):
    hr = scene["hr"]
    z = _targets(scene, 3)
    z_dev = z.to(dev)
    _route(hr, host, dev, route)
    try:
        with torch.no_grad():
            today = hr.render(*scene["args"])                       # (colors, depths, weights, idx)
            plain = hr.render_for_loss(*scene["args"], want_dist=True)
            asked = hr.render_for_loss(*scene["args"], want_dist=True, depth_target=z_dev,
                                       depth_eps=EPS)
            alone = hr.render_for_loss(*scene["args"], depth_target=z_dev, depth_eps=EPS)
    finally:
        hr.set_occupancy(None)
    # with a target: what the call returns without it, bit for bit, plus depth_terms
    assert len(plain) == 6 and len(asked) == 7 and len(alone) == 7
    for a, b in zip(plain, asked[:6]):
        assert (a is None and b is None) or torch.equal(a, b)
    for a, b in zip(plain[:5], alone[:5]):
        assert (a is None and b is None) or torch.equal(a, b)
    assert alone[5] is None and torch.equal(alone[6], asked[6])
    if route == "lean_bucketed":
        assert plain[2] is None and plain[4] is not None            # the route was reached
    terms = asked[6]
    assert terms.shape == (N_RAYS, 3) and terms.dtype == torch.float32

    weights, idx = today[2].cpu(), today[3].cpu()
    count = (idx[:, 1] - idx[:, 0]).long()
    keep = _kept_mask(route, host, dev, scene, count)
    assert torch.equal(keep.sum(1), count) and int(count.sum()) == weights.numel()
    if not route.endswith("grid"):
        assert int(count.max()) > rc.WAVE                           # more than one stride
    lay = rc.Layout(idx.contiguous(), np.zeros(N_RAYS), weights.numel())
    case = dict(weights=weights, t=scene["t"][keep], dt=scene["dt"][keep], z=z,
                d_out=torch.ones(N_RAYS, 3), eps=float(np.float32(EPS)))
    ref = dm.sight_ref(lay, case)
    valid = dm.ray_valid(z.numpy())
    # the case holds what the test is about: all three terms are alive, rays have front, band and
    # behind samples
    assert float(ref["out"][valid, 0].max()) > 1e-6 and float(ref["out"][valid, 2].max()) > 1e-3
    if not route.endswith("grid"):
        assert float(ref["out"][valid, 1].min()) < 0.999            # weight inside some band
    got = dict(out=terms.cpu().numpy())
    for name, (ratio, _) in dm.ratios(lay, case, got, ref).items():
        print("  %s %s: largest (err/u - len M_sum)/M_op = %.3f (K = %g)" % (
            route, name, float(ratio.max()), dm.K_SIGHT))
    rc.assert_no_failures(dm.sight_failures(lay, case, got, ref), route)
    assert bool((terms[torch.from_numpy(~valid).to(dev)] == 0).all())

    # DepthSight on the route's own kept samples: the same launch on the same inputs.  A ray's terms
    # depend on its own samples alone, each taken by the lane of its offset from the ray's start, so
    # they do not depend on where the ray lies in storage: the bucketed route's too
    own = host.depth_sight(today[2], scene["t"][keep].to(dev), scene["dt"][keep].to(dev), today[3],
                           z_dev, EPS)
    same = torch.equal(own, terms)
    print("  %s: depth_terms bit-equal to DepthSight on the caller-order samples: %s" % (route, same))
    rc.assert_no_failures(dm.sight_failures(lay, case, dict(out=own.cpu().numpy()), ref), route + " op")
    assert same

    # the caller's order: the terms of ray r belong to target z[r].  Against the targets in another
    # order (what a result left in the bucketed order, or a target not permuted with its ray, would
    # be) the same assertions fail on most rays
    wrong = dict(case)
    wrong["z"] = z.flip(0)
    bad = dm.sight_failures(lay, wrong, got, dm.sight_ref(lay, wrong))
    assert len({f[0] for f in bad}) > N_RAYS // 2


def test_depth_gradient_comes_back_in_the_callers_order(host, capi, dev, thin_scene):
    """sum_r c_r . terms_r with different factors for every ray: on the lean bucketed route the
    gradient travels back through the per-ray gather of the terms, and the target went out through
    the opposite one.  The table gradient must be the one of the routes that keep the caller's order,
    to 1e-4 of its norm (the figure tests/test_gpu_weight_dist.py holds this comparison to); factors
    or targets handed to other rays are an error of order 1, shown on the same data."""
    scene = thin_scene
    hr = scene["hr"]
    capi.set_option("BWD_PHASES", 1)
    g = torch.Generator().manual_seed(5)
    c = (0.1 + 1.9 * torch.rand(N_TRAIN, 3, generator=g)).to(dev)
    z = _targets(scene, 9).to(dev)
    grads = {}
    for name, route, coeff, target in (
            ("march", "march", c, z), ("dense", "dense", c, z), ("lean_bucketed", "lean_bucketed", c, z),
            ("c_permuted", "march", c.flip(0), z), ("z_permuted", "march", c, z.flip(0))):
        _route(hr, host, dev, route, N_TRAIN)
        hr.zero_grad()
        res = hr.render_for_loss(*scene["args"], depth_target=target, depth_eps=EPS)
        if route == "lean_bucketed":
            assert res[2] is None and res[4] is not None            # the route was reached
        (res[6] * coeff).sum().backward()
        torch.cuda.synchronize()
        grads[name] = hr.grads()["scene_field.feat_pool"].clone()
    ref = grads["march"]
    assert float(ref.norm()) > 0
    for name in ("dense", "lean_bucketed", "c_permuted", "z_permuted"):
        rel = float((grads[name] - ref).norm() / ref.norm())
        print("  %s against march: |dg| / |g| = %.3e" % (name, rel))
        assert (rel > 1e-2) if name.endswith("permuted") else (rel <= 1e-4), (name, rel)


@pytest.mark.parametrize("route", ["march", "dense", "lean_bucketed"])
def test_train_step_with_depth_loss(host, capi, dev, thin_scene, route):
    scene = thin_scene
    hr = scene["hr"]
    _route(hr, host, dev, route, N_TRAIN)
    capi.set_option("BWD_PHASES", 1)          # table gradient sums independent of the order
    z = _targets(scene, 7).to(dev)
    lam = (0.3, 0.05, 0.2)
    opts = host.DepthLossOptions(empty=lam[0], near=lam[1], expected=lam[2], eps=EPS)
    loss0, sq0, ns0, g0, all0 = _step(hr, scene, all_grads=True)    # the existing call
    assert hr.last_depth_loss is None and float(g0.abs().max()) > 0
    # no target, or three zero weights: that call, launch for launch
    for kw in (dict(depth_loss=opts), dict(depth_target=z),
               dict(depth_target=z, depth_loss=host.DepthLossOptions(eps=EPS))):
        loss1, sq1, ns1, g1 = _step(hr, scene, **kw)
        assert torch.equal(loss1, loss0) and torch.equal(sq1, sq0) and ns1 == ns0
        assert torch.equal(g1, g0) and hr.last_depth_loss is None

    with torch.no_grad():
        terms = hr.render_for_loss(*scene["args"], depth_target=z, depth_eps=EPS)[6]
    loss2, sq2, ns2, g2, all2 = _step(hr, scene, all_grads=True, depth_target=z, depth_loss=opts)
    assert torch.equal(sq2, sq0) and ns2 == ns0 == N_TRAIN * S
    n_valid = int((torch.isfinite(z) & (z > 0)).sum())
    assert n_valid == N_TRAIN - N_TRAIN // 8
    m64 = terms.double().sum(0) / n_valid
    last = hr.last_depth_loss
    assert last.shape == (3,) and last.dtype == torch.float32 and not last.requires_grad
    # each mean: a tree sum of 1024 non-negative terms and one division
    assert bool(((last.double() - m64).abs() <= rc.U * (1.0 + math.log2(N_TRAIN)) * m64).all())
    # loss = fl(loss0 + sum_i fl(lam_i mean_i)): each mean a tree sum of 1024 terms and a division, one
    # product each, three additions -- the summation bound of the distortion term, with those counted
    extra = sum(l * float(m) for l, m in zip(lam, m64))
    want = float(loss0) + extra
    tol = rc.U * (5.0 + math.log2(N_TRAIN)) * (abs(float(loss0)) + extra)
    print("  %s: loss %.9g, want %.9g, tol %.3e, means %s" % (
        route, float(loss2), want, tol, [float(m) for m in m64]))
    assert all(float(m) > 1e-6 for m in m64) and abs(float(loss2) - want) <= tol
    assert not torch.equal(g2, g0)
    assert bool(torch.isfinite(g2).all()) and float((g2 - g0).abs().max()) > 0
    # ... and it is the right one: the op-by-op route's
    _term_against_op_by_op(hr, host, dev, scene, route, all2, all0, depth_target=z, depth_loss=opts)

    # a batch without a single return: the terms are exact zeros and so is their gradient
    none = torch.zeros_like(z)
    none[1::2] = float("nan")
    loss3, sq3, ns3, g3 = _step(hr, scene, depth_target=none, depth_loss=opts)
    assert torch.equal(loss3, loss0) and torch.equal(sq3, sq0) and torch.equal(g3, g0)
    assert bool((hr.last_depth_loss == 0).all())
    _step(hr, scene)
    assert hr.last_depth_loss is None
