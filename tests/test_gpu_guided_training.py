"""Error-guided sampling through the host module: ErrorMap against the numpy model,
sample_guided_rays against get_rays_from_cameras and sample_masked_rays, train_step with
RaySupervision.want_colors, and the whole draw -> step -> accumulate -> update sequence run twice
and once under hipGraph capture.  The renderer configurations are those of
tests/test_gpu_supervised_step.py (L = 4, F = 2, T = 2^12, 128 samples, 192 rays) and of the
capture test of tests/test_gpu_render.py (thin medium, dense first pass, deferred check)."""
import importlib

import numpy as np
import pytest
import torch

from tests import error_map_model as em
from tests.test_gpu_render import _setup
from tests.test_gpu_weight_dist import _route

pytestmark = pytest.mark.gpu

E, H, W, GH, GW = 7, 37, 70, 5, 8
SEED = 0x0BADC0DE5EED1234
VW = 1e-2


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


@pytest.fixture(scope="module")
def data(dev):
    """mask (fraction 0.6, image 3 empty), cameras and RGBA images of the set"""
    rng = np.random.RandomState(77)
    mask = (rng.rand(E, H, W) < 0.6).astype(np.uint8)
    mask[3] = 0
    g = torch.Generator().manual_seed(5)
    poses = torch.eye(4)[:3].repeat(E, 1, 1)
    poses[:, :, 3] = torch.randn(E, 3, generator=g) * 0.25
    intr = torch.tensor([[60.0, 0, W / 2], [0, 60.0, H / 2], [0, 0, 1]]).repeat(E, 1, 1)
    images = torch.rand(E, H, W, 4, generator=g)
    return dict(mask=mask, poses=poses.to(dev), intr=intr.to(dev), images=images.to(dev))


def _map(host, dev, data, u=0.25, decay=0.5, attempts=32, masked=True):
    opt = host.ErrorMapOptions(gh=GH, gw=GW, decay=decay, uniform_fraction=u, attempts=attempts)
    pm = host.PixelMask.from_mask(torch.from_numpy(data["mask"]).to(dev)) if masked else None
    return host.ErrorMap(E, H, W, opt, mask=pm), pm


def test_options_defaults(host):
    o = host.ErrorMapOptions()
    assert (o.gh, o.gw, o.attempts, o.init_value) == (32, 32, 32, 1.0)
    assert 0 < o.uniform_fraction < 1 and 0 < o.decay < 1


@pytest.mark.parametrize("masked", [True, False])
def test_error_map_follows_the_model(host, dev, data, masked):
    """a fresh map, one accumulate + update, and the draws before and after, against the model"""
    m, _ = _map(host, dev, data, masked=masked)
    grid = em.Grid(E, H, W, GH, GW)
    mask = data["mask"] if masked else None
    counts = em.cell_counts(grid, mask)
    value = np.ones(grid.n_cells, dtype=np.float32)
    cdf = em.cdf(value, counts)
    assert m.n_cells == grid.n_cells
    assert np.array_equal(m.counts.cpu().numpy(), counts)
    assert np.array_equal(m.cdf.cpu().numpy().view(np.uint64), cdf)
    assert int(m.n_valid) == (int((mask != 0).sum()) if masked else E * H * W)
    n = 1024
    for rnd in range(2):
        cam, ij, tries, wgt = m.draw(n, SEED + rnd)
        want = em.draw(grid, mask, value, cdf, n, SEED + rnd, 32, 0.25)
        assert np.array_equal(cam.cpu().numpy(), want[0]) and np.array_equal(ij.cpu().numpy(), want[1])
        assert np.array_equal(tries.cpu().numpy(), want[2])
        err = np.abs(wgt.cpu().numpy().astype(np.float64) - want[3])
        assert (err <= 2 * em.ulp_f32(want[3])).all()
        if rnd == 0:
            assert (want[3][want[2] > 0] == 1.0).all()        # equal values: a uniform first draw
        colors = (torch.rand(n, 3, generator=torch.Generator().manual_seed(rnd)) * 256).floor() / 256
        gt = torch.zeros(n, 3)
        m.accumulate(colors.to(dev), gt.to(dev), cam, ij, wgt)
        m.update()
        acc_sum = np.zeros(grid.n_cells, dtype=np.uint64)
        acc_cnt = np.zeros(grid.n_cells, dtype=np.uint32)
        em.accumulate(grid, acc_sum, acc_cnt, colors.numpy(), gt.numpy(), want[0], want[1],
                      want[3].astype(np.float32))
        em.apply(value, acc_sum, acc_cnt, 0.5)
        cdf = em.cdf(value, counts)
        assert np.array_equal(m.value.cpu().numpy().view(np.int32), value.view(np.int32))
        assert np.array_equal(m.cdf.cpu().numpy().view(np.uint64), cdf)
        assert not bool(m.acc_sum.any()) and not bool(m.acc_cnt.any())


def test_sample_guided_rays(host, dev, data):
    n = 257
    m, pm = _map(host, dev, data)
    # move the map away from uniform first, so the guided branch has something to follow
    cam, ij, tries, wgt = m.draw(n, 3)
    m.accumulate(torch.rand(n, 3, device=dev), torch.zeros(n, 3, device=dev), cam, ij, wgt)
    m.update()
    b = host.sample_guided_rays(data["poses"], data["intr"], m, n, SEED, images=data["images"])
    cam, ij, tries, wgt = m.draw(n, SEED)
    assert torch.equal(b["cam"], cam) and torch.equal(b["ij"], ij) and torch.equal(b["tries"], tries)
    kept = wgt[tries > 0]
    assert torch.equal(b["ray_weight"], wgt) and 0 < float(kept.min()) < 1 < float(kept.max()) <= 4
    o, d = host.get_rays_from_cameras(data["poses"], data["intr"], b["cam"], b["ij"])
    assert torch.equal(b["rays_o"], o) and torch.equal(b["rays_d"], d)       # the same launch: same bits
    px = data["images"][b["cam"].long(), b["ij"][:, 0].long(), b["ij"][:, 1].long()]
    assert torch.equal(b["gt"], px[:, :3]) and torch.equal(b["alpha"], px[:, 3])
    valid = torch.from_numpy(data["mask"]).to(dev)[b["cam"].long(), b["ij"][:, 0].long(), b["ij"][:, 1].long()]
    assert bool((valid != 0).all()) and bool((b["cam"] != 3).all())
    # lens distortion takes the other launch, on the same pixels
    dist = torch.tensor([[0.05, -0.01, 1e-3, -2e-3]]).repeat(E, 1).to(dev)
    bd = host.sample_guided_rays(data["poses"], data["intr"], m, n, SEED, dist=dist)
    od, dd = host.get_rays_from_cameras(data["poses"], data["intr"], bd["cam"], bd["ij"], dist=dist)
    assert torch.equal(bd["cam"], cam) and torch.equal(bd["rays_o"], od) and torch.equal(bd["rays_d"], dd)
    assert not torch.equal(dd, d) and bd["gt"] is None


@pytest.mark.parametrize("attempts", [32, 2])
def test_uniform_fraction_one_is_sample_masked_rays(host, dev, data, attempts):
    n = 257
    m, pm = _map(host, dev, data, u=1.0, attempts=attempts)
    cam, ij, tries, wgt = m.draw(n, 3)
    m.accumulate(torch.rand(n, 3, device=dev), torch.zeros(n, 3, device=dev), cam, ij, wgt)
    m.update()                                                   # a non-uniform map changes nothing
    a = host.sample_guided_rays(data["poses"], data["intr"], m, n, SEED, images=data["images"])
    b = host.sample_masked_rays(data["poses"], data["intr"], pm, n, SEED, images=data["images"],
                                attempts=attempts)
    assert set(a) == set(b)
    for k in b:
        assert torch.equal(a[k], b[k]), k
    if attempts == 2:
        assert 0 < int((a["ray_weight"] == 0).sum()) < n


def test_want_colors_changes_nothing_else(host, capi, dev):
    N, S = 192, 128
    _, hr, o, d, noise, bg, gt, emb = _setup(host, 4, 2, 12, S, 4.0 / S, N, 4.0, 41)
    o, d, noise, bg, gt, emb = (v.to(dev) for v in (o, d, noise, bg, gt, emb))
    _route(hr, host, dev, "march", N)
    m = torch.rand(N, generator=torch.Generator().manual_seed(1)).to(dev)
    m[::7] = 0.0

    def step(sup):
        hr.zero_grad()
        out = (hr.train_step(o, d, emb, gt, VW, noise, bg, True) if sup is None else
               hr.train_step_supervised(o, d, emb, gt, sup, VW, noise, bg, True))
        torch.cuda.synchronize()
        return out, hr.grads()["scene_field.feat_pool"].clone()

    capi.set_option("BWD_PHASES", 1)
    try:
        colors = hr.render_for_loss(o, d, emb, "train", noise, bg)[0].detach()
        for weights in (m, None):
            off, g_off = step(host.RaySupervision(ray_weight=weights))
            on, g_on = step(host.RaySupervision(ray_weight=weights, want_colors=True))
            assert len(off) == 5 and len(on) == 6
            assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1]) and on[2:4] == off[2:4]
            assert torch.equal(g_on, g_off) and float(g_off.abs().max()) > 0
            assert on[5].shape == (N, 3) and not on[5].requires_grad and torch.equal(on[5], colors)
            if weights is None:
                plain, g_plain = step(None)                    # the unsupervised step itself
                assert on[4] is None and torch.equal(on[0], plain[0]) and torch.equal(g_on, g_plain)
            else:
                assert torch.equal(on[4], off[4])
    finally:
        capi.set_option("BWD_PHASES", 0)


def test_sequence_repeats_and_graphs(host, dev, data):
    """draw -> step -> accumulate -> update: twice from the same state with equal bits, and once
    under capture (warm-up outside it) with the replay equal to eager"""
    n, S = 96, 64
    _, hr, _, _, noise, bg, _, _ = _setup(host, 4, 2, 14, S, 4.0 / S, n, -3.0, 33)
    noise, bg = noise.to(dev), bg.to(dev)
    hr.set_fused(True)
    hr.set_fused_shade(True)
    hr.set_dense_first_pass(1)
    hr.set_deferred_check(True)

    def sequence(m, rounds):
        out = []
        for rnd in range(rounds):
            b = host.sample_guided_rays(data["poses"], data["intr"], m, n, SEED + rnd,
                                        images=data["images"][..., :3])
            hr.zero_grad()
            sup = host.RaySupervision(ray_weight=b["ray_weight"], want_colors=True)
            step = hr.train_step_supervised(b["rays_o"], b["rays_d"], b["cam"], b["gt"], sup, VW, noise,
                                            bg, True)
            m.accumulate(step[5], b["gt"], b["cam"], b["ij"], b["ray_weight"])
            m.update()
            out += [step[0], step[5], b["cam"], b["ij"], b["ray_weight"]]
        return out

    def state(m, out):
        torch.cuda.synchronize()
        return [t.clone() for t in out] + [m.value.clone(), m.cdf.clone()]

    first_map, _ = _map(host, dev, data)
    first = state(first_map, sequence(first_map, 2))
    second_map, _ = _map(host, dev, data)
    second = state(second_map, sequence(second_map, 2))
    assert len(first) == len(second) == 12
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert not torch.equal(first[-2], torch.ones_like(first[-2]))            # the map moved
    assert not torch.equal(first[2], first[7])                               # and so did the draw
    assert hr.deferred_check_ok()
    # one round as a hipGraph: warm-up on a side stream first, as capture requires
    eager_map, _ = _map(host, dev, data)
    eager = state(eager_map, sequence(eager_map, 1))
    warm_map, _ = _map(host, dev, data)
    graph_map, _ = _map(host, dev, data)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sequence(warm_map, 2)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        captured = sequence(graph_map, 1)
    g.replay()
    replayed = state(graph_map, captured)
    for a, b in zip(replayed, eager):
        assert torch.equal(a, b)
    assert hr.deferred_check_ok()
