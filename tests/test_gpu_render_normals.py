"""RendererOptions::normals on the GPU: off by default and then invisible; on, the route's colours,
depths, weights and bounds keep their bits; the normals are the float64 recomposition sum_k w_k n^_k of
tests/density_grad_model.py over the kept samples, within its per-ray bound, on the op-by-op, march and
dense routes; with an occupancy grid; with rays that require grad; whatever one_pass says; and as a
whole image.  130 rays, S = 128, VALIDATE, L F = 32.

The recomposition's bound for samples of a real ray.  The model's generator redraws samples that are
ambiguous (a cell face within the rounding of pt: the kernel may sit in the neighbouring cell, where
the gradient's normal component jumps) or whose gradient is shorter than 64 of its own bound (n^ is
then ill-conditioned and the first-order rule says nothing).  A render cannot redraw its samples, so
exactly those samples take their gradient from f2n_density_grad's own output at the same positions,
with E_g = 0 (the rule of tests/test_gpu_density_grad.py); every other sample keeps the model's n^ and
its bound.  The per-ray bound stays of the order of the rounding on every ray, which the test asserts."""
import importlib

import numpy as np
import pytest
import torch

from tests import density_grad_model as M
from tests.test_gpu_occupancy import _scene_grid
from tests.test_gpu_pose_grad import _intrinsic, _pose
from tests.test_gpu_render import _close, _setup

pytestmark = pytest.mark.gpu

L, F, LOG2_T, S, STEP, N_RAYS = 16, 2, 14, 128, 4.0 / 128, 130
ROUTES = {"op_by_op": (False, 0), "march": (True, 0), "dense": (True, 1)}


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


@pytest.fixture(scope="module")
def scene(host, dev):
    """one renderer and one set of rays for the module.  Every test picks its route itself (_route) and
    leaves the normals option, the occupancy grid, one_pass and the pixel tiles as it found them."""
    oracle, hr, o, d, noise, bg, gt, emb = _setup(host, L, F, LOG2_T, S, STEP, N_RAYS, 5.0, 41)
    return hr, o.to(dev), d.to(dev)


def _route(hr, name):
    fused, dense = ROUTES[name]
    hr.set_fused(fused)
    hr.set_dense_first_pass(dense)


def _render(hr, o, d, normals):
    hr.set_normals(normals)
    try:
        with torch.no_grad():
            r = hr.render_result(o, d, None, "validate")
    finally:
        hr.set_normals(False)
    return r


def _same(a, b):
    for k in ("colors", "depths", "weights", "idx_start_end"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_default_off_and_invisible(host, dev, scene):
    hr, o, d = scene
    fresh = _setup(host, L, F, LOG2_T, S, STEP, N_RAYS, 5.0, 41)[1]      # never heard of the option
    for name in ROUTES:
        _route(hr, name)
        _route(fresh, name)
        with torch.no_grad():
            want = fresh.render_result(o, d, None, "validate")
        assert want.normals is None and not fresh.normals
        _render(hr, o, d, True)                                           # set ...
        got = _render(hr, o, d, False)                                    # ... and unset again
        assert got.normals is None
        _same(got, want)
        # the tuple render() returns is what it was
        with torch.no_grad():
            tup = hr.render(o, d, None, "validate")
        assert len(tup) == 4 and torch.equal(tup[0], want.colors)


@pytest.mark.parametrize("name", list(ROUTES))
def test_same_route_bits_with_normals_on(capi, dev, scene, name):
    """the off arm switches the lean dense route off through its own option, so both arms take the
    same kernels"""
    hr, o, d = scene
    _route(hr, name)
    with capi.option("DENSE_LEAN", 1):
        off = _render(hr, o, d, False)
    on = _render(hr, o, d, True)
    _same(on, off)
    assert on.normals.shape == (N_RAYS, 3) and not on.normals.requires_grad
    assert bool(torch.isfinite(on.normals).all()) and float(on.normals.abs().max()) > 0
    assert torch.equal(on.normals, _render(hr, o, d, True).normals)


@pytest.fixture(scope="module")
def recomposition(scene):
    """the float64 model of every sample of the sampler's grid for these rays, once"""
    hr, o, d = scene
    f = hr.scene_field
    fld = dict(L=L, F=F, T=f.local_size, stride=f.level_stride,
               table16=f.table_f16().cpu().reshape(-1).view(torch.int16), primes=f.prim_pool.cpu(),
               bias=f.bias_pool.detach().cpu(), mul=f.level_mul.cpu())
    w0 = f.density_head()[0].cpu().numpy()
    pts = hr.pts_sampler.get_samples(o, d, "validate", None)[0].cpu().contiguous()
    assert pts.shape == (N_RAYS * S, 3)
    m = M.point_model(fld, pts, w0=w0)
    nh, E_nh = M.normal_model(m["g"], m["E_g"])
    with np.errstate(invalid="ignore"):
        loose = M.ambiguous(fld, pts) | (np.linalg.norm(m["g"], axis=1) <
                                         M.MIN_G_OVER_E * np.linalg.norm(m["E_g"], axis=1))
    # those samples take their gradient from f2n_density_grad at the same positions (held to the model
    # on its own in tests/test_gpu_density_grad.py): what is left is the normalisation and the sum
    g_dev = f.density_grad(pts.to(o.device)).cpu().numpy().astype(np.float64)
    nh_dev, E_dev = M.normal_model(g_dev, np.zeros_like(g_dev))
    nh[loose], E_nh[loose] = nh_dev[loose], E_dev[loose]
    return nh, E_nh, float(loose.mean())


@pytest.mark.parametrize("name", list(ROUTES))
def test_normals_are_the_float64_recomposition(dev, scene, recomposition, name):
    """without a grid the kept samples are a per-ray prefix of the sampler's grid"""
    hr, o, d = scene
    nh_all, E_all, loose = recomposition
    _route(hr, name)
    r = _render(hr, o, d, True)
    b = r.idx_start_end.cpu()
    length = (b[:, 1] - b[:, 0]).numpy()
    assert 0 < length.min() < S                                    # rays terminate: a real prefix
    keep = np.concatenate([np.arange(i * S, i * S + n) for i, n in enumerate(length)])
    N, E_N = M.ray_model(b, r.weights.cpu(), nh_all[keep], E_all[keep])
    ratio = M.ratio(r.normals, N, E_N)
    print("\n%s: largest |err| / E %.3f; %.4f of the samples take the device's own gradient; median E_N %.2e, "
          "largest E_N %.2e" % (name, float(ratio.max()), loose, float(np.median(E_N)), float(E_N.max())))
    # expected share of ambiguous samples: 3 axes x 16 levels x a band of 4 E_pt around each face,
    # E_pt = u |pt| + E_x mul of the order of 1e-4 to 3e-4 cells: a few per cent
    assert loose < 0.1
    # the bound stays small on EVERY ray.  A model sample has |g| >= 64 |E_g|, so per component
    # E_n^ <= E_g,c / |g| + |n^_c| |E_g| / |g| <= (1 + sqrt 3) / 64 < 1 / 16 at the very worst; a device
    # sample carries a few u.  Printed: what it is in fact.
    opacity = np.zeros(N_RAYS)
    np.add.at(opacity, np.repeat(np.arange(N_RAYS), length), r.weights.cpu().numpy().astype(np.float64))
    worst = float((E_N.max(1) / opacity).max())
    print("largest E_N / opacity over the rays %.2e" % worst)
    assert worst < 1.0 / 16
    assert float(ratio.max()) <= M.BAR


def test_occupancy_grid(host, dev, scene):
    hr, o, d = scene
    try:
        _route(hr, "march")
        plain = _render(hr, o, d, True)
        ones = host.OccupancyGrid(64, str(dev))
        hr.set_occupancy(ones)
        got = _render(hr, o, d, True)
        _same(got, plain)
        assert torch.equal(got.normals, plain.normals)
        hr.set_occupancy(_scene_grid(host, dev, 64, "random", 5))
        res = {}
        for name in ("march", "op_by_op"):
            _route(hr, name)
            res[name] = _render(hr, o, d, True)
        assert torch.equal(res["march"].idx_start_end, res["op_by_op"].idx_start_end)
        assert not torch.equal(res["march"].idx_start_end, plain.idx_start_end)         # the grid is in use
        _close(res["march"].normals, res["op_by_op"].normals, 1e-4)
    finally:
        hr.set_occupancy(None)


def test_rays_that_require_grad_and_one_pass(dev, scene):
    hr, o, d = scene
    _route(hr, "march")
    want = _render(hr, o, d, True)
    hr.set_normals(True)
    try:
        og, dg = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
        r = hr.render_result(og, dg, None, "validate")                     # op by op, under autograd
        assert r.colors.requires_grad and not r.normals.requires_grad
        # When this was written the ATen sampler of this route rounded o + t d/|d| in another order than
        # the sampler kernel: a last-bit difference of a position is 2e-4 of a cell at the finest level
        # (pt is of the order of 2000), which the piecewise-linear gradient passes on -- the same vectors,
        # not the same bits.  (The route samples with the kernel now, PtsSampler::get_samples_grad; the
        # allowance stays as it was.)
        assert bool(torch.isfinite(r.normals).all())
        assert float((r.normals - want.normals).abs().max()) <= 1e-2 * float(want.normals.abs().max())
        r.colors.sum().backward()
        assert bool(torch.isfinite(og.grad).all())
    finally:
        hr.set_normals(False)
    with torch.no_grad():
        a = hr.render_all_rays_with_normals(o, d, 48)
        hr.set_one_pass(True)
        try:
            assert hr.one_pass_applies()
            b = hr.render_all_rays_with_normals(o, d, 48)
        finally:
            hr.set_one_pass(False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not hr.normals                                                  # the call left the option off


def test_whole_image(host, dev, scene):
    hr = scene[0]
    _route(hr, "march")
    h, w, batch = 37, 29, 100                                              # 100 divides neither side
    pose = _pose(torch.Generator().manual_seed(3))[0].to(dev)
    K = _intrinsic(1, h, w)[0].to(dev)
    with torch.no_grad():
        colors, depths, normals = hr.render_image_with_normals(pose, K, h, w, batch)
        with hr_capi().option("DENSE_LEAN", 1):
            img, dep = hr.render_image(pose, K, h, w, batch)
        o, d = host.get_view_rays(pose, K, h, w)
        chunks = [_render(hr, o[lo:lo + batch].contiguous(), d[lo:lo + batch].contiguous(), True)
                  for lo in range(0, h * w, batch)]
    assert colors.shape == (h, w, 3) and depths.shape == (h, w, 3) and normals.shape == (h, w, 3)
    assert torch.equal(normals.reshape(-1, 3), torch.cat([c.normals for c in chunks]))
    assert torch.equal(colors.reshape(-1, 3), torch.cat([c.colors for c in chunks]).clip(0, 1))
    assert torch.equal(colors, img) and torch.equal(depths, dep)
    assert float(normals.abs().max()) > 0


def test_whole_image_in_pixel_tiles(dev, scene):
    """a view the default 8 x 8 tiles divide: the tile traversal and its un-permute give the row-major
    image, normals included"""
    hr = scene[0]
    _route(hr, "march")
    h, w, batch = 16, 32, 100
    pose = _pose(torch.Generator().manual_seed(4))[0].to(dev)
    K = _intrinsic(1, h, w)[0].to(dev)
    with torch.no_grad():
        tiled = hr.render_image_with_normals(pose, K, h, w, batch)
        hr.set_pixel_tiles(0)
        try:
            rows = hr.render_image_with_normals(pose, K, h, w, batch)
        finally:
            hr.set_pixel_tiles(8)
        again = hr.render_image_with_normals(pose, K, h, w, batch)
    for a, b, c in zip(tiled, rows, again):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert float(tiled[2].abs().max()) > 0 and float(tiled[2].std()) > 0


def test_dense_guesses_launch_normals_on_the_accepted_result(host, dev, capi):
    """A scene that keeps every sample: the dense route shades all samples as a guess (the small-chunk
    branch, then the density-margin branch) and the normals belong to the accepted result."""
    hr, o, d = _setup(host, L, F, LOG2_T, S, STEP, N_RAYS, 0.0, 43)[1:4]
    o, d = o.to(dev), d.to(dev)
    _route(hr, "march")
    want = _render(hr, o, d, True)
    assert hr.last_kept_fraction == 1.0
    _route(hr, "dense")
    for margin in (2 << 20, 1):
        hr.set_margin_min_samples(margin)
        with capi.option("DENSE_LEAN", 1):
            off = _render(hr, o, d, False)
        on = _render(hr, o, d, True)
        assert hr.last_kept_fraction == 1.0
        _same(on, off)
        assert on.normals.shape == (N_RAYS, 3)
        _close(on.normals, want.normals, 1e-4)


def hr_capi():
    return importlib.import_module("f2-nerf_amd").capi
