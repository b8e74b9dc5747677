"""The one-kernel inference render (f2n_render_rays, Renderer.render_rays, RendererOptions::one_pass)
on the GPU.  Its sample set is the march's, exactly (integer counts, no tolerance); colours, depths and
last_trans meet the bar the project applies between its own routes, _close(a, b, 1e-4), against the
fused march route and the op-by-op route; an all-ones grid gives the bits of no grid; two calls give
the same bits; it reads nothing back, allocates nothing per sample and can be captured in a hipGraph."""
import importlib
import math

import pytest
import torch

from tests.test_gpu_localizer import H_IMG, SIGMAS, W_IMG, _base_pose, _localizer
from tests.test_gpu_occupancy import _march, _march_occ, _pack, _raw_field, _rays, _scene_grid
from tests.test_gpu_pose_grad import _intrinsic, _pose
from tests.test_gpu_render import _close, _setup

pytestmark = pytest.mark.gpu

STEPS = {64: 4.0 / 64, 100: 4.0 / 100, 128: 4.0 / 128, 192: 4.0 / 192, 1024: 1.0 / 256}


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


# ---- 1. the sample set is the march's, exactly ------------------------------------------------------

def _raw_network(f, seed, dev, E=5):
    """The rest of the network around _raw_field's density head: row 0 of w_h / b_h IS that head."""
    g = torch.Generator().manual_seed(seed)
    C = f["L"] * f["F"]
    w_h = (torch.rand(16, C, generator=g) * 2 - 1) / math.sqrt(C)
    w_h[0] = f["w0"].cpu()
    b_h = torch.rand(16, generator=g) * 0.2 - 0.1
    b_h[0] = float(f["b0"][0])
    net = dict(w_h=w_h, b_h=b_h, w1=(torch.rand(64, 32, generator=g) * 2 - 1) / math.sqrt(32),
               b1=torch.rand(64, generator=g) * 0.2 - 0.1,
               w2=(torch.rand(3, 64, generator=g) * 2 - 1) / 8, b2=torch.rand(3, generator=g) * 0.2 - 0.1,
               emb=torch.randn(E, 16, generator=g) * 0.1)
    return {k: v.to(dev).contiguous() for k, v in net.items()}


def _set_bias0(f, net, b):
    f["b0"].fill_(b)
    net["b_h"][0] = b


def _render_rays_raw(capi, f, net, o, d, noise, S, step, words=None, G=0, img=None, bg=None):
    n = o.shape[0]
    dev = o.device
    bg = torch.full((n, 3), 0.5, device=dev) if bg is None else bg
    colors = torch.full((n, 3), float("nan"), device=dev)
    depths = torch.full((n,), float("nan"), device=dev)
    last = torch.full((n,), float("nan"), device=dev)
    kept = torch.full((n,), -1, dtype=torch.int32, device=dev)
    length = torch.full((n,), -1, dtype=torch.int32, device=dev)
    capi.call("render_rays", o, d, noise, f["table16"], f["primes"], f["bias"], f["mul"], net["w_h"],
              net["b_h"], net["w1"], net["b1"], net["w2"], net["b2"],
              net["emb"] if img is not None else None, img, words, G, bg, colors, depths, last, kept,
              length, n, S, step, f["L"], f["F"], f["T"], f["stride"], 1e-4, 3.0, 1e-2)
    return colors, depths, last, kept, length


def _bias_sweep(capi, f, net, o, d, noise, S, step):
    """Biases at which the MARCH itself reports the counts a stride-walking kernel can get wrong: the
    field is a near-uniform fog, so a ray stops where exp(b - 3) * t reaches -ln(1e-4), and the march
    at a probe bias says where that is for these rays.  Everything here comes from f2n_density_march."""
    def bias_for(count, b_ref, c_ref):
        return b_ref + math.log(c_ref / count)
    b_probe = 3.0 + math.log(-math.log(1e-4) / (min(48, S // 2) * step))
    _set_bias0(f, net, b_probe)
    c_probe = float(_march(capi, f, o, d, noise, S, step).float().median())
    assert 4 < c_probe < S, c_probe
    sweep = [0.0, 9.0, 10.0, 12.0]                       # everything; one or two samples
    fine = [64.0 + 0.25 * i for i in range(-12, 13)] if S > 64 else [S - 0.25 * i for i in range(1, 16)]
    sweep += [bias_for(c, b_probe, c_probe) for c in fine]
    last0 = (S - 1) // 64 * 64
    if last0 >= 64:
        sweep += [bias_for(last0 + (S - last0) * fr, b_probe, c_probe) for fr in (0.3, 0.5, 0.7)]
    return sweep


@pytest.mark.parametrize("L,F,T,S,train", [
    (16, 2, 1 << 19, 64, True),
    (16, 2, 1 << 19, 100, True),
    (16, 2, 1 << 19, 128, False),
    (16, 2, 1 << 19, 128, True),
    (16, 2, 1 << 19, 192, False),
    (16, 2, 1 << 19, 1024, True),
    (4, 2, 1 << 19, 192, True),
    (8, 2, 1 << 14, 100, False),
    (8, 8, 1 << 12, 128, True),
    (8, 8, 5000, 192, True),          # T not a power of two
    (8, 1, 3001, 100, False),         # C = 8, F = 1, T not a power of two
    (8, 4, 1 << 12, 128, True),       # C = 32, F = 4
    (16, 4, 1 << 12, 128, True),      # C = 64
])
def test_counts_are_the_marchs_exactly(capi, dev, L, F, T, S, train):
    step = STEPS[S]
    n_rays = 99                                          # not a multiple of the 8 waves of a workgroup
    f = _raw_field(L, F, T, 5.0, seed=5 * L + S + F, dev=dev)
    net = _raw_network(f, seed=S + L, dev=dev)
    o, d, noise = _rays(n_rays, S, seed=S + F + 2, dev=dev, train=train)
    img = torch.randint(0, 5, (n_rays,), generator=torch.Generator().manual_seed(S)).to(torch.int32).to(dev)
    G = 64
    grids = {"ones": torch.full((G ** 3 // 32,), -1, dtype=torch.int32, device=dev),
             "empty": torch.zeros(G ** 3 // 32, dtype=torch.int32, device=dev),
             "random": _pack(torch.rand(G ** 3, generator=torch.Generator().manual_seed(S + 1)) < 0.5).to(dev)}
    c = (torch.arange(G, dtype=torch.float32) + 0.5) * (4.0 / G) - 2.0
    cz, cy, cx = torch.meshgrid(c, c, c, indexing="ij")
    r = (cx * cx + cy * cy + cz * cz).sqrt()
    grids["shell"] = _pack(((r > 0.35) & (r < 1.2)).reshape(-1)).to(dev)

    seen, seen_grid = set(), set()
    for b in _bias_sweep(capi, f, net, o, d, noise, S, step):
        _set_bias0(f, net, b)
        want = _march(capi, f, o, d, noise, S, step)
        colors, depths, last, kept, length = _render_rays_raw(capi, f, net, o, d, noise, S, step, img=img)
        assert torch.equal(kept, want), b
        assert torch.equal(length, want), b
        assert bool(torch.isfinite(colors).all() and torch.isfinite(depths).all() and torch.isfinite(last).all())
        seen |= set(want.cpu().tolist())
        for kind, words in grids.items():
            want_kept, want_len = _march_occ(capi, f, o, d, noise, S, step, words, G)
            got = _render_rays_raw(capi, f, net, o, d, noise, S, step, words, G, img=img)
            assert torch.equal(got[3], want_kept), (b, kind)
            assert torch.equal(got[4], want_len), (b, kind)
            assert bool(torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all())
            if kind == "ones":                           # ... and the bits of no grid
                for x, y in zip(got, (colors, depths, last, kept, length)):
                    assert torch.equal(x, y), (b, kind)
            elif kind == "empty":
                assert int(got[3].sum()) == 0 and bool((got[4] == S).all())
                assert bool((got[0] == 0.5).all() and (got[2] == 1).all() and (got[1] == 0).all())
            else:
                seen_grid.add(len(set(want_len.cpu().tolist())))
    # conditions on the inputs (the march's own counts), not on the kernel under test
    last0 = (S - 1) // 64 * 64
    assert seen & {1, 2}, sorted(seen)
    assert S in seen and 63 in seen, sorted(seen)
    if S > 64:
        assert {64, 65} <= seen, sorted(seen)
    assert any(last0 < k < S for k in seen), sorted(seen)
    assert max(seen_grid) > 3                            # a grid gives rays of one launch different lengths


# ---- 2. colours, depths, last_trans against the existing routes -------------------------------------

_SCENES = {}


def _scene(host, L, F, log2_T, S, n_rays, seed):
    """One oracle-initialised renderer per shape, shared by the tests below (bias 0 of the head is set
    per case; nothing else is changed)."""
    key = (L, F, log2_T, S, n_rays, seed)
    if key not in _SCENES:
        _SCENES[key] = _setup(host, L, F, log2_T, S, STEPS[S], n_rays, 0.0, seed)[1:]
    return _SCENES[key]


def _set_head_bias(hr, b):
    with torch.no_grad():
        hr.named_parameters()["scene_field.mlp.bias"][0] = b


def _seg_sum(weights, idx):
    """per-ray sum of ragged per-sample weights in f64"""
    n = idx.shape[0]
    ray = torch.repeat_interleave(torch.arange(n, device=weights.device), (idx[:, 1] - idx[:, 0]).long())
    return torch.zeros(n, dtype=torch.float64, device=weights.device).index_add_(0, ray, weights.double())


def _against_routes(hr, dev, o, d, emb, noise, bg, mode, routes):
    to = lambda v: None if v is None else v.to(dev)
    with torch.no_grad():
        colors, depths, last, kept = hr.render_rays(to(o), to(d), to(emb), mode, to(noise), to(bg))
        for fused in routes:
            hr.set_fused(fused)
            hr.set_dense_first_pass(0)
            c, dp, w, idx = hr.render(to(o), to(d), to(emb), mode, to(noise), to(bg))
            hr.set_fused(True)
            assert torch.equal(kept, idx[:, 1] - idx[:, 0]), fused
            _close(colors, c, 1e-4)
            _close(depths, dp, 1e-4)
            # last_trans: no existing route hands it out; what they do hand out is the weights, whose
            # sum per ray is the opacity 1 - last_trans.  The bar is applied to that quantity (1 minus
            # a sum of f32 weights cannot resolve a last_trans of 1e-4 to four digits)
            _close(1.0 - last.double(), _seg_sum(w, idx), 1e-4)
    return colors, depths, last, kept


@pytest.mark.parametrize("S,bias0", [
    (128, 0.0), (128, 1.0), (192, 0.0), (192, 1.0),    # nothing terminates: every stride link carries weight
    (100, 0.0), (100, 1.0),                            # a partial last stride
    (128, 4.0), (192, 4.0),                            # stops in the last stride
    (128, 5.0), (192, 5.0), (100, 5.0),                # stops in the first
])
def test_render_rays_against_march_and_op_by_op(host, dev, S, bias0):
    hr, o, d, noise, bg, gt, emb = _scene(host, 16, 2, 19, S, 96, 31)
    _set_head_bias(hr, bias0)
    hr.set_occupancy(None)
    # VALIDATE without noise (grey background), and TRAIN-mode inputs under no_grad: noise, a
    # background per ray and the appearance embedding
    v = _against_routes(hr, dev, o, d, None, None, None, "validate", (True, False))
    t = _against_routes(hr, dev, o, d, emb, noise, bg, "train", (True, False))
    if bias0 <= 1.0:
        # the inputs can show a lost stride link: every ray ends half transparent with more than a
        # tenth of its weight beyond the first stride (a dropped carry is an error of order 0.1)
        for colors, depths, last, kept in (v, t):
            assert bool((kept == S).all())
            assert bool(((last > 0.05) & (last < 0.95)).all())
        to = lambda x: x.to(dev)
        with torch.no_grad():
            hr.set_dense_first_pass(0)
            _, _, w, idx = hr.render(to(o), to(d), None, "validate")
        w = w.reshape(96, S)
        assert bool((w[:, 64:].sum(1) > 0.1 * w.sum(1)).all())
    elif bias0 == 4.0:
        assert bool(((v[3] > (S - 1) // 64 * 64) & (v[3] < S)).any())
    else:
        assert bool((v[3] < 64).all())
    assert not torch.equal(v[0], t[0])                   # the TRAIN inputs are in use


@pytest.mark.parametrize("L,F,log2_T,S,bias0", [
    (4, 2, 19, 192, 1.0),        # C = 8
    (8, 2, 14, 100, 0.0),        # C = 16
    (8, 8, 12, 128, 4.0),        # C = 64, F = 8
])
def test_render_rays_other_widths(host, dev, L, F, log2_T, S, bias0):
    hr, o, d, noise, bg, gt, emb = _scene(host, L, F, log2_T, S, 77, 13)
    _set_head_bias(hr, bias0)
    _against_routes(hr, dev, o, d, None, None, None, "validate", (True, False))
    _against_routes(hr, dev, o, d, emb, noise, bg, "train", (True,))


@pytest.mark.parametrize("kind", ["shell", "random"])
def test_render_rays_with_grid_against_both_routes(host, dev, kind):
    # the shape and seed of test_validate_render_all_rays_with_grid, on which the two existing routes
    # already agree in their bounds
    hr, o, d, noise, bg, gt, emb = _scene(host, 16, 2, 19, 1024, 200, 23)
    _set_head_bias(hr, 5.0)
    hr.set_occupancy(_scene_grid(host, dev, 128, kind, 2))
    try:
        v = _against_routes(hr, dev, o, d, None, None, None, "validate", (True, False))
        _against_routes(hr, dev, o, d, emb, noise, bg, "train", (True,))
        assert len(set(v[3].cpu().tolist())) > 3         # rays of different lengths in one launch
    finally:
        hr.set_occupancy(None)


# ---- 3. grid semantics ------------------------------------------------------------------------------

def test_all_ones_grid_is_no_grid_and_empty_grid_is_background(host, dev):
    hr, o, d, noise, bg, gt, emb = _scene(host, 16, 2, 19, 128, 96, 31)
    _set_head_bias(hr, 4.0)
    to = lambda v: v.to(dev)
    args = (to(o), to(d), to(emb), "train", to(noise), to(bg))
    hr.set_occupancy(None)
    plain = hr.render_rays(*args)
    try:
        hr.set_occupancy(host.OccupancyGrid(64, str(dev)))           # fresh: all ones
        for a, b in zip(hr.render_rays(*args), plain):
            assert torch.equal(a, b)
        empty = host.OccupancyGrid(64, str(dev))
        empty.set_bits(torch.zeros(64, 64, 64, dtype=torch.bool, device=dev))
        hr.set_occupancy(empty)
        colors, depths, last, kept = hr.render_rays(*args)
        assert torch.equal(colors, to(bg)) and int(kept.abs().sum()) == 0
        assert bool((last == 1).all()) and bool((depths == 0).all())
    finally:
        hr.set_occupancy(None)


# ---- 4. determinism and chunking --------------------------------------------------------------------

def test_determinism_chunks_image_and_off_means_off(host, dev):
    hr, o, d, noise, bg, gt, emb = _scene(host, 16, 2, 19, 128, 1000, 29)
    _set_head_bias(hr, 4.0)
    hr.set_occupancy(None)
    to = lambda v: v.to(dev)
    o, d = to(o), to(d)
    with torch.no_grad():
        hr.set_dense_first_pass(0)
        before = hr.render_all_rays(o, d, 256)
        assert not hr.one_pass_applies()
        a = hr.render_rays(o, d, None, "validate")
        b = hr.render_rays(o, d, None, "validate")
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        hr.set_one_pass(True)
        assert hr.one_pass_applies()
        colors, depths = hr.render_all_rays(o, d, 256)
        assert colors.shape == (1000, 3) and depths.shape == (1000, 1)
        for lo in range(0, 1000, 256):
            c, dp, _, _ = hr.render_rays(o[lo:lo + 256], d[lo:lo + 256], None, "validate")
            assert torch.equal(colors[lo:lo + 256], c) and torch.equal(depths[lo:lo + 256, 0], dp)
        _close(colors, before[0], 1e-4)
        _close(depths, before[1], 1e-4)
        # render_image: the default route's image under the same bar
        pose = _pose(torch.Generator().manual_seed(3))[0].to(dev)
        K = _intrinsic(1, 16, 24)[0].to(dev)
        img1, dep1 = hr.render_image(pose, K, 16, 24, 100)
        hr.set_one_pass(False)
        img0, dep0 = hr.render_image(pose, K, 16, 24, 100)
        assert img1.shape == (16, 24, 3) and dep1.shape == (16, 24, 3)
        _close(img1, img0, 1e-4)
        _close(dep1, dep0, 1e-4)
        assert float(img0.std()) > 0
        # off again: what it was before the option was touched
        after = hr.render_all_rays(o, d, 256)
        for x, y in zip(after, before):
            assert torch.equal(x, y)
    # with grad mode on and parameters that require grad the option does not apply
    hr.set_one_pass(True)
    assert not hr.one_pass_applies()
    with torch.no_grad():
        assert hr.one_pass_applies()
    hr.set_one_pass(False)


# ---- 5. no host read, no per-sample memory ----------------------------------------------------------

def test_no_per_sample_memory_and_one_graph(host, dev):
    n, S = 4096, 1024
    hr, o, d, noise, bg, gt, emb = _scene(host, 16, 2, 19, S, n, 37)
    _set_head_bias(hr, 5.0)
    hr.set_occupancy(None)
    to = lambda v: v.to(dev)
    o, d = to(o), to(d)
    bg = to(bg)
    with torch.no_grad():
        hr.render_rays(o, d, None, "validate", None, bg)              # warm-up
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = hr.render_rays(o, d, None, "validate", None, bg)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
        assert rise < 1024 * n, rise                                  # (the sampler's grid: 32 KiB per ray)
        del out
        # one hipGraph: warm-up on a side stream, one stream, a linear chain
        o2, d2 = o.clone(), d.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                hr.render_rays(o2, d2, None, "validate", None, bg)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            captured = hr.render_rays(o2, d2, None, "validate", None, bg)
        # new rays, written in place
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(dev)
        o2.copy_(o[perm])
        d2.copy_(d[perm] * 1.5)
        g.replay()
        torch.cuda.synchronize()
        eager = hr.render_rays(o2, d2, None, "validate", None, bg)
        for x, y in zip(captured, eager):
            assert torch.equal(x, y)
        first = hr.render_rays(o, d, None, "validate", None, bg)
        assert not torch.equal(first[0], eager[0])


# ---- 6. Localizer -----------------------------------------------------------------------------------

def test_localizer_one_pass(host, dev):
    P, K = 8, 64
    loc, hr, Kc = _localizer(host, dev, 31)
    param = host.LocalizerParam()
    assert param.one_pass is False
    param.render_pixel_num = K
    param.one_pass = True
    g = torch.Generator().manual_seed(31)
    poses = host.perturb_poses(_base_pose(31).to(dev), torch.randn(P, 6, generator=g).to(dev), SIGMAS)
    image = torch.rand(H_IMG, W_IMG, 3, generator=g)
    pix = torch.randperm(H_IMG * W_IMG, generator=g)[:K]
    ij = torch.stack([pix // W_IMG, pix % W_IMG], 1).to(torch.int32)
    hr.set_dense_first_pass(0)
    w0, loss0, colors0, _ = loc.evaluate_poses_full(poses, image.to(dev), ij.to(dev))
    assert not hr.one_pass_applies()
    loc1 = host.Localizer(param, hr, Kc.to(dev), H_IMG, W_IMG, torch.zeros(3).to(dev), 1.0)
    with torch.no_grad():
        assert hr.one_pass_applies()
    w1, loss1, colors1, _ = loc1.evaluate_poses_full(poses, image.to(dev), ij.to(dev))
    hr.set_one_pass(False)
    assert colors1.shape == (P, K, 3)
    _close(colors1, colors0, 1e-4)
    assert int(w1.argmax()) == int(w0.argmax())
    assert float(loss0.max() - loss0.min()) > 0
