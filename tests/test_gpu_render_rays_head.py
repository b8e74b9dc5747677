"""The one-pass render with short rays eight to a wavefront (f2n_render_rays_head, f2n_render_rays_tail,
RendererOptions::one_pass_head) on the GPU.  Its sample set is still the march's, exactly, for the whole
ray in the short form (head = -1) and for a head of 64 (or 128) samples handed to the one-ray form;
colours, depths and opacity meet the project's bar between routes, _close(a, b, 1e-4), against the fused
march route, the op-by-op route and the one-launch f2n_render_rays, on inputs where a lost 8-sample link
or a lost hand-over is an error of order 0.1; two calls give the same bits; off means off; head + tail
read nothing back, allocate nothing per sample and are captured as one hipGraph."""
import math

import pytest
import torch

from tests.test_gpu_localizer import H_IMG, SIGMAS, W_IMG, _base_pose, _localizer
from tests.test_gpu_occupancy import _march, _march_occ, _pack, _raw_field, _rays, _scene_grid
from tests.test_gpu_render import _close
from tests.test_gpu_render_rays import (STEPS, _against_routes, _raw_network, _render_rays_raw, _scene,
                                        _set_bias0, _set_head_bias, host)  # noqa: F401 (host: fixture)

pytestmark = pytest.mark.gpu

WHOLE = 1 << 30          # n_head >= S: the whole ray in the short form (one_pass_head = -1)


# ---- 1. the sample set is the march's, exactly ------------------------------------------------------

def _head_raw(capi, f, net, o, d, noise, S, step, n_head, words=None, G=0, img=None, bg=None):
    """f2n_render_rays_head, then f2n_render_rays_tail, as the Renderer issues them.  The state starts
    as garbage (NaN words: a pending flag if it were read): the head has to write all it hands on."""
    n = o.shape[0]
    dev = o.device
    bg = torch.full((n, 3), 0.5, device=dev) if bg is None else bg
    colors = torch.full((n, 3), float("nan"), device=dev)
    depths = torch.full((n,), float("nan"), device=dev)
    last = torch.full((n,), float("nan"), device=dev)
    kept = torch.full((n,), -1, dtype=torch.int32, device=dev)
    length = torch.full((n,), -1, dtype=torch.int32, device=dev)
    state = None
    if n_head < S:
        n_bytes = capi.lib().cdll.f2n_render_rays_state_bytes(n)
        assert n_bytes == 64 * n
        state = torch.full((n_bytes // 4,), float("nan"), device=dev)
    for entry in ("render_rays_head", "render_rays_tail"):
        capi.call(entry, o, d, noise, f["table16"], f["primes"], f["bias"], f["mul"], net["w_h"],
                  net["b_h"], net["w1"], net["b1"], net["w2"], net["b2"],
                  net["emb"] if img is not None else None, img, words, G, bg, colors, depths, last, kept,
                  length, n, S, step, f["L"], f["F"], f["T"], f["stride"], 1e-4, 3.0, 1e-2, n_head, state)
    return colors, depths, last, kept, length


def _bias_sweep8(capi, f, net, o, d, noise, S, step):
    """_bias_sweep of test_gpu_render_rays with fine steps around counts 8 and 16 as well (both halves
    of a DPP row) -- every bias comes from a probe of f2n_density_march, none from the kernel under
    test: the field is a near-uniform fog, a ray stops where exp(b - 3) * t reaches -ln(1e-4)."""
    def bias_for(count, b_ref, c_ref):
        return b_ref + math.log(c_ref / count)
    b_probe = 3.0 + math.log(-math.log(1e-4) / (min(48, S // 2) * step))
    _set_bias0(f, net, b_probe)
    c_probe = float(_march(capi, f, o, d, noise, S, step).float().median())
    assert 4 < c_probe < S, c_probe
    sweep = [0.0, 9.0, 10.0, 12.0]                       # everything; one or two samples
    fine = [64.0 + 0.25 * i for i in range(-12, 13)] if S > 64 else [S - 0.25 * i for i in range(1, 16)]
    fine += [8.0 + 0.25 * i for i in range(-12, 13)]     # 5 .. 11
    fine += [16.0 + 0.25 * i for i in range(-12, 13)]    # 13 .. 19
    fine += [S - 0.25 * i for i in range(2, 31)]         # S - 0.5 .. S - 7.5: the last 8-sample stride
    sweep += [bias_for(c, b_probe, c_probe) for c in fine]
    last0 = (S - 1) // 64 * 64
    if last0 >= 64:
        sweep += [bias_for(last0 + (S - last0) * fr, b_probe, c_probe) for fr in (0.3, 0.5, 0.7)]
    return sweep


def _grids(S, G, dev):
    grids = {"ones": torch.full((G ** 3 // 32,), -1, dtype=torch.int32, device=dev),
             "empty": torch.zeros(G ** 3 // 32, dtype=torch.int32, device=dev),
             "random": _pack(torch.rand(G ** 3, generator=torch.Generator().manual_seed(S + 1)) < 0.5).to(dev)}
    c = (torch.arange(G, dtype=torch.float32) + 0.5) * (4.0 / G) - 2.0
    cz, cy, cx = torch.meshgrid(c, c, c, indexing="ij")
    r = (cx * cx + cy * cy + cz * cz).sqrt()
    grids["shell"] = _pack(((r > 0.35) & (r < 1.2)).reshape(-1)).to(dev)
    return grids


def _heads(S):
    return [WHOLE, 64] + ([128] if S == 192 else [])


@pytest.mark.parametrize("L,F,T,S,train", [
    (16, 2, 1 << 19, 64, True), (16, 2, 1 << 19, 64, False),
    (16, 2, 1 << 19, 100, True), (16, 2, 1 << 19, 100, False),
    (16, 2, 1 << 19, 128, True), (16, 2, 1 << 19, 128, False),
    (16, 2, 1 << 19, 192, True), (16, 2, 1 << 19, 192, False),
    (8, 1, 3001, 100, False),         # C = 8, F = 1, T not a power of two
    (8, 2, 1 << 14, 128, True),       # C = 16
    (8, 4, 1 << 12, 192, True),       # C = 32, F = 4
    (8, 8, 1 << 12, 128, False),      # C = 64, F = 8
])
def test_counts_are_the_marchs_exactly(capi, dev, L, F, T, S, train):
    step = STEPS[S]
    n_rays = 99                       # neither 8 rays nor 8 waves divide it: the last wave has spare groups
    f = _raw_field(L, F, T, 5.0, seed=5 * L + S + F, dev=dev)
    net = _raw_network(f, seed=S + L, dev=dev)
    o, d, noise = _rays(n_rays, S, seed=S + F + 2, dev=dev, train=train)
    img = torch.randint(0, 5, (n_rays,), generator=torch.Generator().manual_seed(S)).to(torch.int32).to(dev)
    G = 64
    grids = _grids(S, G, dev)

    seen, seen_grid = set(), set()
    for b in _bias_sweep8(capi, f, net, o, d, noise, S, step):
        _set_bias0(f, net, b)
        want = _march(capi, f, o, d, noise, S, step)
        seen |= set(want.cpu().tolist())
        want_occ = {kind: _march_occ(capi, f, o, d, noise, S, step, words, G) for kind, words in grids.items()}
        seen_grid.add(len(set(want_occ["random"][1].cpu().tolist())))
        seen_grid.add(len(set(want_occ["shell"][1].cpu().tolist())))
        for n_head in _heads(S):
            plain = _head_raw(capi, f, net, o, d, noise, S, step, n_head, img=img)
            colors, depths, last, kept, length = plain
            assert torch.equal(kept, want), (b, n_head)
            assert torch.equal(length, want), (b, n_head)
            assert bool(torch.isfinite(colors).all() and torch.isfinite(depths).all()
                        and torch.isfinite(last).all()), (b, n_head)
            for kind, words in grids.items():
                got = _head_raw(capi, f, net, o, d, noise, S, step, n_head, words, G, img=img)
                assert torch.equal(got[3], want_occ[kind][0]), (b, n_head, kind)
                assert torch.equal(got[4], want_occ[kind][1]), (b, n_head, kind)
                assert bool(torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
                            and torch.isfinite(got[2]).all()), (b, n_head, kind)
                if kind == "ones":                       # ... and the bits of no grid, per head setting
                    for x, y in zip(got, plain):
                        assert torch.equal(x, y), (b, n_head, kind)
                elif kind == "empty":
                    assert int(got[3].sum()) == 0 and bool((got[4] == S).all())
                    assert bool((got[0] == 0.5).all() and (got[2] == 1).all() and (got[1] == 0).all())
    # conditions on the inputs (the march's own counts), not on the kernel under test
    print("march counts seen:", sorted(seen))
    last0 = (S - 1) // 64 * 64
    assert seen & {1, 2}, sorted(seen)
    assert {7, 8, 9} <= seen, sorted(seen)
    assert {15, 16, 17} <= seen, sorted(seen)            # both halves of a DPP row
    assert S in seen and 63 in seen, sorted(seen)
    if S > 64:
        assert {64, 65} <= seen, sorted(seen)            # the hand-over
    last8 = (S - 1) // 8 * 8                             # first sample of the last 8-sample stride
    assert any(last8 < k < S for k in seen), sorted(seen)               # a ray that stops inside it
    assert any(last0 < k < S for k in seen), sorted(seen)               # ... and inside the last 64
    assert max(seen_grid) > 3                            # a grid gives rays of one launch different lengths


@pytest.mark.parametrize("n_rays", [1, 9])
def test_counts_one_ray_and_nine(capi, dev, n_rays):
    """One ray: seven spare groups.  Nine: a second wave with one ray."""
    L, F, T, S = 16, 2, 1 << 19, 192
    step = STEPS[S]
    f = _raw_field(L, F, T, 5.0, seed=7, dev=dev)
    net = _raw_network(f, seed=11, dev=dev)
    o, d, noise = _rays(n_rays, S, seed=n_rays, dev=dev, train=True)
    words = _grids(S, 64, dev)["shell"]
    seen = set()
    for b in (0.0, 4.0, 4.6, 5.2, 6.0, 7.0, 9.0):
        _set_bias0(f, net, b)
        want = _march(capi, f, o, d, noise, S, step)
        want_occ = _march_occ(capi, f, o, d, noise, S, step, words, 64)
        seen |= set(want.cpu().tolist())
        for n_head in _heads(S):
            got = _head_raw(capi, f, net, o, d, noise, S, step, n_head)
            assert torch.equal(got[3], want) and torch.equal(got[4], want), (b, n_head)
            assert bool(torch.isfinite(got[0]).all())
            got = _head_raw(capi, f, net, o, d, noise, S, step, n_head, words, 64)
            assert torch.equal(got[3], want_occ[0]) and torch.equal(got[4], want_occ[1]), (b, n_head)
    assert S in seen and min(seen) < 64 and any(64 < k < S for k in seen), sorted(seen)


# ---- 2. values against the existing routes ----------------------------------------------------------

def _with_heads(hr, fn):
    """fn() under one_pass_head = 0 (the one-launch kernel), -1 and 64; the option is put back"""
    out = {}
    try:
        for head in (0, -1, 64):
            hr.set_one_pass_head(head)
            assert hr.one_pass_head == head
            out[head] = fn(head)
    finally:
        hr.set_one_pass_head(0)
    return out


def _routes_per_head(hr, dev, o, d, emb, noise, bg, mode, routes):
    """_against_routes for head = -1 and 64 (march route, op-by-op), and both against head = 0"""
    res = _with_heads(hr, lambda head: _against_routes(hr, dev, o, d, emb, noise, bg, mode,
                                                       routes if head else ()))
    for head in (-1, 64):
        assert torch.equal(res[head][3], res[0][3]), head
        _close(res[head][0], res[0][0], 1e-4)
        _close(res[head][1], res[0][1], 1e-4)
        _close(1.0 - res[head][2].double(), 1.0 - res[0][2].double(), 1e-4)
    return res


@pytest.mark.parametrize("S,bias0", [
    (128, 0.0), (128, 1.0), (192, 0.0), (192, 1.0),    # nothing terminates: every link carries weight
    (100, 0.0), (100, 1.0),                            # a partial last stride
    (128, 4.0), (192, 4.0),                            # stops in the last 64-sample block
    (128, 5.0), (192, 5.0), (100, 5.0),                # stops inside the head
])
def test_head_against_march_and_op_by_op(host, dev, S, bias0):
    hr, o, d, noise, bg, gt, emb = _scene(host, 16, 2, 19, S, 96, 31)
    _set_head_bias(hr, bias0)
    hr.set_occupancy(None)
    v = _routes_per_head(hr, dev, o, d, None, None, None, "validate", (True, False))
    t = _routes_per_head(hr, dev, o, d, emb, noise, bg, "train", (True, False))
    if bias0 <= 1.0:
        # the inputs can show a dropped carry: every ray ends half transparent, more than a tenth of
        # its weight (the default route's) lies beyond sample 8 and beyond sample 64
        for res in (v, t):
            for head in (-1, 64):
                colors, depths, last, kept = res[head]
                assert bool((kept == S).all())
                assert bool(((last > 0.05) & (last < 0.95)).all())
        to = lambda x: x.to(dev)
        with torch.no_grad():
            hr.set_dense_first_pass(0)
            _, _, w, idx = hr.render(to(o), to(d), None, "validate")
        w = w.reshape(96, S)
        assert bool((w[:, 8:].sum(1) > 0.1 * w.sum(1)).all())
        assert bool((w[:, 64:].sum(1) > 0.1 * w.sum(1)).all())
    elif bias0 == 4.0:
        assert bool(((v[64][3] > (S - 1) // 64 * 64) & (v[64][3] < S)).any())
    else:
        assert bool((v[64][3] < 64).all())
    assert not torch.equal(v[64][0], t[64][0])           # the TRAIN inputs are in use


@pytest.mark.parametrize("L,F,log2_T,S,bias0", [
    (4, 2, 19, 192, 1.0),        # C = 8
    (8, 2, 14, 100, 0.0),        # C = 16
    (8, 8, 12, 128, 4.0),        # C = 64, F = 8
])
def test_head_other_widths(host, dev, L, F, log2_T, S, bias0):
    hr, o, d, noise, bg, gt, emb = _scene(host, L, F, log2_T, S, 77, 13)
    _set_head_bias(hr, bias0)
    _routes_per_head(hr, dev, o, d, None, None, None, "validate", (True, False))
    _routes_per_head(hr, dev, o, d, emb, noise, bg, "train", (True,))


def test_head_with_shell_grid_against_both_routes(host, dev):
    hr, o, d, noise, bg, gt, emb = _scene(host, 16, 2, 19, 1024, 200, 23)
    _set_head_bias(hr, 5.0)
    hr.set_occupancy(_scene_grid(host, dev, 128, "shell", 2))
    try:
        v = _routes_per_head(hr, dev, o, d, None, None, None, "validate", (True, False))
        _routes_per_head(hr, dev, o, d, emb, noise, bg, "train", (True,))
        assert len(set(v[64][3].cpu().tolist())) > 3     # rays of different lengths in one launch
    finally:
        hr.set_occupancy(None)


def test_set_one_pass_head_rejects_other_values(host, dev):
    hr = _scene(host, 16, 2, 19, 128, 96, 31)[0]
    for bad in (-2, 1, 63, 65, 100):
        with pytest.raises(RuntimeError):
            hr.set_one_pass_head(bad)
        assert hr.one_pass_head == 0


# ---- 3. determinism and off-means-off ---------------------------------------------------------------

def test_determinism_chunks_and_off_means_off(host, dev):
    hr, o, d, noise, bg, gt, emb = _scene(host, 16, 2, 19, 128, 1000, 29)
    _set_head_bias(hr, 4.0)
    hr.set_occupancy(None)
    o, d = o.to(dev), d.to(dev)
    with torch.no_grad():
        today = hr.render_rays(o, d, None, "validate")
        try:
            for head in (-1, 64):
                hr.set_one_pass_head(head)
                a = hr.render_rays(o, d, None, "validate")
                b = hr.render_rays(o, d, None, "validate")
                for x, y in zip(a, b):
                    assert torch.equal(x, y), head
                hr.set_one_pass(True)
                colors, depths = hr.render_all_rays(o, d, 256)
                hr.set_one_pass(False)
                assert colors.shape == (1000, 3) and depths.shape == (1000, 1)
                for lo in range(0, 1000, 256):
                    c, dp, _, _ = hr.render_rays(o[lo:lo + 256], d[lo:lo + 256], None, "validate")
                    assert torch.equal(colors[lo:lo + 256], c) and torch.equal(depths[lo:lo + 256, 0], dp)
                assert torch.equal(a[3], today[3])
                _close(a[0], today[0], 1e-4)
        finally:
            hr.set_one_pass(False)
            hr.set_one_pass_head(0)
        off = hr.render_rays(o, d, None, "validate")     # the option at 0: the kernel of today, its bits
        for x, y in zip(off, today):
            assert torch.equal(x, y)


# ---- 4. no host read, no per-sample memory ----------------------------------------------------------

def test_no_per_sample_memory_and_one_graph_of_two_launches(host, dev):
    n, S = 4096, 1024
    hr, o, d, noise, bg, gt, emb = _scene(host, 16, 2, 19, S, n, 37)
    _set_head_bias(hr, 5.0)
    hr.set_occupancy(None)
    o, d, bg = o.to(dev), d.to(dev), bg.to(dev)
    hr.set_one_pass_head(64)
    try:
        with torch.no_grad():
            hr.render_rays(o, d, None, "validate", None, bg)          # warm-up: the state is allocated here
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = hr.render_rays(o, d, None, "validate", None, bg)
            torch.cuda.synchronize()
            rise = torch.cuda.max_memory_allocated() - base
            assert rise < 1024 * n, rise                              # (the sampler's grid: 32 KiB per ray)
            del out
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
    finally:
        hr.set_one_pass_head(0)


# ---- 5. Localizer -----------------------------------------------------------------------------------

def test_localizer_one_pass_head(host, dev):
    P, K = 8, 64
    loc, hr, Kc = _localizer(host, dev, 31)
    param = host.LocalizerParam()
    assert param.one_pass_head == 0
    param.render_pixel_num = K
    param.one_pass = True
    param.one_pass_head = 64
    g = torch.Generator().manual_seed(31)
    poses = host.perturb_poses(_base_pose(31).to(dev), torch.randn(P, 6, generator=g).to(dev), SIGMAS)
    image = torch.rand(H_IMG, W_IMG, 3, generator=g)
    pix = torch.randperm(H_IMG * W_IMG, generator=g)[:K]
    ij = torch.stack([pix // W_IMG, pix % W_IMG], 1).to(torch.int32)
    hr.set_dense_first_pass(0)
    w0, loss0, colors0, _ = loc.evaluate_poses_full(poses, image.to(dev), ij.to(dev))
    assert not hr.one_pass_applies() and hr.one_pass_head == 0
    try:
        loc1 = host.Localizer(param, hr, Kc.to(dev), H_IMG, W_IMG, torch.zeros(3).to(dev), 1.0)
        assert hr.one_pass_head == 64
        with torch.no_grad():
            assert hr.one_pass_applies()
        w1, loss1, colors1, _ = loc1.evaluate_poses_full(poses, image.to(dev), ij.to(dev))
    finally:
        hr.set_one_pass(False)
        hr.set_one_pass_head(0)
    assert colors1.shape == (P, K, 3)
    _close(colors1, colors0, 1e-4)
    assert int(w1.argmax()) == int(w0.argmax())
    assert float(loss0.max() - loss0.min()) > 0
