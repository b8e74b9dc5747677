"""Level weights on the GPU: Hash3DAnchored::set_level_weights through every Renderer route, the
level-of-detail entries of the one-pass render, train_step, rays as leaves, a captured step and the
Localizer.

The weights are folded into the field head, so a renderer WITH weights must compute what a twin
WITHOUT weights computes whose head columns were scaled by hand -- bit for bit forward (no forward
kernel has atomics, and fma(x, 0, acc) == acc for finite x), and within the bars of
tests/step_terms_cases.py backward (BAR_PARAM = 1e-4 max|g| for parameters, BAR_RAYS = 5e-3 max|g|
for rays).  skip_masked_levels (walk active_levels() levels only) is held against the same renderer
with it off, with the allocator handing NaN to every torch::empty in between.

Shapes: _scene / _route / ROUTES of tests/test_gpu_weight_dist.py (L 8, F 2, T 2^14, S 128): 256 rays
at bias 4 (kept prefixes cross a stride) and the 1024-ray thin scene (131072 samples: the binned
backward).  alpha in {2.5, 1, 7.25, 8} -> 3, 1, 8, 8 active levels; 3 * F = 6 rows is no kernel's
width, so the zeroed tail of the one-pass tile is in play."""
import ctypes
import importlib

import pytest
import torch

from tests import level_weights_model as lm
from tests.step_terms_cases import BAR_PARAM, BAR_RAYS
from tests.test_gpu_localizer import H_IMG, SIGMAS, W_IMG, _base_pose
from tests.test_gpu_pose_grad import _intrinsic, _loss
from tests.test_gpu_render import _copy_params, _setup
from tests.test_gpu_weight_dist import ROUTES, S, _route, _scene
from oracle import ref_render as R

pytestmark = pytest.mark.gpu

L, F, LOG2_T = 8, 2, 14
ALPHAS = (2.5, 1.0, 7.25, 8.0)
ACTIVE = {2.5: 3, 1.0: 1, 7.25: 8, 8.0: 8}
ONE_PASS = (0, 64, -1)                      # one launch; head 64 then tail; whole rays in the head
SCENES = {"stops": (256, 4.0, 31), "thin": (1024, 1.0, 37)}
RAY_ROUTES = {"op_by_op": (False, 0), "march": (True, 0), "dense": (True, 1)}


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


@pytest.fixture(scope="module")
def pairs(host, dev):
    """per scene: renderer A (takes the weights) and its twin B (same seed, same parameters; its
    head is scaled by hand), and the head both started from"""
    out = {}
    for name, (n_rays, bias0, seed) in SCENES.items():
        a, b = _scene(host, dev, n_rays, bias0, seed), _scene(host, dev, n_rays, bias0, seed)
        pa, pb = a["hr"].named_parameters(), b["hr"].named_parameters()
        assert all(torch.equal(pa[k], pb[k]) for k in pa)
        out[name] = (a, b, pa["scene_field.mlp.weight"].detach().clone())
    return out


def _cols(host, dev, alpha, n_levels=L, n_channels=F):
    lw, active = host.level_weights(alpha, n_levels)
    assert active == lm.active_levels(lm.weights(alpha, n_levels))
    return lw, lw.repeat_interleave(n_channels).to(dev), active


def _scale_head(hr, w0, cols):
    with torch.no_grad():
        hr.named_parameters()["scene_field.mlp.weight"].copy_(w0 * cols)


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None and y is None) or torch.equal(x, y), (what, i)


def _one_pass(hr, args, head):
    hr.set_one_pass_head(head)
    try:
        with torch.no_grad():
            return hr.render_rays(*args)
    finally:
        hr.set_one_pass_head(0)


def _grads_after_step(hr, scene):
    o, d, emb, _, noise, bg = scene["args"]
    hr.zero_grad()
    loss, sq, _, n_samp = hr.train_step(o, d, emb, scene["gt"], 1e-2, noise, bg, True)
    torch.cuda.synchronize()
    return (loss.clone(), sq.clone(), n_samp), {k: v.clone() for k, v in hr.grads().items() if v is not None}


def _within(got, want, bar, what):
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    print("  %s: max|dg| = %.3e, bar %.3e (max|g| = %.3e)" % (what, err, bar * scale, scale))
    assert bool(torch.isfinite(got).all()) and err <= bar * scale, (what, err, bar * scale)


def _ray_grads(hr, dev, scene, route, exact):
    fused, dense = RAY_ROUTES[route]
    o, d, emb, mode, noise, bg = scene["args"]
    hr.set_occupancy(None)
    hr.set_fused(True)
    hr.set_fused_ray_grad(fused)
    hr.set_dense_first_pass(dense)
    hr.set_speculate_dense(False)
    hr.set_ray_order_min_rays(1 << 30)
    hr.set_exact_ray_grad(exact)
    try:
        hr.zero_grad()
        o_g, d_g = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
        out = hr.render(o_g, d_g, emb, mode, noise, bg)
        _loss(out[0], out[1]).backward()
        return [v.detach().clone() for v in out], o_g.grad.clone(), d_g.grad.clone()
    finally:
        hr.set_exact_ray_grad(False)
        hr.set_fused_ray_grad(False)
        hr.set_speculate_dense(True)


# ---- 1. the fold against a hand-scaled twin ---------------------------------------------------------

@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", list(SCENES))
def test_fold_against_hand_scaled_twin(host, capi, dev, pairs, name, alpha):
    a, b, w0 = pairs[name]
    A, B = a["hr"], b["hr"]
    lw, cols, active = _cols(host, dev, alpha)
    assert active == ACTIVE[alpha]
    n_rays = a["n_rays"]
    try:
        A.set_skip_masked_levels(False)
        A.set_level_weights(lw)
        assert A.active_levels() == active and torch.equal(A.level_weights(), lw)
        assert B.level_weights() is None and B.active_levels() == L
        _scale_head(B, w0, cols)
        assert torch.equal(A.scene_field.head_weight().detach(),
                           B.named_parameters()["scene_field.mlp.weight"].detach())
        for route in ROUTES:
            for hr in (A, B):
                _route(hr, host, dev, route, n_rays)
            with torch.no_grad():
                _same(A.render(*a["args"]), B.render(*b["args"]), (route, "render"))
            (sa, ga), (sb, gb) = _grads_after_step(A, a), _grads_after_step(B, b)
            assert torch.equal(sa[0], sb[0]) and torch.equal(sa[1], sb[1]) and sa[2] == sb[2], route
            assert set(ga) == set(gb)
            for k in ga:
                # d(W_h) = d(W_eff) * cols: B's parameter IS W_eff
                want = gb[k] * cols if k == "scene_field.mlp.weight" else gb[k]
                _within(ga[k], want, BAR_PARAM, "%s alpha %g %s %s" % (name, alpha, route, k))
        for hr in (A, B):
            _route(hr, host, dev, "march", n_rays)
        for head in ONE_PASS:
            want = _one_pass(B, b["args"], head)
            for skip in (False, True):                   # the twin walks all 8 levels either way
                A.set_skip_masked_levels(skip)
                _same(_one_pass(A, a["args"], head), want, ("render_rays", head, skip))
            A.set_skip_masked_levels(False)
        if name == "stops":
            assert int(want[3].max()) > 64, "no ray outlives the head: the tail would not run"
        for route in RAY_ROUTES:
            for exact in (False, True):
                out_a, do_a, dd_a = _ray_grads(A, dev, a, route, exact)
                out_b, do_b, dd_b = _ray_grads(B, dev, b, route, exact)
                _same(out_a, out_b, (route, exact, "rays as leaves"))
                what = "%s alpha %g %s exact %d " % (name, alpha, route, exact)
                _within(do_a, do_b, BAR_RAYS, what + "d_rays_o")
                _within(dd_a, dd_b, BAR_RAYS, what + "d_rays_d")
                assert float(do_b.abs().max()) > 0 and float(dd_b.abs().max()) > 0
    finally:
        A.clear_level_weights()
        A.set_skip_masked_levels(True)
        _scale_head(B, w0, torch.ones_like(cols))
        for hr in (A, B):
            hr.set_occupancy(None)
            hr.zero_grad()


# ---- 2. skip on against skip off ---------------------------------------------------------------------

def _poison(dev, *sizes):
    """NaN-filled blocks of these sizes, freed: what the caching allocator hands to the next
    torch::empty of the same size (or, split, of a smaller one)"""
    blocks = [torch.full((int(n),), float("nan"), device=dev) for n in sizes if n > 0]
    torch.cuda.synchronize()
    del blocks


def _disjoint_levels_scene(host, dev, n_rays, bias0, seed, E=7):
    """_setup of tests/test_gpu_render.py with level_stride = T * F: level l owns rows [l T, (l + 1) T)
    of the table and nothing else"""
    T = 1 << LOG2_T
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    oracle = R.Renderer(E, L=L, F=F, log2_T=LOG2_T, S=S, step=4.0 / S, gen=g, feat_init="trained")
    with torch.no_grad():
        oracle.scene_field.mlp.bias[0] = bias0
    hr = host.Renderer(E, n_levels=L, n_channels=F, log2_table=LOG2_T, level_stride=T * F,
                       max_samples=S, step=4.0 / S)
    _copy_params(oracle, hr)
    assert hr.scene_field.level_stride == T * F and hr.scene_field.local_size == T
    o = (torch.randn(n_rays, 3, generator=g) * 0.25).to(dev)
    d = torch.randn(n_rays, 3, generator=g).to(dev)
    noise = (torch.rand(n_rays, S, generator=g) + 0.5).to(dev)
    bg = torch.rand(n_rays, 3, generator=g).to(dev)
    gt = torch.rand(n_rays, 3, generator=g).to(dev)
    emb = torch.randint(0, E, (n_rays,), generator=g).to(torch.int32).to(dev)
    return dict(hr=hr, args=(o, d, emb, "train", noise, bg), gt=gt, n_rays=n_rays)


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", list(SCENES))
def test_skip_on_against_skip_off(host, capi, dev, pairs, name, alpha):
    a = pairs[name][0]
    A = a["hr"]
    lw, cols, active = _cols(host, dev, alpha)
    n_rays, C = a["n_rays"], L * F
    try:
        A.set_level_weights(lw)
        for route in ROUTES:
            _route(A, host, dev, route, n_rays)
            runs = {}
            A.set_skip_masked_levels(False)
            with torch.no_grad():
                n_kept = int(A.render(*a["args"])[3][-1, 1])      # sizes the encoding of the kept samples
            for skip in (False, True):
                A.set_skip_masked_levels(skip)
                _poison(dev, C * n_rays * S, C * n_kept)
                with torch.no_grad():
                    out = A.render(*a["args"])
                assert int(out[3][-1, 1]) == n_kept
                assert all(bool(torch.isfinite(v).all()) for v in out if v is not None), (route, skip)
                _poison(dev, C * n_rays * S, C * n_kept)
                step, grads = _grads_after_step(A, a)
                runs[skip] = (out, step, grads)
            (out0, step0, g0), (out1, step1, g1) = runs[False], runs[True]
            _same(out0, out1, (route, "render"))
            assert torch.equal(step0[0], step1[0]) and torch.equal(step0[1], step1[1]), route
            assert step0[2] == step1[2]
            for k in g0:
                _within(g1[k], g0[k], BAR_PARAM, "%s alpha %g %s %s" % (name, alpha, route, k))
        _route(A, host, dev, "march", n_rays)
        for head in ONE_PASS:
            outs = []
            for skip in (False, True):
                A.set_skip_masked_levels(skip)
                _poison(dev, C * n_rays * S)
                outs.append(_one_pass(A, a["args"], head))
            _same(outs[0], outs[1], ("render_rays", head))
            if name == "stops":
                assert int(outs[0][3].max()) > 64
    finally:
        A.clear_level_weights()
        A.set_skip_masked_levels(True)
        A.set_occupancy(None)
        A.zero_grad()


def _lod_raw(capi, hr, args, active, n_levels, n_channels, head):
    """the three entries through the C ABI on the renderer's own tensors, len included:
    (colors, depths, last_trans, kept, len)"""
    o, d, emb, _, noise, bg = args
    f = hr.scene_field
    p = hr.named_parameters()
    n = o.shape[0]
    dev = o.device
    w_h = f.head_weight().detach().contiguous()
    net = [p[k].detach().contiguous() for k in ("scene_field.mlp.bias", "shader.mlp.0.weight",
                                                 "shader.mlp.0.bias", "shader.mlp.2.weight",
                                                 "shader.mlp.2.bias")]
    colors = torch.full((n, 3), float("nan"), device=dev)
    depths, last = torch.full((n,), float("nan"), device=dev), torch.full((n,), float("nan"), device=dev)
    kept = torch.full((n,), -1, dtype=torch.int32, device=dev)
    length = torch.full((n,), -1, dtype=torch.int32, device=dev)
    common = (o, d, noise, f.table_f16(), f.prim_pool, f.bias_pool, f.level_mul, w_h, *net,
              p["app_emb"].detach().contiguous(), emb, None, 0, bg, colors, depths, last, kept, length, n,
              S, ctypes.c_float(4.0 / S), n_levels, active, n_channels, f.local_size, f.level_stride,
              ctypes.c_float(1e-4), ctypes.c_float(3.0), ctypes.c_float(1e-2))
    if head == 0:
        capi.call("render_rays_lod", *common)
    else:
        n_head = S if head < 0 else head
        state = torch.full((16 * n,), float("nan"), device=dev) if n_head < S else None
        capi.call("render_rays_head_lod", *common, n_head, state)
        capi.call("render_rays_tail_lod", *common, n_head, state)
    torch.cuda.synchronize()
    return colors, depths, last, kept, length


@pytest.mark.parametrize("n_levels,n_channels,alpha", [
    (8, 2, 2.5), (8, 2, 1.0), (8, 2, 7.25),      # C = 16: 6, 2 and 16 rows
    (16, 4, 2.5), (16, 4, 9.5),                   # C = 64: 12 and 40 rows of 64
    (8, 1, 2.5), (8, 1, 6.25),                    # C = 8: 3 and 7 rows of 8
])
def test_one_pass_forms_lod_against_the_full_walk(host, capi, dev, n_levels, n_channels, alpha):
    """The kernels themselves, len included: L_active levels against all of them with the same folded
    head, on the three forms; and the Renderer's render_rays with skip on against off."""
    n_rays = 256
    _, hr, o, d, noise, bg, gt, emb = _setup(host, n_levels, n_channels, LOG2_T, S, 4.0 / S, n_rays, 4.0,
                                             41 + n_levels + n_channels)
    args = tuple(v.to(dev) for v in (o, d, emb)) + ("train",) + tuple(v.to(dev) for v in (noise, bg))
    lw, cols, active = _cols(host, dev, alpha, n_levels, n_channels)
    assert active == n_levels or (1 <= active < n_levels and active * n_channels not in (8, 16, 32, 64))
    hr.set_level_weights(lw)
    for head in ONE_PASS:
        _poison(dev, n_levels * n_channels * n_rays * S)
        full = _lod_raw(capi, hr, args, n_levels, n_levels, n_channels, head)
        lod = _lod_raw(capi, hr, args, active, n_levels, n_channels, head)
        _same(lod, full, ("lod", head))
        assert int(full[3].min()) >= 0 and int(full[4].min()) >= 0 and int(full[3].max()) > 64
        assert bool(torch.isfinite(full[0]).all())
        outs = []
        for skip in (False, True):
            hr.set_skip_masked_levels(skip)
            outs.append(_one_pass(hr, args, head))
        _same(outs[0], outs[1], ("render_rays", head))
        _same(outs[1], full[:4], ("render_rays against the entry", head))


@pytest.mark.parametrize("alpha", (2.5, 1.0))
def test_levels_left_out_get_no_table_gradient(host, capi, dev, alpha):
    """disjoint level windows: the rows of every level >= L_active hold exact zeros after a step, with
    the levels skipped and with them walked (d_enc = W_eff^T d_h is an exact zero there)"""
    T = 1 << LOG2_T
    scene = _disjoint_levels_scene(host, dev, 1024, 1.0, 37)
    hr = scene["hr"]
    lw, cols, active = _cols(host, dev, alpha)
    hr.set_level_weights(lw)
    for route in ("march", "dense", "op_by_op"):
        _route(hr, host, dev, route, scene["n_rays"])
        grads = {}
        for skip in (False, True):
            hr.set_skip_masked_levels(skip)
            _poison(dev, L * F * scene["n_rays"] * S)
            grads[skip] = _grads_after_step(hr, scene)[1]
            g = grads[skip]["scene_field.feat_pool"]
            assert not bool(g[active * T:].any()), (route, skip)
            for lvl in range(active):
                assert bool(g[lvl * T:(lvl + 1) * T].any()), (route, skip, lvl)
        for k in grads[False]:
            _within(grads[True][k], grads[False][k], BAR_PARAM, "disjoint alpha %g %s %s" % (alpha, route, k))


# ---- 3. never set against all ones ---------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SCENES))
def test_unset_against_all_ones(host, capi, dev, pairs, name):
    """alpha = L is all ones: W * 1 == W, so outputs are the bits of the renderer without weights on
    every route, and so are the gradients wherever two runs of the renderer WITHOUT weights give the
    same bits themselves (exact sums); where float atomics make two such runs differ, the weighted run
    stays within max(4 spread, 1e-5 max|g|) of them: the rule tests/test_gpu_exact_ray_grad_routes.py
    holds a switch to that must leave a gradient alone (one pair of runs samples the spread of sums
    whose order changes: a single ulp of the largest element is 6e-8 of it)."""
    a = pairs[name][0]
    A = a["hr"]
    lw, cols, active = _cols(host, dev, float(L))
    assert active == L and bool((lw == 1.0).all())
    capi.set_option("BWD_PHASES", 1)
    try:
        for route in ROUTES:
            _route(A, host, dev, route, a["n_rays"])
            A.clear_level_weights()
            with torch.no_grad():
                out0 = A.render(*a["args"])
            s0, g0 = _grads_after_step(A, a)
            _, g0b = _grads_after_step(A, a)
            A.set_level_weights(lw)
            with torch.no_grad():
                out1 = A.render(*a["args"])
            s1, g1 = _grads_after_step(A, a)
            _same(out0, out1, (route, "render"))
            assert torch.equal(s0[0], s1[0]) and torch.equal(s0[1], s1[1]) and s0[2] == s1[2], route
            for k in g0:
                if torch.equal(g0[k], g0b[k]):
                    assert torch.equal(g1[k], g0[k]), (route, k)
                else:
                    spread = float((g0[k] - g0b[k]).abs().max())
                    scale = float(g0[k].abs().max())
                    diff = float((g1[k] - g0[k]).abs().max())
                    print("  %s %s %s: run-to-run spread %.3e, with ones %.3e, max|g| %.3e" % (
                        name, route, k, spread, diff, scale))
                    assert diff <= max(4 * spread, 1e-5 * scale), (route, k, diff, spread, scale)
        _route(A, host, dev, "march", a["n_rays"])
        for head in ONE_PASS:
            A.clear_level_weights()
            want = _one_pass(A, a["args"], head)
            A.set_level_weights(lw)
            _same(_one_pass(A, a["args"], head), want, ("render_rays", head))
    finally:
        A.clear_level_weights()
        A.set_occupancy(None)
        A.zero_grad()


# ---- 4. a captured step sees later values ---------------------------------------------------------------

def test_captured_step_follows_the_weights_in_place(host, dev):
    """test_deferred_check_renders_without_a_host_read_and_graphs' pattern: a train_step captured at
    alpha = 2.3 and replayed after set_coarse_to_fine(2.8) -- still 3 active levels, the values moved in
    place -- is the eager step at 2.8."""
    oracle, hr, o, d, noise, bg, gt, emb = _setup(host, L, F, LOG2_T, 64, 4.0 / 64, 96, -3.0, 33)
    to = lambda x: x.to(dev)
    hr.set_fused(True)
    hr.set_fused_shade(True)
    hr.set_dense_first_pass(1)
    hr.set_deferred_check(True)
    args = (to(o), to(d), to(emb), to(gt), 1e-2, to(noise), to(bg), True)

    def batch():
        hr.zero_grad()
        loss, sq, nv, ns = hr.train_step(*args)
        return loss, sq

    eager = {}
    for alpha in (2.3, 2.8):
        hr.set_coarse_to_fine(alpha)
        assert hr.active_levels() == 3
        loss, sq = batch()
        eager[alpha] = (loss.clone(), sq.clone(), {k: v.clone() for k, v in hr.grads().items() if v is not None})
    assert not torch.equal(eager[2.3][0], eager[2.8][0])
    hr.set_coarse_to_fine(2.3)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            batch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        loss_g, sq_g = batch()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss_g, eager[2.3][0]) and torch.equal(sq_g, eager[2.3][1])
    hr.set_coarse_to_fine(2.8)                       # in place: the graph's tensor, new values
    assert hr.active_levels() == 3
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss_g, eager[2.8][0]) and torch.equal(sq_g, eager[2.8][1])
    for k, want in eager[2.8][2].items():            # (sums by float atomics: equal up to their order)
        _within(hr.grads()[k], want, BAR_PARAM, "replay at 2.8 %s" % k)
    assert hr.deferred_check_ok()


# ---- 5. the Localizer ------------------------------------------------------------------------------------

def _localizer(host, dev, seed, level_alpha=None, K=64):
    _, hr, *_ = _setup(host, L, F, LOG2_T, 64, 4.0 / 64, 1, 3.0, seed)
    param = host.LocalizerParam()
    param.render_pixel_num = K
    assert param.level_alpha < 0                     # off by default
    if level_alpha is not None:
        param.level_alpha = level_alpha
    Kc = _intrinsic(1, H_IMG, W_IMG)[0]
    loc = host.Localizer(param, hr, Kc.to(dev), H_IMG, W_IMG, torch.zeros(3).to(dev), 1.0)
    return loc, hr


def test_localizer_level_alpha(host, dev):
    P, K = 8, 64
    g = torch.Generator().manual_seed(31)
    poses = host.perturb_poses(_base_pose(31).to(dev), torch.randn(P, 6, generator=g).to(dev), SIGMAS)
    image = torch.rand(H_IMG, W_IMG, 3, generator=g).to(dev)
    pix = torch.randperm(H_IMG * W_IMG, generator=g)[:K]
    ij = torch.stack([pix // W_IMG, pix % W_IMG], 1).to(torch.int32).to(dev)

    def scores(loc):
        with torch.no_grad():
            return loc.evaluate_poses_full(poses, image, ij)[:3]

    plain, hr_plain = _localizer(host, dev, 31)
    full, hr_full = _localizer(host, dev, 31, float(L))
    coarse, hr_coarse = _localizer(host, dev, 31, 3.0)
    twin, hr_twin = _localizer(host, dev, 31)
    assert hr_plain.level_weights() is None and hr_full.active_levels() == L
    assert hr_coarse.active_levels() == 3
    _, cols, _ = _cols(host, dev, 3.0)
    _scale_head(hr_twin, hr_twin.named_parameters()["scene_field.mlp.weight"].detach().clone(), cols)
    want = scores(plain)
    _same(scores(full), want, "level_alpha = L")
    want3 = scores(twin)
    _same(scores(coarse), want3, "level_alpha = 3")
    assert not torch.equal(want3[0], want[0])
    # set_level_alpha afterwards: the same, and < 0 clears
    plain.set_level_alpha(3.0)
    assert hr_plain.active_levels() == 3
    plain.set_level_alpha(-1.0)
    assert hr_plain.level_weights() is None and hr_plain.active_levels() == L
