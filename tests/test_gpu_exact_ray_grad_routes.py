"""Hash3DAnchoredOptions::exact_point_grad through the host: the field's autograd node, the Renderer's
three routes for rays with a gradient (op by op, march and dense with fused_ray_grad), the Localizer,
both refiners and a captured graph.  The switch changes d(rays) and nothing else: colours, depths,
weights, bounds and every parameter gradient are those of the run with the switch off.  The kernels
behind it are held to float64 in tests/test_gpu_enc_grad.py; small shapes here (L 16, F 2, T 2^14, at
most 512 rays x 256 samples)."""
import importlib

import pytest
import torch

from tests.test_gpu_localizer import _base_pose
from tests.test_gpu_pose_grad import _intrinsic, _loss, _pose, _render
from tests.test_gpu_render import _setup

pytestmark = pytest.mark.gpu

L, F, LOG2_T = 16, 2, 14
H, W = 16, 24
N_CAMS, N_RAYS, FIXED = 8, 300, 2
ROUTES = {"op_by_op": (False, 0), "march": (True, 0), "dense": (True, 1)}


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def _route(hr, name):
    fused, dense = ROUTES[name]
    hr.set_fused_ray_grad(fused)
    hr.set_dense_first_pass(dense)
    hr.set_speculate_dense(False)


# ---- the field's own node ----------------------------------------------------------------------------

def test_field_node_returns_the_exact_point_gradient(host, capi, dev):
    """Hash3DAnchoredFunction on contracted points that require a gradient: with the switch on the point
    gradient is f2n_hash_pts_grad_exact's, bit for bit, whatever the layout of the incoming gradient;
    the table gradient is the one of the run with the switch off; off again, the old bits return."""
    field = host.Hash3DAnchored(L, F, LOG2_T, 0, str(dev))
    gen = torch.Generator().manual_seed(5)
    n, C = 1000, L * F
    with torch.no_grad():
        field.feat_pool.copy_((torch.randn(field.feat_pool.shape, generator=gen) * 0.1).to(dev))
    x = (torch.rand(n, 3, generator=gen) * 3.0 - 1.5).to(dev)
    g = (torch.randn(n, C, generator=gen) * 5e-3).to(dev)
    g_cm = g.t().contiguous().t()                                   # the same values, channel-major storage

    def run(exact, grad):
        field.set_exact_point_grad(exact)
        field.feat_pool.grad = None
        xg = x.clone().requires_grad_(True)
        field.encode(xg).backward(grad)
        return xg.grad.clone(), field.feat_pool.grad.clone()

    off_x, off_t = run(False, g)
    on_x, on_t = run(True, g)
    on_x_cm, _ = run(True, g_cm)
    again_x, again_t = run(False, g)
    want = torch.full((n, 3), -1.0, device=dev)
    capi.call("hash_pts_grad_exact", x, field.table_f16(), field.prim_pool, field.bias_pool, field.level_mul, g,
              C, 1, want, n, L, F, field.local_size, field.level_stride)
    assert torch.equal(on_x, want) and torch.equal(on_x_cm, want)
    # (f2n_hash_bwd adds its levels into pts_grad with float atomics: the Q5 bits are not the same run to run)
    torch.testing.assert_close(again_x, off_x, rtol=1e-4, atol=1e-5 * float(off_x.abs().max()))
    assert float((on_x - off_x).norm()) > 0.1 * float(off_x.norm())
    # (float atomics on this small batch with the switch off and on: equal up to their order)
    scale = float(off_t.abs().max())
    spread = float((off_t - again_t).abs().max())
    assert float((on_t - off_t).abs().max()) <= max(4 * spread, 1e-5 * scale)
    ratio = float(off_x.norm() / on_x.norm())
    print("\n|Q5| / |exact| over %d points: %.2f" % (n, ratio))
    assert 1.5 < ratio < 10.0                                      # Q5 is of the order of 4 times the derivative


# ---- the Renderer's routes -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chunk(host):
    """512 rays x 256 samples, nothing terminates (131072 samples: the binned, exact table gradient)"""
    return _setup(host, L, F, LOG2_T, 256, 4.0 / 256, 512, 0.0, 7)


@pytest.mark.parametrize("route", list(ROUTES))
def test_switch_changes_the_ray_gradient_and_nothing_else(host, capi, dev, chunk, route):
    """test_fused_ray_grad_leaves_render_and_parameter_gradients' rule between the switch off and on, on
    one route: the outputs bit for bit; the table gradient bit for bit where both runs sum it exactly
    (the fused routes: binned under BWD_PHASES = 1), every other parameter gradient within the
    run-to-run spread of its float atomics; d(rays) differs."""
    oracle, hr, o, d, noise, bg, gt, emb = chunk
    _route(hr, route)
    runs = []
    try:  # the renderer is shared by the three routes: the switch goes back off whatever happens
        with capi.option("BWD_PHASES", 1):
            for exact in (False, False, True):
                hr.set_exact_ray_grad(exact)
                hr.zero_grad()
                o_g, d_g, out = _render(hr, dev, o, d, "train", emb, noise, bg, True)
                _loss(out[0], out[1]).backward()
                runs.append(([v.detach().clone() for v in out],
                             {k: v.clone() for k, v in hr.grads().items() if v is not None},
                             (o_g.grad.clone(), d_g.grad.clone())))
    finally:
        hr.set_exact_ray_grad(False)
    (base, g0, r0), (_, g1, r1), (with_exact, g2, r2) = runs
    assert base[2].numel() >= 65536
    for a, b in zip(base, with_exact):
        assert torch.equal(a, b)
    assert set(g0) == set(g2)
    for k in g0:
        if k.endswith("feat_pool") and route != "op_by_op":
            assert torch.equal(g0[k], g2[k]), k
            continue
        spread = float((g0[k] - g1[k]).abs().max())
        scale = float(g0[k].abs().max())
        diff = float((g0[k] - g2[k]).abs().max())
        assert diff <= max(4 * spread, 1e-5 * scale), (k, diff, spread, scale)
    for off, off_again, on in zip(r0, r1, r2):
        if route != "op_by_op":                                     # no atomics on the fused way to the rays
            assert torch.equal(off, off_again)
        assert bool(torch.isfinite(on).all()) and float(on.abs().max()) > 0
        assert not torch.equal(on, off)
    print("\n%s: |d_o| off %.4g on %.4g, |d_d| off %.4g on %.4g" % (
        route, float(r0[0].norm()), float(r2[0].norm()), float(r0[1].norm()), float(r2[1].norm())))


def test_fused_and_op_by_op_agree_with_the_switch_on(host, dev):
    """The bars test_fused_and_op_by_op_agree_at_reference_sampler holds Q5 to (relative norm below 5e-3,
    at most 0.1 % of the elements outside 2e-3 scale + 5e-2 |ref|) are the ceiling; the figures are
    printed."""
    oracle, hr, o, d, noise, bg, gt, emb = _setup(host, L, F, LOG2_T, 256, 4.0 / 256, 512, 3.0, 23)
    hr.set_exact_ray_grad(True)
    grads = {}
    for route in ROUTES:
        _route(hr, route)
        o_g, d_g, (colors, depths, weights, idx) = _render(hr, dev, o, d, "validate", None, None, None, True)
        _loss(colors, depths).backward()
        grads[route] = (o_g.grad.cpu(), d_g.grad.cpu(), idx.cpu())
    ref_o, ref_d, ref_idx = grads["op_by_op"]
    assert float(ref_o.abs().max()) > 0 and float(ref_d.abs().max()) > 0
    for route in ("march", "dense"):
        assert torch.equal(grads[route][2], ref_idx)
        for name, got, ref in (("d_o", grads[route][0], ref_o), ("d_d", grads[route][1], ref_d)):
            scale = float(ref.abs().max())
            bad = (got - ref).abs() > 2e-3 * scale + 5e-2 * ref.abs()
            rel = float((got - ref).norm() / ref.norm())
            print("\n%s against op by op, %s: relative norm %.3e, largest |diff| / scale %.3e, outside %d of %d"
                  % (route, name, rel, float((got - ref).abs().max()) / scale, int(bad.sum()), ref.numel()))
            assert int(bad.sum()) <= ref.numel() // 1000, int(bad.sum())
            assert rel < 5e-3


# ---- the Localizer -------------------------------------------------------------------------------------

def test_localizer_with_exact_ray_grad(host, dev):
    _, hr, *_ = _setup(host, L, F, LOG2_T, 64, 4.0 / 64, 1, 3.0, 41)
    param = host.LocalizerParam()
    assert param.exact_ray_grad is False
    param.exact_ray_grad = True
    Kc = _intrinsic(1, H, W)[0]
    loc = host.Localizer(param, hr, Kc.to(dev), H, W, torch.zeros(3).to(dev), 1.0)
    g = torch.Generator().manual_seed(41)
    pose0 = _base_pose(41)
    image = torch.rand(H, W, 3, generator=g)
    results = loc.optimize_pose_by_differential(pose0.to(dev), image.to(dev), 3)
    assert len(results) == 3
    for r in results:
        assert r.shape == (3, 4) and bool(torch.isfinite(r).all())
    assert not torch.equal(results[0][:, 3].cpu(), pose0[:, 3])
    assert not torch.equal(results[2][:, 3], results[0][:, 3])
    # the switch reached the field: the same renderer's pose gradient is the exact kernel's, and differs
    # from the one with the switch off
    grads = []
    for exact in (True, False):
        hr.set_exact_ray_grad(exact)
        p = pose0.to(dev).requires_grad_(True)
        colors, _ = hr.render_image(p, Kc.to(dev), H, W, 1 << 16)
        torch.nn.functional.mse_loss(colors, image.to(dev)).backward()
        grads.append(p.grad.cpu())
    assert bool(torch.isfinite(grads[0]).all()) and float(grads[0].abs().max()) > 0
    assert not torch.equal(grads[0], grads[1])


# ---- the refiners ----------------------------------------------------------------------------------------

def test_refiners_with_the_switch_on(host, dev):
    """A PoseRefiner step and an IntrinsicsRefiner step: finite, non-zero delta.grad and gamma.grad; at
    delta = 0 the colours and the loss of the run without a refiner, bit for bit."""
    oracle, hr, o, d, noise, bg, gt, emb = _setup(host, L, F, LOG2_T, 64, 4.0 / 64, N_RAYS, 3.0, 29, E=N_CAMS)
    g = torch.Generator().manual_seed(31)
    to = lambda v: v.to(dev)
    base, K = to(_pose(g, N_CAMS)), to(_intrinsic(N_CAMS, H, W))
    cam = to(torch.randint(0, N_CAMS, (N_RAYS,), generator=g).to(torch.int32))
    ij = to(torch.stack([torch.randint(0, H, (N_RAYS,), generator=g),
                         torch.randint(0, W, (N_RAYS,), generator=g)], 1).to(torch.int32))
    hr.set_fused_ray_grad(True)
    hr.set_exact_ray_grad(True)

    def step(o_, d_):
        hr.zero_grad()
        out = hr.train_step_supervised(o_, d_, cam, to(gt), host.RaySupervision(want_colors=True), 1e-2,
                                       to(noise), to(bg), True)
        return out[0].detach().clone(), out[5].detach().clone()

    with torch.no_grad():
        o0, d0 = host.get_rays_from_cameras(base, K, cam, ij)
    loss_plain, colors_plain = step(o0, d0)
    poser = host.PoseRefiner(base)
    o1, d1, _, _ = poser.sample_random_rays(K, H, W, N_RAYS, cam_idx=cam, ij=ij)
    loss, colors = step(o1, d1)
    assert torch.equal(loss, loss_plain) and torch.equal(colors, colors_plain)
    dg = poser.delta.grad
    assert dg is not None and bool(torch.isfinite(dg).all()) and float(dg.abs().max()) > 0
    exact_delta = dg.clone()
    poser.zero_grad()
    calib = host.IntrinsicsRefiner(K)
    o2, d2, _, _ = calib.sample_random_rays(poser.poses(), H, W, N_RAYS, cam_idx=cam, ij=ij)
    loss2, colors2 = step(o2, d2)
    assert torch.equal(loss2, loss_plain) and torch.equal(colors2, colors_plain)
    gg = calib.gamma.grad
    assert gg is not None and bool(torch.isfinite(gg).all()) and float(gg.abs().max()) > 0
    assert torch.equal(poser.delta.grad, exact_delta)
    # ... and it is not the gradient of the switch-off run
    hr.set_exact_ray_grad(False)
    poser.zero_grad()
    o3, d3, _, _ = poser.sample_random_rays(K, H, W, N_RAYS, cam_idx=cam, ij=ij)
    step(o3, d3)
    assert not torch.equal(poser.delta.grad, exact_delta)


# ---- graph capture -----------------------------------------------------------------------------------------

def test_render_and_backward_with_the_switch_on_capture_in_a_graph(host, dev):
    """The setup of test_gpu_render's captured batch (dense first pass, deferred check: no host read of the
    survivor count) with rays that require a gradient: one train_step, switch on, captured and replayed."""
    oracle, hr, o, d, noise, bg, gt, emb = _setup(host, 4, 2, LOG2_T, 64, 4.0 / 64, 96, -3.0, 33)
    to = lambda x: x.to(dev)
    hr.set_fused(True)
    hr.set_fused_shade(True)
    hr.set_fused_ray_grad(True)
    hr.set_exact_ray_grad(True)
    hr.set_dense_first_pass(1)
    hr.set_deferred_check(True)
    o_g, d_g = to(o).requires_grad_(True), to(d).requires_grad_(True)
    args = (o_g, d_g, to(emb), to(gt), 1e-2, to(noise), to(bg), True)

    def batch():
        hr.zero_grad()
        o_g.grad = d_g.grad = None
        loss, sq, nv, ns = hr.train_step(*args)
        return loss

    loss_ref = batch()
    ref_o, ref_d = o_g.grad.clone(), d_g.grad.clone()
    assert hr.deferred_check_ok()
    assert float(ref_o.abs().max()) > 0 and float(ref_d.abs().max()) > 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            batch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        loss_g = batch()
    got_o, got_d = o_g.grad, d_g.grad
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss_g, loss_ref)
    # (d(enc) comes out of the shade backward's float-atomic weight sums' siblings: equal up to their order)
    for got, want in ((got_o, ref_o), (got_d, ref_d)):
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5 * float(want.abs().max()))
    assert hr.deferred_check_ok()
    hr.set_deferred_check(False)
