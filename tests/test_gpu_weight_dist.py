"""The distortion loss on the GPU: f2n_weight_dist_fwd / _bwd through the C ABI, the autograd op
host.weight_dist, Renderer.render_for_loss(want_dist) on every route and train_step with a
distortion weight -- each against the float64 double sum of tests/dist_cases.py within its bound
tol = u (len_r M_sum + K_DIST M_op)."""
import importlib
import math

import numpy as np
import pytest
import torch

from tests import dist_cases as dc
from tests import ragged_cases as rc
from tests.test_gpu_occupancy import _scene_grid
from tests.test_gpu_render import _setup

pytestmark = pytest.mark.gpu

CASES = [(name, variant) for name in rc.LAYOUTS for variant in dc.T_VARIANTS]


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def _report(lay, got, ref, what):
    """print the figures, then assert"""
    for name, (ratio, _) in dc.ratios(lay, got, ref).items():
        err = np.abs(np.asarray(got[name], dtype=np.float64) - ref[name])[
            (dc._ray_index(lay, name) >= 0)]
        print("  %s %s: largest (err/u - len M_sum)/M_op = %.3f (K = %g), largest err = %.3e" % (
            what, name, float(ratio.max()), dc.K_DIST, float(err.max()) if err.size else 0.0))
    rc.assert_no_failures(dc.dist_failures(lay, got, ref), what)


# ---- kernels through the C ABI --------------------------------------------------------------------

@pytest.mark.parametrize("name,variant", CASES)
def test_kernels_per_element(capi, dev, name, variant):
    lay, case, ref = dc.shared(name, variant)
    w, t, dt, d_out = (case[k].to(dev) for k in ("weights", "t", "dt", "d_out"))
    bounds = lay.bounds.to(dev)
    runs = []
    for _ in range(2):
        D = torch.full((lay.n_rays,), rc.SENTINEL, device=dev)
        dw = torch.full((lay.n_total,), rc.SENTINEL, device=dev)
        capi.call("weight_dist_fwd", w, t, dt, bounds, D, lay.n_rays)
        capi.call("weight_dist_bwd", w, t, dt, bounds, d_out, dw, lay.n_rays)
        runs.append((D, dw))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    got = dict(D=runs[0][0].cpu().numpy(), dw=runs[0][1].cpu().numpy())
    # (empty rays: D exactly 0, nothing of dw written; outside every range dw keeps SENTINEL)
    assert (got["D"][lay.len == 0] == 0.0).all() and (lay.len == 0).sum() == 4
    _report(lay, got, ref, "%s %s" % (name, variant))


def test_no_rays_is_ok_and_writes_nothing(capi, dev):
    out = torch.full((4,), rc.SENTINEL, device=dev)
    z = torch.zeros(4, device=dev)
    idx = torch.zeros(1, 2, dtype=torch.int32, device=dev)
    capi.call("weight_dist_fwd", z, z, z, idx, out, 0)
    capi.call("weight_dist_bwd", z, z, z, idx, z, out, 0)
    assert bool((out == rc.SENTINEL).all())


# ---- the autograd op ------------------------------------------------------------------------------

def _grad_as_kernel_output(lay, grad):
    """the op zero-fills dw; what the kernel must have left alone is checked to be that zero, then
    set to SENTINEL for dist_failures"""
    g = grad.cpu().numpy().copy()
    assert (g[~lay.inside] == 0.0).all()
    g[~lay.inside] = rc.SENTINEL
    return g


class _DropGrad(torch.autograd.Function):
    """identity whose backward hands on no gradient at all"""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return None


def test_autograd_op(host, capi, dev):
    lay, case, ref = dc.shared("gaps", "thinned")
    t, dt, d_out = (case[k].to(dev) for k in ("t", "dt", "d_out"))
    bounds = lay.bounds.to(dev)
    w = case["weights"].to(dev).requires_grad_(True)
    t_req = t.clone().requires_grad_(True)
    D = host.weight_dist(w, t_req, dt, bounds)
    (D * d_out).sum().backward()
    assert t_req.grad is None                           # positions are data: no gradient
    got = dict(D=D.detach().cpu().numpy(), dw=_grad_as_kernel_output(lay, w.grad))
    _report(lay, got, ref, "host.weight_dist")

    # an undefined upstream gradient stays undefined (lean gradients: the default) ...
    w2 = case["weights"].to(dev).requires_grad_(True)
    other = (w2 * 2.0).sum()
    (_DropGrad.apply(host.weight_dist(w2, t, dt, bounds)).sum() + other).backward()
    assert torch.equal(w2.grad, torch.full_like(w2, 2.0))
    # ... and is a zero where the nodes are asked to materialise them
    with capi.option("DENSE_LEAN", 1):
        w3 = case["weights"].to(dev).requires_grad_(True)
        (_DropGrad.apply(host.weight_dist(w3, t, dt, bounds)).sum() + (w3 * 2.0).sum()).backward()
    assert torch.equal(w3.grad, w2.grad)

    # a non-contiguous view of the weights
    pair = torch.stack([case["weights"], torch.rand(lay.n_total)], 1).to(dev).requires_grad_(True)
    D_view = host.weight_dist(pair[:, 0], t, dt, bounds)
    assert not pair[:, 0].is_contiguous() and torch.equal(D_view, D)
    (D_view * d_out).sum().backward()
    assert torch.equal(pair.grad[:, 0], w.grad) and not bool(pair.grad[:, 1].any())


# ---- Renderer routes ------------------------------------------------------------------------------

N_RAYS, N_TRAIN, S = 256, 1024, 128


def _scene(host, dev, n_rays, bias0, seed):
    oracle, hr, o, d, noise, bg, gt, emb = _setup(host, 8, 2, 14, S, 4.0 / S, n_rays, bias0, seed)
    to = lambda v: v.to(dev)
    o, d, noise, bg, gt, emb = (to(v) for v in (o, d, noise, bg, gt, emb))
    pts, _, dt, t, _ = hr.pts_sampler.get_samples(o, d, "train", noise)
    return dict(hr=hr, args=(o, d, emb, "train", noise, bg), gt=gt, pts=pts, n_rays=n_rays,
                t=t.reshape(n_rays, S).cpu(), dt=dt.reshape(n_rays, S).cpu())


@pytest.fixture(scope="module")
def scene(host, dev):
    """the small trained-like renderer of tests/test_gpu_render.py, 256 rays at S = 128; bias 4: many
    rays stop in their second stride, so kept prefixes cross a stride boundary"""
    return _scene(host, dev, N_RAYS, 4.0, 31)


@pytest.fixture(scope="module")
def thin_scene(host, dev):
    """1024 rays of a thin medium: every sample is kept, and 131072 samples put the table gradient on
    the exact binned sums, whose bits do not depend on the order (with BWD_PHASES = 1)"""
    return _scene(host, dev, N_TRAIN, 1.0, 37)


def _route(hr, host, dev, route, n_rays=N_RAYS):
    hr.set_occupancy(None)
    hr.set_fused(route not in ("op_by_op", "op_by_op_grid"))
    hr.set_dense_first_pass(1 if route in ("dense", "lean_bucketed") else 0)
    # the options tests/test_gpu_dense_lean.py reaches the lean bucketed route with, at the smallest
    # ray count they allow: ray_order_min_rays = the batch
    hr.set_ray_order_min_rays(n_rays if route == "lean_bucketed" else 1 << 30)
    if route.endswith("grid"):
        hr.set_occupancy(_scene_grid(host, dev, 64, "shell", 1))


ROUTES = ("op_by_op", "march", "dense", "lean_bucketed", "march_grid", "op_by_op_grid")


@pytest.mark.parametrize("route", ROUTES)
def test_render_for_loss_weight_dist(host, capi, dev, scene, route):
    hr = scene["hr"]
    _route(hr, host, dev, route)
    try:
        with torch.no_grad():
            today = hr.render(*scene["args"])                       # (colors, depths, weights, idx)
            plain = hr.render_for_loss(*scene["args"])
            asked = hr.render_for_loss(*scene["args"], want_dist=True)
    finally:
        hr.set_occupancy(None)
    # without want_dist: what the call returns today; with it: the same, plus weight_dist
    assert plain[5] is None
    for a, b in zip(plain[:5], asked[:5]):
        assert (a is None and b is None) or torch.equal(a, b)
    assert torch.equal(plain[0], today[0]) and torch.equal(plain[1], today[1])
    assert torch.equal(plain[3], today[3])
    if route == "lean_bucketed":
        assert plain[2] is None and plain[4] is not None           # the route was reached
    else:
        assert torch.equal(plain[2], today[2]) and plain[4] is None
    weights, idx, dist = today[2].cpu(), today[3].cpu(), asked[5]
    assert dist.shape == (N_RAYS,)

    # the kept samples of each ray: the first e - s of its S samples, or with a grid the first e - s
    # occupied ones (the occupied among the first len_r)
    count = (idx[:, 1] - idx[:, 0]).long()
    assert int(count.sum()) == weights.numel()
    if not route.endswith("grid"):       # (a thinned list is shorter: 59 samples at the most here)
        assert int(count.max()) > rc.WAVE  # more than one stride: the carries are in play
    if route.endswith("grid"):
        occ = hr_occupied(host, dev, scene).reshape(N_RAYS, S).cpu()
        rank = torch.cumsum(occ.long(), 1)
        keep = occ & (rank <= count[:, None])
    else:
        keep = torch.arange(S)[None, :] < count[:, None]
    assert torch.equal(keep.sum(1), count)
    lay = rc.Layout(idx.contiguous(), np.zeros(N_RAYS), weights.numel())
    case = dict(weights=weights, t=scene["t"][keep], dt=scene["dt"][keep], d_out=torch.ones(N_RAYS))
    ref = dc.dist_ref(lay, case)
    assert float(ref["D"].max()) > 1e-3
    _report(lay, dict(D=dist.cpu().numpy()), ref, route)


def hr_occupied(host, dev, scene):
    return _scene_grid(host, dev, 64, "shell", 1).occupied(scene["pts"])


def test_thinned_lists_have_gaps(host, dev, scene):
    """the grid case above is the one the loss was added for: list neighbours several steps apart"""
    hr = scene["hr"]
    _route(hr, host, dev, "march_grid")
    try:
        with torch.no_grad():
            idx = hr.render(*scene["args"])[3].cpu()
    finally:
        hr.set_occupancy(None)
    count = (idx[:, 1] - idx[:, 0]).long()
    occ = hr_occupied(host, dev, scene).reshape(N_RAYS, S).cpu()
    keep = occ & (torch.cumsum(occ.long(), 1) <= count[:, None])
    first = keep.float().argmax(1)
    last = S - 1 - keep.flip(1).float().argmax(1)
    assert bool(((last - first + 1)[count > 0] > count[count > 0]).any())


# ---- training step --------------------------------------------------------------------------------

def _step(hr, scene, *extra, all_grads=False, **kw):
    """-> (loss, sq_err_sum, n_samples, table gradient), and with all_grads a fifth element: every
    gradient the step left, by name"""
    o, d, emb, _, noise, bg = scene["args"]
    hr.zero_grad()
    loss, sq, n_val, n_samp = hr.train_step(o, d, emb, scene["gt"], 1e-2, noise, bg, True, *extra, **kw)
    torch.cuda.synchronize()
    out = (loss.clone(), sq.clone(), n_samp, hr.grads()["scene_field.feat_pool"].clone())
    if all_grads:
        out += ({k: v.clone() for k, v in hr.grads().items() if v is not None},)
    return out


def _term_against_op_by_op(hr, host, dev, scene, route, with_term, without, **kw):
    """The term's own gradient D = g(with) - g(without), and g(with) itself, against the op-by-op
    route's, which adds the term through ATen's autograd on operators of its own: every gradient the
    step leaves, to 1e-4 of the largest norm among the full gradients involved (the figure this file
    holds a table gradient to between two routes; tests/step_terms_cases.py has the reasoning)."""
    from tests import step_terms_cases as stc
    _route(hr, host, dev, "op_by_op", N_TRAIN)
    ref = dict(none=_step(hr, scene, all_grads=True)[4], all=_step(hr, scene, all_grads=True, **kw)[4])
    _route(hr, host, dev, route, N_TRAIN)
    got = dict(none=without, all=with_term)
    for name, g in (("D", {"none": got["none"], "term": got["all"]}), ("g", got)):
        r = dict(none=ref["none"], term=ref["all"]) if name == "D" else ref
        ratios = stc.against(g, r)
        key, worst = stc.worst(ratios)
        print("  %s: %s against op by op, largest residual / (1e-4 max|g|) = %.4f at %s" % (
            route, name, worst, key))
        assert worst <= 1.0, (route, name, key, worst)
    share = stc.shares(dict(none=got["none"], term=got["all"]))["term"]
    print("  %s: |D| / |g(none)| = %.3f" % (route, share))
    assert share >= stc.MIN_SHARE


@pytest.mark.parametrize("route", ["march", "dense", "lean_bucketed"])
def test_train_step_with_distortion_weight(host, capi, dev, thin_scene, route):
    scene = thin_scene
    hr = scene["hr"]
    _route(hr, host, dev, route, N_TRAIN)
    capi.set_option("BWD_PHASES", 1)          # table gradient sums independent of the order
    loss0, sq0, ns0, g0, all0 = _step(hr, scene, all_grads=True)    # the existing call
    assert hr.last_dist_loss is None
    loss1, sq1, ns1, g1 = _step(hr, scene, dist_loss_weight=0.0)
    assert torch.equal(loss1, loss0) and torch.equal(sq1, sq0) and ns1 == ns0
    assert torch.equal(g1, g0) and float(g0.abs().max()) > 0
    assert hr.last_dist_loss is None

    lam = 0.1
    with torch.no_grad():
        dist = hr.render_for_loss(*scene["args"], want_dist=True)[5]
    loss2, sq2, ns2, g2, all2 = _step(hr, scene, all_grads=True, dist_loss_weight=lam)
    assert torch.equal(sq2, sq0) and ns2 == ns0 == N_TRAIN * S
    mean = dist.mean()
    assert torch.equal(hr.last_dist_loss, mean) and not hr.last_dist_loss.requires_grad
    # loss = fl(loss0 + fl(lam mean)): the mean's pairwise sum of 1024 terms, one product, one sum
    want = float(loss0) + lam * float(dist.double().mean())
    tol = rc.U * (2.0 + math.log2(N_TRAIN)) * (abs(float(loss0)) + lam * float(mean))
    print("  %s: loss %.9g, want %.9g, tol %.3e, dist mean %.6g" % (
        route, float(loss2), want, tol, float(mean)))
    assert float(mean) > 1e-3 and abs(float(loss2) - want) <= tol
    assert not torch.equal(g2, g0)
    # the term pulls: its gradient is there, and finite
    assert bool(torch.isfinite(g2).all()) and float((g2 - g0).abs().max()) > 0
    # ... and it is the right one: the op-by-op route's
    _term_against_op_by_op(hr, host, dev, scene, route, all2, all0, dist_loss_weight=lam)
    _step(hr, scene)
    assert hr.last_dist_loss is None


def test_per_ray_gradient_comes_back_in_the_callers_order(host, capi, dev, thin_scene):
    """sum_r c_r D_r with a different c_r for every ray: on the lean bucketed route the gradient of
    weight_dist travels back through RayUnpermuteFn's per-ray gather, and a wrong map there would hand
    ray r the factor of another ray.  The table gradient must be the one of the routes that keep the
    caller's order: to 1e-4 of its norm (the figure tests/test_gpu_render.py holds a table gradient
    to: a route may flip single f16 roundings of contributions; a permuted c is an error of order 1,
    which the last assertion shows on the same data)."""
    scene = thin_scene
    hr = scene["hr"]
    capi.set_option("BWD_PHASES", 1)
    g = torch.Generator().manual_seed(5)
    c = (0.1 + 1.9 * torch.rand(N_TRAIN, generator=g)).to(dev)
    grads = {}
    for route, coeff in (("march", c), ("dense", c), ("lean_bucketed", c), ("permuted", c.flip(0))):
        _route(hr, host, dev, "march" if route == "permuted" else route, N_TRAIN)
        hr.zero_grad()
        res = hr.render_for_loss(*scene["args"], want_dist=True)
        if route == "lean_bucketed":
            assert res[2] is None and res[4] is not None            # the route was reached
        (res[5] * coeff).sum().backward()
        torch.cuda.synchronize()
        grads[route] = hr.grads()["scene_field.feat_pool"].clone()
    ref = grads["march"]
    assert float(ref.norm()) > 0
    for route in ("dense", "lean_bucketed", "permuted"):
        rel = float((grads[route] - ref).norm() / ref.norm())
        print("  %s against march: |dg| / |g| = %.3e" % (route, rel))
        assert (rel > 1e-2) if route == "permuted" else (rel <= 1e-4), (route, rel)
