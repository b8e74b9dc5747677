"""The loss terms of f2n::train_step together, on the HIP step: the gradient of every term alone and of
all at once, on two scenes, six routes and four contexts (tests/step_terms_cases.py has the inputs, the
bars and their reasons; tests/test_step_terms_cpu.py the model and the mutants these assertions catch).

  1. g(all) - g(none) = sum_i [g(only i) - g(none)] for every gradient the step leaves;
  2. every fused route's D_i = g(only i) - g(none) and g(all) against the op-by-op route's, which adds
     its terms through ATen's autograd with a node per term and shares neither the fused compositing
     backward nor an unpermute node.

Contexts: "plain" no supervision; "masked" ray weights in (0, 2] with a fifth at 0, an alpha target,
composite_target on; "sky" the same with composite_target off and an EnvMap attached (its texel
gradient joins the compared set); "pose" rays from a PoseRefiner with set_fused_ray_grad(True)
(delta.grad joins).  Routes that an attachment closes are asserted to fall back, not skipped:
  * a sky or rays that carry a gradient take the caller's order: a lean_bucketed request renders on the
    plain dense route (weights handed back, no weight_var);
  * on the terminating scene the dense and the bucketed requests keep their first pass but compact: the
    step shades fewer than n S samples, every ray keeps fewer than S.

With rays that carry a gradient the op-by-op route renders the sampler kernel's own positions
(PtsSampler::get_samples_grad), as every other route does: the comparison in "pose" is on identical
samples, parameters and delta.grad alike.
"""
import importlib
import math

import numpy as np
import pytest
import torch

from tests import step_terms_cases as C
from tests.test_gpu_pose_grad import H, W, _intrinsic, _pose
from tests.test_gpu_ssim_step import _term_model
from tests.test_gpu_weight_dist import ROUTES, _route

pytestmark = pytest.mark.gpu

SCENE_NAMES = tuple(C.SCENES)
FUSED = tuple(r for r in ROUTES if not r.startswith("op_by_op"))
ENV_R = 8


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


@pytest.fixture(scope="module")
def scenes(host, dev):
    out = {}
    for name, (bias0, seed) in C.SCENES.items():
        _, hr, o, d, noise, bg, gt, emb = C.setup(host, bias0, seed)
        cpu = C.scene(name)
        assert torch.equal(o, cpu["o"]) and torch.equal(gt, cpu["gt"])       # the model's inputs
        ex = C.extras(name, noise)
        g = torch.Generator().manual_seed(seed + 5)
        base = _pose(g, C.E_IMG)
        cam = (torch.arange(C.N_PATCH) % C.E_IMG).repeat_interleave(C.P * C.P).to(torch.int32)
        i0 = torch.randint(0, H - C.P + 1, (C.N_PATCH,), generator=g)
        j0 = torch.randint(0, W - C.P + 1, (C.N_PATCH,), generator=g)
        ii, jj = torch.meshgrid(torch.arange(C.P), torch.arange(C.P), indexing="ij")
        ij = torch.stack([(i0[:, None, None] + ii).reshape(-1), (j0[:, None, None] + jj).reshape(-1)], 1)
        env = host.EnvMap(ENV_R)
        with torch.no_grad():
            env.texture.copy_(torch.from_numpy(
                (np.random.RandomState(seed).randn(6, ENV_R, ENV_R, 3) * 1.5).astype(np.float32)))
        sc = dict(name=name, hr=hr, env=env, refiner=host.PoseRefiner(base.to(dev)),
                  K=_intrinsic(C.E_IMG, H, W).to(dev), cam=cam.to(dev), ij=ij.to(torch.int32).to(dev))
        sc.update({k: v.to(dev) for k, v in dict(o=o, d=d, noise=noise, bg=bg, gt=gt, emb=emb, z=ex["z"],
                                                 alpha=ex["alpha"], m=ex["ray_weight"],
                                                 patch_weight=ex["patch_weight"]).items()})
        out[name] = sc
    return out


def _rays(sc, context):
    if context != "pose":
        return sc["o"], sc["d"], sc["emb"]
    sc["refiner"].zero_grad()
    o, d, _, cam = sc["refiner"].sample_random_rays(sc["K"], H, W, C.N, cam_idx=sc["cam"], ij=sc["ij"])
    assert o.requires_grad and d.requires_grad
    return o, d, cam


def _sup(host, sc, context, opacity_weight=0.0):
    if context not in ("masked", "sky"):
        return host.RaySupervision(want_colors=True)
    return host.RaySupervision(ray_weight=sc["m"], alpha=sc["alpha"], opacity_weight=opacity_weight,
                               want_colors=True, composite_target=context == "masked")


def _one_step(host, sc, route, context, step):
    hr, w = sc["hr"], C.weights(sc["name"], route)
    lam = {k: (w[k] if k in C.terms_on(step) else 0.0) for k in C.TERMS}
    o, d, emb = _rays(sc, context)
    bg = None if context == "sky" else sc["bg"]
    if context == "sky":
        sc["env"].zero_grad()
    opts = host.DepthLossOptions(empty=lam["empty"], near=lam["near"], expected=lam["expected"], eps=C.DEPTH_EPS)
    hr.zero_grad()
    out = hr.train_step_patches(o, d, emb, sc["gt"], host.PatchLoss(C.P, lam["ssim"], sc["patch_weight"]),
                                _sup(host, sc, context, lam["opacity"]), lam["var"], sc["noise"], bg, True,
                                dist_loss_weight=lam["dist"], depth_target=sc["z"], depth_loss=opts)
    torch.cuda.synchronize()
    grads = {k: v.clone() for k, v in hr.grads().items() if v is not None}
    if context == "sky":
        grads["sky.texture"] = sc["env"].texture.grad.clone()
    if context == "pose":
        grads["delta"] = sc["refiner"].delta.grad.clone()
    last_depth = hr.last_depth_loss
    return dict(loss=float(out[0]), n_samples=out[3], colors=out[5].clone(), grads=grads,
                last_depth=None if last_depth is None else last_depth.clone())


def _probe(sc, context, step):
    """the render a step makes -- the same flags, gradients enabled as in the step (the route depends on
    it) -- handed back with its bounds, which train_step does not return"""
    o, d, emb = _rays(sc, context)
    bg = None if context == "sky" else sc["bg"]
    on = C.terms_on(step)
    depth = bool(on & {"empty", "near", "expected"})
    opacity = "opacity" in on and context in ("masked", "sky")
    if not (depth or opacity or "dist" in on):
        return sc["hr"].render_for_loss_result(o, d, emb, "train", sc["noise"], bg)
    return sc["hr"].render_for_loss_result(o, d, emb, "train", sc["noise"], bg, "dist" in on,
                                           sc["z"] if depth else None, C.DEPTH_EPS if depth else 0.0, opacity)


_RUNS = {}


def _runs(host, capi, dev, scenes, name, route, context):
    """every step of one (scene, route, context), run once and shared by the tests"""
    key = (name, route, context)
    if key in _RUNS:
        return _RUNS[key]
    sc = scenes[name]
    hr = sc["hr"]
    _route(hr, host, dev, route, C.N)
    hr.set_fused_ray_grad(context == "pose")
    capi.set_option("BWD_PHASES", 1)
    try:
        if context == "sky":
            hr.set_background(sc["env"])
        plain, asked = _probe(sc, context, "none"), _probe(sc, context, "all")
        # The route that was reached, or the fallback it took.  What a render hands back tells the lean
        # bucketed route from the rest (no weights, a weight_var); march, dense and op by op hand back
        # the same fields, and that one of them ran rests on _route's settings, as in the tests this
        # follows.  Dense on the thin scene is at least held to its uncompacted form below
        # (n_samples == n S), and the assertion is made on a probe with the step's flags, not in the step.
        bucketed = route == "lean_bucketed" and context in ("plain", "masked")
        if bucketed:
            assert plain.weights is None and plain.weight_var is not None
        else:
            assert plain.weights is not None and plain.weight_var is None
        assert torch.equal(plain.idx_start_end, asked.idx_start_end) and torch.equal(plain.colors, asked.colors)
        count = (plain.idx_start_end[:, 1] - plain.idx_start_end[:, 0]).long()
        steps = {}
        for s in ("none",) + C.live_terms(context) + ("all",):
            steps[s] = _one_step(host, sc, route, context, s)
            # the step hands back no bounds: those of a render with the step's own flags, which is
            # tied to the step by its colours
            with_flags = _probe(sc, context, s)
            assert torch.equal(with_flags.colors, steps[s]["colors"]), s
            assert torch.equal(with_flags.idx_start_end, plain.idx_start_end), s
        terms = asked.depth_terms.detach().clone()
    finally:
        capi.set_option("BWD_PHASES", 0)
        hr.set_occupancy(None)
        hr.set_background(None)
        hr.set_fused_ray_grad(False)
    n_samples = steps["none"]["n_samples"]
    assert n_samples == int(count.sum())
    if name == "thin" and not route.endswith("grid"):
        assert n_samples == C.N * C.S
    if name == "terminating":
        # compacted: no ray keeps all S, so whatever a term's gradient touches belongs to such a ray
        assert n_samples < C.N * C.S and int(count.max()) < C.S and int(count.min()) > 0
    if not route.endswith("grid"):
        assert int(count.max()) > 64
    for s, run in steps.items():                          # no term changes the render (bounds: above)
        assert run["n_samples"] == n_samples and torch.equal(run["colors"], steps["none"]["colors"]), s
    _RUNS[key] = dict(steps=steps, grads={s: r["grads"] for s, r in steps.items()}, terms=terms)
    return _RUNS[key]


def _precondition(tag, grads):
    sh = C.shares(grads)
    print("[step-terms] %s: |D_i| / |g(none)| = %s" % (tag, {k: round(v, 3) for k, v in sh.items()}))
    assert min(sh.values()) >= C.MIN_SHARE, sh


@pytest.mark.parametrize("context", C.CONTEXTS)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_sum_of_the_parts(host, capi, dev, scenes, name, route, context):
    run = _runs(host, capi, dev, scenes, name, route, context)
    tag = "%s %s %s" % (name, route, context)
    grads, steps = run["grads"], run["steps"]
    assert all(g.keys() == grads["none"].keys() for g in grads.values())
    assert "scene_field.feat_pool" in grads["none"] and ("delta" in grads["none"]) == (context == "pose")
    assert ("sky.texture" in grads["none"]) == (context == "sky")
    _precondition(tag, grads)
    ratios = C.sum_of_parts(grads)
    for cls in ("table", "net", "rays"):
        r = {k: v for k, v in ratios.items() if C.key_class(k) == cls}
        if r:
            k, v = C.worst(r)
            print("[step-terms] %s sum of parts, %s: residual / bar = %.4f (accepted %.3g) at %s" % (
                tag, cls, v, C.allowed(name, "a1", k), k))
    for k, v in ratios.items():
        assert v <= C.allowed(name, "a1", k), (tag, k, v)
    # the loss: each step's is formed from non-negative pieces with the roundings the per-term tests
    # count, (5 + log2 n) u of itself; k + 2 of them meet here
    terms = C.live_terms(context)
    loss = {s: steps[s]["loss"] for s in steps}
    resid = abs((loss["all"] - loss["none"]) - sum(loss[t] - loss["none"] for t in terms))
    tol = C.U * (5.0 + math.log2(C.N)) * sum(abs(v) for v in loss.values())
    print("[step-terms] %s loss(all) %.7f, sum of the parts off by %.2e of %.2e" % (tag, loss["all"], resid, tol))
    assert resid <= tol and all(loss[t] > loss["none"] for t in terms)
    if context in ("masked", "sky"):
        # the depth terms' divisor under a mask: n_valid, with invalid targets in the batch
        sc = scenes[name]
        want = (run["terms"].double() * sc["m"].double()[:, None]).sum(0) / C.depth_n_valid(sc["z"].cpu())
        got = steps["all"]["last_depth"].double()
        assert bool(((got - want).abs() <= 32 * C.U * want).all()) and float(want.min()) > 0


@pytest.mark.parametrize("context", C.CONTEXTS)
@pytest.mark.parametrize("route", FUSED)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_each_term_against_op_by_op(host, capi, dev, scenes, name, route, context):
    run = _runs(host, capi, dev, scenes, name, route, context)
    ref_route = "op_by_op_grid" if route == "march_grid" else "op_by_op"
    ref = _runs(host, capi, dev, scenes, name, ref_route, context)
    tag = "%s %s %s" % (name, route, context)
    _precondition(tag, run["grads"])
    _precondition(tag + " (op by op)", ref["grads"])
    ratios = C.against(run["grads"], ref["grads"])
    for cls in ("table", "net", "rays"):
        r = {k: v for k, v in ratios.items() if C.key_class(k[1]) == cls}
        if r:
            k, v = C.worst(r)
            print("[step-terms] %s against op by op, %s: residual / bar = %.4f (accepted %.3g) at %s" % (
                tag, cls, v, C.allowed(name, "a2", k[1]), k))
    for (s, k), v in ratios.items():
        assert v <= C.allowed(name, "a2", k), (tag, s, k, v)


@pytest.mark.parametrize("context", ["plain", "masked"])
@pytest.mark.parametrize("route", ["lean_bucketed", "op_by_op"])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_ssim_term_on_the_routes_left_open(host, capi, dev, scenes, name, route, context):
    """the loss identity of tests/test_gpu_ssim_step.py where NOTES section 35 had left it unchecked"""
    run = _runs(host, capi, dev, scenes, name, route, context)
    sc, steps = scenes[name], run["steps"]
    lam = C.weights(name, route)["ssim"]
    gt, bg = sc["gt"].cpu().numpy(), sc["bg"].cpu().numpy()
    a = sc["alpha"].cpu().numpy()[:, None]
    target = a * gt + (np.float32(1) - a) * bg if context == "masked" else gt
    term, bound, _ = _term_model(steps["none"]["colors"].cpu().numpy(), target, C.N_PATCH, C.P,
                                 sc["patch_weight"].cpu().numpy())
    loss, loss0 = steps["ssim"]["loss"], steps["none"]["loss"]
    err = abs(loss - (loss0 + lam * term))
    allowed = lam * bound + 4 * 2.0 ** -24 * max(1.0, abs(loss))
    print("[step-terms] %s %s %s: loss %.7f = %.7f + %.3g * %.6f, err %.2e of %.2e" % (
        name, route, context, loss, loss0, lam, term, err, allowed))
    assert err <= allowed and term > 0.1
