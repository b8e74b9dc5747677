"""The CPU half of the step-terms tests: the model of tests/step_terms_cases.py against the per-term
models the suite already has, the two assertions of tests/test_gpu_step_terms.py on the unmutated model,
and on every mutant -- which must fail one of them, while passing what the suite asserted about a step's
gradient before."""
import math

import numpy as np
import pytest
import torch

from oracle import ref_render as R
from tests import depth_sight_model as dm
from tests import dist_cases as dc
from tests import ragged_cases as rc
from tests import ssim_model as ssm
from tests import step_terms_cases as C
from tests import supervision_model as sm

SCENE_NAMES = tuple(C.SCENES)
CASES = [(s, c) for s in SCENE_NAMES for c in C.CONTEXTS]
# mutants that the assertions the suite had before already catch, through the LOSS they change; they
# are kept out of the list the new assertions must catch (test_todays_assertions_pass_every_mutant
# checks both halves of this)
CAUGHT_TODAY = {
    "mask_after_reduction": "tests/test_gpu_supervised_step.py::test_masked_rays_regularise_nothing",
    "ssim_target_plain":
        "tests/test_gpu_ssim_step.py::test_with_ray_supervision_the_target_is_the_composited_one",
}
ELIGIBLE = tuple(m for m in C.MUTANTS if m not in CAUGHT_TODAY)
# the widest relative tolerance a loss value is held to by the tests of a step today
# (tests/test_gpu_render.py::test_train_step_matches_oracle); the per-term tests are tighter
TODAY_LOSS_RTOL = 1e-5


def test_scene_conditions():
    for name in SCENE_NAMES:
        r = C.model_render(name, "plain", "f32")
        count = (r.idx[:, 1] - r.idx[:, 0]).long()
        z = C.scene(name)["z"]
        m = C.scene(name)["ray_weight"]
        print("%s: %d samples kept, %d..%d per ray" % (name, int(count.sum()), int(count.min()), int(count.max())))
        assert int(count.sum()) >= 65536                       # the binned table gradient
        assert int(count.min()) > 64                           # more than one 64-sample stride per ray
        assert bool((count == C.S).all()) if name == "thin" else bool((count < C.S).all())
        assert C.depth_n_valid(z) == C.N - C.N // 8
        assert int(m.eq(0).sum()) == C.N // 5 and float(m.max()) <= 2.0 and float(m[m > 0].min()) > 0


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_terms_agree_with_the_per_term_models(name):
    """the per-ray quantities and the loss pieces of the float64 model against dist_cases, depth_sight_model,
    supervision_model, ssim_model and the oracle's weight_var, on the render's own weights"""
    inp = C.scene(name)
    r = C.model_render(name, "masked", "f32")
    w32 = r.weights.detach()
    var, dist, terms, opacity = C.per_ray(r, w32.double(), inp["z"])
    n_total = w32.numel()
    lay = rc.Layout(r.idx.contiguous(), np.zeros(C.N), n_total)
    ref_d = dc.dist_ref(lay, dict(weights=w32, t=r.t, dt=r.dt, d_out=torch.ones(C.N)))
    assert np.abs(dist.numpy() - ref_d["D"]).max() <= 1e-9 * max(1.0, float(ref_d["D"].max()))
    case = dict(weights=w32, t=r.t, dt=r.dt, z=inp["z"], d_out=torch.ones(C.N, 3),
                eps=float(np.float32(C.DEPTH_EPS)))
    ref_s = dm.sight_ref(lay, case)
    assert np.abs(terms.numpy() - ref_s["out"]).max() <= 1e-9 * max(1.0, float(np.abs(ref_s["out"]).max()))
    assert float(terms[:, 0].max()) > 0 and float(terms[:, 1].min()) < 0.999 and float(terms[:, 2].max()) > 0
    var32 = R.weight_var(w32, r.idx)
    assert float((var.float() - var32).abs().max()) <= 1e-5 * float(var32.abs().max())
    assert float((opacity.float() - R.flex_sum(w32, r.idx)).abs().max()) <= 1e-5
    # the loss pieces: the supervised loss with the composited target and the opacity term
    W = C.WEIGHTS[name]
    _, _, pieces = C.model_step(name, "masked", "f64", "all")
    np32 = lambda t: t.detach().numpy().astype(np.float32)
    case = dict(colors=np32(r.colors), gt=np32(inp["gt"]), bg=np32(inp["bg"]), var=np32(var32),
                ray_weight=np32(inp["ray_weight"]), alpha=np32(inp["alpha"]), opacity=np32(opacity.float()))
    ref_l = sm.loss_ref(case, W["var"], W["opacity"], True)
    got = pieces["colour"] + pieces["var"] + pieces["opacity"]
    assert abs(got - ref_l["out"][0]) <= 1e-5 * ref_l["out"][0]
    # the patch term on the composited target
    a = inp["alpha"].double()[:, None]
    target = (a * inp["gt"].double() + (1 - a) * inp["bg"].double()).numpy().reshape(C.N_PATCH, C.P, C.P, 3)
    x = C.model_render(name, "masked", "f64").colors.detach().numpy().reshape(C.N_PATCH, C.P, C.P, 3)
    s64 = np.array([ssm.ssim64(x[b], target[b], False)[0] for b in range(C.N_PATCH)])
    pw = inp["patch_weight"].double().numpy()
    want = W["ssim"] * float((pw * (1 - s64)).sum() / pw.sum())
    assert abs(pieces["ssim"] - want) <= 1e-9 and want > 0
    # the regularisers: masked before their reductions, which keep their divisors (1e-5: the pieces
    # are the twin's, on its float64 weights; `dist` and `terms` here come from the float32 ones)
    m = inp["ray_weight"].double()
    want = W["dist"] * float((dist * m).sum()) / C.N
    assert abs(pieces["dist"] - want) <= 1e-5 * want
    lam = torch.tensor([W["empty"], W["near"], W["expected"]], dtype=torch.float64)
    want = float(((terms * m[:, None]).sum(0) * lam).sum()) / C.depth_n_valid(inp["z"])
    assert abs(pieces["depth"] - want) <= 1e-5 * want


def _model_ratios(name, context):
    g32, g64 = C.model_grads(name, context, "f32"), C.model_grads(name, context, "f64")
    common = {s: {k: v for k, v in g32[s].items() if k in g64[s]} for s in g32}
    return C.sum_of_parts(g32), C.against(common, g64)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_model_residuals_are_the_recorded_ones(name):
    """how much of each bar a correct float32 step uses; the recorded figures set the widened bars"""
    worst = {}
    for context in C.CONTEXTS:
        a1, a2 = _model_ratios(name, context)
        for k, v in a1.items():
            key = ("a1", C.key_class(k))
            worst[key] = max(worst.get(key, 0.0), v)
        for (_, k), v in a2.items():
            key = ("a2", C.key_class(k))
            worst[key] = max(worst.get(key, 0.0), v)
    for (which, cls), v in sorted(worst.items()):
        rec = C.MODEL_RESIDUAL[(name, which, cls)]
        print("  %s %s %s: model residual / bar = %.4f (recorded %.4g, accepted %.3g)" % (
            name, which, cls, v, rec, 4.0 * rec if rec > 0.25 else 1.0))
        if rec <= 0.25:
            assert v <= 0.25, (which, cls, v, rec)             # the bar stands as it is
        if cls != "net":
            # driven by the f16 roundings: the figure repeats, and a widened bar stays 4 x the model
            assert rec == 0.0 or abs(v / rec - 1.0) <= 0.03, (which, cls, v, rec)
        elif rec > 0.25:
            # BLAS reassociation noise, which moves with the machine and its thread count (0.243 and
            # 0.260 on two): not above the recorded figure by more than that, nor far below it
            assert 0.8 * rec <= v <= 1.03 * rec, (which, cls, v, rec)


@pytest.mark.parametrize("name,context", CASES)
def test_unmutated_model_passes(name, context):
    g32 = C.model_grads(name, context, "f32")
    sh = C.shares(g32)
    print("  %s %s: |D_i| / |g(none)| = %s" % (name, context, {k: round(v, 3) for k, v in sh.items()}))
    assert set(sh) == set(C.live_terms(context)) and min(sh.values()) >= C.MIN_SHARE
    a1, a2 = _model_ratios(name, context)
    for k, v in a1.items():
        assert v <= C.allowed(name, "a1", k), (k, v)
    for (s, k), v in a2.items():
        assert v <= C.allowed(name, "a2", k), (s, k, v)
    # the float64 twin: the sum of the parts is exact but for the f16 contributions of the table
    g64 = C.model_grads(name, context, "f64")
    for k, v in C.sum_of_parts(g64).items():
        assert v <= (C.allowed(name, "a1", k) if C.key_class(k) == "table" else 1e-6), (k, v)


def _violations(name, context, mut):
    """residual / accepted of both assertions for a mutant (the op-by-op side: the unmutated model)"""
    g = C.model_grads(name, context, "f32", mut)
    ref = C.model_grads(name, context, "f32")
    v1 = {("a1", k): v / C.allowed(name, "a1", k) for k, v in C.sum_of_parts(g).items()}
    v2 = {("a2",) + sk: v / C.allowed(name, "a2", sk[1]) for sk, v in C.against(g, ref).items()}
    return v1, v2


@pytest.mark.parametrize("mut", ELIGIBLE)
def test_mutant_is_caught(mut):
    rows = []
    for name, context in CASES:
        if not C.applies(mut, name, context):
            continue
        v1, v2 = _violations(name, context, mut)
        k1, k2 = C.worst(v1), C.worst(v2)
        rows.append((name, context, k1[1], k2[1]))
        print("  %-24s %-11s %-6s sum of parts %9.2f x accepted, against op-by-op %9.2f x (%s)" % (
            mut, name, context, k1[1], k2[1], k2[0][1]))
    assert rows
    smallest = min(max(r[2], r[3]) for r in rows)
    print("  %-24s caught in %d of %d contexts, smallest violation / bar %.2f" % (
        mut, sum(max(r[2], r[3]) > 1.0 for r in rows), len(rows), smallest))
    assert smallest > 1.0


def _today(name, context, mut, step):
    """what the suite asserted about a step with a term on before: its loss; a finite gradient; and, on
    a thin medium only (the scenes of test_train_step_with_distortion_weight, _with_depth_loss and
    test_loss_gains_the_weighted_term), a table gradient that differs from g(none)'s.  The one test of
    the depth terms under a mask has a valid target on every ray: n_for_n_valid is judged on that."""
    inp, r = C.scene(name), C.model_render(name, context, "f32")
    if mut == "n_for_n_valid":
        inp = dict(inp, z=torch.full((C.N,), 1.5))
    on = C.terms_on(step)
    loss, g, _ = C.step_grads(r, inp, context, on, mut if C.affected(mut, step) else None)
    want = C.step_grads(r, inp, context, on)[0]
    g0 = C.step_grads(r, inp, context, set(), mut if C.affected(mut, "none") else None)[1]
    key = "scene_field.feat_pool"
    ok = abs(loss - want) <= TODAY_LOSS_RTOL * abs(want) and all(bool(torch.isfinite(v).all()) for v in g.values())
    return ok and (name != "thin" or not torch.equal(g[key], g0[key]))


@pytest.mark.parametrize("mut", tuple(C.MUTANTS))
def test_todays_assertions_pass_every_mutant(mut):
    """the mirror of test_the_old_inputs_hide_the_suffix_carry: each mutant the new assertions are
    asked to catch is green under the old ones -- and the two set aside in CAUGHT_TODAY are not"""
    green = []
    for name, context in CASES:
        if not C.applies(mut, name, context):
            continue
        steps = [s for s in C.live_terms(context) + ("all",) if C.affected(mut, s)]
        green.append(all(_today(name, context, mut, s) for s in steps))
    assert green
    if mut in CAUGHT_TODAY:
        assert not any(green), "caught by %s: in every context" % CAUGHT_TODAY[mut]
    else:
        assert all(green)


def test_n_for_n_valid_changes_a_loss_nobody_checks():
    """n_for_n_valid does change the loss -- by n_valid / n -- but the one test of a mask with the depth
    terms (test_masked_rays_regularise_nothing) uses a target that is valid on every ray, where n_valid
    = n: on its inputs the mutant's loss is the right one.  The GPU file therefore holds
    last_depth_loss to sum m terms / n_valid with invalid targets in the batch."""
    name, context = "terminating", "masked"
    right = C.model_step(name, context, "f32", "all")[0]
    wrong = C.model_step(name, context, "f32", "all", "n_for_n_valid")[0]
    assert abs(wrong - right) > 1e-3 * right
    inp = dict(C.scene(name))
    inp["z"] = torch.full((C.N,), 1.5)
    r = C.model_render(name, context, "f32")
    on = C.terms_on("all")
    a = C.step_grads(r, inp, context, on)[0]
    b = C.step_grads(r, inp, context, on, "n_for_n_valid")[0]
    assert a == b and math.isfinite(a)
