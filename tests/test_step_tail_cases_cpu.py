"""The power of the GPU tests of the step's tail (tests/test_gpu_adam.py, test_gpu_loss.py,
test_gpu_scatter_bwd.py), checked without a GPU: the float64 references of tests/step_tail_cases.py
agree with torch in float64, the constants K are re-measured on the f32 restatements, the assertion
functions accept the restatements and reject every mutant on the cases it names, and f2n_adam_step
validates its arguments before any HIP work."""
import math

import numpy as np
import pytest
import torch

from tests import step_tail_cases as st

SMALL = [(n, wd) for n in st.SMALL_SIZES for wd in st.WDS]


def _pow2_of_4x(x):
    return 2.0 ** math.ceil(math.log2(4.0 * x))


# ---- Adam -----------------------------------------------------------------------------------------

def test_adam_inputs_are_what_the_docstring_says():
    assert st.P == 256 * 16 * 256 * 4 and 4 * st.P == 16 * 2 * 2 ** 19
    assert set(st.BIG_PAIRS) == set(st.BIG_SIZES)
    assert len(set(st.BIG_PAIRS.values())) == len(st.BIG_SIZES)          # different pairs
    case = st.adam_case(1025, 1e-6)
    p, g, m, v = (case[k] for k in ("p", "g", "m", "v"))
    assert all(a.dtype == np.float32 for a in (p, g, m, v))
    ag = np.abs(g[g != 0])
    assert ag.min() < 1e-12 and ag.max() > 1.0
    assert ((g == 0) & (m != 0) & (v != 0)).sum() > 50
    assert ((g == 0) & (m == 0) & (v == 0)).sum() > 100
    vv = v[v != 0]
    assert vv.min() < 1e-28 and vv.max() > 1e-6
    # sqrt(v) on both sides of eps
    assert (np.sqrt(vv.astype(np.float64)) < st.EPS * 10).any() and (np.sqrt(vv) > 1e-5).any()
    chosen = p[(case["cat"] == 15) | (case["cat"] == 16)]
    h = st.f16_rne_bits(chosen).view(np.float16)
    assert np.isinf(h).any() and (np.abs(h) == 65504).any()               # +-65520 -> inf, 65504 stays
    sub = (np.abs(chosen) < 2.0 ** -14) & (chosen != 0)
    assert sub.sum() > 5 and (chosen == 0).any() and np.signbit(chosen[chosen == 0]).any()
    # ties: the f32 value lies exactly between two f16 neighbours
    c64 = chosen.astype(np.float64)
    down, up = (st._f16_trunc_bits(chosen).view(np.float16).astype(np.float64),
                h.astype(np.float64))
    tie = np.isfinite(up) & (down != up) & (np.abs(c64 - down) == np.abs(up - c64))
    assert tie.sum() >= 3
    # the table regime: f16 subnormals and the first normals
    t = p[case["cat"] >= 18]
    assert t.size > 50 and (np.abs(t) < 2.0 ** -14 * 2).all()


def test_adam_reference_is_torch_adam_in_float64():
    b1, b2 = float(np.float32(st.BETA1)), float(np.float32(st.BETA2))
    for wd in st.WDS:
        wd64 = float(np.float32(wd))
        case = st.adam_case(1024, wd)
        p = torch.tensor(case["p"].astype(np.float64), requires_grad=True)
        opt = torch.optim.Adam([p], lr=float(np.float32(st.LR)), betas=(b1, b2),
                               eps=float(np.float32(st.EPS)), weight_decay=wd64)
        m, v = np.zeros(1024), np.zeros(1024)
        cur = case["p"].astype(np.float64)
        rng = np.random.RandomState(5)
        for step in range(1, 5):
            g = case["g"].astype(np.float64) * rng.rand(1024)
            p.grad = torch.tensor(g)
            opt.step()
            r = st.adam_ref(cur, g, m, v, step, wd)
            cur, m, v = r["P"], r["M"], r["V"]
            np.testing.assert_allclose(p.detach().numpy(), cur, rtol=1e-12, atol=1e-300)
            state = opt.state[p]
            np.testing.assert_allclose(state["exp_avg"].numpy(), m, rtol=1e-13, atol=1e-300)
            np.testing.assert_allclose(state["exp_avg_sq"].numpy(), v, rtol=1e-13, atol=1e-300)


def test_adam_measured_K():
    """K >= 4 x the largest ratio of the f32 restatement (module docstring), a power of two, over the
    small sizes and over the TILE-element draws that every larger case repeats: all the elements a
    GPU test sees.  Prints the figures the module docstring and NOTES.md quote."""
    worst = {}
    for label, sizes in (("small sizes", st.SMALL_SIZES), ("TILE draw", (st.TILE,))):
        w = dict(m=-np.inf, v=-np.inf, p=-np.inf)
        for n in sizes:
            for wd in st.WDS:
                case = st.adam_case(n, wd)
                for step in st.STEPS:
                    r = st.adam_measure(case, step, wd, st.adam_f32(case, step, wd))
                    for k in w:
                        w[k] = max(w[k], r[k])
        print("  [step-tail] adam restatement, %s: largest ratio m %.3f  v %.3f  p %.3f (K_V = %g)" % (
            label, w["m"], w["v"], w["p"], st.K_V))
        for k in w:
            worst[k] = max(worst.get(k, -np.inf), w[k])
    assert min(worst.values()) > 0
    for k, K in (("m", st.K_M), ("v", st.K_V), ("p", st.K_P)):
        assert K >= 4.0 * worst[k] and math.log2(K) == int(math.log2(K)), (k, K, worst[k])
        assert K <= 2 * _pow2_of_4x(worst[k]), (k, K, worst[k])          # ... and no looser than it has to be


@pytest.mark.parametrize("n,wd", SMALL)
def test_adam_assertions_accept_the_f32_restatement(n, wd):
    case = st.adam_case(n, wd)
    for step in st.STEPS:
        got = st.adam_f32(case, step, wd)
        plain = dict(got, shadow=None)
        fails, worst = st.adam_failures(case, step, wd, got, plain)
        st.assert_none(fails, "n=%d wd=%g step=%d" % (n, wd, step))
        # K = 4 x measured, at the least (p's bound also holds the denominator interval, which no K scales)
        assert max(worst["m"], worst["v"], worst["p_update"]) <= 0.25 + 1e-9 and worst["p"] <= 1.0
    # the assertions themselves: a touched guard, a run that depends on the shadow pointer
    got = st.adam_f32(case, 1, wd)
    for name in ("p", "m", "v", "shadow"):
        bad = {k: a.copy() for k, a in got.items()}
        bad[name][n + 63] = 0
        assert any(f[2].startswith("guard") and f[1] == name for f in st.adam_failures(case, 1, wd, bad)[0])
    plain = {k: a.copy() for k, a in got.items()}
    plain["v"][n - 1] = np.nextafter(plain["v"][n - 1], np.float32(1))
    assert any("without a shadow" in f[2] for f in st.adam_failures(case, 1, wd, got, plain)[0])


@pytest.mark.parametrize("mutant", [m for m in st.ADAM_MUTANTS if not m.startswith("pass_")])
def test_adam_mutants_are_rejected(mutant):
    named = 0
    for n, wd in SMALL:
        case = st.adam_case(n, wd)
        for step in st.STEPS:
            if not st.adam_mutant_applies(mutant, n, step, wd):
                continue
            named += 1
            fails, _ = st.adam_failures(case, step, wd, st.adam_mutant(case, step, wd, mutant))
            assert fails, (mutant, n, wd, step)
            if mutant.startswith("shadow_"):               # the shadow alone is wrong
                assert {f[1] for f in fails} == {"shadow"}
    assert named >= 15, (mutant, named)


def test_adam_tail_skipped_shows_in_p_m_v_alone():
    """without a shadow pointer nothing but the bounds of p, m, v can catch a skipped tail: they do,
    wherever the tail holds an element that a step moves"""
    named = 0
    for n, wd in SMALL:
        case = st.adam_case(n, wd)
        tail = slice(n - n % st.ADAM_VEC, n)
        if not st.adam_mutant_applies("tail_skipped", n, 1, wd) or not st.adam_is_live(case, wd, tail).any():
            continue
        for step in st.STEPS:
            named += 1
            fails, _ = st.adam_failures(case, step, wd, st.adam_mutant(case, step, wd, "tail_skipped", shadow=False))
            assert fails and {f[1] for f in fails} <= {"p", "m", "v"}, (n, wd, step)
            assert min(f[0] for f in fails) >= tail.start
    assert named >= 60, named


def test_adam_pass_mutants_are_rejected_past_P():
    n = st.P + 5
    step, wd = st.BIG_PAIRS[n]
    case = st.adam_case(n, wd)
    good = st.adam_f32(case, step, wd)
    st.assert_none(st.adam_failures(case, step, wd, good)[0], "P + 5")
    assert st.adam_is_live(case, wd, slice(st.P, n)).any()
    for mutant in ("pass_dropped", "pass_twice"):
        assert st.adam_mutant_applies(mutant, n, step, wd) and not st.adam_mutant_applies(mutant, st.P, step, wd)
        for shadow in (True, False):       # without a shadow: through the bounds of p, m, v alone
            fails, _ = st.adam_failures(case, step, wd, st.adam_mutant(case, step, wd, mutant, shadow=shadow))
            assert fails and min(f[0] for f in fails) >= st.P, mutant
            if not shadow:
                assert {f[1] for f in fails} <= {"p", "m", "v"}


def test_the_rare_shadow_mutants_show_at_a_small_size():
    """shadow_truncated and shadow_single_rounding differ from the truth on few elements: n = 1023
    holds some of each (the second through the nudged ties, with wd = 0)."""
    case = st.adam_case(1023, 0.0)
    truth = st.adam_f32(case, 1, 0.0)["shadow"]
    for mutant, least in (("shadow_truncated", 100), ("shadow_single_rounding", 5)):
        differs = st.adam_mutant(case, 1, 0.0, mutant)["shadow"] != truth
        print("  [step-tail] %s differs on %d of 1023 elements" % (mutant, differs.sum()))
        assert differs.sum() >= least
        if mutant == "shadow_single_rounding":
            assert (case["cat"][differs[:1023]] == 17).sum() >= 5            # the nudged ties


def test_adam_argument_validation_without_gpu(capi):
    """every call here is refused, or has n == 0: nothing is launched"""
    fn = capi.lib().cdll.f2n_adam_step
    ok = 0x1000
    rest = (1e-2, 0.9, 0.99, 1e-15, 0.0)
    call = lambda p, g, m, v, h, n, step: fn(p, g, m, v, h, n, *rest, step, None)
    for i in range(4):                                          # param, grad, exp_avg, exp_avg_sq
        ptrs = [ok] * 4
        ptrs[i] = ok + 4
        assert call(*ptrs, ok, 8, 1) == -1, i
        ptrs[i] = None
        assert call(*ptrs, ok, 8, 1) == -1, i
    assert call(ok, ok, ok, ok, ok + 2, 8, 1) == -1             # shadow off by one f16
    assert call(ok, ok, ok, ok, ok, 8, 0) == -1                 # step < 1
    assert call(ok, ok, ok, ok, None, 8, -3) == -1
    assert call(ok, ok, ok, ok, ok, -1, 1) == -1                # n < 0
    assert call(ok, ok, ok, ok, ok, 0, 1) == 0                  # nothing to do
    assert call(ok, ok, ok, ok, None, 0, 1) == 0


# ---- loss -----------------------------------------------------------------------------------------

LOSS_CASES = [(n, kind) for n in st.LOSS_SIZES for kind in st.LOSS_KINDS]


def test_loss_inputs_are_what_the_docstring_says():
    case = st.loss_case(70001, "mixed")
    e = np.abs(case["colors"].astype(np.float64) - case["gt"])
    assert (e == 0).mean() > 0.2 and ((e > 0.5e-6) & (e < 2e-6)).mean() > 0.2
    assert ((e > 0.9e-3) & (e < 1.1e-3)).mean() > 0.2 and (e > 0.1).mean() > 0.15
    v = case["var"]
    assert (v == 0).mean() > 0.25 and (v == np.float32(1e-6)).mean() > 0.25 and (v > 0.1).mean() > 0.25
    assert (st.loss_case(257, "zero")["colors"] == st.loss_case(257, "zero")["gt"]).all()
    # the finish kernel's loop edge: 255, 256, 257 partials
    assert [-(-n // st.LOSS_BLOCK) for n in (65280, 65536, 65537)] == [255, 256, 257]


def test_loss_reference_is_autograd_in_float64():
    for n, w in ((257, 0.3), (1, 0.0), (70001, 1e-2)):
        case = st.loss_case(n, "mixed")
        ref = st.loss_ref(n, "mixed", w)
        c = torch.tensor(case["colors"].astype(np.float64), requires_grad=True)
        var = torch.tensor(case["var"].astype(np.float64), requires_grad=True)
        err = c - torch.tensor(case["gt"].astype(np.float64))
        fc, fv = float(np.float32(1e-4)), float(np.float32(1e-2))
        color_loss = torch.sqrt(err.square() + fc).mean()
        var_loss = torch.sqrt(var + fv).mean()
        loss = color_loss + float(np.float32(w)) * var_loss
        loss.backward()
        want = [loss.item(), color_loss.item(), var_loss.item(), err.square().sum().item()]
        np.testing.assert_allclose(ref["out4"], want, rtol=1e-12)
        np.testing.assert_allclose(ref["d_colors"], c.grad.numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(ref["d_var"], var.grad.numpy(), rtol=1e-12, atol=0)


def test_loss_measured_K():
    worst = dict(d_colors=-np.inf, d_var=-np.inf, sums=-np.inf)
    for n, kind in LOSS_CASES:
        case = st.loss_case(n, kind)
        for w in st.LOSS_WEIGHTS:
            ref, got = st.loss_ref(n, kind, w), st.loss_f32(case, w)
            for name in ("d_colors", "d_var"):
                e = np.abs(got[name].astype(np.float64) - ref[name])
                worst[name] = max(worst[name], float(st.safe_ratio(e, st.U * np.abs(ref[name])).max()))
            e = np.abs(got["out4"].astype(np.float64) - ref["out4"])
            worst["sums"] = max(worst["sums"], float(
                st.safe_ratio(e - ref["any_order"], st.U * np.abs(ref["out4"])).max()))
    print("  [step-tail] loss restatement: largest err/(u |value|): d_colors %.3f  d_var %.3f; "
          "sums (err - n u sum|x|)/(u |result|) %.3f" % (worst["d_colors"], worst["d_var"], worst["sums"]))
    assert st.K_LOSS == _pow2_of_4x(max(worst.values())), worst


@pytest.mark.parametrize("n,kind", LOSS_CASES)
def test_loss_assertions_accept_the_f32_restatement(n, kind):
    case = st.loss_case(n, kind)
    for w in st.LOSS_WEIGHTS:
        fails, _ = st.loss_failures(case, st.loss_ref(n, kind, w), st.loss_f32(case, w))
        st.assert_none(fails, "n=%d %s w=%g" % (n, kind, w))
    # a NaN colour, through the same restatement
    poisoned = {k: a.copy() for k, a in case.items()}
    ray = n // 2
    poisoned["colors"][ray, 1] = np.nan
    got = st.loss_f32(poisoned, 0.3)
    assert not st.loss_nan_failures(got, ray, 1)
    if n > 1:
        got["d_colors"][(ray + 1) % n, 0] = np.nan
        assert st.loss_nan_failures(got, ray, 1)


@pytest.mark.parametrize("mutant", st.LOSS_MUTANTS)
def test_loss_mutants_are_rejected(mutant):
    named = 0
    for n, kind in LOSS_CASES:
        case = st.loss_case(n, kind)
        for w in st.LOSS_WEIGHTS:
            if st.loss_mutant_applies(mutant, n, w, kind):
                named += 1
                fails, _ = st.loss_failures(case, st.loss_ref(n, kind, w), st.loss_mutant(case, w, mutant))
                assert fails, (mutant, n, kind, w)
    assert named >= 6, (mutant, named)
    # the loop edge itself: 257 partials, the last one holding a single ray
    if mutant == "partials_past_256_dropped":
        assert st.loss_mutant_applies(mutant, 65537, 0.0, "spike")
        assert not st.loss_mutant_applies(mutant, 65536, 0.0, "spike")


# ---- embedding gradient ---------------------------------------------------------------------------

SCATTER_CASES = [(n, C) for n in st.SCATTER_N for C in st.SCATTER_C]


def test_scatter_layout_is_what_the_docstring_says():
    facts = st.scatter_layout_facts(3000)
    starts, ends, lengths = facts["starts"], facts["ends"], facts["lengths"]
    assert {1, 63, 64, 65, 200} <= set(lengths.tolist())
    for ln in (1, 63, 64, 65, 200):
        at = lengths == ln
        if ln != 1:           # starts on an edge, ends on an edge (a run of one does both or neither)
            assert (starts[at] % st.K_SPAN == 0).any() or (ends[at] % st.K_SPAN == 0).any(), ln
    assert (starts[lengths == 1] % st.K_SPAN == 0).any()
    crossing = (starts // st.K_SPAN) != ((ends - 1) // st.K_SPAN)
    assert crossing[lengths == 65].any() and crossing[lengths == 200].all() and crossing[lengths == 63].any()
    ids = st.scatter_ids(3000)
    assert (ids == -1).sum() > 0 and (ids == st.SCATTER_E).sum() > 0
    named = set(ids.tolist())
    assert not named & set(st.SCATTER_UNNAMED) and named >= {0, 1, 2, 4, 5, 7}
    for n, C in SCATTER_CASES:
        case = st.scatter_case(n, C)
        k = case["k"]
        assert np.abs(k).max() <= 4096 and case["dsum"].dtype == np.float32
        ref = st.scatter_ref(case)
        assert not np.signbit(ref[list(st.SCATTER_UNNAMED)]).any() and (ref[list(st.SCATTER_UNNAMED)] == 0).all()
        # against a plain float64 loop
        want = np.zeros((st.SCATTER_E, C))
        for i, e in enumerate(case["ids"]):
            if 0 <= e < st.SCATTER_E:
                want[e] += case["dsum"][i].astype(np.float64)
        assert (ref.astype(np.float64) == want).all()


@pytest.mark.parametrize("n,C", SCATTER_CASES)
def test_scatter_assertions_accept_any_order_and_reject_mutants(n, C):
    case = st.scatter_case(n, C)
    # f32 sums in two orders: exact either way
    for order in (np.arange(n), np.random.RandomState(n + C).permutation(n)):
        acc = np.zeros((st.SCATTER_E, C), dtype=np.float32)
        for i in order:
            e = case["ids"][i]
            if 0 <= e < st.SCATTER_E:
                acc[e] = acc[e] + case["dsum"][i]
        assert not st.scatter_failures(case, st.with_guard(acc.ravel()))
    for mutant in st.SCATTER_MUTANTS:
        fails = st.scatter_failures(case, st.scatter_mutant(case, mutant))
        if st.scatter_mutant_applies(mutant, n, C):
            assert fails, (mutant, n, C)
    good = st.with_guard(st.scatter_ref(case).ravel())
    good[-1] = 0.0
    assert any("guard" in f[2] for f in st.scatter_failures(case, good))
    neg = st.with_guard(st.scatter_ref(case).ravel())
    neg[st.SCATTER_UNNAMED[0] * C] = -0.0
    assert any("not +0" in f[2] for f in st.scatter_failures(case, neg))
