"""tests/ray_walk_model.py on the CPU: the float64 restatement is the oracle's sampler, the f32
restatement lies within the model's bound, the three width forms add the same bits, the designed-stop
condition holds, and every mutant fails the assertion of tests/test_gpu_ray_walk.py it is listed with."""
import numpy as np
import pytest
import torch

from tests import ray_walk_model as M

F32 = np.float32


def _case(n_rays=37, S=129, with_noise=True, **kw):
    return M.sample_case(n_rays, S, with_noise, **kw)


def test_float64_restatement_is_get_samples_in_float64():
    """walk_f64 against oracle.ref_render.get_samples run in float64 on the same f32 inputs: the two
    are the same formula, so they agree to float64 rounding (cumsum order, the norm)."""
    from oracle import ref_render as R
    for S, with_noise in ((100, True), (129, False), (1024, True)):
        c = _case(S=S, with_noise=with_noise)
        ref = M.walk_f64(c["o"], c["d"], c["noise"], S, c["step"])
        noise = None if c["noise"] is None else torch.from_numpy(c["noise"]).double()
        pts, dirs, dt, t, bounds = R.get_samples(
            torch.from_numpy(c["o"]).double(), torch.from_numpy(c["d"]).double(), noise, S,
            float(F32(c["step"])))
        n = c["n_rays"]
        for name, got in (("pts", pts.reshape(n, S, 3)), ("dt", dt.reshape(n, S)), ("t", t.reshape(n, S)),
                          ("dirs", dirs.reshape(n, S, 3)[:, 0])):
            want = ref[name]
            scale = np.abs(want).max() + 30.0           # |o| reaches 30: dt cancels from there
            assert np.abs(got.numpy() - want).max() <= 1e-12 * scale, name
        assert bounds.dtype == torch.int32 and bounds[-1, 1] == n * S


@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("S", M.SAMPLE_S)
def test_f32_restatement_within_the_bound(S, with_noise):
    """The numpy-f32 kernel restatement passes every assertion the GPU test makes on f2n_sample_rays."""
    for n_rays in M.SAMPLE_RAYS:
        c = _case(n_rays, S, with_noise)
        got = M.walk_f32(c["o"], c["d"], c["noise"], S, c["step"])
        ref = M.walk_f64(c["o"], c["d"], c["noise"], S, c["step"])
        assert M.sample_failures(got, ref, got["t"]) == []
        worst = M.sample_ratios(got, ref)
        assert max(worst.values()) <= M.BAR
        print("S %d noise %d rays %d: worst |err| / E %s" % (
            S, with_noise, n_rays, " ".join("%s %.2f" % kv for kv in worst.items())))


def test_zero_direction_ray_is_nan_and_leaves_the_others_alone():
    c = _case(8, 65, True, zero_ray=3)
    clean = _case(8, 65, True)
    got = M.walk_f32(c["o"], c["d"], c["noise"], 65, c["step"])
    ref = M.walk_f64(c["o"], c["d"], c["noise"], 65, c["step"])
    assert M.sample_failures(got, ref, got["t"]) == []
    assert np.isnan(ref["dirs"][3]).all() and np.isnan(ref["pts"][3]).all()
    assert np.isnan(ref["dt"][3, 1:]).all() and ref["dt"][3, 0] == 0 and np.isfinite(ref["t"][3]).all()
    other = M.walk_f32(clean["o"], clean["d"], clean["noise"], 65, clean["step"])
    keep = np.arange(8) != 3
    for k in ("t", "pts", "dt", "dirs"):
        assert M.bits_equal(got[k][keep], other[k][keep]), k


@pytest.mark.parametrize("S", [1, 3, 5, 8, 11, 13, 16, 21, 27, 37, 45, 53, 59, 64, 67, 100, 129, 1024])
def test_width_forms_agree_in_bits(S):
    """RayLanes<64>, <16> and <8> spell different additions; as algebra they are the same ones, so
    numpy's IEEE f32 gives the same bits -- on lengths that end inside every half row."""
    rng = np.random.RandomState(S)
    v = (rng.random_sample((40, S)) + 0.5).astype(F32)
    want = M.incl_in_block(v, 64)
    for W in (16, 8):
        assert M.bits_equal(M.incl_in_block(v, W), want), W
        assert M.bits_equal(M.cum_noise32(v, W), M.cum_noise32(v, 64)), W
        assert M.bits_equal(M.depth32(v, W), M.depth32(v, 64)), W
    d64, E = M.depth_model(v)
    assert M.within(M.depth32(v, 64), d64, E).all()
    c64 = np.cumsum(v.astype(np.float64), 1)
    assert M.within(M.cum_noise32(v, 64), c64, M.U * M.D(np.arange(S))[None, :] * c64).all()


def test_all_lengths_end_inside_every_half_row():
    """every residue of a length modulo 64 (so every half row of every row), all three forms"""
    rng = np.random.RandomState(4)
    for S in range(1, 131):
        v = (rng.random_sample((3, S)) + 0.5).astype(F32)
        want = M.cum_noise32(v, 64)
        assert M.bits_equal(M.cum_noise32(v, 16), want) and M.bits_equal(M.cum_noise32(v, 8), want), S


# ---- designed stops ------------------------------------------------------------------------------------

_stops = {}


def _stop(S):
    if S not in _stops:
        _stops[S] = M.stop_case(S)
    return _stops[S]


@pytest.mark.parametrize("S", M.STOP_S)
def test_designed_stop_condition(S):
    """Condition, not measurement: the float64 rule keeps exactly `target` samples on every designed
    ray, no ray lies in the ambiguity band and half the crossing sample's optical depth is at least
    STOP_MARGIN bands; the ray count is odd."""
    case = _stop(S)
    cond = M.stop_condition(case)
    print("S %d: %d rays, %d in the band, worst band / half sample %.3f, %d rays with a raised crossing "
          "multiplier (largest factor %d)" % (S, case["n_rays"], int(cond["in_band"].sum()),
                                              float(cond["margin"].max()), int((case["boosted"] > 0).sum()),
                                              2 ** int(case["boosted"].max())))
    assert case["n_rays"] % 2 == 1 and case["n_rays"] % 8 != 0
    assert set(case["target"]) == set(M.stop_targets(S))
    assert np.array_equal(cond["kept"], case["target"])
    assert not cond["in_band"].any()
    assert (cond["margin"] <= 1.0 / M.STOP_MARGIN).all()
    assert np.linalg.norm(case["o"], axis=1).max() <= M.STOP_O_MAX * (1 + 1e-6)
    if S < 1024:
        assert not case["boosted"].any()        # the plain construction suffices
    # the f32 restatement of the whole chain stops there too
    got = M.walk_f32(case["o"], case["d"], case["noise"], S, case["step"])
    sec = (F32(np.exp(F32(M.STOP_B0 - M.DENSITY_SHIFT))) * got["dt"]).astype(F32)
    for W in M.WIDTHS:
        keep = np.exp(-M.depth32(sec, W).astype(np.float64)) > float(F32(M.THRESH))
        assert np.array_equal(M.kept_from_keep(keep), case["target"]), W
    # and the probe's designed sec_in
    s32 = M.stop_sec32(case)
    assert M.keep_failures(M.depth32(s32, 64), np.exp(-M.depth32(s32, 64).astype(np.float64)) > float(
        F32(M.THRESH)), s32, 64, designed=True) == []
    assert np.array_equal(M.keep_model(s32, np.zeros(s32.shape))["kept"], case["target"])


def test_random_sec_band_cap():
    for S in M.SAMPLE_S:
        sec = M.random_sec(37, S)
        d32 = M.depth32(sec, 64)
        keep = np.exp(-d32.astype(np.float64)) > float(F32(M.THRESH))
        assert M.keep_failures(d32, keep, sec, 64) == [], S


# ---- power ----------------------------------------------------------------------------------------------

def _chain_counts(case, W, mut, b0=M.STOP_B0):
    """kept counts of the march's chain in numpy f32 at W lanes to a ray, density exp(b0 - shift):
    walk_f32 -> sec = sigma dt -> depth32 -> the leading samples with exp(-depth) > THRESH"""
    keep_mut = mut if mut in M.KEEP_MUTANTS else None
    w = M.walk_f32(case["o"], case["d"], case["noise"], case["S"], case["step"], W=W,
                   mut=None if keep_mut else mut)
    sec = (F32(np.exp(F32(b0 - M.DENSITY_SHIFT))) * w["dt"]).astype(F32)
    depth = M.depth32(sec, W, keep_mut)
    return M.kept_from_keep(np.exp(-depth.astype(np.float64)) > float(F32(M.THRESH)))


def _mutant_failures(name):
    """the names of the GPU test's assertions that the mutant fails, on the committed cases"""
    failed = set()
    if name in M.SAMPLE_MUTANTS:
        for S, noise, affine in ((129, True, False), (1024, True, True), (100, False, False)):
            c = _case(37, S, noise)
            mult = M.multipliers(c["noise"], affine)
            ref = M.walk_f64(c["o"], c["d"], mult, S, c["step"])
            t32 = M.walk_f32(c["o"], c["d"], mult, S, c["step"])["t"]
            if name == "affine_twice" and not affine:
                continue
            got = M.walk_f32(c["o"], c["d"], mult, S, c["step"], mut=name)
            failed |= {f[0] for f in M.sample_failures(got, ref, t32)}
    elif name in M.WIDTH_MUTANTS:
        W = M.MUTANTS[name][1][0]
        c = _case(37, 129, True)
        base = M.walk_f32(c["o"], c["d"], c["noise"], 129, c["step"])
        got = M.walk_f32(c["o"], c["d"], c["noise"], 129, c["step"], W=W, mut=name)
        if not all(M.bits_equal(got[k], base[k]) for k in ("pts", "dt", "t")):
            failed.add("probe_bits")
        sec = M.random_sec(37, 129)
        d = M.depth32(sec, W, name)
        failed |= {f[0] for f in M.keep_failures(d, np.exp(-d.astype(np.float64)) > 1e-4, sec, W)}
        if not np.array_equal(_chain_counts(_stop(129), W, name), _stop(129)["target"]):
            failed.add("march_target")
    else:
        for sec, designed in ((M.random_sec(37, 129), False), (M.stop_sec32(_stop(129)), True)):
            for W in M.MUTANTS[name][1]:
                d = M.depth32(sec, W, name)
                keep = np.exp(-d.astype(np.float64)) > float(F32(M.THRESH))
                failed |= {f[0] for f in M.keep_failures(d, keep, sec, W, designed)}
                if designed and not np.array_equal(M.kept_from_keep(keep), _stop(129)["target"]):
                    failed.add("march_target")
    return failed


@pytest.mark.parametrize("name", sorted(M.MUTANTS))
def test_every_mutant_fails_its_named_assertion(name):
    failed = _mutant_failures(name)
    print("%s (%s): fails %s" % (name, M.MUTANTS[name][0], sorted(failed)))
    assert M.MUTANTS[name][2] in failed
    assert set(M.MUTANTS) == set(M.SAMPLE_MUTANTS + M.WIDTH_MUTANTS + M.KEEP_MUTANTS)


def test_keep_and_width_mutants_move_the_designed_march_counts():
    """The designed rays of (c): a wrong depth, or a wrong noise scan in the 16- or 8-lane form, moves
    the count of the real march on some designed ray, and (c) asks for equality."""
    for name in M.KEEP_MUTANTS + M.WIDTH_MUTANTS:
        assert "march_target" in _mutant_failures(name), name


# ---- the gap: what the old bars let through ------------------------------------------------------------

def _old_march_forgives(kept, want):
    """tests/test_gpu_fused.py::test_density_march_and_compact: counts within one sample, and
    different on at most 2 % of the rays"""
    diff = np.abs(kept.astype(np.int64) - want.astype(np.int64))
    return bool(diff.max() <= 1 and (diff != 0).mean() <= 0.02)


def _old_sample_bars(mut):
    """test_sample_rays' own assertions (its 97 rays of |o| ~ 0.3, S = 128, against the f32 oracle) on
    what f2n_sample_rays -- the 64-lane form, the only one that writes samples -- would write"""
    from oracle import ref_render as R
    g = torch.Generator().manual_seed(1)
    n, S, step = 97, 128, 4.0 / 128
    o, d = torch.randn(n, 3, generator=g) * 0.3, torch.randn(n, 3, generator=g)
    noise = torch.rand(n, S, generator=g) - 0.5 + 1.0
    pts, dirs, dt, t, _ = R.get_samples(o, d, noise, S, step)
    want = dict(pts=pts.reshape(n, S, 3).numpy(), dirs=dirs.reshape(n, S, 3).numpy()[:, 0],
                dt=dt.reshape(n, S).numpy(), t=t.reshape(n, S).numpy())
    return M.old_bar_passes(M.walk_f32(o.numpy(), d.numpy(), noise.numpy(), S, step, W=64, mut=mut), want)


def _old_count_bars(name, W):
    """the kept counts of the W-lane form at T = 1e-4 on 150 random rays (the march test's rays, a
    constant density of exp(6 - 3) standing in for its field), mutant against clean, under that
    test's forgiveness"""
    g = torch.Generator().manual_seed(2)
    n, S, step = 150, 128, 4.0 / 128
    case = dict(o=(torch.randn(n, 3, generator=g) * 0.25).numpy(), d=torch.randn(n, 3, generator=g).numpy(),
                noise=(torch.rand(n, S, generator=g) + 0.5).numpy(), S=S, step=step)
    return _old_march_forgives(_chain_counts(case, W, name, b0=6.0), _chain_counts(case, W, None, b0=6.0))


def test_old_bars_on_the_mutants():
    """The gap this closes.  A fault confined to the 16- or 8-lane form never reaches f2n_sample_rays:
    test_sample_rays' tolerances pass it whatever it is (here: the unmutated 64-lane samples pass).
    What is left is the counts.  The carry-lane mutant of keep_step, the stale ds.last and the 16-lane
    width mutant stay inside the old forgiveness (one sample on 2 % of 150 random rays) and so passed
    the old suite altogether; the two 8-lane width mutants and a dt_0 in the 8-lane form are seen by
    the counts, never as samples.  The new assertions reject every one (tests above)."""
    assert _old_sample_bars(None)
    seen = {name: _old_count_bars(name, min(M.MUTANTS[name][1]))
            for name in ("keep_carry62", "keep_last_stale", "w16_t1p", "w8_fill6", "w8_no_pc")}
    seen["dt0 (8-lane form only)"] = _old_count_bars("dt0", 8)
    for name, ok in sorted(seen.items()):
        print("old bars on %-24s samples: not observed, counts forgiven: %s" % (name, ok))
    for name in ("keep_carry62", "keep_last_stale", "w16_t1p"):
        assert seen[name], name
    # in the 64-lane form the old sampler assertions do see the sample mutants they can see
    assert not _old_sample_bars("carry62") and not _old_sample_bars("dt0")


