"""tests/supervision_model.py checked on the CPU: the Philox4x32-10 known-answer vector, the masked
draw's invariants and the number of rays that miss for the seeds the GPU tests use, the pack, and the
loss model's gradients (finite differences), its agreement with loss.hip's formula and the W = 0 case."""
import numpy as np
import pytest

from tests import supervision_model as sm


def test_philox_known_answer():
    """Random123's kat_vectors entry for philox4x32 10: counter 0, key 0"""
    want = (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert sm.philox_scalar((0, 0, 0, 0), (0, 0)) == want
    got = sm.philox4x32_10(np.zeros(3), 0, 0, 0, 0, 0)
    assert tuple(int(x[1]) for x in got) == want


def test_philox_vectorised_is_the_scalar_one():
    rng = np.random.RandomState(3)
    c = rng.randint(0, 1 << 32, size=(4, 50), dtype=np.uint64)
    k0, k1 = 0x9C3B7D11, 0x5EED0F2A
    got = sm.philox4x32_10(c[0], c[1], c[2], c[3], k0, k1)
    for n in range(50):
        assert tuple(int(x[n]) for x in got) == sm.philox_scalar(c[:, n], (k0, k1))
    # all-ones counter and key: the multipliers and the Weyl constants wrap
    ones = 0xFFFFFFFF
    got = sm.philox4x32_10(np.array([ones]), ones, ones, ones, ones, ones)
    assert tuple(int(x[0]) for x in got) == sm.philox_scalar((ones,) * 4, (ones, ones))
    assert all(0 <= int(x[0]) <= ones for x in got)


def test_pack_bits_and_tail():
    for name in sm.MASKS:
        m = sm.mask(name)
        words, count = sm.pack(m)
        assert words.dtype == np.uint32 and words.shape == ((sm.E * sm.H * sm.W + 31) // 32,)
        flat = m.reshape(-1) != 0
        assert count == int(flat.sum())
        for g in range(flat.shape[0]):
            assert bool((int(words[g >> 5]) >> (g & 31)) & 1) == bool(flat[g])
        used = flat.shape[0] & 31
        assert used != 0 and int(words[-1]) >> used == 0            # unused bits of the last word
    assert sm.pack(sm.mask("one_pixel"))[1] == 1


def test_half_valid_mask_keeps_only_valid_pixels():
    rng = np.random.RandomState(11)
    m = (rng.rand(4, 33, 47) < 0.5).astype(np.uint8)
    cam, ij, tries = sm.draw(m, 1 << 16, 0xABCDEF0123456789, 32)
    kept = tries > 0
    assert kept.sum() >= (1 << 16) - 2            # 2^16 rays, 2^-32 each to miss 32 times
    assert m[cam[kept], ij[kept, 0], ij[kept, 1]].all()
    assert (m[cam[~kept], ij[~kept, 0], ij[~kept, 1]] == 0).all()
    assert 0 <= cam.min() and cam.max() < 4 and ij[:, 0].max() < 33 and ij[:, 1].max() < 47
    # the attempts are geometric: about half the rays need one, a quarter two
    assert abs((tries == 1).mean() - 0.5) < 0.02 and abs((tries == 2).mean() - 0.25) < 0.02
    # uniform over the valid pixels: every camera gets its share of them
    share = np.array([m[e].sum() for e in range(4)]) / m.sum()
    got = np.bincount(cam[kept], minlength=4) / kept.sum()
    assert np.abs(got - share).max() < 0.01


def test_all_ones_mask_takes_one_attempt():
    for n in sm.DRAW_N:
        for A in sm.DRAW_A:
            assert (sm.shared_draw("ones", n, A)[2] == 1).all()


# rays with tries == 0 in the model's draw for (mask, n, A) of tests/test_gpu_pixel_mask.py, seed
# DRAW_SEED; test_misses_of_the_gpu_cases recomputes them with the scalar generator
def _scalar_misses(name, n, A):
    m = sm.mask(name)
    lo, hi = sm.DRAW_SEED & sm.MASK32, sm.DRAW_SEED >> 32
    miss = 0
    for r in range(n):
        for a in range(A):
            x = sm.philox_scalar((r, a, 0, 0), (lo, hi))
            c, i, j = (x[0] * sm.E) >> 32, (x[1] * sm.H) >> 32, (x[2] * sm.W) >> 32
            if m[c, i, j]:
                break
        else:
            miss += 1
    return miss


@pytest.mark.parametrize("name", sm.MASKS)
def test_misses_of_the_gpu_cases(name):
    for n in sm.DRAW_N:
        for A in sm.DRAW_A:
            cam, ij, tries = sm.shared_draw(name, n, A)
            misses = int((tries == 0).sum())
            assert misses == _scalar_misses(name, n, A), (name, n, A)
            assert ((tries >= 0) & (tries <= A)).all()
            if name == "ones":
                assert misses == 0
            if name == "one_pixel":
                # the miss branch is exercised at every size, the hit branch where 257 x 32 draws
                # meet a 1 / 1050 target
                assert misses >= 1
                if (n, A) == (257, 32):
                    assert 0 < misses < n
                kept = tries > 0
                assert (cam[kept] == sm.ONE_PIXEL[0]).all()
                assert (ij[kept] == np.array(sm.ONE_PIXEL[1:])).all()
            if name == "image1_off":
                assert (cam[tries > 0] != 1).all()
            if A == 1 and name == "checker" and n == 257:
                assert 0 < misses < n             # about half


@pytest.mark.parametrize("weight_kind", sm.WEIGHT_KINDS)
@pytest.mark.parametrize("with_alpha", [False, True])
def test_loss_gradients_by_finite_differences(weight_kind, with_alpha):
    n = 9
    case = sm.loss_case(n, weight_kind, with_alpha)
    vw, ow = sm.VAR_WEIGHT, sm.OPACITY_WEIGHT
    ref = sm.loss_ref(case, vw, ow, True)
    base = {k: case[k].astype(np.float64) for k in ("colors", "var", "opacity")}
    on = ~ref["masked"]
    h = 1e-6

    def fd(name, idx):
        hi, lo = ({k: v.copy() for k, v in base.items()} for _ in range(2))
        hi[name][idx] += h
        lo[name][idx] -= h
        return (sm.loss_value(hi["colors"], hi["var"], hi["opacity"], case, vw, ow, True) -
                sm.loss_value(lo["colors"], lo["var"], lo["opacity"], case, vw, ow, True)) / (2 * h)

    for r in range(n):
        for c in range(3):
            want = ref["d_colors"][r, c]
            if on[r]:
                assert abs(fd("colors", (r, c)) - want) < 1e-6 * max(1.0, abs(want)) + 1e-8
            else:
                assert want == 0.0
        if on[r]:
            assert abs(fd("var", r) - ref["d_var"][r]) < 1e-7
            if with_alpha:
                assert abs(fd("opacity", r) - ref["d_opacity"][r]) < 1e-7
        else:
            assert ref["d_var"][r] == 0.0
    assert (ref["d_opacity"] is not None) == with_alpha


@pytest.mark.parametrize("n", sm.LOSS_SIZES)
def test_no_weight_no_alpha_is_the_plain_loss(n):
    case = sm.loss_case(n, None, False)
    ref = sm.loss_ref(case, sm.VAR_WEIGHT, sm.OPACITY_WEIGHT, False)
    plain = sm.plain_loss(case["colors"], case["gt"], case["var"], sm.VAR_WEIGHT)
    np.testing.assert_allclose(ref["out"][[0, 1, 2, 4]], plain, rtol=1e-13, atol=0)
    assert ref["out"][3] == 0.0 and ref["out"][5] == n
    # ... and so with every weight exactly 1
    ones = dict(case)
    ones["ray_weight"] = np.ones(n, dtype=np.float32)
    again = sm.loss_ref(ones, sm.VAR_WEIGHT, sm.OPACITY_WEIGHT, False)
    assert np.array_equal(again["out"], ref["out"]) and np.array_equal(again["d_colors"], ref["d_colors"])


@pytest.mark.parametrize("n", sm.LOSS_SIZES)
@pytest.mark.parametrize("with_alpha", [False, True])
def test_all_weights_zero(n, with_alpha):
    ref = sm.loss_ref(sm.loss_case(n, "allzero", with_alpha), sm.VAR_WEIGHT, sm.OPACITY_WEIGHT, True)
    assert (ref["out"] == 0.0).all()
    assert not ref["d_colors"].any() and not ref["d_var"].any()
    assert ref["d_opacity"] is None or not ref["d_opacity"].any()
    assert (ref["tol_out"] == 0).all()


def test_bounds_are_tight_enough_to_mean_something():
    """the bound of every output is a few hundred u of its scale at most: a dropped term, a wrong
    divisor or a missing weight is orders of magnitude outside"""
    for n in sm.LOSS_SIZES:
        ref = sm.loss_ref(sm.loss_case(n, "mixed", True), sm.VAR_WEIGHT, sm.OPACITY_WEIGHT, True)
        if ref["out"][5] == 0:
            continue
        assert ref["tol_out"][0] < 200 * sm.U * abs(ref["out"][0])
        assert (ref["tol_d_var"] <= 40 * sm.U * np.abs(ref["d_var"])).all()
        assert (ref["tol_d_opacity"] <= 40 * sm.U * np.abs(ref["d_opacity"])).all()
        assert (ref["tol_d_colors"] <= 40 * sm.U * (np.abs(ref["d_colors"]) + 4.0 / ref["out"][5])).all()
