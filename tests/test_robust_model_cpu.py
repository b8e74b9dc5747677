"""The numpy model of the robust weights (tests/robust_model.py) against the properties the rule is
meant to have.  No GPU: tests/test_gpu_robust_weights.py holds the kernels to this model."""
import numpy as np

from tests import robust_model as M

F32 = np.float32


def _batch(eps):
    """colours (e, 0, 0) against a zero target: the residual of ray r is e_r * e_r"""
    e = np.asarray(eps, dtype=F32)
    colors = np.zeros((e.size, 3), dtype=F32)
    colors[:, 0] = e
    return colors, np.zeros_like(colors)


def test_quantile_one_gives_all_ones():
    g = np.random.default_rng(1)
    colors, target = g.random((512, 3), dtype=F32), g.random((512, 3), dtype=F32)
    for P in (0, 16):
        out = M.robust_weights(colors, target, None, P=P, quantile=1.0)
        assert out["omega"].all() and np.array_equal(out["weight"], np.ones(512, dtype=F32))
        assert out["k"] == 512 and out["T"] == out["eps"].max()
        assert np.array_equal(out["stats"], np.array([out["T"], 512, 512, 512], dtype=F32))


def test_labels_are_monotone_in_the_quantile():
    g = np.random.default_rng(2)
    colors, target = g.random((3 * 169, 3), dtype=F32), g.random((3 * 169, 3), dtype=F32)
    m = (g.random(3 * 169) > 0.1).astype(F32)
    for P, nbhd in ((0, 8), (13, 8), (13, 1), (13, 13)):
        before = np.zeros(3 * 169, dtype=bool)
        before0 = before.copy()
        for q in (0.01, 0.1, 0.25, 0.5, 0.6, 0.75, 0.9, 1.0):
            out = M.robust_weights(colors, target, m, P=P, nbhd=nbhd, quantile=q)
            now = out["omega"].astype(bool)
            assert not (before & ~now).any() and not (before0 & ~out["w0"]).any(), (P, nbhd, q)
            before, before0 = now, out["w0"]
        assert np.array_equal(before, m != 0)


def test_isolated_outliers_are_restored_by_the_box():
    """16 x 16, small residuals except single pixels at most one per 3 x 3 window (a lattice of period
    3), the quantile chosen so that exactly those are cut: step 5 alone brings every one back"""
    P = 16
    eps = np.full((P, P), 1e-3, dtype=F32)
    hot = np.zeros((P, P), dtype=bool)
    hot[1::3, 1::3] = True                                   # 25 pixels, never two in one window
    eps[hot] = 0.5
    colors, target = _batch(eps.reshape(-1))
    q = (P * P - hot.sum()) / (P * P)
    out = M.robust_weights(colors, target, None, P=P, quantile=q)
    assert out["k"] == P * P - hot.sum()
    assert np.array_equal(out["w0"], ~hot.reshape(-1))       # exactly those pixels are cut ...
    assert out["W"][hot.reshape(-1)].all()                   # ... and step 5 restores each of them
    assert out["omega"].all() and out["stats"][2] == P * P - 25 and out["stats"][3] == P * P
    # without patches they stay out
    flat = M.robust_weights(colors, target, None, P=0, quantile=q)
    assert np.array_equal(flat["omega"].astype(bool), ~hot.reshape(-1))


def test_a_whole_patch_distractor_stays_out():
    P = 16
    g = np.random.default_rng(4)
    eps = np.concatenate([g.random(P * P) * 1e-3, 0.5 + g.random(P * P) * 0.1]).astype(F32)
    colors, target = _batch(eps)
    out = M.robust_weights(colors, target, None, P=P, **M.DEFAULTS)
    assert out["omega"][:P * P].all() and not out["omega"][P * P:].any()
    assert np.array_equal(out["weight"], np.repeat(np.array([1, 0], dtype=F32), P * P))


def test_ties_at_the_threshold_are_all_inliers():
    eps = np.array([1, 2, 2, 2, 2, 3, 3, 4], dtype=F32)
    colors, target = _batch(eps)
    out = M.robust_weights(colors, target, None, quantile=0.25)      # k = 2: T is the first 2
    assert out["k"] == 2 and out["T"] == F32(4)                     # (residual = eps^2)
    assert np.array_equal(out["omega"], np.array([1, 1, 1, 1, 1, 0, 0, 0], dtype=np.uint8))
    assert out["stats"][2] == 5


def test_all_masked_gives_zeros():
    g = np.random.default_rng(6)
    colors, target = g.random((2 * 121, 3), dtype=F32), g.random((2 * 121, 3), dtype=F32)
    colors[5] = np.nan
    for P in (0, 11):
        out = M.robust_weights(colors, target, np.zeros(2 * 121, dtype=F32), P=P)
        assert not out["omega"].any() and not out["weight"].any()
        assert np.array_equal(out["stats"], np.zeros(4, dtype=F32))
        assert not np.signbit(out["weight"]).any()


def test_non_finite_residuals_are_outliers_and_masked_rays_are_not_read():
    colors = np.array([[0.1, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [3e19, 3e19, 0], [0.2, 0, 0],
                       [np.nan, np.nan, np.nan]], dtype=F32)
    m = np.array([1, 1, 1, 1, 1, 0], dtype=F32)
    out = M.robust_weights(colors, np.zeros_like(colors), m, quantile=1.0)
    assert out["n_c"] == 5 and out["k"] == 5 and np.isinf(out["T"])
    assert np.array_equal(out["omega"], np.array([1, 0, 0, 0, 1, 0], dtype=np.uint8))
    assert np.isfinite(out["weight"]).all()


def test_rank_is_the_ceiling_clamped():
    assert M.rank(0.5, 1) == 1 and M.rank(0.5, 2) == 1 and M.rank(0.5, 3) == 2
    assert M.rank(1e-9, 1000) == 1 and M.rank(1.0, 1000) == 1000 and M.rank(0.75, 1000) == 750
    # the quantile is a float32 before it meets N_c: 0.1f > 0.1, so 0.1 * 10 rounds up to 2
    assert M.rank(0.1, 10) == 2
