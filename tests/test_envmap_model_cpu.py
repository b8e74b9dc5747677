"""The model of the learned background (tests/envmap_model.py) checked against itself: finite
differences of the float64 forward, the weights, every tie rule of the face choice, the zero texture,
degenerate rays, the integer backward against plain float64 sums, and the fit constant."""
import numpy as np
import pytest

from tests import envmap_model as em

F32 = np.float32


def _tex(R, seed, scale=2.0):
    return (np.random.RandomState(seed).randn(6, R, R, 3) * scale).astype(F32)


@pytest.mark.parametrize("R", [2, 5, 64])
def test_weights_sum_to_one_and_are_non_negative(R):
    d = np.concatenate([em.special_dirs(), em.random_dirs(400, R)])
    geo = em.geometry(d, R)
    assert geo["live"].all()
    w = geo["w"]
    assert (w >= 0).all() and (w <= 1).all()
    total = ((w[:, 0] + w[:, 1]).astype(F32) + (w[:, 2] + w[:, 3]).astype(F32)).astype(F32)
    assert np.abs(total.astype(np.float64) - 1.0).max() <= 2 * 2.0 ** -23       # 2 ulp of 1
    assert (geo["fx"] >= 0).all() and (geo["fx"] < 1).all() and (geo["fy"] >= 0).all() and (geo["fy"] < 1).all()


def test_tie_rules():
    """x before y before z on equal magnitudes; the sign of the winning component picks the face;
    -0.0 is not negative"""
    R = 4
    face = lambda v: int(em.geometry(np.array([v], dtype=F32), R)["face"][0])
    assert [face(v) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))] == list(range(6))
    for x in (1.0, -1.0):
        for y in (1.0, -1.0):
            for z in (1.0, -1.0):
                assert face((x, y, z)) == (0 if x > 0 else 1)             # corner: x wins
            assert face((x, y, 0.0)) == (0 if x > 0 else 1)               # edge x = y: x wins
            assert face((0.0, x, y)) == (2 if x > 0 else 3)               # edge y = z: y wins
            assert face((x, 0.0, y)) == (0 if x > 0 else 1)               # edge x = z: x wins
            assert face((x, -0.0, y * 0.5)) == (0 if x > 0 else 1)
    # scaling by a power of ten that keeps float32 finite changes nothing but rounding of the inputs
    d = np.array([(1, 1, 1), (-1, 0.5, 0.25), (0.25, -1, 1)], dtype=F32)
    for scale in (1e-20, 1e20):
        a, b = em.geometry(d, R), em.geometry(d * F32(scale), R)
        assert (a["face"] == b["face"]).all() and (a["idx"] == b["idx"]).all()
    # an axis direction looks up the middle of its face, a corner direction its corner texel
    g = em.geometry(np.array([(0, 0, 1), (1, 1, 1), (-1, -1, -1)], dtype=F32), R)
    assert np.allclose(g["w"][0], 0.25) and set(g["idx"][0]) == {4 * 16 + 5, 4 * 16 + 6, 4 * 16 + 9, 4 * 16 + 10}
    assert g["idx"][1, 0] == 0 * 16 + 3 * 4 + 3 and g["w"][1, 0] == 1
    assert g["idx"][2, 0] == 1 * 16 + 0 and g["w"][2, 0] == 1


def test_zero_texture_is_exactly_half_and_degenerate_rays():
    R = 5
    d = np.concatenate([em.special_dirs(), em.degenerate_dirs()])
    bg, tol = em.forward(d, np.zeros((6, R, R, 3), F32), R)
    assert (bg == 0.5).all()
    dead = em.degenerate_dirs()
    geo = em.geometry(dead, R)
    assert not geo["live"].any() and (geo["w"] == 0).all()
    bg, tol = em.forward(dead, _tex(R, 1), R)
    assert (bg == 0.5).all() and (tol == 0).all()
    acc, flags = em.backward(dead, bg.astype(F32), np.full((len(dead), 3), np.inf, F32), R)
    assert flags == 0 and not any(acc)                                   # no gradient, no flag


@pytest.mark.parametrize("R", [2, 5])
def test_finite_differences_of_the_forward(R):
    """d (sum G bg) / d tex from backward_float64 against central differences of forward()"""
    rng = np.random.RandomState(R)
    d = np.concatenate([em.special_dirs(), em.random_dirs(64, 7)])
    tex = _tex(R, 3, 1.0)
    G = rng.randn(len(d), 3)
    geo = em.geometry(d, R)
    bg, _ = em.forward(d, tex, R, geo)
    grad = em.backward_float64(d, bg, G, R, geo)
    h = 2.0 ** -10
    flat = tex.reshape(-1).astype(np.float64)
    f = lambda t: float((G * em.forward(d, t.astype(F32), R, geo)[0]).sum())
    worst = 0.0
    for e in rng.choice(flat.size, 40, replace=False):
        up, dn = flat.copy(), flat.copy()
        up[e] += h
        dn[e] -= h
        fd = (f(up) - f(dn)) / (2 * h)
        worst = max(worst, abs(fd - grad[e]) / (abs(grad[e]) + 1e-3))
    assert worst <= 1e-5, worst


@pytest.mark.parametrize("n", [1, 63, 257])
def test_integer_backward_against_float64(n):
    R = 5
    d = em.random_dirs(n, n)
    tex = _tex(R, 9)
    bg = em.forward(d, tex, R)[0].astype(F32)
    g = (np.random.RandomState(n).randn(n, 3) * 300).clip(-1e3, 1e3).astype(F32)
    g[::3] = 0
    acc, flags = em.backward(d, bg, g, R)
    assert flags == 0
    got = em.apply(acc).astype(np.float64)
    want = em.backward_float64(d, bg, g, R)
    # three float32 roundings in gl (relative 3 u on each contribution), half a quantum per
    # contribution, one rounding of the sum to float32; 5 u leaves room for the second-order terms
    mag = em.backward_float64(d, bg, np.abs(g), R)
    assert (np.abs(got - want) <= 5 * em.U * mag + 4 * n * 2.0 ** -49 + 2.0 ** -149).all()
    # accumulate: the previous gradient plus this one, rounded once
    prev = np.random.RandomState(1).randn(acc.size).astype(F32)
    assert (em.apply(acc, prev) == (prev + em.apply(acc)).astype(F32)).all()
    assert (em.acc_int64(acc) == np.array([int(a) for a in acc])).all()


def test_flags_and_cap():
    R = 5
    d = em.random_dirs(8, 2)
    bg = np.full((8, 3), 0.5, F32)
    g = np.zeros((8, 3), F32)
    g[1, 0] = 3.0
    g[2, 1] = np.inf
    acc, flags = em.backward(d, bg, g, R)
    assert flags == 1
    g[2, 1] = np.nan
    assert em.backward(d, bg, g, R)[1] == 1
    g[2, 1] = 1e30                                    # finite, far beyond the cap
    acc2, flags2 = em.backward(d, bg, g, R)
    assert flags2 == 2 and max(abs(int(a)) for a in acc2) == em.CAP
    g[3, 2] = -np.inf
    assert em.backward(d, bg, g, R)[1] == 3
    # the finite ray is summed exactly in every case
    geo = em.geometry(d, R)
    e = geo["idx"][1] * 3
    alone = em.backward(d[1:2], bg[1:2], g[1:2], R)[0]
    assert all(int(acc[i]) == int(alone[i]) == int(acc2[i]) for i in e) and any(int(acc[i]) for i in e)


def test_fit_constant():
    """the committed constant is what fit() gives on the CPU oracle's scene"""
    dirs, A, T = em.fit_scene_cpu()
    assert len(set(em.geometry(dirs, em.FIT_R)["face"])) == 6             # the batch covers every face
    final, first = em.fit(dirs, A, T)
    assert first > 50 * final
    assert final == pytest.approx(em.FIT_MODEL_MAE, rel=1e-3)
