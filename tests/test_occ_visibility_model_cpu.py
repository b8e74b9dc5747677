"""tests/occ_visibility_model.py on the CPU: the float32 restatement against a float64 one away from the
cell faces, the dilation at the grid's border, the view counts, and the soundness of the defaults (every
TRAIN sample of a walked ray lies in the dilated set; without the dilation some do not)."""
import numpy as np
import pytest

from tests import occ_visibility_model as M
from tests.util import _cells

F32 = np.float32


def test_walked_pixels_always_hold_the_border():
    assert M.walked(12, 1).tolist() == list(range(12))
    assert M.walked(12, 3).tolist() == [0, 3, 6, 9, 11]          # 11 is no multiple of 3
    assert M.walked(20, 3).tolist() == [0, 3, 6, 9, 12, 15, 18, 19]
    assert M.walked(13, 3).tolist() == [0, 3, 6, 9, 12]          # ... and 12 is: no duplicate
    assert M.walked(1, 4).tolist() == [0]
    assert M.walked(5, 100).tolist() == [0, 4]
    ij = M.walked_pixels(12, 20, 3)
    assert ij.shape == (5 * 8, 2) and ij[-1].tolist() == [11, 19]
    mask = np.ones((12, 20), dtype=np.uint8)
    mask[3, 6] = 0
    assert M.walked_pixels(12, 20, 3, mask).shape[0] == 39


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_float32_model_against_float64_away_from_the_faces(seed):
    sc = M.scene(seed)
    ij = M.walked_pixels(M.H, M.W, 1)
    n_far = 0
    for cam in range(3):
        args = (sc["poses"][cam], sc["K"][cam], sc["dist"][cam], ij, M.N_STEPS, M.STEP)
        x32 = M.validate_points(*args).reshape(-1, 3)
        x64 = M.validate_points64(*args).reshape(-1, 3)
        assert x32.dtype == F32 and np.isfinite(x32).all() and np.isfinite(x64).all()
        # the two agree far better than the face tolerance ...
        assert np.abs(x32.astype(np.float64) - x64).max() < M.FACE_TOL / 10
        # ... so away from the faces they name the same cell
        far = (M.face_distance(x64, M.G) > M.FACE_TOL).all(1)
        c64 = _cells(x64.astype(F32), M.G)   # (the rounding to float32 moves a far sample across no face)
        assert np.array_equal(_cells(x32, M.G)[far], c64[far])
        n_far += int(far.sum())
        assert far.mean() > 0.9
        # the contraction keeps every sample inside the ball of radius 2
        assert np.sqrt((x64 * x64).sum(1)).max() < 2.0
    assert n_far > 3 * 240 * M.N_STEPS * 0.9
    # the scene has what the tests want from it
    assert np.any(sc["dist"][1] != 0) and not np.any(sc["dist"][0] != 0)
    assert np.linalg.norm(sc["poses"][2][:, 3]) > 1.0 > np.linalg.norm(sc["poses"][0][:, 3])


def test_mark_bounds_enclose_the_marks():
    sc = M.scene(0)
    for cam in range(3):
        marks = M.camera_marks(sc, cam, M.G, M.N_STEPS, M.STEP)
        sure, maybe = M.camera_mark_bounds(sc, cam, M.G, M.N_STEPS, M.STEP)
        assert not (sure & ~marks).any() and not (marks & ~maybe).any()
        assert 0 < sure.sum() <= marks.sum() <= maybe.sum() < M.G ** 3 // 2
        assert maybe.sum() - sure.sum() < 0.05 * marks.sum()      # the bounds are tight


def test_contract_at_the_origin_marks_nothing():
    x = M.contract(np.array([[0, 0, 0], [0.5, 0, 0], [3.0, 0, 0]], dtype=F32), F32)
    assert np.isnan(x[0]).all() and x[1].tolist() == [0.5, 0, 0]
    assert abs(float(x[2, 0]) - (2 - 1 / 3)) < 1e-6
    marks = M.marks_of_points(x, 32)
    assert marks.sum() == 2


def _single(G, x, y, z):
    b = np.zeros((G, G, G), dtype=bool)
    b[z, y, x] = True
    return b.reshape(-1)


@pytest.mark.parametrize("G", [32, 64])
def test_dilation_does_not_wrap_around(G):
    e = G - 1
    # a corner, an edge, a face and the interior: 8, 12, 18 and 27 cells
    for (x, y, z), n in (((0, 0, 0), 8), ((e, e, e), 8), ((e, 0, 5), 12), ((7, e, e), 12),
                         ((0, 9, 9), 18), ((9, 9, e), 18), ((31, 9, 9), 27 if G > 32 else 18),
                         ((32 % G, 9, 9), 27 if G > 32 else 18), ((5, 6, 7), 27)):
        out = M.dilate(_single(G, x, y, z), G).reshape(G, G, G)
        assert out.sum() == n, (x, y, z)
        zz, yy, xx = np.nonzero(out)
        assert max(abs(xx - x).max(), abs(yy - y).max(), abs(zz - z).max()) <= 1
    # x = G - 1 of one row and x = 0 of the next are neighbours in memory, not in space
    out = M.dilate(_single(G, e, 4, 4), G).reshape(G, G, G)
    assert not out[:, :, 0].any()
    # two passes reach two cells
    assert M.dilate(_single(G, 10, 10, 10), G, 2).sum() == 125
    assert M.dilate(_single(G, 0, 0, 0), G, 2).sum() == 27
    assert np.array_equal(M.dilate(_single(G, 3, 3, 3), G, 0), _single(G, 3, 3, 3))


def test_counts_saturate_and_threshold():
    count = np.array([0, 1, 254, 255, 254, 255], dtype=np.uint8)
    bits = np.array([1, 1, 1, 1, 0, 0], dtype=bool)
    got = M.count_add(count, bits)
    assert got.dtype == np.uint8 and got.tolist() == [1, 2, 255, 255, 254, 255]
    G = 32
    ones = np.ones(G ** 3, dtype=bool)
    assert M.view_counts([ones] * 300, G, 0).max() == 255        # 300 cameras: saturated, not wrapped
    a, b, c = _single(G, 4, 4, 4), _single(G, 5, 4, 4), _single(G, 20, 20, 20)
    cnt = M.view_counts([a, b, c], G, 1).reshape(G, G, G)
    assert cnt[4, 4, 4] == 2 and cnt[4, 4, 3] == 1 and cnt[4, 4, 6] == 1 and cnt[20, 20, 20] == 1
    assert cnt.max() == 2 and (cnt == 2).sum() == 18
    assert M.visible([a, b, c], G, 1, 2).sum() == 18
    assert M.visible([a, b, c], G, 1, 3).sum() == 0


@pytest.mark.parametrize("d", [0, 1, 2])
def test_min_views_one_is_the_dilated_union(d):
    sc = M.scene(0)
    marks = [M.camera_marks(sc, c, M.G, M.N_STEPS, M.STEP) for c in range(3)]
    union = marks[0] | marks[1] | marks[2]
    assert np.array_equal(M.visible(marks, M.G, d, 1), M.dilate(union, M.G, d))
    two = M.visible(marks, M.G, d, 2)
    assert 0 < two.sum() < M.visible(marks, M.G, d, 1).sum()


def _soundness(seed, d):
    """worst camera's share of TRAIN samples outside visible(min_views = 1), and the samples counted"""
    sc = M.scene(seed, outside=seed % 2 == 0)
    marks = [M.camera_marks(sc, c, M.G, M.N_STEPS, M.STEP) for c in range(3)]
    vis = M.visible(marks, M.G, d, 1)
    worst, total = 0.0, 0
    for cam in range(3):
        x, _ = M.train_points(sc, cam, M.S_TRAIN, M.STEP, seed=7 * seed + cam)
        frac, n = M.outside_fraction(x, vis, M.G)
        worst, total = max(worst, frac), total + n
    return worst, total


def test_the_defaults_are_sound_and_the_dilation_is_what_makes_them():
    """step / 2 = 1/64 <= 4 / G = 1/8, n_steps = 96 = ceil(1.5 * 64): with one dilation no TRAIN sample of
    any pixel falls outside the carve, zero exceptions; with none, some do."""
    assert 0.5 * M.STEP <= 4.0 / M.G and M.N_STEPS == int(np.ceil(1.5 * M.S_TRAIN))
    worst_plain = 0.0
    for seed in range(20):
        worst, total = _soundness(seed, 1)
        assert total == 3 * M.H * M.W * M.S_TRAIN == 46080
        assert worst == 0.0, (seed, worst)
        worst_plain = max(worst_plain, _soundness(seed, 0)[0])
    print("without dilation: worst camera has %.3f %% of its TRAIN samples outside" % (100 * worst_plain))
    assert worst_plain > 0.0
