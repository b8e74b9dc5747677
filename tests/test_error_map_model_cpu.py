"""The numpy model of error-guided sampling (tests/error_map_model.py) against its own definitions:
the Philox known answer, the cell partition, the pdf and the importance weight, the uniform_fraction
= 1 identity with the masked draw, and the cell frequencies of the draw.  No GPU."""
import functools

import numpy as np
import pytest

from tests import error_map_model as em
from tests import supervision_model as sm

SEED = 0x0BADC0DE5EED1234               # both key words non-zero
E, H, W, GH, GW = 3, 37, 70, 5, 8


@functools.lru_cache(maxsize=None)
def _scene():
    """grid, mask (image 1 all zero, fractions 0.6 and 0.3 elsewhere), value with a few hot cells"""
    rng = np.random.RandomState(11)
    grid = em.Grid(E, H, W, GH, GW)
    mask = np.zeros((E, H, W), dtype=np.uint8)
    mask[0] = rng.rand(H, W) < 0.6
    mask[2] = rng.rand(H, W) < 0.3
    value = (0.02 + 0.1 * rng.rand(grid.n_cells)).astype(np.float32)
    value[[3, 17, 95, 110]] = 1.5
    for a in (mask, value):
        a.setflags(write=False)
    return grid, mask, value


def test_philox_known_answer():
    assert sm.philox_scalar((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    x = sm.philox4x32_10(np.zeros(2), 0, 0, 0, 0, 0)
    assert [int(v[0]) for v in x] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


@pytest.mark.parametrize("h,gh", [(37, 5), (70, 8), (37, 37), (9, 4)])
def test_partition(h, gh):
    """every pixel row lies in exactly one cell row, the one the forward formula names, and no cell
    row is empty"""
    grid = em.Grid(1, h, h, gh, gh)
    first = grid.first(np.arange(gh + 1), h, gh)
    assert first[0] == 0 and first[-1] == h and (np.diff(first) >= 1).all()
    owner = np.full(h, -1)
    for a in range(gh):
        assert (owner[first[a]:first[a + 1]] == -1).all()
        owner[first[a]:first[a + 1]] = a
    assert np.array_equal(owner, (np.arange(h) * gh) // h)
    # ... and in two dimensions the counts of the closed form are those of the pixels' cells
    grid = em.Grid(2, h, 70, gh, 8)
    assert np.array_equal(em.cell_counts(grid), np.bincount(grid.pixel_cells().reshape(-1),
                                                            minlength=grid.n_cells))
    assert em.cell_counts(grid).min() >= 1


@pytest.mark.parametrize("u", [0.0, 0.25, 1.0])
def test_pdf_sums_to_one_and_weight_has_expectation_one(u):
    grid, mask, value = _scene()
    pdf = em.pixel_pdf(grid, mask, value, u)
    valid = mask.reshape(-1) != 0
    assert abs(pdf.sum() - 1.0) <= 1e-12
    counts = em.cell_counts(grid, mask)
    total = int(em.cdf(value, counts)[-1])
    q = em.quant(value)[grid.pixel_cells().reshape(-1)]
    m = em.weight_f64(u, q, int(valid.sum()), total)
    assert abs((pdf * m)[valid].sum() - 1.0) <= 1e-12                  # E[m] = 1
    assert np.allclose(m[valid], (1.0 / valid.sum()) / pdf[valid], rtol=1e-12)
    if u > 0:
        assert m[valid].max() <= 1.0 / u
    if u == 1.0:
        assert (m == 1.0).all()


@pytest.mark.parametrize("attempts", [32, 2])
def test_uniform_fraction_one_is_the_masked_draw(attempts):
    grid, mask, value = _scene()
    counts = em.cell_counts(grid, mask)
    cam, ij, tries, weight, guided = em.draw(grid, mask, value, em.cdf(value, counts), 4096, SEED,
                                             attempts, 1.0)
    want = sm.draw(mask, 4096, SEED, attempts)
    assert not guided.any()
    assert np.array_equal(cam, want[0]) and np.array_equal(ij, want[1]) and np.array_equal(tries, want[2])
    assert np.array_equal(weight, (tries > 0).astype(np.float64))


@pytest.mark.parametrize("u", [0.0, 0.25, 1.0])
def test_cell_frequencies(u):
    """4096 draws: every cell with n P > 5 is hit within 4.5 binomial standard deviations of P(cell)
    (the prototype's largest deviation with these seeds was 3.05)"""
    grid, mask, value = _scene()
    n = 4096
    counts = em.cell_counts(grid, mask)
    cam, ij, tries, _, _ = em.draw(grid, mask, value, em.cdf(value, counts), n, SEED, 64, u)
    assert (tries > 0).mean() > 0.999          # 64 attempts: next to nothing is lost
    assert (mask[cam, ij[:, 0], ij[:, 1]][tries > 0] != 0).all()
    P = np.bincount(grid.pixel_cells().reshape(-1), weights=em.pixel_pdf(grid, mask, value, u),
                    minlength=grid.n_cells)
    hits = np.bincount(grid.cell_of(cam, ij[:, 0], ij[:, 1])[tries > 0], minlength=grid.n_cells)
    big = n * P > 5
    assert big.sum() > 20
    dev = np.abs(hits[big] - n * P[big]) / np.sqrt(n * P[big] * (1 - P[big]))
    print("largest deviation at u = %g: %.2f sigma" % (u, dev.max()))
    assert dev.max() <= 4.5
    assert hits[counts == 0].sum() == 0


def test_quant_and_cdf_edges():
    v = np.array([0.0, np.nan, 1e-9, 300.0, np.inf, -np.inf, -3.0, 1.0, 0.5], dtype=np.float32)
    assert em.quant(v).tolist() == [1, 1, 1, 1 << 24, 1, 1, 1, 65536, 32768]
    counts = np.array([2, 0, 3, 1, 0, 5, 1, 1, 1], dtype=np.int32)
    c = em.cdf(v, counts)
    assert c.dtype == np.uint64 and c[-1] == 2 + 3 + (1 << 24) + 5 + 1 + 65536 + 32768
    assert c[1] == c[0] and c[4] == c[3]       # a cell without valid pixels has no mass
