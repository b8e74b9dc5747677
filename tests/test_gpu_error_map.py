"""The error map's kernels (error_map.hip) through the C ABI against the integer / float64 model of
tests/error_map_model.py: counts, cdf, draw and accumulators with array_equal, the importance weight
within 2 f32 ulp of the model's float64 value, apply exactly on dyadic inputs and within 1 ulp on
random ones, and a closed loop of three rounds.

Shapes: "masked" E=3, 37x70, 5x8 cells (nothing divides, nothing is a multiple of 32; image 1 has no
valid pixel, images 0 and 2 have valid fractions 0.6 and 0.3); "fine" E=7, 37x70, one pixel per cell
(18 130 cells: nine scan workgroups of 2048 cells, the last with 1746); "open" E=2, 9x40, 4x5 cells,
no mask."""
import functools

import numpy as np
import pytest
import torch

from tests import error_map_model as em
from tests import supervision_model as sm

pytestmark = pytest.mark.gpu

GUARD = 8
SENT = -7777
N = 4096
SEED = 0x0BADC0DE5EED1234               # both key words non-zero
SHAPES = {"masked": (3, 37, 70, 5, 8), "fine": (7, 37, 70, 37, 70), "open": (2, 9, 40, 4, 5)}


@functools.lru_cache(maxsize=None)
def scene(name):
    """grid, mask (uint8 [E,h,w] or None), value (f32 [n_cells]): read-only"""
    grid = em.Grid(*SHAPES[name])
    rng = np.random.RandomState(23 + len(name))
    mask = None
    if name == "masked":
        mask = np.zeros((grid.E, grid.h, grid.w), dtype=np.uint8)
        mask[0] = rng.rand(grid.h, grid.w) < 0.6
        mask[2] = (rng.rand(grid.h, grid.w) < 0.3) * 200       # any non-zero is valid
    elif name == "fine":
        mask = (rng.rand(grid.E, grid.h, grid.w) < 0.5).astype(np.uint8)
    value = (0.01 + rng.rand(grid.n_cells)).astype(np.float32)
    # the edges of the quantiser: zero, NaN, below the floor, above the cap, infinities, negative
    edge = np.array([0.0, np.nan, 1e-9, 300.0, np.inf, -np.inf, -2.0], dtype=np.float32)
    spots = rng.choice(grid.n_cells, size=3 * edge.size, replace=False)
    value[spots] = np.tile(edge, 3)
    if name == "masked":
        # ... and the cap inside images that have valid pixels, so the draw meets it
        value[[7, 2 * 40 + 11]] = 300.0
    for a in (mask, value):
        if a is not None:
            a.setflags(write=False)
    return grid, mask, value


@functools.lru_cache(maxsize=None)
def model_state(name):
    grid, mask, value = scene(name)
    counts = em.cell_counts(grid, mask)
    cdf = em.cdf(value, counts)
    for a in (counts, cdf):
        a.setflags(write=False)
    return counts, cdf


@functools.lru_cache(maxsize=None)
def model_draw(name, u, attempts):
    grid, mask, value = scene(name)
    out = em.draw(grid, mask, value, model_state(name)[1], N, SEED, attempts, u)
    for a in out:
        a.setflags(write=False)
    return out


def guarded(n, dtype, dev):
    return torch.full((n + GUARD,), SENT, dtype=dtype, device=dev)


def guards_intact(*bufs):
    for buf, used in bufs:
        assert bool((buf[used:] == SENT).all()), "guard overwritten"


def as_u64(t):
    return t.cpu().numpy().view(np.uint64)


class DeviceScene:
    """bits, n_valid and counts of one shape on the device, through the C ABI"""

    def __init__(self, capi, dev, name):
        self.capi, self.dev, self.name = capi, dev, name
        self.grid, mask, value = scene(name)
        g = self.grid
        self.geometry = (g.E, g.h, g.w, g.gh, g.gw)
        c = capi.lib().cdll
        self.bits = None
        if mask is not None:
            m = torch.from_numpy(mask.copy()).to(dev)
            self.bits = torch.zeros(c.f2n_mask_words(g.E, g.h, g.w), dtype=torch.int32, device=dev)
            self.n_valid = torch.zeros(1, dtype=torch.int64, device=dev)
            part = torch.zeros(c.f2n_mask_pack_workspace_words(g.E, g.h, g.w), dtype=torch.int32,
                               device=dev)
            capi.call("mask_pack", m, g.E, g.h, g.w, self.bits, self.n_valid, part)
        else:
            self.n_valid = torch.tensor([g.E * g.h * g.w], dtype=torch.int64, device=dev)
        self.counts = guarded(g.n_cells, torch.int32, dev)
        capi.call("mask_cell_counts", self.bits, *self.geometry, self.counts)
        self.value = torch.from_numpy(value.copy()).to(dev)
        self.cdf = self.make_cdf(self.value)

    def make_cdf(self, value):
        g = self.grid
        n_part = self.capi.lib().cdll.f2n_error_cdf_workspace_words(g.n_cells)
        cdf = guarded(g.n_cells, torch.int64, self.dev)
        part = guarded(n_part, torch.int64, self.dev)
        self.capi.call("error_cdf", value, self.counts, g.n_cells, cdf, part)
        torch.cuda.synchronize()
        guards_intact((cdf, g.n_cells), (part, n_part))
        return cdf[:g.n_cells].clone()

    def draw(self, u, attempts, seed=SEED, n=N, value=None, cdf=None):
        cam, ij = guarded(n, torch.int32, self.dev), guarded(2 * n, torch.int32, self.dev)
        tries, wgt = guarded(n, torch.int32, self.dev), guarded(n, torch.float32, self.dev)
        self.capi.call("draw_pixels_guided", self.bits, self.counts,
                       self.value if value is None else value, self.cdf if cdf is None else cdf,
                       self.n_valid, *self.geometry, seed & sm.MASK32, seed >> 32, attempts, u, cam,
                       ij, tries, wgt, n)
        torch.cuda.synchronize()
        guards_intact((cam, n), (ij, 2 * n), (tries, n), (wgt, n))
        return (cam[:n].cpu().numpy(), ij[:2 * n].reshape(n, 2).cpu().numpy(), tries[:n].cpu().numpy(),
                wgt[:n].cpu().numpy())


@pytest.fixture(scope="module")
def scenes(capi, dev):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = DeviceScene(capi, dev, name)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(SHAPES))
def test_counts_equal_model(scenes, name):
    ds = scenes(name)
    grid, mask, _ = scene(name)
    torch.cuda.synchronize()
    guards_intact((ds.counts, grid.n_cells))
    got = ds.counts[:grid.n_cells].cpu().numpy()
    assert np.array_equal(got, model_state(name)[0])
    if mask is None:
        _, _, rows, _, cols = grid.cell_box(np.arange(grid.n_cells))
        assert np.array_equal(got, rows * cols) and got.sum() == grid.E * grid.h * grid.w
    else:
        assert got.sum() == int((mask != 0).sum())
        if name == "masked":
            per = grid.gh * grid.gw
            assert (got[per:2 * per] == 0).all()               # image 1 has no valid pixel


@pytest.mark.parametrize("name", list(SHAPES))
def test_cdf_equals_model(capi, scenes, name):
    ds = scenes(name)
    n_tiles = capi.lib().cdll.f2n_error_cdf_workspace_words(ds.grid.n_cells)
    if name == "fine":
        assert n_tiles >= 3 and ds.grid.n_cells % em.SCAN_TILE != 0
        assert n_tiles == -(-ds.grid.n_cells // em.SCAN_TILE)
    assert np.array_equal(as_u64(ds.cdf), model_state(name)[1])


CASES = [("masked", u, a) for u in (0.0, 0.25, 1.0) for a in (32, 2)] + [
    ("fine", 0.0, 32), ("fine", 0.25, 2), ("open", 0.25, 32), ("open", 0.0, 2)]


@pytest.mark.parametrize("name,u,attempts", CASES)
def test_draw_equals_model(scenes, name, u, attempts):
    ds = scenes(name)
    want_cam, want_ij, want_tries, want_w, guided = model_draw(name, u, attempts)
    missed = float((want_tries == 0).mean())
    print("%s u=%g A=%d: the model misses %.1f %% of the rays, %d guided" % (
        name, u, attempts, 100 * missed, int(guided.sum())))
    if name == "masked" and attempts == 2:
        assert 0.05 <= missed <= 0.60                           # the miss path is really exercised
    if 0 < u < 1:
        assert 0 < guided.sum() < N                             # both branches
    cam, ij, tries, wgt = ds.draw(u, attempts)
    assert np.array_equal(tries, want_tries)
    assert np.array_equal(cam, want_cam)
    assert np.array_equal(ij, want_ij)
    err = np.abs(wgt.astype(np.float64) - want_w)
    ulps = err / em.ulp_f32(want_w)
    print("largest weight error: %.3f f32 ulp" % ulps.max())
    assert (ulps <= 2.0).all()
    assert (wgt[want_tries == 0].view(np.int32) == 0).all()    # exactly +0
    if u > 0:
        assert wgt.max() <= np.float32(1.0 / u)
    # a repeated call gives the same bits
    again = ds.draw(u, attempts)
    for a, b in zip((cam, ij, tries, wgt.view(np.int32)), (again[0], again[1], again[2],
                                                             again[3].view(np.int32))):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("attempts", [32, 2])
def test_uniform_fraction_one_is_the_masked_draw(capi, dev, scenes, attempts):
    ds = scenes("masked")
    g = ds.grid
    cam, ij, tries = (guarded(N, torch.int32, dev), guarded(2 * N, torch.int32, dev),
                      guarded(N, torch.int32, dev))
    capi.call("draw_pixels_masked", ds.bits, g.E, g.h, g.w, SEED & sm.MASK32, SEED >> 32, attempts,
              cam, ij, tries, N)
    torch.cuda.synchronize()
    got = ds.draw(1.0, attempts)
    assert np.array_equal(got[0], cam[:N].cpu().numpy())
    assert np.array_equal(got[1], ij[:2 * N].reshape(N, 2).cpu().numpy())
    assert np.array_equal(got[2], tries[:N].cpu().numpy())
    assert np.array_equal(got[3], (got[2] > 0).astype(np.float32))   # every kept weight is 1


# ------------------------------------------------------------------------------ accumulate --------

CROWDED = 13                            # a cell of image 0 that 500 rays fall in


@functools.lru_cache(maxsize=None)
def accum_case(kind):
    """4096 rays on images 0 and 2 of the "masked" shape: cam, ij, colors, gt, bg, alpha, ray_weight
    (read-only).  500 rays fall in one cell; some rays have m = 0, a NaN colour, or lie outside the
    set.  No ray lands in image 1, whose cells stay untouched."""
    grid, _, _ = scene("masked")
    rng = np.random.RandomState(5 if kind == "dyadic" else 6)
    cam = rng.choice([0, 2], N).astype(np.int32)
    ij = np.stack([rng.randint(0, grid.h, N), rng.randint(0, grid.w, N)], 1).astype(np.int32)
    e, i0, rows, j0, cols = grid.cell_box(CROWDED)
    cam[:500] = e
    ij[:500, 0] = i0 + rng.randint(0, rows, 500)
    ij[:500, 1] = j0 + rng.randint(0, cols, 500)
    if kind == "dyadic":
        colors, gt, bg = (rng.randint(0, 257, (N, 3)).astype(np.float32) / 256 for _ in range(3))
        alpha = rng.choice([0.0, 0.5, 1.0], N).astype(np.float32)
    else:
        colors, gt, bg = (rng.rand(N, 3).astype(np.float32) for _ in range(3))
        colors[1000:1010] *= 3.0                                # some errors above the cap of 4
        alpha = rng.rand(N).astype(np.float32)
    m = rng.choice([0.0, 1.0, 0.37, 2.5], N).astype(np.float32)
    odd = np.zeros(N, dtype=bool)                               # rays that must leave no trace
    m[10:20] = 0.0
    m[20:50] = 1.0
    odd |= m == 0
    colors[20:30, 1], odd[20:30] = np.nan, True
    colors[30, 0], odd[30] = np.inf, True
    cam[31:35], odd[31:35] = grid.E, True
    cam[35], odd[35] = -1, True
    ij[36, 0], odd[36] = grid.h, True
    ij[37, 1], odd[37] = grid.w, True
    ij[38, 0], odd[38] = -1, True
    colors[3, 2] = np.nan                                       # in the crowded cell, m may be non-zero
    odd[3] = True
    out = dict(cam=cam, ij=ij, colors=colors, gt=gt, bg=bg, alpha=alpha, ray_weight=m, odd=odd)
    for a in out.values():
        a.setflags(write=False)
    return out


def run_accum(capi, dev, grid, case, keep=None, with_alpha=True):
    sel = slice(None) if keep is None else keep
    t = {k: torch.from_numpy(np.array(v[sel])).to(dev) for k, v in case.items()
         if k != "odd"}
    n = t["cam"].shape[0]
    acc_sum, acc_cnt = guarded(grid.n_cells, torch.int64, dev), guarded(grid.n_cells, torch.int32, dev)
    acc_sum[:grid.n_cells] = 0
    acc_cnt[:grid.n_cells] = 0
    capi.call("error_map_accum", t["colors"], t["gt"], t["alpha"] if with_alpha else None,
              t["bg"] if with_alpha else None, t["ray_weight"], t["cam"], t["ij"], n, grid.E, grid.h,
              grid.w, grid.gh, grid.gw, acc_sum, acc_cnt)
    torch.cuda.synchronize()
    guards_intact((acc_sum, grid.n_cells), (acc_cnt, grid.n_cells))
    return acc_sum, acc_cnt


def model_accum(grid, case, with_alpha=True):
    acc_sum = np.zeros(grid.n_cells, dtype=np.uint64)
    acc_cnt = np.zeros(grid.n_cells, dtype=np.uint32)
    em.accumulate(grid, acc_sum, acc_cnt, case["colors"], case["gt"], case["cam"], case["ij"],
                  case["ray_weight"], case["alpha"] if with_alpha else None,
                  case["bg"] if with_alpha else None)
    return acc_sum, acc_cnt


@pytest.mark.parametrize("with_alpha", [True, False])
@pytest.mark.parametrize("kind", ["dyadic", "random"])
def test_accumulate(capi, dev, kind, with_alpha):
    grid, _, _ = scene("masked")
    case = accum_case(kind)
    want_sum, want_cnt = model_accum(grid, case, with_alpha)
    assert want_cnt[CROWDED] > 300 and int(want_cnt.sum()) == int((~case["odd"]).sum())
    acc_sum, acc_cnt = run_accum(capi, dev, grid, case, with_alpha=with_alpha)
    got_sum = as_u64(acc_sum[:grid.n_cells])
    got_cnt = acc_cnt[:grid.n_cells].cpu().numpy().view(np.uint32)
    assert np.array_equal(got_cnt, want_cnt)
    diff = np.abs(got_sum.astype(np.int64) - want_sum.astype(np.int64))
    print("largest |acc_sum - model| / acc_cnt: %.3f" % (diff / np.maximum(want_cnt, 1)).max())
    if kind == "dyadic":
        assert np.array_equal(got_sum, want_sum)
    else:
        assert (diff <= want_cnt).all()                        # one quantisation unit per ray
    # the odd rays leave no trace: the same call without them gives the same bits
    keep = np.flatnonzero(~case["odd"])
    clean_sum, clean_cnt = run_accum(capi, dev, grid, case, keep=keep, with_alpha=with_alpha)
    assert torch.equal(clean_sum, acc_sum) and torch.equal(clean_cnt, acc_cnt)


@pytest.mark.parametrize("kind,decay", [("dyadic", 0.5), ("random", 0.9)])
def test_apply(capi, dev, kind, decay):
    grid, _, value0 = scene("masked")
    case = accum_case(kind)
    value0 = np.where(np.isfinite(value0), value0, np.float32(0.25)).astype(np.float32)
    if kind == "dyadic":
        value0 = (np.round(value0 * 256) / 256).astype(np.float32)
    acc_sum, acc_cnt = run_accum(capi, dev, grid, case)
    want_sum, want_cnt = (a.copy() for a in (as_u64(acc_sum[:grid.n_cells]),
                                             acc_cnt[:grid.n_cells].cpu().numpy().view(np.uint32)))
    hit = want_cnt > 0
    assert hit.any() and (~hit).sum() >= grid.gh * grid.gw      # image 1's cells stay untouched
    want = value0.copy()
    em.apply(want, want_sum, want_cnt, decay)
    value = guarded(grid.n_cells, torch.float32, dev)
    value[:grid.n_cells] = torch.from_numpy(value0).to(dev)
    capi.call("error_map_apply", value, acc_sum, acc_cnt, grid.n_cells, decay)
    torch.cuda.synchronize()
    guards_intact((value, grid.n_cells), (acc_sum, grid.n_cells), (acc_cnt, grid.n_cells))
    got = value[:grid.n_cells].cpu().numpy()
    assert np.array_equal(got[~hit].view(np.int32), value0[~hit].view(np.int32))
    assert not bool(acc_sum[:grid.n_cells].any()) and not bool(acc_cnt[:grid.n_cells].any())
    if kind == "dyadic":
        # the model evaluates the same float64 expression on the same integers: equal bits
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
    else:
        ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / em.ulp_f32(want)
        assert (ulps <= 1.0).all()
    assert (got[hit] != value0[hit]).any()


def test_accumulate_cell_is_the_pixels_cell(capi, dev):
    """one ray per pixel of an image: acc_cnt is the closed-form count of every cell"""
    grid, _, _ = scene("masked")
    i, j = np.meshgrid(np.arange(grid.h), np.arange(grid.w), indexing="ij")
    n = i.size
    case = dict(cam=np.full(n, 2, dtype=np.int32),
                ij=np.stack([i.reshape(-1), j.reshape(-1)], 1).astype(np.int32),
                colors=np.ones((n, 3), dtype=np.float32), gt=np.zeros((n, 3), dtype=np.float32),
                bg=np.zeros((n, 3), dtype=np.float32), alpha=np.ones(n, dtype=np.float32),
                ray_weight=np.ones(n, dtype=np.float32))
    acc_sum, acc_cnt = run_accum(capi, dev, grid, case)
    want = em.cell_counts(grid)
    per = grid.gh * grid.gw
    want[:2 * per] = 0
    got = acc_cnt[:grid.n_cells].cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(as_u64(acc_sum[:grid.n_cells]), want.astype(np.uint64) * np.uint64(3 << 20))


# ------------------------------------------------------------------------------ closed loop -------

HOT = (4, 9, 2 * 40 + 17, 2 * 40 + 30)     # high-error cells of images 0 and 2


def loop_colors(grid, cam, ij):
    """a fixed dyadic function of (cam, i, j): colour 1 in the HOT cells, small elsewhere; gt is 0"""
    cells = grid.cell_of(cam, ij[:, 0], ij[:, 1])
    base = ((cam.astype(np.int64) + ij[:, 0] + 2 * ij[:, 1]) % 5).astype(np.float32) / 32
    c = np.stack([base, base / 2, base / 4], 1).astype(np.float32)
    c[np.isin(cells, HOT)] = 1.0
    return c


def test_closed_loop(capi, dev, scenes):
    ds = scenes("masked")
    grid, mask, _ = scene("masked")
    u, attempts, decay = 0.25, 32, 0.5
    counts = model_state("masked")[0]
    m_value = np.ones(grid.n_cells, dtype=np.float32)
    m_cdf = em.cdf(m_value, counts)
    g_value = torch.ones(grid.n_cells, dtype=torch.float32, device=dev)
    g_cdf = ds.make_cdf(g_value)
    acc_sum = torch.zeros(grid.n_cells, dtype=torch.int64, device=dev)
    acc_cnt = torch.zeros(grid.n_cells, dtype=torch.int32, device=dev)
    m_sum = np.zeros(grid.n_cells, dtype=np.uint64)
    m_cnt = np.zeros(grid.n_cells, dtype=np.uint32)
    gt = np.zeros((N, 3), dtype=np.float32)
    for rnd in range(4):
        seed = SEED + 0x100000001 * rnd
        m_cam, m_ij, m_tries, m_w, _ = em.draw(grid, mask, m_value, m_cdf, N, seed, attempts, u)
        cam, ij, tries, wgt = ds.draw(u, attempts, seed=seed, value=g_value, cdf=g_cdf)
        assert np.array_equal(cam, m_cam) and np.array_equal(ij, m_ij), "round %d" % rnd
        assert np.array_equal(tries, m_tries)
        g_share = float(np.isin(grid.cell_of(cam, ij[:, 0], ij[:, 1])[tries > 0], HOT).mean())
        m_share = float(np.isin(grid.cell_of(m_cam, m_ij[:, 0], m_ij[:, 1])[m_tries > 0], HOT).mean())
        print("round %d: %.1f %% of the kept draws land in the hot cells" % (rnd, 100 * g_share))
        if rnd == 0:
            first_share = m_share
        if rnd == 3:
            # after three updates the draw has moved to the hot cells, by the model's share exactly
            assert g_share == m_share and m_share > 3 * first_share
            break
        # each side closes its own loop: its own draw, its own weights
        em.accumulate(grid, m_sum, m_cnt, loop_colors(grid, m_cam, m_ij), gt, m_cam, m_ij,
                      m_w.astype(np.float32))
        em.apply(m_value, m_sum, m_cnt, decay)
        m_cdf = em.cdf(m_value, counts)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        capi.call("error_map_accum", t(loop_colors(grid, cam, ij)), t(gt), None, None, t(wgt), t(cam),
                  t(ij), N, grid.E, grid.h, grid.w, grid.gh, grid.gw, acc_sum, acc_cnt)
        capi.call("error_map_apply", g_value, acc_sum, acc_cnt, grid.n_cells, decay)
        g_cdf = ds.make_cdf(g_value)
        assert np.array_equal(g_value.cpu().numpy().view(np.int32), m_value.view(np.int32))
        assert np.array_equal(as_u64(g_cdf), m_cdf), "round %d" % rnd
