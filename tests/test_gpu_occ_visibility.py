"""The camera-visibility carve on the GPU: f2n_occ_mark_rays against the chain of kernels that already
produce its samples (f2n_gen_rays_dist -> f2n_sample_rays -> f2n_contract_fwd, cells in numpy) bit for
bit and against the numpy model within its face bounds; dilation, counts and threshold against the
model; the soundness of the defaults on TRAIN samples; the host functions; the OccupancyGrid's allowed
mask through update(), set_bits() and the render routes."""
import importlib

import numpy as np
import pytest
import torch

from tests import occ_visibility_model as M
from tests.test_gpu_render import _setup
from tests.util import _cells, _pack

pytestmark = pytest.mark.gpu

G, H, W, STEP = M.G, M.H, M.W, M.STEP
CELLS = G ** 3


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


@pytest.fixture(scope="module")
def sc():
    return M.scene(0)


@pytest.fixture(scope="module")
def tables(sc, dev):
    """the camera tables on the device, poses as [3,3,4] (pose_ld 12) and as [3,4,4] (16)"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return {12: t(sc["poses"]), 16: t(M.poses44(sc["poses"])), "K": t(sc["K"]), "dist": t(sc["dist"])}


# ---- helpers -------------------------------------------------------------------------------------

def _pack_pixels(mask, dev):
    """[E, h, w] 0/1 -> the uint32 words of f2n_mask_pack's layout (padded to whole words)"""
    flat = np.asarray(mask, dtype=bool).reshape(-1)
    pad = (-flat.shape[0]) % 32
    return _pack(torch.from_numpy(np.concatenate([flat, np.zeros(pad, dtype=bool)]))).to(dev)


def _masks():
    rng = np.random.default_rng(5)
    scattered = (rng.random((3, H, W)) < 0.7).astype(np.uint8)
    scattered[:, H - 1, W - 1] = 0          # the always-walked corner among the blanked ones
    one_cam = np.ones((3, H, W), dtype=np.uint8)
    one_cam[1] = 0
    return {"none": None, "scattered": scattered, "camera1": one_cam}


MASKS = _masks()
_chain_cache = {}


def _chain_marks(capi, dev, tables, cam, n_steps, stride, mask_kind, with_dist=True):
    """bool [G^3] (numpy): the cells of the VALIDATE samples of camera cam's walked pixels, from the
    existing kernels.  Computed once per key."""
    key = (cam, n_steps, stride, mask_kind, with_dist)
    if key in _chain_cache:
        return _chain_cache[key]
    mask = MASKS[mask_kind]
    ij_np = M.walked_pixels(H, W, stride, None if mask is None else mask[cam])
    marks = np.zeros(CELLS, dtype=bool)
    n = ij_np.shape[0]
    if n:
        ij = torch.from_numpy(ij_np).to(dev)
        cam_idx = torch.full((n,), cam, dtype=torch.int32, device=dev)
        o, d = torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev)
        capi.call("gen_rays_dist", tables[12], 12, tables["K"], tables["dist"] if with_dist else None,
                  3, cam_idx, ij, 0, 1, o, d, n)
        pts = torch.empty(n * n_steps, 3, device=dev)
        dirs, dt, t = torch.empty_like(pts), torch.empty(n * n_steps, device=dev), torch.empty(n * n_steps, device=dev)
        bounds = torch.zeros(n, 2, dtype=torch.int32, device=dev)
        capi.call("sample_rays", o, d, None, pts, dirs, dt, t, bounds, n, n_steps, STEP)
        x = torch.empty_like(pts)
        capi.call("contract_fwd", pts, x, n * n_steps)
        marks = M.marks_of_points(x.cpu().numpy(), G)
    _chain_cache[key] = marks
    return marks


def _mark(capi, dev, tables, pose_ld, cam_first, n_cams, stride, mask_kind, n_steps, bits=None,
          with_dist=True, step=STEP, res=G):
    if bits is None:
        bits = torch.zeros(res ** 3 // 32, dtype=torch.int32, device=dev)
    mask = MASKS[mask_kind]
    mask_bits = None if mask is None else _pack_pixels(mask, dev)
    capi.call("occ_mark_rays", tables[pose_ld], pose_ld, tables["K"],
              tables["dist"] if with_dist else None, cam_first, n_cams, H, W, stride, mask_bits,
              n_steps, step, bits, res)
    return bits


def _unpack(words):
    w = words.cpu().numpy().view(np.uint8)
    return np.unpackbits(w, bitorder="little").astype(bool)


def _words(bits_bool, dev):
    return _pack(torch.from_numpy(np.asarray(bits_bool, dtype=bool))).to(dev)


# ---- 1. the marks --------------------------------------------------------------------------------

@pytest.mark.parametrize("n_steps,stride,cam_first,n_cams,mask_kind,pose_ld,with_dist", [
    (96, 1, 0, 3, "none", 12, True),
    (70, 1, 0, 3, "none", 16, True),         # a partial last stride; [4,4] poses
    (96, 3, 0, 3, "none", 12, True),         # neither h - 1 = 11 nor w - 1 = 19 is a multiple of 3
    (70, 3, 1, 2, "none", 16, True),         # cameras 1 and 2 of the tables
    (96, 1, 1, 2, "none", 12, True),
    (96, 1, 0, 3, "scattered", 12, True),
    (70, 3, 0, 3, "scattered", 16, True),
    (96, 1, 0, 3, "camera1", 12, True),      # a whole camera blanked
    (96, 1, 1, 1, "camera1", 12, True),      # ... and nothing else walked: no mark at all
    (96, 1, 0, 3, "none", 12, False),        # dist = NULL: every camera a pinhole
    (96, 1, 2, 1, "none", 12, True),         # the camera outside the unit ball alone
])
def test_mark_rays_against_the_kernel_chain(capi, dev, sc, tables, n_steps, stride, cam_first, n_cams,
                                            mask_kind, pose_ld, with_dist):
    cams = range(cam_first, cam_first + n_cams)
    per_cam = [_chain_marks(capi, dev, tables, c, n_steps, stride, mask_kind, with_dist) for c in cams]
    want = np.logical_or.reduce(per_cam)
    got = _mark(capi, dev, tables, pose_ld, cam_first, n_cams, stride, mask_kind, n_steps,
                with_dist=with_dist)
    assert torch.equal(got.cpu(), _words(want, dev).cpu())
    if mask_kind == "camera1" and n_cams == 1:
        assert not want.any()
        return
    assert 0 < want.sum() < CELLS // 2
    # bits already set survive, and nothing else changes
    rng = np.random.default_rng(n_steps + stride)
    preset = rng.random(CELLS) < 0.1
    got2 = _mark(capi, dev, tables, pose_ld, cam_first, n_cams, stride, mask_kind, n_steps,
                 bits=_words(preset, dev), with_dist=with_dist)
    assert torch.equal(got2.cpu(), _words(want | preset, dev).cpu())
    assert (preset & ~want).sum() > 0
    # the numpy model: sure <= marks <= maybe (tests/occ_visibility_model.py)
    if with_dist:
        mask = MASKS[mask_kind]
        sure, maybe = np.zeros(CELLS, dtype=bool), np.zeros(CELLS, dtype=bool)
        for c in cams:
            s, m = M.camera_mark_bounds(sc, c, G, n_steps, STEP, stride, None if mask is None else mask[c])
            sure |= s
            maybe |= m
        g = _unpack(got)
        assert not (sure & ~g).any() and not (g & ~maybe).any()
        assert sure.sum() > 0.9 * g.sum()


def test_marks_differ_where_they_should(capi, dev, tables):
    """the cases above are not one set under many names"""
    a = _chain_marks(capi, dev, tables, 1, 96, 1, "none", True)
    assert not np.array_equal(a, _chain_marks(capi, dev, tables, 1, 96, 1, "none", False))   # the lens
    assert not np.array_equal(a, _chain_marks(capi, dev, tables, 1, 70, 1, "none", True))    # the reach
    assert not np.array_equal(a, _chain_marks(capi, dev, tables, 1, 96, 3, "none", True))    # the stride
    assert not np.array_equal(_chain_marks(capi, dev, tables, 0, 96, 1, "none", True),
                              _chain_marks(capi, dev, tables, 0, 96, 1, "scattered", True))  # the mask


def test_larger_grid_and_finer_step(capi, dev, tables):
    """G = 128 with the reference's step: indices beyond 2^16, several samples to a cell"""
    n_steps, res, step = 200, 128, 1.0 / 256
    got = _mark(capi, dev, tables, 12, 0, 3, 1, "none", n_steps, step=step, res=res)
    want = np.zeros(res ** 3, dtype=bool)
    for cam in range(3):
        ij_np = M.walked_pixels(H, W, 1)
        n = ij_np.shape[0]
        ij = torch.from_numpy(ij_np).to(dev)
        cam_idx = torch.full((n,), cam, dtype=torch.int32, device=dev)
        o, d = torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev)
        capi.call("gen_rays_dist", tables[12], 12, tables["K"], tables["dist"], 3, cam_idx, ij, 0, 1, o, d, n)
        pts = torch.empty(n * n_steps, 3, device=dev)
        dirs, dt, t = torch.empty_like(pts), torch.empty(n * n_steps, device=dev), torch.empty(n * n_steps, device=dev)
        bounds = torch.zeros(n, 2, dtype=torch.int32, device=dev)
        capi.call("sample_rays", o, d, None, pts, dirs, dt, t, bounds, n, n_steps, step)
        x = torch.empty_like(pts)
        capi.call("contract_fwd", pts, x, n * n_steps)
        want |= M.marks_of_points(x.cpu().numpy(), res)
    assert torch.equal(got.cpu(), _words(want, dev).cpu())
    assert want.sum() > 1000


# ---- 2. two launches, the same words ---------------------------------------------------------------

def test_the_same_launch_twice_gives_equal_words(capi, dev, tables):
    a = _mark(capi, dev, tables, 12, 0, 3, 1, "scattered", 96)
    b = _mark(capi, dev, tables, 12, 0, 3, 1, "scattered", 96)
    assert torch.equal(a, b) and int((a != 0).sum()) > 0
    # a second launch over bits that are all set already writes nothing new
    c = _mark(capi, dev, tables, 12, 0, 3, 1, "scattered", 96, bits=a.clone())
    assert torch.equal(a, c)


def test_no_cameras_writes_nothing(capi, dev, tables):
    bits = torch.full((CELLS // 32,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    out = _mark(capi, dev, tables, 12, 1, 0, 1, "none", 96, bits=bits.clone())
    assert torch.equal(out, bits)


# ---- 3. dilation -----------------------------------------------------------------------------------

def _dilate(capi, words, res):
    out = torch.full_like(words, 0x77777777)
    capi.call("occ_dilate", words, out, res)
    return out


@pytest.mark.parametrize("res", [32, 64])
def test_dilate_against_the_model(capi, dev, res):
    rng = np.random.default_rng(res)
    e = res - 1
    cases = [rng.random(res ** 3) < 0.02, rng.random(res ** 3) < 0.3, np.zeros(res ** 3, dtype=bool),
             np.ones(res ** 3, dtype=bool)]
    # single bits: corners, edges, faces, both sides of a word boundary, the interior
    for x, y, z in ((0, 0, 0), (e, e, e), (e, 0, 0), (0, e, 5), (e, 7, e), (0, 9, 9), (9, 9, e),
                    (9, 0, 9), (31, 9, 9), (32 % res, 9, 9), (e, 4, 4), (0, 5, 4), (5, 6, 7)):
        b = np.zeros((res, res, res), dtype=bool)
        b[z, y, x] = True
        cases.append(b.reshape(-1))
    for bits in cases:
        words = _words(bits, dev)
        once = _dilate(capi, words, res)
        assert torch.equal(once.cpu(), _words(M.dilate(bits, res, 1), dev).cpu())
        assert torch.equal(words.cpu(), _words(bits, dev).cpu())          # the input is left alone
        twice = _dilate(capi, once, res)
        assert torch.equal(twice.cpu(), _words(M.dilate(bits, res, 2), dev).cpu())


# ---- 4. counts ---------------------------------------------------------------------------------------

def test_count_add_and_count_bits(capi, dev):
    rng = np.random.default_rng(3)
    start = np.tile(np.array([0, 1, 254, 255], dtype=np.uint8), CELLS // 4)
    rng.shuffle(start)
    bits = rng.random(CELLS) < 0.5
    count = torch.from_numpy(start.copy()).to(dev)
    capi.call("occ_count_add", _words(bits, dev), count, G)
    want = M.count_add(start, bits)
    assert np.array_equal(count.cpu().numpy(), want)
    for value in (0, 1, 254, 255):                    # every preloaded value met both a 0 and a 1
        assert (bits[start == value]).any() and (~bits[start == value]).any()
    assert want[(start == 255) & bits].max() == 255 and want[(start == 254) & bits].min() == 255
    for min_count in (1, 2, 255):
        out = torch.full((CELLS // 32,), 0x77777777, dtype=torch.int32, device=dev)
        capi.call("occ_count_bits", count, min_count, out, G)
        assert torch.equal(out.cpu(), _words(want >= min_count, dev).cpu())
        assert 0 < (want >= min_count).sum() < CELLS


# ---- 5. soundness --------------------------------------------------------------------------------------

def test_every_train_sample_lies_in_the_default_carve(host, capi, dev, sc, tables):
    """step / 2 <= 4 / G, dilate = 1, n_steps = ceil(1.5 S): zero exceptions"""
    opts = host.VisibilityOptions(resolution=G, n_steps=M.N_STEPS, step=STEP, dilate=1)
    vis = host.camera_visibility(tables[12], tables["K"], H, W, opts, tables["dist"])
    plain = host.camera_visibility(
        tables[12], tables["K"], H, W,
        host.VisibilityOptions(resolution=G, n_steps=M.N_STEPS, step=STEP, dilate=0), tables["dist"])
    S = M.S_TRAIN
    n = H * W
    ij = torch.from_numpy(M.walked_pixels(H, W, 1)).to(dev)
    total, outside, outside_plain = 0, 0, 0
    g = torch.Generator().manual_seed(11)
    for cam in range(3):
        cam_idx = torch.full((n,), cam, dtype=torch.int32, device=dev)
        o, d = torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev)
        capi.call("gen_rays_dist", tables[12], 12, tables["K"], tables["dist"], 3, cam_idx, ij, 0, 1, o, d, n)
        noise = (torch.rand(n, S, generator=g) + 0.5).to(dev)
        pts = torch.empty(n * S, 3, device=dev)
        dirs, dt, t = torch.empty_like(pts), torch.empty(n * S, device=dev), torch.empty(n * S, device=dev)
        bounds = torch.zeros(n, 2, dtype=torch.int32, device=dev)
        capi.call("sample_rays", o, d, noise, pts, dirs, dt, t, bounds, n, S, STEP)
        assert bool(torch.isfinite(pts).all())
        for words, name in ((vis, "dilated"), (plain, "plain")):
            out = torch.empty(n * S, dtype=torch.uint8, device=dev)
            capi.call("occ_lookup", pts, n * S, words, G, out)
            miss = int((out == 0).sum())
            if name == "dilated":
                outside += miss
            else:
                outside_plain += miss
        total += n * S
    print("TRAIN samples %d, outside the carve %d, outside without dilation %d" % (total, outside, outside_plain))
    assert total == 46080
    assert outside == 0


# ---- 6. the host functions -------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [0, 1, 2])
@pytest.mark.parametrize("rows,mask_kind,stride", [(12, "none", 1), (16, "scattered", 3)])
def test_view_counts_and_visibility_against_the_model(host, capi, dev, sc, tables, d, rows, mask_kind, stride):
    n_steps = 96
    mask = MASKS[mask_kind]
    pm = None if mask is None else host.PixelMask.from_mask(torch.from_numpy(mask).to(dev))
    mk = lambda mv: host.VisibilityOptions(resolution=G, pixel_stride=stride, n_steps=n_steps, step=STEP,
                                           min_views=mv, dilate=d)
    args = (tables[rows], tables["K"], H, W)
    counts = host.camera_view_counts(*args, mk(1), tables["dist"], pm)
    assert counts.dtype == torch.uint8 and tuple(counts.shape) == (G, G, G)
    got = counts.cpu().numpy().reshape(-1)
    # the model's composition on the marks of the kernel chain: exact
    marks = [_chain_marks(capi, dev, tables, c, n_steps, stride, mask_kind) for c in range(3)]
    want = M.view_counts(marks, G, d)
    assert np.array_equal(got, want)
    assert want.max() == 3 or d == 0 and want.max() >= 2
    # the numpy model from end to end: between the counts of its sure and its maybe marks
    bounds = [M.camera_mark_bounds(sc, c, G, n_steps, STEP, stride, None if mask is None else mask[c])
              for c in range(3)]
    lo, hi = M.view_counts([b[0] for b in bounds], G, d), M.view_counts([b[1] for b in bounds], G, d)
    assert (lo <= got).all() and (got <= hi).all()
    assert (lo != hi).mean() < 0.02
    for mv in (1, 2, 3):
        words = host.camera_visibility(*args, mk(mv), tables["dist"], pm)
        assert words.dtype == torch.int32 and tuple(words.shape) == (CELLS // 32,)
        assert torch.equal(words.cpu(), _words(want >= mv, dev).cpu()), mv
    # min_views = 1 took the single launch; the per-camera route says the same
    one = host.camera_visibility(*args, mk(1), tables["dist"], pm)
    assert torch.equal(one.cpu(), _words(M.dilate(np.logical_or.reduce(marks), G, d), dev).cpu())
    assert 0 < (want >= 2).sum() < (want >= 1).sum()


def test_host_checks(host, dev, tables):
    args = (tables[12], tables["K"], H, W)
    ok = host.VisibilityOptions(resolution=32, n_steps=8, step=0.25, dilate=1)      # 1/8 <= 1/8
    assert tuple(host.camera_visibility(*args, ok).shape) == (CELLS // 32,)
    with pytest.raises(RuntimeError, match="half a step"):
        host.camera_visibility(*args, host.VisibilityOptions(resolution=32, n_steps=8, step=0.26, dilate=1))
    with pytest.raises(RuntimeError, match="half a step"):
        host.camera_view_counts(*args, host.VisibilityOptions(resolution=256, n_steps=8, step=1.0 / 16, dilate=2))
    host.camera_visibility(*args, host.VisibilityOptions(resolution=32, n_steps=8, step=0.26, dilate=0))
    for bad in (dict(resolution=48), dict(dilate=3), dict(dilate=-1), dict(min_views=0), dict(min_views=256),
                dict(pixel_stride=0), dict(n_steps=0), dict(n_steps=65537), dict(step=0.0),
                dict(step=float("nan"))):
        with pytest.raises(RuntimeError):
            host.camera_visibility(*args, host.VisibilityOptions(**{"resolution": 32, "step": STEP, **bad}))
    wrong = host.PixelMask.from_mask(torch.ones(2, H, W, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="mask"):
        host.camera_visibility(*args, ok, None, wrong)
    o = host.VisibilityOptions()
    assert (o.resolution, o.pixel_stride, o.n_steps, o.min_views, o.dilate) == (128, 1, -1, 1, 1)
    assert o.step == 1.0 / 256
    # n_steps = -1: ceil(1.5 * 1024) samples of the default sampler, not its 1024 (at a step of 1/1024
    # the two reach 1.5 and 1.0 from the camera)
    vo = lambda **kw: host.VisibilityOptions(resolution=32, dilate=0, step=1.0 / 1024, **kw)
    a = host.camera_visibility(*args, vo(), tables["dist"])
    assert torch.equal(a, host.camera_visibility(*args, vo(n_steps=1536), tables["dist"]))
    assert not torch.equal(a, host.camera_visibility(*args, vo(n_steps=1024), tables["dist"]))


# ---- 7. the grid's allowed mask ------------------------------------------------------------------------------

def test_grid_allowed_mask(host, capi, dev, tables):
    oracle, hr, o, d, noise, bg, gt, emb = _setup(host, 8, 2, 14, 64, 4.0 / 64, 96, 3.0, 11)
    field = hr.scene_field
    opts = host.VisibilityOptions(resolution=G, n_steps=M.N_STEPS, step=STEP)
    allowed = host.camera_visibility(tables[12], tables["K"], H, W, opts, tables["dist"])
    allowed_b = torch.from_numpy(_unpack(allowed)).reshape(G, G, G).to(dev)
    assert 0.02 < float(allowed_b.float().mean()) < 0.9

    probe = host.OccupancyGrid(G, str(dev))
    probe.update(field, 0.0, 0.95)
    thr = float(probe.density().median())

    plain, carved = host.OccupancyGrid(G, str(dev)), host.OccupancyGrid(G, str(dev))
    assert carved.allowed() is None
    carved.set_allowed(allowed)
    assert torch.equal(carved.allowed(), allowed) and carved.allowed().data_ptr() != allowed.data_ptr()
    # at once: a fresh grid is all ones, so its bits are the mask
    assert torch.equal(carved.words, allowed) and torch.equal(carved.bits(), allowed_b)
    assert abs(carved.fraction() - float(allowed_b.float().mean())) < 1e-6
    for g in (plain, carved):
        g.update(field, thr, 0.95)
    assert torch.equal(carved.words, plain.words & allowed)
    assert torch.equal(carved.density(), plain.density())
    assert torch.equal(carved.bits(), plain.bits() & allowed_b)
    assert 0 < int(carved.bits().sum()) < int(plain.bits().sum())
    assert bool((plain.bits() & ~allowed_b).any())                  # the mask took something away

    # set_bits is ANDed as well
    rnd = torch.rand(G, G, G, generator=torch.Generator().manual_seed(1)) < 0.5
    carved.set_bits(rnd.to(dev))
    assert torch.equal(carved.bits(), rnd.to(dev) & allowed_b)
    assert torch.equal(carved.words.cpu(), _pack(rnd.reshape(-1)) & allowed.cpu())

    # carve_to_cameras is set_allowed(camera_visibility) at the grid's own resolution
    other = host.OccupancyGrid(G, str(dev))
    other.carve_to_cameras(tables[16], tables["K"], H, W,
                           host.VisibilityOptions(resolution=128, n_steps=M.N_STEPS, step=STEP), tables["dist"])
    assert torch.equal(other.allowed(), allowed) and torch.equal(other.words, allowed)

    # the render routes see the effective bits: the same outputs as a plain grid holding that AND
    carved.update(field, thr, 0.95)
    twin = host.OccupancyGrid(G, str(dev))
    twin.set_bits(carved.bits())
    assert twin.allowed() is None and torch.equal(twin.words, carved.words)
    to = lambda v: v.to(dev)
    outs = {}
    for name, grid in (("carved", carved), ("twin", twin), ("plain", plain)):
        hr.set_occupancy(grid)
        with torch.no_grad():
            outs[name] = tuple(hr.render(to(o), to(d), to(emb), "validate", None, to(bg))) + \
                tuple(hr.render_rays(to(o), to(d), to(emb), "validate", None, to(bg)))
    for a, b in zip(outs["carved"], outs["twin"]):
        assert torch.equal(a, b)
    assert not torch.equal(outs["carved"][3], outs["plain"][3])      # the carve is in use
    hr.set_occupancy(None)

    # clearing the mask and updating restores the plain grid
    carved.clear_allowed()
    assert carved.allowed() is None
    for g in (plain, carved):
        g.update(field, thr, 0.95)
    assert torch.equal(carved.words, plain.words) and torch.equal(carved.density(), plain.density())

    with pytest.raises(RuntimeError, match="set_allowed"):
        carved.set_allowed(allowed[:-1])
    with pytest.raises(RuntimeError, match="set_allowed"):
        carved.set_allowed(allowed.float())
