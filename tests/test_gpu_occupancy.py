"""The occupancy bitfield on the GPU: the lookup against its f32 cell expression in numpy, the masked
march and compaction against the existing kernels (no tolerance: the same samples, the same scan),
the update pass against the oracle's hash forward, and the Renderer's fused route against its
op-by-op route and the CPU oracle with the same grid attached."""
import importlib
import math

import numpy as np
import pytest
import torch

from oracle import kernels as K
from oracle import ref_render as R
from tests.test_gpu_render import _close, _copy_params, _oracle_grads, _setup
from tests.util import _cells, _pack, _raw_field  # noqa: F401 (other test modules import them from here)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


# ---- helpers -------------------------------------------------------------------------------------

def _expected_mask(x, bits_bool, G):
    """x: contracted points (numpy [n,3]); non-finite coordinates read as occupied."""
    finite = np.isfinite(x).all(axis=1)
    idx = _cells(np.where(finite[:, None], x, 0.0), G)
    return np.where(finite, bits_bool.reshape(-1).numpy()[idx], True)


def _contract(capi, pts):
    x = torch.empty_like(pts)
    capi.call("contract_fwd", pts, x, pts.shape[0])
    return x


def _lookup(capi, pts, words, G):
    out = torch.empty(pts.shape[0], dtype=torch.uint8, device=pts.device)
    capi.call("occ_lookup", pts, pts.shape[0], words, G, out)
    return out


def _rays(n_rays, S, seed, dev, train):
    g = torch.Generator().manual_seed(seed)
    o = (torch.randn(n_rays, 3, generator=g) * 0.25).to(dev)
    d = torch.randn(n_rays, 3, generator=g).to(dev)
    noise = (torch.rand(n_rays, S, generator=g) - 0.5 + 1.0).to(dev) if train else None
    return o, d, noise


def _march(capi, f, o, d, noise, S, step):
    n = o.shape[0]
    kept = torch.full((n,), -1, dtype=torch.int32, device=o.device)
    capi.call("density_march", o, d, noise, f["table16"], f["primes"], f["bias"], f["mul"], f["w0"],
              f["b0"], kept, n, S, step, f["L"], f["F"], f["T"], f["stride"], 1e-4, 3.0)
    return kept


def _march_occ(capi, f, o, d, noise, S, step, words, G):
    n = o.shape[0]
    kept = torch.full((n,), -1, dtype=torch.int32, device=o.device)
    length = torch.full((n,), -1, dtype=torch.int32, device=o.device)
    capi.call("density_march_occ", o, d, noise, f["table16"], f["primes"], f["bias"], f["mul"],
              f["w0"], f["b0"], words, G, kept, length, n, S, step, f["L"], f["F"], f["T"],
              f["stride"], 1e-4, 3.0)
    return kept, length


def _bounds(capi, counts):
    n = counts.shape[0]
    bounds = torch.zeros(n, 2, dtype=torch.int32, device=counts.device)
    total = torch.zeros(1, dtype=torch.int32, device=counts.device)
    capi.call("bounds_from_counts", counts, bounds, total, n)
    return bounds, int(total.item())


def _empty_samples(n, dev):
    return (torch.full((n, 3), float("nan"), device=dev), torch.full((n, 3), float("nan"), device=dev),
            torch.full((n,), float("nan"), device=dev), torch.full((n,), float("nan"), device=dev))


def _sample_all(capi, o, d, noise, S, step):
    n = o.shape[0]
    pts, dirs, dt, t = _empty_samples(n * S, o.device)
    bounds = torch.zeros(n, 2, dtype=torch.int32, device=o.device)
    capi.call("sample_rays", o, d, noise, pts, dirs, dt, t, bounds, n, S, step)
    return pts, dirs, dt, t, bounds


# ---- lookup --------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [32, 128])
def test_lookup_matches_the_cell_expression(capi, dev, G):
    g = torch.Generator().manual_seed(G)
    n = 200000
    pts = torch.randn(n, 3, generator=g) * torch.logspace(-2, 2, n).unsqueeze(1)
    pts[0] = 0.0                                   # |p| = 0 contracts to NaN (quirk Q6)
    pts[1] = torch.tensor([1e6, -2e6, 3e5])        # far outside: close to the sphere of radius 2
    pts[2] = torch.tensor([0.0, 0.0, 1.0])         # on the unit sphere
    norm = pts.norm(dim=1)
    assert (norm < 1).sum() > n // 10 and (norm > 1).sum() > n // 10
    bits = torch.rand(G ** 3, generator=g) < 0.5
    words = _pack(bits).to(dev)
    d_pts = pts.to(dev)
    got = _lookup(capi, d_pts, words, G).cpu().numpy().astype(bool)
    x = _contract(capi, d_pts).cpu().numpy()
    assert np.isnan(x[0]).all()
    want = _expected_mask(x, bits, G)
    assert np.array_equal(got, want)
    assert got[0]                                  # the origin reads occupied
    assert 0.3 < got.mean() < 0.7                  # the random bitfield is actually consulted
    # the same answers from the bound class
    H = importlib.import_module("f2-nerf_amd").load_host()
    grid = H.OccupancyGrid(G, str(dev))
    grid.set_bits(bits.reshape(G, G, G).to(dev))
    assert torch.equal(grid.words.cpu(), words.cpu())
    assert torch.equal(grid.bits().cpu().reshape(-1), bits)
    assert np.array_equal(grid.occupied(d_pts).cpu().numpy(), want)
    assert abs(grid.fraction() - float(bits.float().mean())) < 1e-6


# ---- an all-ones grid is today's march -----------------------------------------------------------

@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("L,F,T,S,step,bias0", [
    (16, 2, 1 << 19, 1024, 1.0 / 256, 8.0),    # reference sampler, terminating
    (16, 2, 1 << 19, 1024, 1.0 / 256, 0.0),    # dense: nothing terminates
    (16, 2, 1 << 19, 128, 4.0 / 128, 6.0),     # S = 128, terminating
    (8, 8, 1 << 14, 128, 4.0 / 128, 0.0),      # F = 8, dense
    (8, 8, 5000, 1024, 1.0 / 256, 7.0),        # F = 8, T not a power of two
    (8, 2, 5000, 100, 0.04, 6.0),              # S not a multiple of 64, T not a power of two
])
def test_all_ones_grid_is_the_plain_march(capi, dev, L, F, T, S, step, bias0, train):
    n_rays = 300
    f = _raw_field(L, F, T, bias0, seed=L + S, dev=dev)
    o, d, noise = _rays(n_rays, S, seed=S + F, dev=dev, train=train)
    G = 64
    words = torch.full((G ** 3 // 32,), -1, dtype=torch.int32, device=dev)
    ref = _march(capi, f, o, d, noise, S, step)
    with capi.option("MARCH", 1):
        assert torch.equal(_march(capi, f, o, d, noise, S, step), ref)
    kept, length = _march_occ(capi, f, o, d, noise, S, step, words, G)
    assert torch.equal(kept, ref) and torch.equal(length, ref)
    if bias0 >= 6.0:
        assert bool((ref < S).any())
    else:
        assert bool((ref == S).all())
    bounds, n_kept = _bounds(capi, ref)
    a = _empty_samples(n_kept, dev)
    capi.call("sample_compact", o, d, noise, bounds, *a, n_rays, S, step)
    b = _empty_samples(n_kept, dev)
    capi.call("sample_compact_occ", o, d, noise, bounds, length, words, G, *b, n_rays, S, step)
    for x, y, name in zip(a, b, ("pts", "dirs", "dt", "t")):
        assert not bool(torch.isnan(x).any()), name
        assert torch.equal(x, y), name


# ---- random and structured grids against the existing kernels ------------------------------------

def _grid_bits(kind, G, o, d, noise, S, step, capi, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        return torch.rand(G ** 3, generator=g) < 0.5
    if kind == "empty":
        return torch.zeros(G ** 3, dtype=torch.bool)
    c = (torch.arange(G, dtype=torch.float32) + 0.5) * (4.0 / G) - 2.0
    cz, cy, cx = torch.meshgrid(c, c, c, indexing="ij")
    if kind == "box":  # a solid box off the origin: rays enter and leave it
        inside = (cx > 0.1) & (cx < 1.1) & (cy > -0.9) & (cy < 0.7) & (cz > -0.5) & (cz < 1.3)
        return inside.reshape(-1)
    assert kind == "one_cell"  # the cell of sample 20 of ray 0
    pts = _sample_all(capi, o, d, noise, S, step)[0]
    x = _contract(capi, pts[20:21].contiguous()).cpu().numpy()
    bits = torch.zeros(G ** 3, dtype=torch.bool)
    bits[int(_cells(x, G)[0])] = True
    return bits


@pytest.mark.parametrize("kind", ["random", "box", "empty", "one_cell"])
@pytest.mark.parametrize("L,F,T,S,step,bias0,train,G", [
    (16, 2, 1 << 19, 1024, 1.0 / 256, 8.0, True, 128),   # terminating
    (16, 2, 1 << 19, 1024, 1.0 / 256, 0.0, False, 128),  # dense, VALIDATE
    (8, 8, 5000, 128, 4.0 / 128, 6.0, True, 32),         # F = 8, T not a power of two
    (8, 2, 1 << 14, 100, 0.04, 6.0, True, 64),           # S not a multiple of 64
])
def test_masked_march_and_compaction_against_the_existing_kernels(
        capi, dev, kind, L, F, T, S, step, bias0, train, G):
    n_rays = 200
    f = _raw_field(L, F, T, bias0, seed=3 * L + S, dev=dev)
    o, d, noise = _rays(n_rays, S, seed=S + F + 1, dev=dev, train=train)
    bits = _grid_bits(kind, G, o, d, noise, S, step, capi, seed=G + S)
    words = _pack(bits).to(dev)

    # the restatement: dt zeroed where the mask is 0, then the existing encode + scan
    pts, dirs, dt, t, _ = _sample_all(capi, o, d, noise, S, step)
    n_all = n_rays * S
    mask = _lookup(capi, pts, words, G).bool()
    dt_masked = torch.where(mask, dt, torch.zeros_like(dt))
    x = _contract(capi, pts)
    C = L * F
    enc_cm = torch.empty(C, n_all, device=dev)
    capi.call("hash_fwd", x, f["table16"], f["primes"], f["bias"], f["mul"], enc_cm, 1, n_all, None,
              n_all, L, F, T, f["stride"])
    assert bool(torch.isfinite(enc_cm).all())
    want_len = torch.full((n_rays,), -1, dtype=torch.int32, device=dev)
    capi.call("density_scan", enc_cm, C, dt_masked, f["w0"], f["b0"], want_len, n_rays, S, 1e-4, 3.0)
    k = torch.arange(S, device=dev).unsqueeze(0)
    sel = mask.reshape(n_rays, S) & (k < want_len.unsqueeze(1))
    want_kept = sel.sum(1).to(torch.int32)

    kept, length = _march_occ(capi, f, o, d, noise, S, step, words, G)
    assert torch.equal(length, want_len)
    assert torch.equal(kept, want_kept)
    if kind == "empty":
        assert int(kept.sum()) == 0 and bool((length == S).all())   # every ray is empty
    elif kind == "one_cell":
        assert int(kept[0]) >= 1 and int(kept.sum()) < n_rays * 8
    else:
        assert 0 < int(kept.sum()) < int(length.sum())               # the grid does thin the list
    if kind == "random" and bias0 >= 6.0:
        # rays run further than without a grid: half their samples carry no density
        assert int(length.sum()) > int(_march(capi, f, o, d, noise, S, step).sum())

    bounds, n_kept = _bounds(capi, kept)
    assert n_kept == int(sel.sum())
    got = _empty_samples(n_kept, dev)
    capi.call("sample_compact_occ", o, d, noise, bounds, length, words, G, *got, n_rays, S, step)
    flat = sel.reshape(-1)
    for a, b, name in zip(got, (pts[flat], dirs[flat], dt[flat], t[flat]), ("pts", "dirs", "dt", "t")):
        assert torch.equal(a, b), name


# ---- update --------------------------------------------------------------------------------------

def _probe_points(G, u):
    """x = ((float)c + u) * (4.f / G) - 2.f per axis in f32; rows in bit-index order, u [G^3, 3]."""
    c = np.arange(G, dtype=np.float32)
    cz, cy, cx = np.meshgrid(c, c, c, indexing="ij")
    cell = np.stack([cx.reshape(-1), cy.reshape(-1), cz.reshape(-1)], 1).astype(np.float32)
    return (cell + u.astype(np.float32)) * np.float32(4.0 / G) - np.float32(2.0)


def _expected_density(oracle, x):
    """sigma = exp(w0 . f16(enc(x)) + b0 - 3): the oracle's hash forward (bit-exact features), the FMA
    chain in level order through float64 (each product exact, one rounding per step)."""
    fld = oracle.scene_field
    enc = K.hash_fwd(torch.from_numpy(x), K.cast_f16(fld.feat_pool.detach().reshape(-1)), fld.prim_pool,
                     fld.bias_pool.detach(), fld.mul, fld.L, fld.F, fld.T, fld.level_stride).numpy()
    w0 = fld.mlp.weight.detach()[0].numpy().astype(np.float32)
    logit = np.full(x.shape[0], fld.mlp.bias.detach()[0].item(), dtype=np.float32)
    for c in range(enc.shape[1]):
        logit = (enc[:, c].astype(np.float64) * np.float64(w0[c]) + logit.astype(np.float64)).astype(np.float32)
    arg = (logit - np.float32(3.0)).astype(np.float32)
    # the device expf's last bits plus the rounding of its argument, which exp turns into a relative
    # error of the result
    tol = 4.0 * 2.0 ** -24 * np.maximum(1.0, np.abs(arg.astype(np.float64)))
    return np.exp(arg.astype(np.float64)), tol


def _gap_threshold(expected, tol):
    """Midpoint of the widest relative gap between neighbouring sorted densities around the median
    (the central 1/16 of the cells): no cell is within rounding of it."""
    order = np.argsort(expected)
    s = expected[order]
    n = s.shape[0]
    lo, hi = n // 2 - n // 32, n // 2 + n // 32
    rel = (s[lo + 1:hi + 1] - s[lo:hi]) / s[lo:hi]
    j = lo + int(np.argmax(rel))
    thr = 0.5 * (s[j] + s[j + 1])
    # derived precondition, not a tuned one: the gap is wider than both neighbours' error bars
    assert s[j + 1] * (1 - tol[order[j + 1]]) > np.float32(thr) > s[j] * (1 + tol[order[j]])
    return float(np.float32(thr))


@pytest.mark.parametrize("G,L,F,log2_T", [(32, 16, 2, 19), (64, 8, 4, 12)])
def test_update_matches_oracle(host, dev, G, L, F, log2_T):
    oracle, hr, *_ = _setup(host, L, F, log2_T, 64, 4.0 / 64, 4, 1.5, seed=G + L)
    field = hr.scene_field
    rng = np.random.default_rng(G)
    cells = G ** 3
    centre = np.full((cells, 3), 0.5, dtype=np.float32)
    exp1, tol1 = _expected_density(oracle, _probe_points(G, centre))
    thr1 = _gap_threshold(exp1, tol1)

    grid = host.OccupancyGrid(G, str(dev))
    assert bool(grid.bits().all())                       # fresh: all ones
    grid.update(field, thr1, 0.95)
    d1 = grid.density().cpu().numpy().reshape(-1).astype(np.float64)
    assert np.all(np.abs(d1 - exp1) <= tol1 * exp1), float(np.max(np.abs(d1 - exp1) / (tol1 * exp1)))
    want1 = exp1 > thr1
    assert np.array_equal(grid.bits().cpu().numpy().reshape(-1), want1)
    assert 0.4 < want1.mean() < 0.6                      # the threshold sits at the median
    assert abs(grid.fraction() - want1.mean()) < 1e-6

    # two runs give the same density and bits
    again = host.OccupancyGrid(G, str(dev))
    again.update(field, thr1, 0.95)
    assert torch.equal(again.density(), grid.density()) and torch.equal(again.words, grid.words)

    # a second pass with a supplied probe offset: density = max(density * decay, sigma)
    u = rng.random((cells, 3), dtype=np.float32)
    u = np.minimum(u, np.float32(1.0 - 2.0 ** -24))
    exp_s2, tol2 = _expected_density(oracle, _probe_points(G, u))
    decay = np.float32(0.98)
    prev = grid.density().cpu().numpy().reshape(-1)
    decayed = (prev * decay).astype(np.float32).astype(np.float64)   # one exact-or-rounded f32 product
    exp2 = np.maximum(decayed, exp_s2)
    # a decayed value is reproduced exactly (unless the fresh density is within rounding of it)
    tol2 = np.where(decayed >= exp_s2 * (1 + tol2), 0.0, tol2)
    thr2 = _gap_threshold(exp2, np.maximum(tol2, 2.0 ** -24))
    probe = torch.from_numpy(u).reshape(G, G, G, 3).to(dev)
    grid.update(field, thr2, float(decay), probe)
    d2 = grid.density().cpu().numpy().reshape(-1).astype(np.float64)
    assert np.all(np.abs(d2 - exp2) <= tol2 * exp2 + 0.0)
    assert (decayed >= exp_s2).mean() > 0.05 and (decayed < exp_s2).mean() > 0.05   # both arms of the max
    assert np.array_equal(grid.bits().cpu().numpy().reshape(-1), exp2 > thr2)


# ---- Renderer: fused against op-by-op, both with the same grid -----------------------------------

def _scene_grid(host, dev, G, kind, seed):
    g = torch.Generator().manual_seed(seed)
    c = (torch.arange(G, dtype=torch.float32) + 0.5) * (4.0 / G) - 2.0
    cz, cy, cx = torch.meshgrid(c, c, c, indexing="ij")
    r = (cx * cx + cy * cy + cz * cz).sqrt()
    if kind == "shell":      # empty around the cameras, a shell of matter, empty far field
        bits = (r > 0.35) & (r < 1.2)
    else:                    # half the cells at random
        bits = torch.rand(G, G, G, generator=g) < 0.5
    grid = host.OccupancyGrid(G, str(dev))
    grid.set_bits(bits.to(dev))
    return grid


def _train_step_grads(hr, dev, o, d, emb, gt, noise, bg, vw):
    to = lambda v: v.to(dev)
    hr.zero_grad()
    colors, depths, weights, idx = hr.render(to(o), to(d), to(emb), "train", to(noise), to(bg))
    out = [v.detach().clone() for v in (colors, depths, weights, idx)]
    hr.zero_grad()
    loss, sq, n_val, n_samp = hr.train_step(to(o), to(d), to(emb), to(gt), vw, to(noise), to(bg), True)
    grads = {k: v.clone() for k, v in hr.grads().items() if v is not None}
    return out, float(loss), n_samp, grads


def _assert_standing_bars(got, ref):
    """bounds exact, colours / depths / weights / loss 1e-4 relative, MLP and
    embedding gradients 1e-3 relative + 1e-4 of the maximum absolute, table gradient rel-L2 < 1e-4."""
    (g_out, g_loss, g_n, g_grads), (r_out, r_loss, r_n, r_grads) = got, ref
    assert torch.equal(g_out[3], r_out[3]), "bounds differ"
    assert g_n == r_n
    for a, b in zip(g_out[:3], r_out[:3]):
        _close(a, b, 1e-4)
    assert abs(g_loss - r_loss) <= 1e-4 * abs(r_loss)
    assert set(g_grads) == set(r_grads)
    for k, rg in r_grads.items():
        if float(rg.abs().max()) == 0:
            assert float(g_grads[k].abs().max()) == 0, k
        elif k.endswith("feat_pool"):
            rel = float((g_grads[k] - rg).norm() / rg.norm())
            assert rel < 1e-4, (k, rel)
        else:
            _close(g_grads[k], rg, 1e-3, 1e-4)


@pytest.mark.parametrize("kind", ["shell", "random"])
@pytest.mark.parametrize("L,F,log2_T,S,step,n_rays,bias0,seed", [
    (16, 2, 19, 1024, 1.0 / 256, 512, 5.0, 31),   # the C4 shape: 512 rays x 1024 samples of 1/256
    (8, 2, 14, 64, 4.0 / 64, 96, 3.0, 11),        # a smaller one
])
def test_train_step_fused_against_op_by_op_with_grid(
        host, dev, kind, L, F, log2_T, S, step, n_rays, bias0, seed):
    oracle, hr, o, d, noise, bg, gt, emb = _setup(host, L, F, log2_T, S, step, n_rays, bias0, seed)
    vw = 1e-2
    runs = {}
    for with_grid in (False, True):
        hr.set_occupancy(_scene_grid(host, dev, 128, kind, seed) if with_grid else None)
        for fused in (False, True):
            hr.set_fused(fused)
            hr.set_dense_first_pass(0)
            runs[with_grid, fused] = _train_step_grads(hr, dev, o, d, emb, gt, noise, bg, vw)
    # the seeds are valid: the same comparison without a grid is exact in its bounds
    assert torch.equal(runs[False, True][0][3], runs[False, False][0][3])
    print("kept samples: no grid %d, grid %d" % (runs[False, True][2], runs[True, True][2]))
    assert 0 < runs[True, True][2] < runs[False, True][2] or kind == "random"
    assert not torch.equal(runs[True, True][0][3], runs[False, True][0][3])   # the grid is in use
    _assert_standing_bars(runs[True, True], runs[True, False])


def test_grid_never_takes_the_dense_route(host, dev):
    """dense_first_pass = 1 and the adaptive choice both yield to the grid: the render is the march's."""
    oracle, hr, o, d, noise, bg, gt, emb = _setup(host, 8, 2, 14, 64, 4.0 / 64, 96, -8.0, 17)
    to = lambda v: v.to(dev)
    hr.set_occupancy(_scene_grid(host, dev, 64, "shell", 1))
    outs = []
    for dense in (0, 1, -1, -1):
        hr.set_dense_first_pass(dense)
        outs.append(hr.render(to(o), to(d), to(emb), "train", to(noise), to(bg)))
        assert 0 < hr.last_n_samples < 96 * 64
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)


def test_validate_render_all_rays_with_grid(host, dev):
    oracle, hr, o, d, noise, bg, gt, emb = _setup(host, 16, 2, 19, 1024, 1.0 / 256, 1000, 5.0, 23)
    to = lambda v: v.to(dev)
    hr.set_occupancy(_scene_grid(host, dev, 128, "shell", 2))
    res = {}
    for fused in (False, True):
        hr.set_fused(fused)
        with torch.no_grad():
            res[fused] = hr.render_all_rays(to(o), to(d), 256)
            res[fused] += tuple(hr.render(to(o), to(d), None, "validate"))
    assert torch.equal(res[True][5], res[False][5])          # bounds
    for i in (0, 1, 2, 3, 4):
        _close(res[True][i], res[False][i], 1e-4)
    # render_all_rays = the chunks of render
    assert torch.equal(res[True][0][:256], hr.render(to(o[:256]), to(d[:256]), None, "validate")[0])


def test_fused_ray_grad_against_op_by_op_with_grid(host, dev):
    """Pose optimisation renders the same scene on both routes.  (The op-by-op route samples rays that
    carry a gradient with ATen ops, whose positions differ from the sampler kernel's in the last bit;
    a batch this size has no sample within that distance of a cell face.)"""
    oracle, hr, o, d, noise, bg, gt, emb = _setup(host, 8, 2, 14, 64, 4.0 / 64, 24, 3.0, 11)
    to = lambda v: v.to(dev)
    hr.set_occupancy(_scene_grid(host, dev, 64, "shell", 3))
    hr.set_dense_first_pass(0)
    got = {}
    for fused in (False, True):
        hr.set_fused_ray_grad(fused)
        o_g, d_g = to(o).requires_grad_(True), to(d).requires_grad_(True)
        colors, depths, weights, idx = hr.render(o_g, d_g, None, "validate")
        (colors.square().sum() + depths.sum() * 0.1).backward()
        got[fused] = (colors.detach(), depths.detach(), weights.detach(), idx, o_g.grad, d_g.grad)
    assert torch.equal(got[True][3], got[False][3])
    for i in (0, 1, 2):
        _close(got[True][i], got[False][i], 1e-4)
    # the bars of tests/test_gpu_pose_grad.py::test_fused_ray_grad_matches_oracle
    _close(got[True][4], got[False][4], 5e-2, 2e-3)
    _close(got[True][5], got[False][5], 5e-2, 2e-3)
    assert float(got[True][5].abs().max()) > 0


# ---- op-by-op with a grid against the CPU oracle on the explicit subset --------------------------

def _oracle_render_subset(oracle, o, d, emb, noise, bg, occupied):
    """src/renderer.cpp:58-118 with the density of unoccupied samples set to zero and those samples
    dropped: the oracle's own per-sample and compositing functions on the subset.  occupied: bool
    [n_rays * S] as the kernels see it."""
    n_rays, S = o.shape[0], oracle.S
    pts, dirs, dt, t, bounds = R.get_samples(o, d, noise, S, oracle.step)
    with torch.no_grad():
        feat = oracle.scene_field.query(pts)
        sec = oracle.density_act(feat[:, 0:1])[:, 0] * dt * occupied.to(dt.dtype)
        acc = R.flex_accumulate_sum(sec, bounds, False)
        mask = (torch.exp(-acc) > 1e-4) & occupied
    sel = torch.where(mask)[0]
    pts2, dirs2, dt2, t2 = pts[sel].contiguous(), dirs[sel].contiguous(), dt[sel].contiguous(), t[sel].contiguous()
    num = mask.reshape(n_rays, S).sum(1)
    cum = torch.cumsum(num, 0)
    idx = torch.stack([cum - num, cum], -1).to(torch.int32).contiguous()
    feat = oracle.scene_field.query(pts2)
    density = oracle.density_act(feat[:, 0:1])
    shading = torch.cat([torch.ones_like(feat[:, 0:1]), feat[:, 1:]], 1)
    shading = R.ScatterAddFunc.apply(oracle.app_emb, K.scatter_idx(pts2.shape[0], idx, emb), shading)
    rgb = oracle.shader.query(shading, dirs2)
    sec = density[:, 0] * dt2
    alphas = 1.0 - torch.exp(-sec)
    weights = torch.exp(-R.flex_accumulate_sum(sec, idx, False)) * alphas
    last = torch.exp(-R.flex_sum(sec, idx))
    colors = R.flex_sum(weights.unsqueeze(-1) * rgb, idx) + last.unsqueeze(-1) * bg
    depths = R.flex_sum(weights * (t2 + 1e-2), idx) / (1.0 - last + 1e-4)
    return colors, depths, weights, idx


@pytest.mark.parametrize("L,F,log2_T,S,step,bias0,seed", [
    (16, 2, 19, 1024, 1.0 / 256, 7.0, 7 + 1024),   # the shape and seed of test_train_step_matches_oracle
    (16, 2, 19, 128, 4.0 / 128, 5.0, 7 + 128),
])
def test_op_by_op_with_grid_matches_oracle_on_the_subset(host, capi, dev, L, F, log2_T, S, step, bias0, seed):
    n_rays, vw = 48, 1e-2
    oracle, hr, o, d, noise, bg, gt, emb = _setup(host, L, F, log2_T, S, step, n_rays, bias0, seed)
    grid = _scene_grid(host, dev, 128, "shell", seed)
    to = lambda v: v.to(dev)
    # the mask the kernels see: the lookup on the sampler kernel's points
    pts = _sample_all(capi, to(o), to(d), to(noise), S, step)[0]
    occupied = grid.occupied(pts).cpu()
    colors, depths, weights, idx = _oracle_render_subset(oracle, o, d, emb, noise, bg, occupied)
    color_loss = torch.sqrt((colors - gt).square() + 1e-4).mean()
    var_loss = (R.weight_var(weights, idx) + 1e-2).sqrt().mean()
    loss = color_loss + var_loss * vw
    loss.backward()
    ref_grads = {k: v for k, v in _oracle_grads(oracle).items() if v is not None}
    ref = ([colors.detach(), depths.detach(), weights.detach(), idx], float(loss), weights.numel(), ref_grads)
    hr.set_occupancy(grid)
    for fused in (False, True):
        hr.set_fused(fused)
        hr.set_dense_first_pass(0)
        out, h_loss, n_samp, grads = _train_step_grads(hr, dev, o, d, emb, gt, noise, bg, vw)
        got = ([v.cpu() for v in out], h_loss, n_samp,
               {k: v.cpu() for k, v in grads.items() if k in ref_grads})
        _assert_standing_bars(got, ref)
    assert 0 < weights.numel() < int(occupied.numel())


# ---- off means off -------------------------------------------------------------------------------

@pytest.mark.parametrize("dense", [0, 1])
def test_detached_grid_changes_nothing(host, dev, dense):
    oracle, hr, o, d, noise, bg, gt, emb = _setup(host, 16, 2, 19, 128, 4.0 / 128, 200, 5.0, 5)
    hr2 = host.Renderer(7, n_levels=16, n_channels=2, log2_table=19, max_samples=128, step=4.0 / 128)
    _copy_params(oracle, hr2)
    to = lambda v: v.to(dev)
    hr2.set_occupancy(_scene_grid(host, dev, 64, "shell", 9))
    hr2.set_dense_first_pass(dense)
    with_grid = hr2.render(to(o), to(d), to(emb), "train", to(noise), to(bg))
    hr2.set_occupancy(None)
    assert hr2.occupancy is None
    for r in (hr, hr2):
        r.set_dense_first_pass(dense)
        r.set_speculate_dense(False)
    a = _train_step_grads(hr, dev, o, d, emb, gt, noise, bg, 1e-2)
    b = _train_step_grads(hr2, dev, o, d, emb, gt, noise, bg, 1e-2)
    assert not torch.equal(with_grid[3], a[0][3])       # the grid did something while attached
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    assert a[1] == b[1] and a[2] == b[2]
    assert torch.equal(a[3]["scene_field.feat_pool"] != 0, b[3]["scene_field.feat_pool"] != 0)


# ---- rows only skipped samples touch get exactly zero gradient -----------------------------------

def test_rows_of_skipped_samples_get_zero_gradient(host, capi, dev):
    L, F, log2_T, S, step = 4, 2, 19, 64, 4.0 / 64
    oracle, hr, o, d, noise, bg, gt, emb = _setup(host, L, F, log2_T, S, step, 64, 2.0, 3)
    grid = _scene_grid(host, dev, 64, "shell", 4)
    to = lambda v: v.to(dev)
    fld = hr.scene_field
    pts = _sample_all(capi, to(o), to(d), to(noise), S, step)[0]
    n_all = pts.shape[0]
    x = _contract(capi, pts)
    enc = torch.empty(n_all, L * F, device=dev)
    rows = torch.zeros(n_all, L, 8, dtype=torch.int32, device=dev)
    capi.call("hash_fwd", x, fld.table_f16(), fld.prim_pool, fld.bias_pool, fld.level_mul, enc, L * F, 1,
              rows, n_all, L, F, fld.local_size, fld.level_stride)
    hr.set_occupancy(grid)
    hr.set_dense_first_pass(0)
    for fused in (True, False):
        hr.set_fused(fused)
        out, loss, n_samp, grads = _train_step_grads(hr, dev, o, d, emb, gt, noise, bg, 1e-2)
        idx = out[3]
        # which samples were rendered: the occupied ones inside each ray's prefix; their rows
        occupied = grid.occupied(pts).reshape(64, S)
        kept = (idx[:, 1] - idx[:, 0]).to(torch.int64)
        rank = occupied.to(torch.int64).cumsum(1)
        used = (occupied & (rank <= kept.unsqueeze(1))).reshape(-1)
        assert int(used.sum()) == n_samp and 0 < n_samp < n_all
        elem = (rows.to(torch.int64) & 0xFFFFFFFF) * F \
            + (torch.arange(L, device=dev) * fld.level_stride).view(1, L, 1)
        touched = torch.zeros(fld.feat_pool.numel(), dtype=torch.bool, device=dev)
        for k in range(F):
            touched[(elem[used] + k).reshape(-1)] = True
        g = grads["scene_field.feat_pool"].reshape(-1)
        assert int((g != 0).sum()) > 0
        assert float(g[~touched].abs().max()) == 0.0       # exactly zero, not small
        skipped_only = torch.zeros_like(touched)
        for k in range(F):
            skipped_only[(elem[~used] + k).reshape(-1)] = True
        skipped_only &= ~touched
        assert int(skipped_only.sum()) > 0                  # such rows exist in this batch
