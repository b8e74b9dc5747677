"""hash_fwd_raytile_kernel_groups: one workgroup takes a ray tile through a group of consecutive levels.
Whatever the groups, the output is f2n_hash_fwd's -- the per-point kernel that tests/test_gpu_ops.py
holds bit-exact to the oracle -- in every bit, through both entries:

  f2n_hash_fwd_raytile_groups   under an explicit mask (bit l set: level l opens a group),
  f2n_hash_fwd_raytile          under F2N_OPT_RAYTILE = 0, which takes the default mask.

Shapes: F in {1, 2, 4, 8}; T a power of two and odd; the reference's overlapping level stride and a
disjoint one; L in {1, 2, 5, 16}; n_rays in {1, 63, 64, 65, 130} (tail rays, a second ray tile); S in
{16, 32, 48, 96} (16-sample tiles, 32-sample tiles, several tiles per ray).  Masks: every level alone,
one group of all levels, the defaults for few and for many tiles, {0-2} {3} {4-...} (a group of three
levels and more brings both result tiles round again; a group of one level follows a longer one) and
a last group of one level.
Points: raw points out to |p| = 3 contracted on the device, with a NaN point and a point at the origin;
for the walks, 130 neighbouring pixels of a view with jittered steps (the rule sorts them by depth),
the same un-jittered (across) and random rays (along) -- the test evaluates the kernel's rule on the
first tile and asserts that it chooses that way.  A NaN equals a NaN; everything else is compared
with ==.  Every output is guarded on both sides."""
import importlib

import pytest
import torch

from tests.test_gpu_dense_lean import N_RAYS, S as S_REN, _Guarded, _launches, _profiled_train_step, \
    _renderer, _view, W_IMG

pytestmark = pytest.mark.gpu

LOG2T = 12
LEVELS = (1, 2, 5, 16)
RAYS = (1, 63, 64, 65, 130)
SAMPLES = (16, 32, 48, 96)


def _field(L, F, T, stride, dev):
    """L levels of T rows, level l at element l * stride; element e of the pool has the f16 bit pattern
    0x2000 + (5 e) mod 2^14 (finite, 2^-7 .. 2^9): neighbouring rows and neighbouring levels differ, with
    overlapping windows too.  Level 1 (where there is one) has a bias of -6: most coordinates saturate
    to cell 0 there, the rest do not."""
    g = torch.Generator().manual_seed(L * 131 + F * 7 + T)
    numel = stride * (L - 1) + T * F
    table16 = (0x2000 + (5 * torch.arange(numel)) % 16384).to(torch.int16).contiguous()
    primes = (torch.randint(1 << 28, 1 << 30, (L, 3), generator=g) | 1).to(torch.int32)
    primes[0, 0] = 1
    mul = torch.tensor([2.0 ** (7.0 * l / max(L - 1, 1) + 3.0) for l in range(L)])
    bias = torch.rand(L, 3, generator=g) * 1000.0 + 100.0
    if L > 1:
        bias[1] = -6.0
    return [t.to(dev) for t in (table16, primes, bias, mul)]


def _ball(capi, dev, n, seed):
    """raw points out to |p| = 3 through f2n_contract_fwd; then one NaN point and one at the origin"""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=g)
    raw = (d / d.norm(dim=1, keepdim=True) * (torch.rand(n, 1, generator=g) * 3.0)).to(dev).contiguous()
    x = torch.empty_like(raw)
    capi.call("contract_fwd", raw, x, n)
    nrm = raw.norm(dim=1)
    assert n < 64 or (bool((nrm > 1).any()) and bool((nrm <= 1).any()))
    x[n // 2] = float("nan")
    if n > 2:
        x[1] = 0.0
    return x


def _no_nan(t):
    return torch.nan_to_num(t, nan=7777.0, posinf=8888.0, neginf=-8888.0)


def _default_mask(capi, L, tiles):
    return int(capi.lib().cdll.f2n_hash_raytile_default_groups(L, tiles))


def _masks(capi, L):
    """{what: mask}, without repeats (at L = 1 they are all the one mask)"""
    named = {"alone": (1 << L) - 1, "one group": 1, "default, many tiles": _default_mask(capi, L, 4096),
             "default, few tiles": _default_mask(capi, L, 1),
             "0-2, 3, 4-": 1 | ((1 << 3) if L > 3 else 0) | ((1 << 4) if L > 4 else 0),
             "last alone": 1 | (1 << (L - 1))}
    out = {}
    for what, m in named.items():
        if m not in out.values():
            out[what] = m
    return out


def _reference(capi, pts, fld, n, L, F, T, stride):
    ref = torch.empty(L * F, n, device=pts.device)
    capi.call("hash_fwd", pts, *fld, ref, 1, n, None, n, L, F, T, stride)
    return _no_nan(ref)


def _check_entries(capi, dev, pts, fld, ref, n_rays, S, L, F, T, stride, masks, tag):
    n = n_rays * S
    out = _Guarded((L * F, n), dev)
    capi.call("hash_fwd_raytile", pts, *fld, out.t, n_rays, S, L, F, T, stride)
    assert out.guards_intact(), tag
    assert torch.equal(_no_nan(out.t), ref), (tag, "default route")
    for what, mask in masks.items():
        out = _Guarded((L * F, n), dev)
        capi.call("hash_fwd_raytile_groups", pts, *fld, out.t, n_rays, S, L, F, T, stride, mask)
        assert out.guards_intact(), (tag, what)
        assert torch.equal(_no_nan(out.t), ref), (tag, what, hex(mask))


@pytest.mark.parametrize("pow2", [True, False])
@pytest.mark.parametrize("F", [1, 2, 4, 8])
def test_both_entries_equal_hash_fwd(capi, dev, F, pow2):
    T = (1 << LOG2T) if pow2 else (1 << LOG2T) - 3            # 4096 | 4093
    for stride in (T - T % F, T * F):                         # the reference's (T elements: windows overlap) | disjoint
        for L in LEVELS:
            fld = _field(L, F, T, stride, dev)
            masks = _masks(capi, L)
            assert L < 5 or len(masks) == 6
            for n_rays in RAYS:
                for S in SAMPLES:
                    n = n_rays * S
                    pts = _ball(capi, dev, n, n + F + L)
                    ref = _reference(capi, pts, fld, n, L, F, T, stride)
                    assert bool((ref[:, n // 2] == 7777.0).all())         # the NaN point
                    assert bool((ref != 7777.0).any())
                    _check_entries(capi, dev, pts, fld, ref, n_rays, S, L, F, T, stride, masks,
                                   (stride, L, n_rays, S))
                    with capi.option("RAYTILE", 32):                      # the parent's kernel: the other arm
                        out = _Guarded((L * F, n), dev)
                        capi.call("hash_fwd_raytile", pts, *fld, out.t, n_rays, S, L, F, T, stride)
                    assert out.guards_intact() and torch.equal(_no_nan(out.t), ref), (stride, L, n_rays, S)


# ---- the walks ------------------------------------------------------------------------------------------


def _contracted(p):
    nrm = p.norm(dim=-1, keepdim=True)
    return torch.where(nrm <= 1, p, (2 - 1 / nrm) * p / nrm)


def _view_points(n_rays, S, jitter, seed):
    """n_rays neighbouring pixels of one row of an 800-wide view (focal 1111, camera at (1, 0, 0) looking
    at the origin), S steps of 1/32; jitter: every step scaled by U[0.5, 1.5) as TRAIN does"""
    g = torch.Generator().manual_seed(seed)
    j = (torch.arange(n_rays) + 300).float()
    d = torch.stack([-torch.ones(n_rays), (j - 400) / 1111.1, torch.zeros(n_rays)], 1)
    d = d / d.norm(dim=1, keepdim=True)
    if jitter:
        t = (torch.rand(n_rays, S, generator=g) + 0.5).cumsum(1) / 32.0
    else:
        t = ((torch.arange(S).float() + 0.5) / 32.0).expand(n_rays, S)
    o = torch.tensor([1.0, 0.0, 0.0])
    return _contracted(o + d[:, None, :] * t[:, :, None]).reshape(-1, 3).contiguous()


def _random_ray_points(n_rays, S, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n_rays, 1, 3, generator=g) * 0.3
    d = torch.randn(n_rays, 1, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    t = ((torch.arange(S).float() + 0.5) / 32.0).view(1, S, 1)
    return _contracted(o + d * t).reshape(-1, 3).contiguous()


def _rule(pts, S, ts):
    """the kernel's walk rule on the first tile (64 rays x ts samples): 'along' | 'across' | 'sorted'"""
    p = pts.view(-1, S, 3)[:64, :ts].double()
    m = ts // 2
    dist = lambda ra, sa, rb, sb: float((p[ra, sa] - p[rb, sb]).norm())
    e, e1, sl = dist(63, m, 0, m), dist(1, m, 0, m), dist(0, ts - 1, 0, 0)
    if not e + 8.0 * e1 < 2.0 * sl:
        return "along"
    apart = max(e1, dist(33, m, 32, m), dist(63, m, 62, m))
    return "sorted" if apart * (ts - 1) > 0.35 * sl else "across"


@pytest.mark.parametrize("F", [1, 2, 4, 8])
def test_every_walk_and_both_corner_orders(capi, dev, F):
    T, n_rays = 1 << LOG2T, 130
    for L in (5, 16):
        stride = T * F if L == 5 else T
        fld = _field(L, F, T, stride, dev)
        masks = _masks(capi, L)
        for S, ts in ((96, 32), (48, 16)):
            kinds = {"sorted": _view_points(n_rays, S, True, 3), "across": _view_points(n_rays, S, False, 3),
                     "along": _random_ray_points(n_rays, S, 5)}
            for want, host_pts in kinds.items():
                assert _rule(host_pts, S, ts) == want, (S, want)          # the premise: the rule goes that way
                pts = host_pts.to(dev)
                ref = _reference(capi, pts, fld, n_rays * S, L, F, T, stride)
                for walk in (0, 1, 2, 3):
                    for order in (0, 1):
                        with capi.option("RAYTILE_WALK", walk), capi.option("GATHER_PAIRED", order):
                            _check_entries(capi, dev, pts, fld, ref, n_rays, S, L, F, T, stride, masks,
                                           (L, S, want, walk, order))


# ---- which kernel a route launches ---------------------------------------------------------------------


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def test_routes_launch_one_kernel_each(host, capi, dev):
    ren = _renderer(host, False)
    ren.set_ray_order_min_rays(256)
    o, d = _view(host, dev)
    lo = 300 * W_IMG + 240
    o, d = o[lo:lo + N_RAYS].contiguous(), d[lo:lo + N_RAYS].contiguous()
    g = torch.Generator(device=dev).manual_seed(11)
    noise = torch.rand(N_RAYS, S_REN, device=dev, generator=g) + 0.5
    bg = torch.rand(N_RAYS, 3, device=dev, generator=g)
    gt = torch.rand(N_RAYS, 3, device=dev, generator=g)
    emb = torch.randint(0, 2, (N_RAYS,), device=dev, generator=g, dtype=torch.int32)
    chunk = (o, d, emb, noise, bg, gt)
    new, _ = _profiled_train_step(host, capi, ren, chunk, 0)
    assert _launches(new, "hash_fwd_raytile_kernel_groups<") == 1, sorted(new)
    assert _launches(new, "hash_fwd_raytile_kernel<") == 0, sorted(new)
    with capi.option("RAYTILE", 32):
        old, _ = _profiled_train_step(host, capi, ren, chunk, 0)
    assert _launches(old, "hash_fwd_raytile_kernel<") == 1, sorted(old)
    assert _launches(old, "hash_fwd_raytile_kernel_groups<") == 0, sorted(old)
