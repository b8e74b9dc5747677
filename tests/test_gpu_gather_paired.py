"""The paired gather of f2n_hash_fwd_raytile (F2N_OPT_GATHER_PAIRED = 0: a sample's 8 corner rows are
loaded in vertex-parity order and brought back to corner order before the blend) against the corner
order it replaces (= 1) and against the oracle: the same bits for every input.

The inputs are chosen so that a wrong slot, a wrong un-permute or a wrong parity cannot pass:
  table     every row of a level holds its own values (row index -> bit pattern), so two rows
            exchanged change the output instead of cancelling;
  lattice   points one cell of level 0 apart, half a cell off the vertices, the cell of point
            (ray, sample) chosen from ray + sample: any 8 consecutive rays at one sample index, and
            any 8 consecutive samples of one ray, hold all 8 parity classes, so in every wave
            instruction every slot carries a different corner per lane -- for every walk;
  ball      raw points out to |p| = 3, contracted by f2n_contract_fwd, one of them NaN;
  level 1   a bias so negative that most coordinates saturate to cell 0 (parity 0), the rest not.

Through the Renderer: one bucketed train_step on 320 rays x 128, option 1 against option 0.

The density chain of the march and of the one-pass render takes the same option: the march's counts
(all three lane mappings, with and without a grid) and every output of f2n_render_rays and of
f2n_render_rays_head / _tail are the same under both values, on 67 rays, S in {63, 64, 65, 128}, a thin
and a terminating medium."""
import importlib

import pytest
import torch

from oracle import kernels as K
from tests.test_gpu_dense_lean import N_RAYS, S as S_REN, _Guarded, _renderer, _view, W_IMG
from tests.test_gpu_occupancy import _march, _march_occ, _pack, _raw_field, _rays
from tests.test_gpu_render_rays import _raw_network, _render_rays_raw
from tests.test_gpu_render_rays_head import WHOLE, _head_raw

pytestmark = pytest.mark.gpu

L = 4
LOG2T = 12
RAYS = (1, 5, 64, 67)
SAMPLES = (16, 32, 48, 128)
ROUTES = [(tile, walk) for tile in (16, 32) for walk in (1, 2, 3)]


def _field(F, T):
    """L disjoint levels of T rows; channel k of row r of level l has the f16 bit pattern
    0x2000 + (5 r + 977 k + 131 l) mod 2^14: finite, positive (2^-7 .. 2^9), and since 5 is odd the
    rows of a level differ from each other in every channel."""
    g = torch.Generator().manual_seed(F * 7 + T)
    r = torch.arange(T).view(1, T, 1)
    k = torch.arange(F).view(1, 1, F)
    lv = torch.arange(L).view(L, 1, 1)
    table16 = (0x2000 + (5 * r + 977 * k + 131 * lv) % 16384).to(torch.int16).reshape(-1).contiguous()
    assert len({tuple(row) for row in table16[:T * F].view(T, F).tolist()}) == T
    primes = torch.tensor([[1, 805459861, 673348561], [295478839, 805459861, 673348561],
                           [1, 295478839, 951274213], [951274213, 1, 295478839]],
                          dtype=torch.int32)
    # level 0: the lattice's level, cell 1/8, integer bias: the cell of x = (i + .5) / 8 is i + 100
    # level 1: pt = 16 x - 6: negative (cell 0) for x < 3/8, up to cell 25 for contracted x near 2
    mul = torch.tensor([8.0, 16.0, 64.0, 1024.0])
    bias = torch.rand(L, 3, generator=g) * 1000.0 + 100.0
    bias[0] = 100.0
    bias[1] = -6.0
    return dict(table16=table16, primes=primes, bias=bias, mul=mul, stride=T * F)


def _lattice(n_rays, S):
    ray = torch.arange(n_rays).view(n_rays, 1).expand(n_rays, S)
    smp = torch.arange(S).view(1, S).expand(n_rays, S)
    c = ray + smp

    def axis(lo_bit, hi_bit):      # cells -2 .. 1: the parity from one low bit of ray + sample
        return (((c >> lo_bit) & 1) + 2 * ((c >> hi_bit) & 1) - 2).float()

    cell = torch.stack([axis(2, 3), axis(1, 4), axis(0, 5)], 2)          # x = bit 2, y = bit 1, z = bit 0
    return ((cell + 0.5) / 8.0).reshape(-1, 3).contiguous()              # inside the unit ball


def _ball(capi, dev, n, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=g)
    raw = d / d.norm(dim=1, keepdim=True) * (torch.rand(n, 1, generator=g) * 3.0)
    raw[n // 2] = float("nan")
    raw = raw.to(dev).contiguous()
    x = torch.empty_like(raw)
    capi.call("contract_fwd", raw, x, n)
    nrm = raw.norm(dim=1)
    assert n < 64 or (bool((nrm > 1).any()) and bool((nrm <= 1).any()))
    return x


def _no_nan(t):
    return torch.nan_to_num(t, nan=7777.0, posinf=8888.0, neginf=-8888.0)


@pytest.mark.parametrize("pow2", [True, False])
@pytest.mark.parametrize("F", [1, 2, 4, 8])
def test_paired_gather_equals_corner_order_and_oracle(capi, dev, F, pow2):
    T = (1 << LOG2T) if pow2 else (1 << LOG2T) - 16
    fld = _field(F, T)
    d_fld = [fld[k].to(dev) for k in ("table16", "primes", "bias", "mul")]
    for n_rays in RAYS:
        for S in SAMPLES:
            n = n_rays * S
            for kind in ("lattice", "ball"):
                pts = _lattice(n_rays, S).to(dev) if kind == "lattice" else _ball(capi, dev, n, n + F)
                host_pts = pts.cpu()
                if kind == "lattice" and n_rays >= 8:
                    # the premise: at level 0 all 8 parity classes among 8 neighbouring rays / samples
                    cell = torch.floor(host_pts * 8.0 + 100.0).long().view(n_rays, S, 3)
                    m = 4 * (cell[..., 0] & 1) + 2 * (cell[..., 1] & 1) + (cell[..., 2] & 1)
                    assert sorted(m[:8, 0].tolist()) == sorted(m[0, :8].tolist()) == list(range(8))
                if kind == "ball" and n >= 64:
                    p1 = host_pts * 16.0 - 6.0
                    assert bool((p1 < 0).any()) and bool((p1 >= 1).any())     # level 1: both sides
                ref = K.hash_fwd(host_pts, fld["table16"], fld["primes"], fld["bias"], fld["mul"], L, F,
                                 T, fld["stride"])
                ref = _no_nan(ref.t().contiguous().to(dev))                   # [L * F, n]
                if kind == "ball":
                    assert bool((ref[:, n // 2] == 7777.0).all())             # the NaN point
                for tile, walk in ROUTES:
                    got = {}
                    for order in (1, 0):
                        out = _Guarded((L * F, n), dev)
                        with capi.option("RAYTILE", tile), capi.option("RAYTILE_WALK", walk), \
                                capi.option("GATHER_PAIRED", order):
                            capi.call("hash_fwd_raytile", pts, *d_fld, out.t, n_rays, S, L, F, T,
                                      fld["stride"])
                        assert out.guards_intact(), (n_rays, S, kind, tile, walk, order)
                        got[order] = out.t
                    tag = (n_rays, S, kind, tile, walk)
                    assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32)), tag
                    assert torch.equal(_no_nan(got[1]), ref), tag
                    assert torch.equal(_no_nan(got[0]), ref), tag


# ---- through the Renderer ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def _train_step(host, capi, ren, chunk, order):
    o, d, emb, noise, bg, gt = chunk
    with capi.option("GATHER_PAIRED", order), capi.option("BWD_PHASES", 1):
        ren.render(o, d, emb, "train", noise, bg)          # same renderer state before both routes
        with torch.no_grad():
            colors = ren.render(o, d, emb, "train", noise, bg)[0].clone()
        ren.zero_grad()
        loss, sq, nv, ns = ren.train_step(o, d, emb, gt, 1e-2, noise, bg, True)
        torch.cuda.synchronize()
    return colors, loss.clone(), sq.clone(), ns, ren.grads()["scene_field.feat_pool"].clone()


def test_train_step_is_the_same_under_both_orders(host, capi, dev):
    ren = _renderer(host, False)
    ren.set_ray_order_min_rays(256)                        # bucketed
    o, d = _view(host, dev)
    lo = 300 * W_IMG + 240
    o, d = o[lo:lo + N_RAYS].contiguous(), d[lo:lo + N_RAYS].contiguous()
    g = torch.Generator(device=dev).manual_seed(11)
    noise = torch.rand(N_RAYS, S_REN, device=dev, generator=g) + 0.5
    bg = torch.rand(N_RAYS, 3, device=dev, generator=g)
    gt = torch.rand(N_RAYS, 3, device=dev, generator=g)
    emb = torch.randint(0, 2, (N_RAYS,), device=dev, generator=g, dtype=torch.int32)
    chunk = (o, d, emb, noise, bg, gt)
    c1, loss1, sq1, ns1, g1 = _train_step(host, capi, ren, chunk, 1)
    c0, loss0, sq0, ns0, g0 = _train_step(host, capi, ren, chunk, 0)
    assert ns0 == ns1 == N_RAYS * S_REN
    assert torch.equal(loss0, loss1) and torch.equal(sq0, sq1)
    assert torch.equal(c0, c1)
    assert torch.equal(g0, g1) and float(g0.abs().max()) > 0


# ---- the density chain: the march and the one-pass render ---------------------------------------------


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("L,F,T", [(16, 2, 1 << 19), (8, 8, 5000)])
@pytest.mark.parametrize("bias0", [0.0, 8.0])            # nothing terminates / two or three samples kept
@pytest.mark.parametrize("S", [63, 64, 65, 128])
def test_march_and_one_pass_render_are_the_same_under_both_orders(capi, dev, S, bias0, L, F, T):
    n_rays, step = 67, 4.0 / S
    f = _raw_field(L, F, T, bias0, seed=S + L, dev=dev)
    net = _raw_network(f, seed=S + F, dev=dev)
    o, d, noise = _rays(n_rays, S, seed=S + 3, dev=dev, train=True)
    img = torch.randint(0, 5, (n_rays,), generator=torch.Generator().manual_seed(S)).to(torch.int32).to(dev)
    G = 64
    c = (torch.arange(G, dtype=torch.float32) + 0.5) * (4.0 / G) - 2.0
    cz, cy, cx = torch.meshgrid(c, c, c, indexing="ij")
    r = (cx * cx + cy * cy + cz * cz).sqrt()
    shell = _pack(((r > 0.35) & (r < 1.2)).reshape(-1)).to(dev)
    res = {}
    for order in (1, 0):
        with capi.option("GATHER_PAIRED", order):
            out = []
            for lanes in (0, 1, 2):                          # 8, 64 and 16 lanes to a ray
                with capi.option("MARCH", lanes):
                    out.append(_march(capi, f, o, d, noise, S, step))
            out += list(_march_occ(capi, f, o, d, noise, S, step, shell, G))
            out += list(_render_rays_raw(capi, f, net, o, d, noise, S, step, img=img))
            out += list(_render_rays_raw(capi, f, net, o, d, noise, S, step, shell, G, img=img))
            for n_head in [WHOLE] + ([64] if S > 64 else []):
                out += list(_head_raw(capi, f, net, o, d, noise, S, step, n_head, img=img))
                out += list(_head_raw(capi, f, net, o, d, noise, S, step, n_head, shell, G, img=img))
        res[order] = out
    assert len(res[0]) == len(res[1])
    for i, (a, b) in enumerate(zip(res[0], res[1])):
        assert torch.equal(_bits(a), _bits(b)), i
    kept = res[0][0]
    assert torch.equal(res[0][1], kept) and torch.equal(res[0][2], kept)
    if bias0 == 0.0:
        assert bool((kept == S).all())
    else:
        assert bool((kept < 8).all()) and int(kept.min()) >= 1
    assert bool(torch.isfinite(res[0][5]).all())             # colours of the render without a grid
