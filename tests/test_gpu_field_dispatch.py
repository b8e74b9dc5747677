"""Every kernel entry that walks the hash grid, once per instantiation its launch dispatcher
(csrc/kernels/field_dispatch.hiph) can pick: F in {1, 2, 4, 8} x T in {4096, 5000}, and for the one-pass
render family all 30 (C, F, POW2) triples.  A power-of-two kernel handed T = 5000 would mask with 4999
and read other rows, an F mix-up would read rows of the wrong width: both are gross errors against the
expectation each entry's own test already uses, which is the one applied here, with its tolerance:

  f2n_hash_fwd, f2n_hash_fwd_raytile     bit-exact to the oracle's hash_fwd          (test_gpu_ops)
  f2n_hash_bwd (atomic, sliced), _binned the exact integer sums, element by element  (test_gpu_ops)
  f2n_hash_rays_grad                     the oracle's composition, 5e-2 / 2e-3       (test_gpu_pose_grad)
  f2n_occ_update                         the oracle's hash forward + f64 chain       (test_gpu_occupancy)
  f2n_density_march[_occ]                the oracle's first pass                     (test_gpu_fused)
  f2n_render_rays[_head, _tail]          kept and len the march's; colours and depths at 1e-4

Shapes: 9 rays (one full group of eight plus one) of S = 128 samples (two 64-sample strides), a head of
64 samples, 9 * 128 points; L = C / F for the family and 4 elsewhere.  f2n_hash_bwd_binned refuses
fewer than 65536 points, so it runs on exactly that many.

The field is the oracle's (oracle.ref_render), drawn for 2^13 rows per level and then told to wrap at T:
the C++ Renderer only has tables of 2^k rows, so for the colours the one-pass entries are held directly
to what the existing routes are themselves held to at 1e-4 -- the oracle's Renderer.render."""
import functools

import numpy as np
import pytest
import torch

from oracle import kernels as K
from oracle import ref_render as R
from tests import util
from tests.test_gpu_fused import _oracle_first_pass
from tests.test_gpu_occupancy import (_expected_density, _gap_threshold, _march, _march_occ, _pack,
                                      _probe_points)
from tests.test_gpu_ops import _assert_hash_values, _binned_launch, _check
from tests.test_gpu_pose_grad import _oracle_rays_grad
from tests.test_gpu_render import _close
from tests.test_gpu_render_rays import _render_rays_raw
from tests.test_gpu_render_rays_head import _head_raw

pytestmark = pytest.mark.gpu

N_RAYS, S, STEP, N_HEAD = 9, 128, 4.0 / 128, 64
N = N_RAYS * S
LOG2_POOL = 13                                   # rows per level the pool is drawn for: both T fit
FT = [(F, T) for F in (1, 2, 4, 8) for T in (4096, 5000)]
TRIPLES = [(C, F, T) for C in (8, 16, 32, 64) for F in (1, 2, 4, 8) if C // F <= 32 for T in (4096, 5000)]
assert len(TRIPLES) == 30


@functools.lru_cache(maxsize=2)
def _oracle(L, F, T):
    """The oracle's renderer over a field that wraps its rows at T, and its rays (TRAIN inputs)."""
    g = torch.Generator().manual_seed(100 * L + 10 * F)
    torch.manual_seed(100 * L + F)
    oracle = R.Renderer(5, L=L, F=F, log2_T=LOG2_POOL, S=S, step=STEP, gen=g, feat_init="trained")
    assert T <= oracle.scene_field.T
    oracle.scene_field.T = T                     # (level_stride stays 2^13 elements: quirk Q2's overlap)
    o = torch.randn(N_RAYS, 3, generator=g) * 0.25
    d = torch.randn(N_RAYS, 3, generator=g)
    noise = torch.rand(N_RAYS, S, generator=g) - 0.5 + 1.0
    bg = torch.rand(N_RAYS, 3, generator=g)
    img = torch.randint(0, 5, (N_RAYS,), generator=g).to(torch.int32)
    return oracle, o, d, noise, bg, img


def _field(oracle):
    """util.make_field's dictionary for the oracle's field (CPU tensors)."""
    fld = oracle.scene_field
    table = fld.feat_pool.detach().reshape(-1).contiguous()
    return dict(L=fld.L, F=fld.F, T=fld.T, stride=fld.level_stride, table=table, numel=table.numel(),
                table16=K.cast_f16(table), primes=fld.prim_pool, bias=fld.bias_pool.detach(), mul=fld.mul)


def _on(dev, fld, oracle):
    """... and test_gpu_occupancy._raw_field's: device tensors and the density head."""
    f = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in fld.items()}
    mlp = oracle.scene_field.mlp
    f["w0"] = mlp.weight.detach()[0].contiguous().to(dev)
    f["b0"] = mlp.bias.detach()[0:1].clone().to(dev)
    return f


def _network(dev, oracle):
    """test_gpu_render_rays._raw_network's dictionary for the oracle's parameters."""
    sh = oracle.shader.mlp
    net = dict(w_h=oracle.scene_field.mlp.weight, b_h=oracle.scene_field.mlp.bias, w1=sh[0].weight,
               b1=sh[0].bias, w2=sh[2].weight, b2=sh[2].bias, emb=oracle.app_emb)
    return {k: v.detach().clone().contiguous().to(dev) for k, v in net.items()}


def _set_bias0(oracle, b):
    with torch.no_grad():
        oracle.scene_field.mlp.bias[0] = b


# ---- entries without a C: L = 4 ----------------------------------------------------------------------

@pytest.mark.parametrize("F,T", FT)
def test_hash_forward_entries(capi, dev, F, T):
    L = 4
    fld = _field(_oracle(L, F, T)[0])
    pts = util.ball_points(N, seed=F)
    ref = K.hash_fwd(pts, fld["table16"], fld["primes"], fld["bias"], fld["mul"], L, F, T, fld["stride"])
    d = [v.to(dev) for v in (pts, fld["table16"], fld["primes"], fld["bias"], fld["mul"])]
    out = torch.full((N, L * F), 7.0, device=dev)
    capi.call("hash_fwd", *d, out, L * F, 1, None, N, L, F, T, fld["stride"])
    _assert_hash_values(out.cpu(), ref)
    for tile in (0, 16):                          # 32 samples per tile (S % 32 == 0), and 16
        with capi.option("RAYTILE", tile):
            out_cm = torch.full((L * F, N), 7.0, device=dev)
            capi.call("hash_fwd_raytile", *d, out_cm, N_RAYS, S, L, F, T, fld["stride"])
        _assert_hash_values(out_cm.t().contiguous().cpu(), ref)


@pytest.mark.parametrize("F,T", FT)
def test_hash_backward_entries(capi, dev, F, T):
    L = 4
    fld = _field(_oracle(L, F, T)[0])
    g = torch.Generator().manual_seed(4 + F)
    for n, routes in ((N, ("atomic", "atomic+points", "sliced")), (65536, ("binned",))):
        pts = util.ball_points(n, seed=6)
        grad = torch.randn(n, L * F, generator=g) * 1e-3
        grad[torch.rand(n, L * F, generator=g) < 0.2] = 0.0
        sums = K.hash_bwd_exact(pts, fld["primes"], fld["bias"], fld["mul"], grad, L, F, T, 128.0)
        ex = util.table_grad_expectation(*sums, L, F, T, fld["stride"], 128.0, fld["numel"])
        d = [v.to(dev) for v in (pts, fld["table16"], fld["primes"], fld["bias"], fld["mul"], grad)]
        for route in routes:
            tg = torch.zeros(fld["numel"], device=dev)
            if route == "binned":
                c = _binned_launch(capi, dev, fld, pts, grad, L, F, T, 128.0, tg)
                _check("binned", tg.cpu(), ex, exact=True, max_inexact=c * F)
                continue
            pg = torch.full((n, 3), 7.0, device=dev) if route == "atomic+points" else None
            with capi.option("HASH_BWD", 2 if route == "sliced" else 1):
                capi.call("hash_bwd", *d, L * F, 1, tg, pg, n, L, F, T, fld["stride"], 128.0)
            _check("forced-" + route, tg.cpu(), ex)
            if pg is not None:                    # as test_hash_bwd_parity holds the point gradient
                _, ref_pg = K.hash_bwd(pts, fld["table16"], fld["primes"], fld["bias"], fld["mul"], grad,
                                       fld["numel"], L, F, T, fld["stride"], 128.0, need_pts_grad=True)
                assert (pg.cpu() - ref_pg).abs().max().item() <= 1e-5 * ref_pg.abs().max().item() + 1e-12


@pytest.mark.parametrize("F,T", FT)
def test_hash_rays_grad_entry(capi, dev, F, T):
    L = 4
    oracle, o, d, *_ = _oracle(L, F, T)
    fld = _field(oracle)
    gen = torch.Generator().manual_seed(3 + F)
    t = torch.rand(N, generator=gen) * 3.0 + 0.01
    ray = torch.arange(N_RAYS).repeat_interleave(S)
    ends = torch.arange(1, N_RAYS + 1, dtype=torch.int32) * S
    bounds = torch.stack([ends - S, ends], 1).contiguous()
    pts = (o[ray] + (d / d.norm(dim=1, keepdim=True))[ray] * t[:, None]).contiguous()
    g = torch.randn(N, L * F, generator=gen) * 5e-3
    to = lambda v: v.to(dev)
    pts_d = to(pts)
    x_d = torch.empty_like(pts_d)
    capi.call("contract_fwd", pts_d, x_d, N)
    ref_o, ref_d = _oracle_rays_grad(fld, L, F, T, o, d, ray, t, pts, x_d.cpu(), g)
    d_o = torch.full((N_RAYS, 3), float("nan"), device=dev)
    d_d = torch.full((N_RAYS, 3), float("nan"), device=dev)
    capi.call("hash_rays_grad", pts_d, to(t), to(bounds), to(d), to(fld["table16"]), to(fld["primes"]),
              to(fld["bias"]), to(fld["mul"]), to(g.t().contiguous()), 1, N, d_o, d_d, N_RAYS, L, F, T,
              fld["stride"], 128.0)
    assert ref_o.abs().max() > 0
    _close(d_o.cpu(), ref_o, 5e-2, 2e-3)
    _close(d_d.cpu(), ref_d, 5e-2, 2e-3)


@pytest.mark.parametrize("F,T", FT)
def test_occ_update_entry(capi, dev, F, T):
    L, G = 4, 32
    oracle = _oracle(L, F, T)[0]
    _set_bias0(oracle, 1.5)
    f = _on(dev, _field(oracle), oracle)
    cells = G ** 3
    centre = np.full((cells, 3), 0.5, dtype=np.float32)
    expected, tol = _expected_density(oracle, _probe_points(G, centre))
    thr = _gap_threshold(expected, tol)
    density = torch.zeros(cells, device=dev)
    words = torch.full((cells // 32,), -1, dtype=torch.int32, device=dev)
    capi.call("occ_update", f["table16"], f["primes"], f["bias"], f["mul"], f["w0"], f["b0"], None,
              density, words, G, L, F, T, f["stride"], 3.0, thr, 0.95)
    got = density.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - expected) <= tol * expected), float(np.max(np.abs(got - expected) / (tol * expected)))
    want = expected > thr
    assert torch.equal(words.cpu(), _pack(torch.from_numpy(want)))
    assert 0.4 < want.mean() < 0.6


@pytest.mark.parametrize("F,T", FT)
def test_march_entries(capi, dev, F, T):
    L = 4
    oracle, o, d, noise, *_ = _oracle(L, F, T)
    _set_bias0(oracle, 4.5)                       # rays stop around the middle of their 128 samples
    num = _oracle_first_pass(oracle.scene_field, o, d, noise, S, STEP)[0]
    assert bool((num < S).any())
    f = _on(dev, _field(oracle), oracle)
    od, dd, nd = o.to(dev), d.to(dev), noise.to(dev)
    got = _march(capi, f, od, dd, nd, S, STEP)
    print("march counts", got.cpu().tolist(), "oracle", num.tolist())
    for route in (1, 2):                          # one and four rays per wavefront: the same additions
        with capi.option("MARCH", route):
            assert torch.equal(_march(capi, f, od, dd, nd, S, STEP), got), route
    words = torch.full((64 ** 3 // 32,), -1, dtype=torch.int32, device=dev)
    kept, length = _march_occ(capi, f, od, dd, nd, S, STEP, words, 64)
    assert torch.equal(kept, got) and torch.equal(length, got)
    # a transmittance within rounding of the threshold may keep one sample more or less
    diff = (got.cpu() - num).abs()
    assert diff.max().item() <= 1, diff.max()
    assert (diff != 0).float().mean().item() <= 0.02


# ---- the one-pass render family: every (C, F, POW2) --------------------------------------------------

@pytest.mark.parametrize("C,F,T", TRIPLES)
def test_one_pass_entries(capi, dev, C, F, T):
    L = C // F
    oracle, o, d, noise, bg, img = _oracle(L, F, T)
    od, dd, nd, bgd, imgd = (v.to(dev) for v in (o, d, noise, bg, img))
    fld = _field(oracle)
    seen = set()
    for bias0 in (4.0, 5.0):                      # rays that outlive the head, rays that stop inside it
        _set_bias0(oracle, bias0)
        f, net = _on(dev, fld, oracle), _network(dev, oracle)
        with torch.no_grad():
            res = oracle.render(o, d, img, R.TRAIN, noise, bg)
        want = _march(capi, f, od, dd, nd, S, STEP)
        seen |= set(want.cpu().tolist())
        whole = _render_rays_raw(capi, f, net, od, dd, nd, S, STEP, img=imgd, bg=bgd)
        split = _head_raw(capi, f, net, od, dd, nd, S, STEP, N_HEAD, img=imgd, bg=bgd)
        for name, (colors, depths, last, kept, length) in (("one launch", whole), ("head + tail", split)):
            assert torch.equal(kept, want) and torch.equal(length, want), (name, bias0)
            _close(colors.cpu(), res.colors, 1e-4)
            _close(depths.cpu(), res.depths, 1e-4)
    print("march counts seen:", sorted(seen))
    assert any(k > N_HEAD for k in seen) and any(k < N_HEAD for k in seen), sorted(seen)
