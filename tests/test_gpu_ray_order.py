"""Bucketed dense first pass (F2N_OPT_RAY_ORDER): rays sorted into pixel-compact bundles inside
Renderer::render_fused give the caller-order route's results bit for bit -- colours, depths,
weights, bounds and loss -- and the same gradients (the table's exactly under BWD_PHASES = 1, the
network's up to the order of their float atomics)."""
import importlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

L, F, LOG2T, S = 16, 2, 19, 128
H_IMG = W_IMG = 800
FOCAL = 1111.1
N_RAYS = 65536          # RendererOptions::ray_order_min_rays: bucketed


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def _pose(dev, k=0, n=50):
    """One camera of an arc around the origin looking at it (-z forward, z up)."""
    ang = (-100.0 + 200.0 * k / (n - 1)) * math.pi / 180.0
    pos = torch.tensor([math.cos(ang), math.sin(ang), 0.1], dtype=torch.float64)
    zc = pos / pos.norm()
    xc = torch.linalg.cross(torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64), zc)
    xc = xc / xc.norm()
    yc = torch.linalg.cross(zc, xc)
    return torch.cat([torch.stack([xc, yc, zc], 1), pos.unsqueeze(1)], 1).float().to(dev)


def _view(host, dev):
    intr = torch.tensor([[FOCAL, 0, W_IMG / 2], [0, FOCAL, H_IMG / 2], [0, 0, 1.0]], device=dev)
    return host.get_view_rays(_pose(dev), intr, H_IMG, W_IMG)


def _renderer(host, dev, opaque):
    host.manual_seed(7)
    ren = host.Renderer(2, n_levels=L, n_channels=F, log2_table=LOG2T, max_samples=S, step=4.0 / S)
    with torch.no_grad():
        p = ren.named_parameters()
        p["scene_field.feat_pool"].normal_(0.0, 0.1)
        if opaque:                       # rays terminate: compacted, ragged weights
            p["scene_field.mlp.bias"][0] = 6.0
    ren.set_dense_first_pass(1)
    return ren


def _chunk(host, dev, kind):
    o, d = _view(host, dev)
    g = torch.Generator(device=dev).manual_seed(11)
    if kind == "rows":
        lo = 200 * W_IMG
        o, d = o[lo:lo + N_RAYS], d[lo:lo + N_RAYS]
    else:
        pick = torch.randperm(o.shape[0], device=dev, generator=g)[:N_RAYS]
        o, d = o[pick], d[pick]
    noise = torch.rand(N_RAYS, S, device=dev, generator=g) + 0.5
    bg = torch.rand(N_RAYS, 3, device=dev, generator=g)
    gt = torch.rand(N_RAYS, 3, device=dev, generator=g)
    emb = torch.randint(0, 2, (N_RAYS,), device=dev, generator=g, dtype=torch.int32)
    return o.contiguous(), d.contiguous(), emb, noise, bg, gt


def _run(capi, ren, chunk, route, var_w):
    o, d, emb, noise, bg, gt = chunk
    capi.set_option("RAY_ORDER", route)
    ren.render(o, d, emb, "train", noise, bg)          # same renderer state before both routes
    with torch.no_grad():
        res = [t.clone() for t in ren.render(o, d, emb, "train", noise, bg)]
    ren.zero_grad()
    loss, sq, nv, ns = ren.train_step(o, d, emb, gt, var_w, noise, bg, True)
    torch.cuda.synchronize()
    grads = {k: v.clone() for k, v in ren.grads().items() if v is not None}
    return res, loss.clone(), sq.clone(), ns, grads


@pytest.mark.parametrize("kind,opaque,var_w", [
    ("rows", False, 0.0), ("random", False, 0.0), ("rows", True, 0.0), ("rows", True, 1e-2),
    ("random", True, 1e-2)])
def test_bucketed_route_matches_caller_order(host, capi, dev, kind, opaque, var_w):
    ren = _renderer(host, dev, opaque)
    chunk = _chunk(host, dev, kind)
    capi.set_option("BWD_PHASES", 1)     # per-chunk table gradient sums independent of the order
    ref = _run(capi, ren, chunk, 1, var_w)
    got = _run(capi, ren, chunk, 0, var_w)
    (c0, d0, w0, i0), loss0, sq0, ns0, g0 = ref
    (c1, d1, w1, i1), loss1, sq1, ns1, g1 = got
    if opaque:
        assert ns0 < N_RAYS * S          # the compacted (ragged) route was exercised
    else:
        assert ns0 == N_RAYS * S
    assert ns1 == ns0
    assert torch.equal(i1, i0)
    assert torch.equal(c1, c0) and torch.equal(d1, d0) and torch.equal(w1, w0)
    assert torch.equal(loss1, loss0) and torch.equal(sq1, sq0)
    assert torch.equal(g1["scene_field.feat_pool"], g0["scene_field.feat_pool"])
    assert float(g0["scene_field.feat_pool"].abs().max()) > 0
    for k, want in g0.items():          # network gradients: float atomics, order-dependent sums
        err = float((g1[k] - want).norm()) / (float(want.norm()) + 1e-30)
        # app_emb: two rows, each a float-atomic sum over ~4 M samples
        assert err <= (5e-5 if k == "app_emb" else 1e-5), (k, err)


def test_bucketed_row_chunk_forms_pixel_blobs(host, dev):
    """64 consecutive rays of a sorted 800-wide row chunk: a compact blob, not a 64 x 1 strip."""
    o, d = _view(host, dev)
    lo, n = 200 * W_IMG, 65536
    order = host.ray_order(d[lo:lo + n].contiguous())
    assert order.dtype == torch.int64
    assert torch.equal(order.sort()[0], torch.arange(n, device=dev))      # a permutation
    assert torch.equal(host.ray_order(d[lo:lo + n].contiguous()), order)  # deterministic
    px = (order + lo).cpu()
    rows, cols = (px // W_IMG)[: n // 64 * 64].view(-1, 64), (px % W_IMG)[: n // 64 * 64].view(-1, 64)
    h = (rows.max(1)[0] - rows.min(1)[0] + 1).double()
    w = (cols.max(1)[0] - cols.min(1)[0] + 1).double()
    assert float((h * w).mean()) <= 144.0, (float(h.mean()), float(w.mean()))
    assert float(h.mean()) <= 13.0 and float(w.mean()) <= 13.0


def test_ray_order_ties_keep_caller_order(host, dev):
    d = torch.tensor([[0.1, 0.2, -1.0]], device=dev).repeat(1000, 1)
    assert torch.equal(host.ray_order(d), torch.arange(1000, device=dev))
