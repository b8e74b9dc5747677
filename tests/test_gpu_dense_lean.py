"""The lean dense first pass (F2N_OPT_DENSE_LEAN = 0) against the route it replaces (= 1):

  f2n_sample_dense           against f2n_sample_rays + f2n_contract_fwd, bit for bit;
  f2n_shade_*_raydirs        (one direction row per ray) against f2n_shade_*_rays, bit for bit;
  Renderer.render/train_step option 1 against option 0: colours, depths, weights, bounds, kept counts,
                             loss, squared error and the table gradient equal, the network gradients
                             within the bars tests/test_gpu_ray_order.py uses between routes;
  launches                   of one bucketed train_step at var_loss_weight = 0 (torch profiler): no
                             contraction pass, no [n, S] row gather, no fill of n * S floats.

A NaN equals a NaN here and a zero equals a zero of the other sign: everything else is compared with
==, element by element."""
import importlib

import pytest
import torch

from tests.test_gpu_ray_order import F, L, LOG2T, S as S_VIEW, W_IMG, _view
from tests.test_gpu_shade_bwd_waves import _check

pytestmark = pytest.mark.gpu
PAD = 64          # guard elements around every output buffer
FILL = 7.0


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def _same(a, b):
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


class _Guarded:
    """An output buffer pre-filled with 7 and guarded on both sides: `t` is what the kernel gets."""

    def __init__(self, shape, dev, dtype=torch.float32):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * PAD,), FILL, device=dev, dtype=dtype)
        self.t = self.buf[PAD:PAD + n].view(*shape)

    def guards_intact(self):
        return bool((self.buf[:PAD] == FILL).all()) and bool((self.buf[-PAD:] == FILL).all())


# ---- the sampler entry ------------------------------------------------------------------------------

def _rays(n_rays, dev, seed):
    """origins inside the unit ball, directions of any length; from five rays on, ray 2 has a zero
    direction (its samples are NaN in both routes)"""
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n_rays, 3, generator=g) * 0.25
    d = torch.randn(n_rays, 3, generator=g) * 2.0
    if n_rays >= 5:
        d[2] = 0.0
    return o.to(dev), d.to(dev), g


def _row_maps(n_rays, g, dev):
    perm = torch.arange(n_rays)
    if n_rays >= 5:            # a permutation that has fixed points: half the rows moved in a cycle
        moved = torch.randperm(n_rays, generator=g)[: n_rays // 2]
        perm[moved] = moved.roll(1)
        assert 1 <= int((perm == torch.arange(n_rays)).sum()) < n_rays
    rev = torch.empty_like(perm)
    rev[perm] = torch.arange(n_rays)
    return {"none": None, "perm": perm.to(torch.int32).to(dev), "reverse": rev.to(torch.int32).to(dev)}


@pytest.mark.parametrize("S", [1, 63, 64, 65, 128, 192])
@pytest.mark.parametrize("n_rays", [1, 5, 67])
def test_sample_dense_matches_sample_rays_and_contract(capi, dev, n_rays, S):
    step = 4.0 / max(S, 8)
    o, d, g = _rays(n_rays, dev, 100 * n_rays + S)
    u = torch.rand(n_rays, S, generator=g).to(dev)            # the raw uniform draw
    cooked = (u - .5) + 1.                                     # ATen's two passes
    n = n_rays * S
    crossed = False
    for noise_kind in ("none", "cooked", "raw"):
        for map_kind, rows in _row_maps(n_rays, g, dev).items():
            # ---- the two existing entries, on the noise rows in ray order
            nz = None if noise_kind == "none" else (cooked if rows is None else cooked[rows.long()]).contiguous()
            pts, dirs = torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev)
            dt, t = torch.empty(n, device=dev), torch.empty(n, device=dev)
            bounds = torch.empty(n_rays, 2, device=dev, dtype=torch.int32)
            capi.call("sample_rays", o, d, nz, pts, dirs, dt, t, bounds, n_rays, S, step)
            x = torch.empty(n, 3, device=dev)
            capi.call("contract_fwd", pts, x, n)
            # ---- the new entry, on the noise where it lies
            src = None if noise_kind == "none" else (u if noise_kind == "raw" else cooked)
            gx, gdt, gt_ = _Guarded((n, 3), dev), _Guarded((n,), dev), _Guarded((n,), dev)
            gb = _Guarded((n_rays, 2), dev, torch.int32)
            gd = _Guarded((n_rays, 3), dev)
            capi.call("sample_dense", o, d, src, rows, 1 if noise_kind == "raw" else 0, gx.t, gdt.t,
                      gt_.t, gb.t, gd.t, n_rays, S, step)
            tag = (noise_kind, map_kind)
            assert _same(gx.t, x), tag
            assert _same(gdt.t, dt) and _same(gt_.t, t), tag
            assert torch.equal(gb.t, bounds), tag
            assert _same(gd.t.unsqueeze(1).expand(n_rays, S, 3), dirs.view(n_rays, S, 3)), tag
            for buf in (gx, gdt, gt_, gb, gd):
                assert buf.guards_intact(), tag
            r = pts.norm(dim=1)
            crossed = crossed or (bool((r <= 1).any()) and bool((r > 1).any()))
            if n_rays >= 5:
                assert bool(x.view(n_rays, S, 3)[2].isnan().all())     # the zero direction
    if S >= 63:
        assert crossed        # samples on both sides of the contraction radius


def test_sample_dense_on_the_workload_stride_count(capi, dev):
    """More rays than one workgroup takes, two strides per ray, every lane of the last stride valid."""
    n_rays, S, step = 301, 128, 4.0 / 128
    o, d, g = _rays(n_rays, dev, 9)
    u = torch.rand(n_rays, S, generator=g).to(dev)
    rows = torch.randperm(n_rays, generator=g).to(torch.int32).to(dev)
    n = n_rays * S
    pts, dirs = torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev)
    dt, t, x = torch.empty(n, device=dev), torch.empty(n, device=dev), torch.empty(n, 3, device=dev)
    bounds = torch.empty(n_rays, 2, device=dev, dtype=torch.int32)
    capi.call("sample_rays", o, d, ((u - .5) + 1.)[rows.long()].contiguous(), pts, dirs, dt, t, bounds,
              n_rays, S, step)
    capi.call("contract_fwd", pts, x, n)
    gx, gdt, gt_ = _Guarded((n, 3), dev), _Guarded((n,), dev), _Guarded((n,), dev)
    gb, gd = _Guarded((n_rays, 2), dev, torch.int32), _Guarded((n_rays, 3), dev)
    capi.call("sample_dense", o, d, u, rows, 1, gx.t, gdt.t, gt_.t, gb.t, gd.t, n_rays, S, step)
    assert _same(gx.t, x) and _same(gdt.t, dt) and _same(gt_.t, t) and torch.equal(gb.t, bounds)
    assert _same(gd.t.unsqueeze(1).expand(n_rays, S, 3), dirs.view(n_rays, S, 3))
    assert all(b.guards_intact() for b in (gx, gdt, gt_, gb, gd))


# ---- the network entries with one direction row per ray -----------------------------------------------

E = 5
KEYS = ("w_h", "b_h", "w1", "b1", "w2", "b2", "emb")


def _net_inputs(C, n_rays, S, n_img, seed):
    g = torch.Generator().manual_seed(seed)
    n = n_rays * S
    enc = (torch.randn(n, C, generator=g) * 0.1).to(torch.float16).float()
    ray_dirs = torch.randn(n_rays, 3, generator=g)
    ray_dirs = ray_dirs / ray_dirs.norm(dim=1, keepdim=True)
    ray_img = (torch.arange(n_rays) % n_img).to(torch.int32)
    P = {"w_h": torch.randn(16, C, generator=g) * 0.3, "b_h": torch.randn(16, generator=g) * 0.1,
         "w1": torch.randn(64, 32, generator=g) * 0.3, "b1": torch.randn(64, generator=g) * 0.1,
         "w2": torch.randn(3, 64, generator=g) * 0.3, "b2": torch.randn(3, generator=g) * 0.1,
         "emb": torch.randn(E, 16, generator=g) * 0.1}
    return enc, ray_dirs, ray_img, P, torch.randn(n, generator=g), torch.randn(n, 3, generator=g)


def _net_both(capi, dev, C, n_rays, S, n_img, waves):
    """{"raydirs" | "rays": (logit, rgb, [d_enc], G)} under SHADE_BWD_WAVES = waves, and the
    per-sample inputs tests/test_gpu_shade_bwd_waves.py::_check bounds the gradients from"""
    enc, ray_dirs, ray_img, P, d_logit, d_rgb = _net_inputs(C, n_rays, S, n_img, 31 * C + n_rays + S)
    n = n_rays * S
    dv = lambda t: t.to(dev).contiguous()
    dirs = ray_dirs.repeat_interleave(S, 0).contiguous()
    enc_cm, Pd, img_d = dv(enc.t()), {k: dv(v) for k, v in P.items()}, dv(ray_img)
    w = tuple(Pd[k] for k in KEYS)
    dl, dr = dv(d_logit), dv(d_rgb)
    out = {}
    with capi.option("SHADE_BWD_WAVES", waves):
        for entry, dd in (("rays", dv(dirs)), ("raydirs", dv(ray_dirs))):
            logit, rgb = torch.full((n,), FILL, device=dev), torch.full((n, 3), FILL, device=dev)
            capi.call("shade_fwd_" + entry, enc_cm, C, dd, img_d, *w, logit, rgb, n_rays, S)
            d_enc = torch.full((C, n), FILL, device=dev)
            G = {k: torch.zeros_like(v) for k, v in Pd.items()}
            capi.call("shade_bwd_" + entry, enc_cm, C, dd, img_d, *w, dl, dr, d_enc,
                      *(G[k] for k in KEYS), n_rays, S)
            torch.cuda.synchronize()
            out[entry] = (logit, rgb, [d_enc], G)
    inputs = (enc, dirs, ray_img.repeat_interleave(S), P, d_logit, d_rgb, 1)
    return out, inputs


@pytest.mark.parametrize("waves", [1, 2])
def test_raydirs_entries_equal_rays_entries_one_workgroup(capi, dev, waves):
    """4 rays x 64 samples, two image ids: 4 strides of 64 (8 of 32 at two waves), all in one workgroup.
    Every output is the same bit for bit -- with one exception that the kernels themselves set.  The
    waves of a workgroup meet in LDS for the six network gradients, but each adds its share of an
    embedding row with a float atomic of its own: at one wave per SIMD a row gets two addends (a sum
    of two is the same in either order), at two waves per SIMD four, from four waves, in the order the
    hardware takes them.  Two launches of ONE entry differ there in the last bit (measured on an
    MI355X: twenty launches of f2n_shade_bwd_rays on these inputs gave four different d emb at two
    waves and one at one wave; the other six gradients one each), so d emb of the two-wave form is
    held to the bound
    tests/test_gpu_shade_bwd_waves.py sets for reordered float sums."""
    out, inputs = _net_both(capi, dev, 32, 4, 64, 2, waves)
    a, b = out["raydirs"], out["rays"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2][0], b[2][0])
    assert not bool((a[0] == FILL).any()) and not bool((a[2][0] == FILL).any())
    for k in KEYS:
        if k == "emb" and waves == 2:
            continue
        assert torch.equal(a[3][k], b[3][k]), k
        assert bool(a[3][k].any()), k
    res = {"raydirs": (a[2], a[3]), "rays": (b[2], b[3]), "inputs": inputs}
    _check(res, True, arms=("raydirs", "rays"))       # d emb at two waves: the reordered-sum bound
    assert bool(a[3]["emb"][:2].any()) and not bool(a[3]["emb"][2:].any())   # two image ids


def test_raydirs_entries_equal_rays_entries_many_workgroups(capi, dev):
    """300 rays x 128 samples, three image ids: outputs per sample bit for bit, parameter gradients
    (float atomics of many workgroups) within the bound of tests/test_gpu_shade_bwd_waves.py."""
    out, inputs = _net_both(capi, dev, 32, 300, 128, 3, 0)
    a, b = out["raydirs"], out["rays"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    res = {"raydirs": (a[2], a[3]), "rays": (b[2], b[3]), "inputs": inputs}
    _check(res, True, arms=("raydirs", "rays"))       # d_enc torch.equal, gradients within the bound


# ---- through the Renderer: option 1 against option 0 ------------------------------------------------------

N_RAYS = 320
S = S_VIEW


def _renderer(host, opaque):
    host.manual_seed(7)
    ren = host.Renderer(2, n_levels=L, n_channels=F, log2_table=LOG2T, max_samples=S, step=4.0 / S)
    with torch.no_grad():
        p = ren.named_parameters()
        p["scene_field.feat_pool"].normal_(0.0, 0.1)
        if opaque:                       # rays terminate: the exact scan and the compaction run
            p["scene_field.mlp.bias"][0] = 6.0
    ren.set_dense_first_pass(1)
    ren.set_margin_min_samples(0)        # (thin medium: the guess is accepted on the margin flag)
    return ren


@pytest.fixture(scope="module")
def renderers(host):
    return {False: _renderer(host, False), True: _renderer(host, True)}


@pytest.fixture(scope="module")
def chunk(host, dev):
    """320 consecutive rays of one 800-wide image row"""
    o, d = _view(host, dev)
    lo = 300 * W_IMG + 240
    o, d = o[lo:lo + N_RAYS].contiguous(), d[lo:lo + N_RAYS].contiguous()
    g = torch.Generator(device=dev).manual_seed(11)
    noise = torch.rand(N_RAYS, S, device=dev, generator=g) + 0.5
    bg = torch.rand(N_RAYS, 3, device=dev, generator=g)
    gt = torch.rand(N_RAYS, 3, device=dev, generator=g)
    emb = torch.randint(0, 2, (N_RAYS,), device=dev, generator=g, dtype=torch.int32)
    return o, d, emb, noise, bg, gt


def _run(host, capi, ren, chunk, lean_option, var_w, drawn):
    """as tests/test_gpu_ray_order.py::_run; drawn: the renderer draws the noise itself, from the
    same seed before every call"""
    o, d, emb, noise, bg, gt = chunk
    capi.set_option("DENSE_LEAN", lean_option)
    nz = None if drawn else noise
    host.manual_seed(1234)
    ren.render(o, d, emb, "train", nz, bg)             # same renderer state before both routes
    with torch.no_grad():
        host.manual_seed(1234)
        res = [t.clone() for t in ren.render(o, d, emb, "train", nz, bg)]
    ren.zero_grad()
    host.manual_seed(1234)
    loss, sq, nv, ns = ren.train_step(o, d, emb, gt, var_w, nz, bg, True)
    torch.cuda.synchronize()
    grads = {k: v.clone() for k, v in ren.grads().items() if v is not None}
    return res, loss.clone(), sq.clone(), ns, grads


@pytest.mark.parametrize("drawn", [False, True])
@pytest.mark.parametrize("opaque", [False, True])
@pytest.mark.parametrize("var_w", [0.0, 1e-2])
@pytest.mark.parametrize("bucketed", [True, False])
def test_lean_route_matches_parent_route(host, capi, renderers, chunk, bucketed, var_w, opaque, drawn):
    ren = renderers[opaque]
    ren.set_ray_order_min_rays(256 if bucketed else 1 << 30)
    capi.set_option("BWD_PHASES", 1)     # per-chunk table gradient sums independent of the order
    ref = _run(host, capi, ren, chunk, 1, var_w, drawn)
    got = _run(host, capi, ren, chunk, 0, var_w, drawn)
    (c0, d0, w0, i0), loss0, sq0, ns0, g0 = ref
    (c1, d1, w1, i1), loss1, sq1, ns1, g1 = got
    if opaque:
        assert ns0 < N_RAYS * S          # the fall-back (exact scan, compaction) was exercised
    else:
        assert ns0 == N_RAYS * S
    assert ns1 == ns0
    assert torch.equal(i1, i0)
    assert torch.equal(c1, c0) and torch.equal(d1, d0) and torch.equal(w1, w0)
    assert torch.equal(loss1, loss0) and torch.equal(sq1, sq0)
    assert set(g1) == set(g0)
    assert torch.equal(g1["scene_field.feat_pool"], g0["scene_field.feat_pool"])
    assert float(g0["scene_field.feat_pool"].abs().max()) > 0
    for k, want in g0.items():          # network gradients: float atomics, order-dependent sums
        err = float((g1[k] - want).norm()) / (float(want.norm()) + 1e-30)
        assert err <= (5e-5 if k == "app_emb" else 1e-5), (k, err)


def _profiled_train_step(host, capi, ren, chunk, lean_option):
    """one train_step at var_loss_weight = 0 under the torch profiler: ({kernel name: launches},
    [element counts of every tensor an aten::fill_ / aten::zero_ filled])"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile

    o, d, emb, noise, bg, gt = chunk
    capi.set_option("DENSE_LEAN", lean_option)
    ren.render(o, d, emb, "train", noise, bg)          # (the previous chunk kept everything)
    ren.zero_grad()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], record_shapes=True) as prof:
        ren.train_step(o, d, emb, gt, 0.0, noise, bg, True)
        torch.cuda.synchronize()
    kernels, fills = {}, []
    for e in prof.events():
        if e.device_type == DeviceType.CUDA:
            kernels[e.name] = kernels.get(e.name, 0) + 1
        elif e.name in ("aten::fill_", "aten::zero_") and e.input_shapes and e.input_shapes[0]:
            numel = 1
            for dim in e.input_shapes[0]:
                numel *= dim
            fills.append(numel)
    return kernels, fills


def _launches(kernels, *parts):
    return sum(c for name, c in kernels.items() if all(p in name for p in parts))


def test_lean_bucketed_train_step_drops_the_passes(host, capi, renderers, chunk):
    """One bucketed train_step at var_loss_weight = 0, thin medium.  Option 1 shows that the profiler
    sees the passes in question; option 0 runs none of them."""
    ren = renderers[False]
    ren.set_ray_order_min_rays(256)
    n = N_RAYS * S
    old, old_fills = _profiled_train_step(host, capi, ren, chunk, 1)
    assert _launches(old, "sample_rays_kernel") == 1 and _launches(old, "contract_fwd_kernel") == 1
    # [n, S] rows move as float4: the noise, the weights forward, their zero gradient back
    assert _launches(old, "gather_rows_kernel", "float, 4") == 3, sorted(old)
    assert n in old_fills                              # the materialised zero d_weights
    new, new_fills = _profiled_train_step(host, capi, ren, chunk, 0)
    assert _launches(new, "sample_dense_kernel") == 1 and _launches(new, "sample_rays_kernel") == 0
    assert _launches(new, "contract_fwd_kernel") == 0             # no contraction pass
    assert _launches(new, "gather_rows_kernel", "float, 4") == 0  # no gather of [n, S] rows
    assert n not in new_fills and 3 * n not in new_fills           # no fill of n * S floats
    for k in ("hash_fwd_raytile_kernel", "shade_fwd_mfma_rays_kernel", "shade_bwd_mfma_rays_kernel",
              "composite_fwd_kernel", "composite_bwd_kernel", "weight_var_fwd_kernel"):
        assert _launches(new, k) == _launches(old, k) == 1, k     # the kernels that stay: as before
    assert sum(new.values()) < sum(old.values())
