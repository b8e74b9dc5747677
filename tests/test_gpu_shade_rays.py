"""Ray-uniform matrix-core network kernels (f2n_shade_fwd_rays / f2n_shade_bwd_rays): a dense
[n_rays, S] grid of samples, S % 64 == 0, where the direction, SH16(dir), the embedding row and the SH
half of the hidden layer are formed once per stride.  Checked against the op-by-op torch-CPU
composition of tests/test_gpu_shade.py with that file's bars, against the per-sample kernels (logit bit
for bit), and through the Renderer (F2N_OPT_SHADE_RAYS = 0 against 1).

Shapes: S = 64 / 128 / 192 gives a new ray every stride, two and three strides per ray (one and a half
to six per ray for the backward's 32-sample strides); 37 rays, every ray its own direction; image ids in
runs that change at ray boundaries.  Seeds are fixed and chosen, by a float64 evaluation on the CPU,
so that no hidden pre-activation lies within 2e-6 of zero: which side of the ReLU a rounding error
lands on is not what these tests measure (2e-6 ~ 32 terms of size <= 1 at 2^-24 each)."""
import functools
import importlib

import pytest
import torch

from oracle import kernels as K
from oracle import ref_render as R

pytestmark = pytest.mark.gpu
EPS = 1e-3
E = 5
IMG_RUNS = [0, 0, 2, 1, 1, 1, 0, 3, 3, 1]     # runs of equal ids and changes, over four images


def _reference(enc, dirs, img, P, d_logit, d_rgb):
    """as tests/test_gpu_shade.py::_reference, in the dtype of its inputs; also the hidden
    pre-activations"""
    enc = enc.clone().requires_grad_(True)
    P = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    h = enc @ P["w_h"].t() + P["b_h"]
    logit = h[:, 0]
    X = torch.cat([torch.ones_like(h[:, :1]), h[:, 1:]], 1)
    if img is not None:
        X = X + P["emb"][img.long()]
    X = torch.cat([X, K.sh_encode(dirs.float(), 4).to(enc.dtype)], 1)   # the SH basis is an input
    pre = X @ P["w1"].t() + P["b1"]
    o = torch.relu(pre) @ P["w2"].t() + P["b2"]
    rgb = (1 + 2 * EPS) / (1 + torch.exp(-o)) - EPS
    ((logit * d_logit).sum() + (rgb * d_rgb).sum()).backward()
    return logit.detach(), rgb.detach(), enc.grad, {k: v.grad for k, v in P.items()}, pre.detach()


def _inputs(C, n_rays, S, seed, far_bias):
    g = torch.Generator().manual_seed(seed)
    n = n_rays * S
    enc = (torch.randn(n, C, generator=g) * 0.1).to(torch.float16).float()
    ray_dirs = torch.randn(n_rays, 3, generator=g)
    ray_dirs = ray_dirs / ray_dirs.norm(dim=1, keepdim=True)
    dirs = ray_dirs.repeat_interleave(S, 0).contiguous()       # the sampler's per-sample [n, 3] array
    ray_img = torch.tensor([IMG_RUNS[i % len(IMG_RUNS)] for i in range(n_rays)], dtype=torch.int32)
    P = {"w_h": torch.randn(16, C, generator=g) * 0.3, "b_h": torch.randn(16, generator=g) * 0.1,
         "w1": torch.randn(64, 32, generator=g) * 0.3, "b1": torch.randn(64, generator=g) * 0.1,
         "w2": torch.randn(3, 64, generator=g) * 0.3, "b2": torch.randn(3, generator=g) * 0.1,
         "emb": torch.randn(E, 16, generator=g) * 0.1}
    if far_bias:   # many samples: keep every pre-activation far from zero, half the neurons on
        P["w1"] = P["w1"] * 0.25
        P["b1"] = torch.where(torch.arange(64) % 2 == 0, 4.0, -4.0) + P["b1"]
    d_logit = torch.randn(n, generator=g)
    d_rgb = torch.randn(n, 3, generator=g)
    return enc, dirs, ray_img, P, d_logit, d_rgb


def _bars_hold(got, ref):
    """the bars of tests/test_gpu_shade.py::test_shade_fwd_bwd, on (logit, rgb, d_enc, grads)"""
    torch.testing.assert_close(got[0], ref[0], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(got[1], ref[1], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(got[2], ref[2], rtol=1e-3, atol=1e-4 * float(ref[2].abs().max()))
    for k in got[3]:
        if ref[3][k] is not None:
            torch.testing.assert_close(got[3][k], ref[3][k], rtol=1e-3,
                                       atol=2e-4 * float(ref[3][k].abs().max()), msg=lambda m, k=k: k + ": " + m)


@functools.lru_cache(maxsize=None)
def _case(C, n_rays, S, with_emb, far_bias=False):
    """inputs and the torch-CPU reference of one case, computed once and shared (read only)"""
    for bump in range(32):
        seed = 1000 * C + S + n_rays + (7 if with_emb else 0) + 100000 * bump
        enc, dirs, ray_img, P, d_logit, d_rgb = _inputs(C, n_rays, S, seed, far_bias)
        img = ray_img.repeat_interleave(S) if with_emb else None
        f64 = lambda t: t.double()
        ref64 = _reference(f64(enc), f64(dirs), img, {k: f64(v) for k, v in P.items()}, f64(d_logit),
                           f64(d_rgb))
        if float(ref64[4].abs().min()) > 2e-6:
            break
    else:
        raise AssertionError("no seed keeps the pre-activations away from zero")
    ref = _reference(enc, dirs, img, P, d_logit, d_rgb)
    if not with_emb:
        ref[3]["emb"] = None
    # the float64 evaluation meets the same bars: the f32 reference is not what is being measured
    g64 = {k: (None if v is None or ref[3][k] is None else v.float()) for k, v in ref64[3].items()}
    _bars_hold((ref64[0].float(), ref64[1].float(), ref64[2].float(), g64), ref)
    return enc, dirs, ray_img, img, P, d_logit, d_rgb, ref


def _run(capi, dev, C, n_rays, S, with_emb, case, waves_list):
    enc, dirs, ray_img, img, P, d_logit, d_rgb, ref = case
    n = n_rays * S
    dv = lambda t: t.to(dev).contiguous()
    enc_cm, d_dirs = dv(enc.t()), dv(dirs)
    Pd = {k: dv(v) for k, v in P.items()}
    d_ray_img = dv(ray_img) if with_emb else None
    d_img = dv(img) if with_emb else None
    emb = Pd["emb"] if with_emb else None
    w = (Pd["w_h"], Pd["b_h"], Pd["w1"], Pd["b1"], Pd["w2"], Pd["b2"], emb)

    logit = torch.full((n,), 7.0, device=dev)
    rgb = torch.full((n, 3), 7.0, device=dev)
    capi.call("shade_fwd_rays", enc_cm, C, d_dirs, d_ray_img, *w, logit, rgb, n_rays, S)
    torch.testing.assert_close(logit.cpu(), ref[0], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(rgb.cpu(), ref[1], rtol=1e-4, atol=1e-5)
    # the head layer is untouched: the per-sample kernel's logit bit for bit, its colours to rounding
    logit_ps = torch.full((n,), 7.0, device=dev)
    rgb_ps = torch.full((n, 3), 7.0, device=dev)
    capi.call("shade_fwd", enc_cm, C, d_dirs, d_img, *w, logit_ps, rgb_ps, None, n)
    assert torch.equal(logit, logit_ps)
    torch.testing.assert_close(rgb, rgb_ps, rtol=1e-4, atol=1e-5)

    keys = ("w_h", "b_h", "w1", "b1", "w2", "b2") + (("emb",) if with_emb else ())
    for waves in waves_list:
        d_enc = torch.full((C, n), 7.0, device=dev)      # must be overwritten
        G = {k: torch.zeros_like(v) for k, v in Pd.items()}

        def bwd():
            capi.call("shade_bwd_rays", enc_cm, C, d_dirs, d_ray_img, *w, dv(d_logit), dv(d_rgb),
                      d_enc, G["w_h"], G["b_h"], G["w1"], G["b1"], G["w2"], G["b2"],
                      G["emb"] if with_emb else None, n_rays, S)

        with capi.option("SHADE_BWD_WAVES", waves):
            bwd()
            tag = lambda m, k: "%s [waves %d]: %s" % (k, waves, m)
            torch.testing.assert_close(d_enc.t().cpu(), ref[2], rtol=1e-3,
                                       atol=1e-4 * float(ref[2].abs().max()),
                                       msg=lambda m: tag(m, "d_enc"))

            def check(k, got, want, factor=1.0):
                torch.testing.assert_close(got.cpu(), factor * want, rtol=1e-3,
                                           atol=factor * 2e-4 * float(want.abs().max()),
                                           msg=lambda m: tag(m, k))

            for k in keys:
                check(k, G[k], ref[3][k])
            # on their own: a wrong ray's SH or a dropped stride shows in the SH half of d w1 and in
            # d b1 (its per-stride factor), a missed embedding flush in d emb -- each against its own
            # largest element, not the whole tensor's
            check("w1[:, 16:]", G["w1"][:, 16:], ref[3]["w1"][:, 16:])
            check("w1[:, :16]", G["w1"][:, :16], ref[3]["w1"][:, :16])
            check("b1", G["b1"], ref[3]["b1"])
            if with_emb:
                for e in range(E):
                    if float(ref[3]["emb"][e].abs().max()) > 0:
                        check("emb[%d]" % e, G["emb"][e], ref[3]["emb"][e])
                    else:
                        assert not G["emb"][e].any(), e
            # the parameter gradients accumulate: a second call doubles them
            bwd()
            for k in keys:
                check(k + " accumulate", G[k], ref[3][k], 2.0)


@pytest.mark.parametrize("with_emb", [True, False])
@pytest.mark.parametrize("C", [8, 32, 64])
@pytest.mark.parametrize("S", [64, 128, 192])
def test_shade_rays_fwd_bwd(capi, dev, S, C, with_emb):
    # SHADE_BWD_WAVES 1: 64-sample strides at one wave per SIMD (also the default at this size);
    # 2 / 3: 32-sample strides at two waves, fenced / mixed
    _run(capi, dev, C, 37, S, with_emb, _case(C, 37, S, with_emb), (1, 2, 3))


def test_shade_rays_stride_loop_wraps(capi, dev):
    """4 500 forward strides on 4 096 persistent waves, 9 000 / 4 500 backward strides on 2 048 /
    1 024: the stride loop of every form wraps."""
    C, n_rays, S = 32, 1500, 192
    assert n_rays * S // 64 > 256 * 16
    _run(capi, dev, C, n_rays, S, True, _case(C, n_rays, S, True, True), (1, 2))


def test_shade_rays_rejects_other_strides(capi, dev):
    C, n_rays, S = 32, 4, 96
    z = lambda *s: torch.zeros(*s, device=dev)
    P = (z(16, C), z(16), z(64, 32), z(64), z(3, 64), z(3))
    with pytest.raises(capi.F2NError, match=r"\(-1\)"):
        capi.call("shade_fwd_rays", z(C, n_rays * S), C, z(n_rays * S, 3), None, *P, None,
                  z(n_rays * S), z(n_rays * S, 3), n_rays, S)
    G = tuple(torch.zeros_like(p) for p in P)
    with pytest.raises(capi.F2NError, match=r"\(-1\)"):
        capi.call("shade_bwd_rays", z(C, n_rays * S), C, z(n_rays * S, 3), None, *P, None,
                  z(n_rays * S), z(n_rays * S, 3), z(C, n_rays * S), *G, None, n_rays, S)
    with pytest.raises(capi.F2NError, match=r"\(-3\)"):     # no matrix-core tiling for C = 24
        capi.call("shade_fwd_rays", z(24, n_rays * 64), 24, z(n_rays * 64, 3), None, z(16, 24), *P[1:],
                  None, z(n_rays * 64), z(n_rays * 64, 3), n_rays, 64)


# ---- through the Renderer: F2N_OPT_SHADE_RAYS = 0 (ray-uniform kernels) against 1 (per-sample) ----

@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def _renderer(host, bias0, seed, L=4, F=2, log2_T=14, S=64, step=4.0 / 64, n_rays=96, n_img=7):
    """a small Renderer with trained-looking parameters, as tests/test_gpu_render.py sets one up"""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    oracle = R.Renderer(n_img, L=L, F=F, log2_T=log2_T, S=S, step=step, gen=g, feat_init="trained")
    with torch.no_grad():
        oracle.scene_field.mlp.bias[0] = bias0
    hr = host.Renderer(n_img, n_levels=L, n_channels=F, log2_table=log2_T, max_samples=S, step=step)
    src = {
        "scene_field.feat_pool": oracle.scene_field.feat_pool,
        "scene_field.prim_pool": oracle.scene_field.prim_pool,
        "scene_field.bias_pool": oracle.scene_field.bias_pool,
        "scene_field.mlp.weight": oracle.scene_field.mlp.weight,
        "scene_field.mlp.bias": oracle.scene_field.mlp.bias,
        "shader.mlp.0.weight": oracle.shader.mlp[0].weight,
        "shader.mlp.0.bias": oracle.shader.mlp[0].bias,
        "shader.mlp.2.weight": oracle.shader.mlp[2].weight,
        "shader.mlp.2.bias": oracle.shader.mlp[2].bias,
        "app_emb": oracle.app_emb,
    }
    hp = hr.named_parameters()
    with torch.no_grad():
        for k, v in src.items():
            hp[k].copy_(v.detach().to(hp[k].device))
    o = torch.randn(n_rays, 3, generator=g) * 0.25
    d = torch.randn(n_rays, 3, generator=g)
    noise = torch.rand(n_rays, S, generator=g) - 0.5 + 1.0
    bg = torch.rand(n_rays, 3, generator=g)
    gt = torch.rand(n_rays, 3, generator=g)
    emb = torch.randint(0, n_img, (n_rays,), generator=g).to(torch.int32)
    hr.set_fused(True)
    hr.set_fused_shade(True)
    hr.set_dense_first_pass(1)
    return hr, o, d, noise, bg, gt, emb


def _step(host, capi, hr, args, rays_option):
    o, d, emb, gt, noise, bg = args
    with capi.option("SHADE_RAYS", rays_option):
        hr.zero_grad()
        out = [t.detach().clone() for t in hr.render(o, d, emb, "train", noise, bg)]
        hr.zero_grad()
        host.kernel_timer_enable(True)
        loss, sq, _, _ = hr.train_step(o, d, emb, gt, 1e-2, noise, bg, True)
        timed = set(host.kernel_timer_collect())
        host.kernel_timer_enable(False)
        grads = {k: v.clone() for k, v in hr.grads().items() if v is not None}
    return out, loss.clone(), sq.clone(), grads, timed, hr.last_kept_fraction


def test_renderer_takes_ray_uniform_kernels_on_the_dense_grid(host, capi, dev):
    """Thin medium, every sample kept: the samples are the [n_rays, S] grid."""
    hr, o, d, noise, bg, gt, emb = _renderer(host, -3.0, 41)
    args = tuple(t.to(dev) for t in (o, d, emb, gt, noise, bg))
    rays = _step(host, capi, hr, args, 0)
    per_sample = _step(host, capi, hr, args, 1)
    assert rays[5] == 1.0 and per_sample[5] == 1.0
    # the image id goes in per ray: no per-sample ids are written
    assert "shade_fwd" in rays[4] and "shade_bwd" in rays[4] and "scatter_idx" not in rays[4]
    assert "scatter_idx" in per_sample[4]
    colors, depths, weights, bounds = rays[0][:4]
    colors_ps, depths_ps, weights_ps, bounds_ps = per_sample[0][:4]
    # what derives from logit alone is the same bit for bit
    assert torch.equal(bounds, bounds_ps)
    assert torch.equal(weights, weights_ps) and torch.equal(depths, depths_ps)
    torch.testing.assert_close(colors, colors_ps, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(rays[1], per_sample[1], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(rays[2], per_sample[2], rtol=1e-4, atol=1e-5)
    assert set(rays[3]) == set(per_sample[3])
    for k, ref in per_sample[3].items():
        torch.testing.assert_close(rays[3][k], ref, rtol=1e-3, atol=2e-4 * float(ref.abs().max()),
                                   msg=lambda m, k=k: k + ": " + m)


def test_renderer_keeps_per_sample_kernels_on_compacted_samples(host, capi, dev):
    """Opaque medium: the rays terminate, the samples are compacted, the option changes nothing."""
    hr, o, d, noise, bg, gt, emb = _renderer(host, 8.0, 43)
    args = tuple(t.to(dev) for t in (o, d, emb, gt, noise, bg))
    rays = _step(host, capi, hr, args, 0)
    per_sample = _step(host, capi, hr, args, 1)
    assert rays[5] < 0.9 and rays[5] == per_sample[5]
    assert "scatter_idx" in rays[4] and "scatter_idx" in per_sample[4]
    for a, b in zip(rays[0], per_sample[0]):
        assert torch.equal(a, b)
    assert torch.equal(rays[1], per_sample[1]) and torch.equal(rays[2], per_sample[2])
    for k, ref in per_sample[3].items():   # sums by float atomics: equal up to their order
        torch.testing.assert_close(rays[3][k], ref, rtol=1e-4, atol=1e-5 * float(ref.abs().max()) + 1e-30)
