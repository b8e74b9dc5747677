"""The per-ray constant of the ray-uniform network kernels: f2n_shade_ray_const forms
c = b1 + w1[:, 16:32] . SH16(dir) and SH16(dir) once per ray, f2n_shade_fwd_rays_const /
f2n_shade_bwd_rays_const load them where f2n_shade_fwd_raydirs / f2n_shade_bwd_raydirs form them per
stride.

  the entries   logit, rgb, d_enc equal to the forming entries' (a NaN equals a NaN); parameter
                gradients equal where one workgroup sends them, otherwise within the reordered-sum
                bound of tests/test_gpu_shade_bwd_waves.py::_check (fixed there, before any run);
                nothing written outside [n_rays, 80], logit, rgb, d_enc
  the buffer    SH columns equal to f2n_sh_encode's (the same sh_basis<4>) and within the existing SH
                test's tolerance of the CPU oracle; c within 2 gamma(17) (|b1| + |w1| |SH|) of a float32
                fmaf chain in the order the products walk k (b1[j], then SH index 0, 4, 8, 12, 1, 5, ...):
                tests/shade_model.py's count for a 16-term matrix-core sum onto a bias, once for the
                kernel and once for the chain.  (Whether the two are the same bits is printed: the
                matrix instruction's internal order is not documented, so equality is not asserted.
                On an MI355X 0 of the 4288 elements differed.)
  the Renderer  the lean dense route (which takes the new entries) against F2N_OPT_DENSE_LEAN = 1
                (which takes per-sample directions and so the forming kernels): results equal, the
                launches of each as stated.
"""
import importlib

import numpy as np
import pytest
import torch

from oracle import kernels as K
from tests import shade_model as sm
from tests.mesh_model import fmaf32
from tests.test_gpu_dense_lean import (FILL, KEYS, N_RAYS, S as S_REN, _Guarded, _launches,
                                       _profiled_train_step, _renderer, _run, _same)
from tests.test_gpu_ray_order import _pose, _view, W_IMG
from tests.test_gpu_shade_bwd_waves import _check

pytestmark = pytest.mark.gpu
E = 5
RC = 80           # F2N_SHADE_RAY_CONST_FLOATS


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def _directions(n_rays, g):
    """17 rows: two random unit vectors, the six axis directions, a zero vector, a unit vector with a
    denormal component, seven more random unit vectors; fewer rays take the first rows, more repeat
    the table with fresh random rows"""
    rnd = torch.randn(max(n_rays, 17), 3, generator=g)
    d = rnd / rnd.norm(dim=1, keepdim=True)
    d[2:8] = torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [-1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]])
    d[8] = 0.0
    d[9] = torch.tensor([1e-41, 0.6, 0.8])
    assert 0 < float(d[9, 0]) < 1.2e-38
    return d[:n_rays].contiguous()


def _inputs(C, n_rays, S, n_img, seed):
    g = torch.Generator().manual_seed(seed)
    n = n_rays * S
    enc = (torch.randn(n, C, generator=g) * 0.1).to(torch.float16).float()
    ray_dirs = _directions(n_rays, g)
    ray_img = (torch.arange(n_rays) % n_img).to(torch.int32)
    P = {"w_h": torch.randn(16, C, generator=g) * 0.3, "b_h": torch.randn(16, generator=g) * 0.1,
         "w1": torch.randn(64, 32, generator=g) * 0.3, "b1": torch.randn(64, generator=g) * 0.1,
         "w2": torch.randn(3, 64, generator=g) * 0.3, "b2": torch.randn(3, generator=g) * 0.1,
         "emb": torch.randn(E, 16, generator=g) * 0.1}
    return enc, ray_dirs, ray_img, P, torch.randn(n, generator=g), torch.randn(n, 3, generator=g)


def _both(capi, dev, C, n_rays, S, with_emb, n_img=2):
    """{waves: {"const" | "raydirs": (logit, rgb, [d_enc], G)}}, the guarded buffers of the const arm,
    and the per-sample inputs _check bounds the gradients from"""
    enc, ray_dirs, ray_img, P, d_logit, d_rgb = _inputs(C, n_rays, S, n_img, 97 * C + 11 * n_rays + S)
    n = n_rays * S
    dv = lambda t: t.to(dev).contiguous()
    enc_cm, Pd, dd = dv(enc.t()), {k: dv(v) for k, v in P.items()}, dv(ray_dirs)
    img_d = dv(ray_img) if with_emb else None
    keys = KEYS if with_emb else KEYS[:-1]
    w = tuple(Pd[k] for k in KEYS[:-1]) + (Pd["emb"] if with_emb else None,)
    dl, dr = dv(d_logit), dv(d_rgb)
    rc = _Guarded((n_rays, RC), dev)
    capi.call("shade_ray_const", dd, Pd["w1"], Pd["b1"], rc.t, n_rays)
    out, guarded = {}, [rc]
    for waves in (1, 2):
        with capi.option("SHADE_BWD_WAVES", waves):
            arms = {}
            for arm in ("raydirs", "const"):
                logit, rgb, d_enc = _Guarded((n,), dev), _Guarded((n, 3), dev), _Guarded((C, n), dev)
                G = {k: torch.zeros_like(Pd[k]) for k in keys}
                gargs = tuple(G[k] for k in KEYS[:-1]) + (G["emb"] if with_emb else None,)
                if arm == "const":
                    capi.call("shade_fwd_rays_const", enc_cm, C, rc.t, img_d, *w, logit.t, rgb.t, n_rays, S)
                    capi.call("shade_bwd_rays_const", enc_cm, C, dd, rc.t, img_d, *w, dl, dr, d_enc.t,
                              *gargs, n_rays, S)
                    guarded += [logit, rgb, d_enc]
                else:
                    capi.call("shade_fwd_raydirs", enc_cm, C, dd, img_d, *w, logit.t, rgb.t, n_rays, S)
                    capi.call("shade_bwd_raydirs", enc_cm, C, dd, img_d, *w, dl, dr, d_enc.t, *gargs,
                              n_rays, S)
                torch.cuda.synchronize()
                arms[arm] = (logit.t, rgb.t, [d_enc.t], G)
            out[waves] = arms
    inputs = (enc, ray_dirs.repeat_interleave(S, 0).contiguous(),
              ray_img.repeat_interleave(S) if with_emb else None, P, d_logit, d_rgb, 1)
    return out, guarded, inputs, (ray_dirs, P, rc.t)


def _compare(out, guarded, inputs, C, n_rays, S, with_emb, n_img=2):
    n = n_rays * S
    for waves in (1, 2):
        a, b = out[waves]["const"], out[waves]["raydirs"]
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2][0], b[2][0]), waves
        for t in (a[0], a[1], a[2][0]):
            assert not bool((t == FILL).any()), waves          # every element written
        # one workgroup: 4 waves of 64-sample strides, or 8 waves of 32-sample strides
        strides = n // (64 if waves == 1 else 32)
        if strides <= (4 if waves == 1 else 8):
            for k in KEYS[:-1]:
                assert torch.equal(a[3][k], b[3][k]), (waves, k)
                assert bool(a[3][k].any()), k
            # d emb: every wave adds its stride's share to its image's row with a float atomic of its
            # own; a row that gets at most two addends is the same sum in either order
            per_img = (strides // n_rays) * -(-n_rays // n_img)
            if with_emb and waves == 1 and per_img <= 2:
                assert torch.equal(a[3]["emb"], b[3]["emb"]), waves
        res = {"const": (a[2], a[3]), "raydirs": (b[2], b[3]), "inputs": inputs}
        _check(res, with_emb, arms=("const", "raydirs"))
        if with_emb:
            used = min(n_img, n_rays)
            assert bool(a[3]["emb"][:used].any()) and not bool(a[3]["emb"][used:].any())
    for buf in guarded:
        assert buf.guards_intact()


@pytest.mark.parametrize("with_emb", [True, False])
@pytest.mark.parametrize("S", [64, 128, 192])
@pytest.mark.parametrize("n_rays", [1, 2, 17])
@pytest.mark.parametrize("C", [8, 16, 32, 64])
def test_const_entries_equal_forming_entries(capi, dev, C, n_rays, S, with_emb):
    out, guarded, inputs, _ = _both(capi, dev, C, n_rays, S, with_emb)
    _compare(out, guarded, inputs, C, n_rays, S, with_emb)


def test_const_entries_where_a_wave_changes_image(capi, dev):
    """2100 rays x 64 samples, image id = ray % 3: more strides than the 1024 (one-wave form) and 2048
    (two-wave form) persistent waves, and a wave's next stride lies 1024 rays on, under another image
    id -- the backward's flush of the embedding row on a change of id runs in both forms."""
    out, guarded, inputs, _ = _both(capi, dev, 32, 2100, 64, True, n_img=3)
    _compare(out, guarded, inputs, 32, 2100, 64, True, n_img=3)


def test_buffer_rows(capi, dev):
    """[n_rays, 80] for 67 rays (five wavefronts of 16, the last one partial)"""
    n_rays = 67
    g = torch.Generator().manual_seed(5)
    ray_dirs = _directions(n_rays, g)
    w1, b1 = torch.randn(64, 32, generator=g) * 0.3, torch.randn(64, generator=g) * 0.1
    rc = _Guarded((n_rays, RC), dev)
    capi.call("shade_ray_const", ray_dirs.to(dev), w1.to(dev), b1.to(dev), rc.t, n_rays)
    sh_dev = torch.empty(n_rays, 16, device=dev)
    capi.call("sh_encode", ray_dirs.to(dev), sh_dev, n_rays, 4)
    torch.cuda.synchronize()
    assert rc.guards_intact() and not bool((rc.t == FILL).any())
    got = rc.t.cpu()
    # ---- SH16(dir): the bits of f2n_sh_encode, and the CPU oracle as tests/test_gpu_ops.py holds it
    assert _same(got[:, 64:], sh_dev.cpu())
    torch.testing.assert_close(got[:, 64:], K.sh_encode(ray_dirs, 4), rtol=1e-6, atol=1e-7)
    # ---- c: the float32 chain from b1[j], k-step t' = 0..3, quarter q = 0..3: SH index 4 q + t'
    sh = got[:, 64:].numpy()
    w1n, b1n = w1.numpy(), b1.numpy()
    c = np.broadcast_to(b1n, (n_rays, 64)).astype(np.float32)
    for t in range(4):
        for q in range(4):
            i = 4 * q + t
            c = fmaf32(np.broadcast_to(w1n[:, 16 + i], (n_rays, 64)), sh[:, i:i + 1], c).reshape(n_rays, 64)
    A = np.abs(b1n).astype(np.float64) + np.abs(sh.astype(np.float64)) @ np.abs(w1n[:, 16:].astype(np.float64)).T
    diff = np.abs(got[:, :64].numpy().astype(np.float64) - c.astype(np.float64))
    tol = 2 * sm.gamma(17) * A
    print("c against the fmaf chain: %d of %d elements differ, largest |diff| / tol %.3g" %
          (int((diff > 0).sum()), diff.size, float((diff / tol).max())))
    assert bool((diff <= tol).all()), float((diff / tol).max())


def test_entries_refuse_a_misaligned_buffer(capi, dev):
    """the row is read and written as float4: 16-byte alignment is part of the contract"""
    buf = torch.zeros(4 * RC + 4, device=dev)
    z = lambda *s: torch.zeros(*s, device=dev)
    c = capi.lib().cdll
    bad = buf.data_ptr() + 4
    assert c.f2n_shade_ray_const(z(4, 3).data_ptr(), z(64, 32).data_ptr(), z(64).data_ptr(), bad, 4, None) == -1
    P = [z(16, 32), z(16), z(64, 32), z(64), z(3, 64), z(3)]
    assert c.f2n_shade_fwd_rays_const(z(32, 256).data_ptr(), 32, bad, None, *[p.data_ptr() for p in P], None,
                                      z(256).data_ptr(), z(256, 3).data_ptr(), 4, 64, None) == -1


# ---- through the Renderer: the lean dense route against F2N_OPT_DENSE_LEAN = 1 ------------------------

@pytest.fixture(scope="module")
def renderers(host):
    return {False: _renderer(host, False), True: _renderer(host, True)}


@pytest.fixture(scope="module")
def chunk(host, dev):
    """320 consecutive rays of one 800-wide image row (tests/test_gpu_dense_lean.py's chunk)"""
    o, d = _view(host, dev)
    lo = 300 * W_IMG + 240
    o, d = o[lo:lo + N_RAYS].contiguous(), d[lo:lo + N_RAYS].contiguous()
    g = torch.Generator(device=dev).manual_seed(11)
    noise = torch.rand(N_RAYS, S_REN, device=dev, generator=g) + 0.5
    bg = torch.rand(N_RAYS, 3, device=dev, generator=g)
    gt = torch.rand(N_RAYS, 3, device=dev, generator=g)
    emb = torch.randint(0, 2, (N_RAYS,), device=dev, generator=g, dtype=torch.int32)
    return o, d, emb, noise, bg, gt


@pytest.mark.parametrize("opaque", [False, True])
@pytest.mark.parametrize("bucketed", [True, False])
def test_train_step_equals_the_forming_route(host, capi, renderers, chunk, bucketed, opaque):
    """320 rays x 128, noise passed.  Network gradients: the bars tests/test_gpu_dense_lean.py holds
    the same two routes to (float atomics of many workgroups)."""
    ren = renderers[opaque]
    ren.set_ray_order_min_rays(256 if bucketed else 1 << 30)
    try:
        capi.set_option("BWD_PHASES", 1)     # per-chunk table gradient sums independent of the order
        ref = _run(host, capi, ren, chunk, 1, 1e-2, False)
        got = _run(host, capi, ren, chunk, 0, 1e-2, False)
    finally:
        capi.set_option("BWD_PHASES", 0)
        capi.set_option("DENSE_LEAN", 0)
    (c0, d0, w0, i0), loss0, sq0, ns0, g0 = ref
    (c1, d1, w1, i1), loss1, sq1, ns1, g1 = got
    assert (ns0 < N_RAYS * S_REN) if opaque else (ns0 == N_RAYS * S_REN)
    assert ns1 == ns0 and torch.equal(i1, i0)
    assert torch.equal(c1, c0) and torch.equal(d1, d0) and torch.equal(w1, w0)
    assert torch.equal(loss1, loss0) and torch.equal(sq1, sq0)
    assert set(g1) == set(g0)
    assert torch.equal(g1["scene_field.feat_pool"], g0["scene_field.feat_pool"])
    assert float(g0["scene_field.feat_pool"].abs().max()) > 0
    for k, want in g0.items():
        err = float((g1[k] - want).norm()) / (float(want.norm()) + 1e-30)
        assert err <= (5e-5 if k == "app_emb" else 1e-5), (k, err)


FORMING = ("shade_fwd_mfma_rays_kernel<", "shade_bwd_mfma_rays_kernel<")
LOADING = ("shade_fwd_mfma_rays_kernel_const<", "shade_bwd_mfma_rays_kernel_const<")


@pytest.mark.parametrize("bucketed", [True, False])
def test_train_step_launches(host, capi, renderers, chunk, bucketed):
    """thin medium: the dense guess is accepted, one forward and one backward of the network"""
    ren = renderers[False]
    ren.set_ray_order_min_rays(256 if bucketed else 1 << 30)
    try:
        new, _ = _profiled_train_step(host, capi, ren, chunk, 0)
        old, _ = _profiled_train_step(host, capi, ren, chunk, 1)
    finally:
        capi.set_option("DENSE_LEAN", 0)
    assert _launches(new, "shade_ray_const_kernel") == 1, sorted(new)
    assert [_launches(new, k) for k in LOADING] == [1, 1], sorted(new)
    assert [_launches(new, k) for k in FORMING] == [0, 0], sorted(new)
    assert _launches(old, "shade_ray_const_kernel") == 0, sorted(old)
    assert [_launches(old, k) for k in LOADING] == [0, 0], sorted(old)
    assert [_launches(old, k) for k in FORMING] == [1, 1], sorted(old)


def test_validate_image_takes_the_constant_forward(host, capi, renderers, dev):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile

    ren = renderers[False]
    h = w = 64
    pose = _pose(dev)
    intr = torch.tensor([[90.0, 0, w / 2], [0, 90.0, h / 2], [0, 0, 1.0]], device=dev)

    def image(lean_option):
        with capi.option("DENSE_LEAN", lean_option), torch.no_grad():
            ren.render_image(pose, intr, h, w, h * w)                   # (warm: the route's buffers)
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                img, dep = ren.render_image(pose, intr, h, w, h * w)
                torch.cuda.synchronize()
        kernels = {}
        for e in prof.events():
            if e.device_type == DeviceType.CUDA:
                kernels[e.name] = kernels.get(e.name, 0) + 1
        return img, dep, kernels

    img1, dep1, new = image(0)
    img0, dep0, old = image(1)
    assert _launches(new, LOADING[0]) >= 1 and _launches(new, FORMING[0]) == 0, sorted(new)
    assert _launches(new, "shade_ray_const_kernel") == _launches(new, LOADING[0]), sorted(new)
    assert _launches(old, LOADING[0]) == 0 and _launches(old, FORMING[0]) >= 1, sorted(old)
    assert torch.equal(img1, img0) and torch.equal(dep1, dep0)
    assert float(img1.std()) > 0
