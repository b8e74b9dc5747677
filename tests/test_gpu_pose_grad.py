"""Camera-pose gradients through ray generation and the fused render (pose optimisation of the
reference's Localizer, src/localizer.cpp:142-167): get_rays_from_pose / get_view_rays carry a
gradient to the pose, f2n_hash_rays_grad turns the encoding's gradient into the rays' gradient, and
the Renderer's fused path with set_fused_ray_grad(True) agrees with the CPU oracle, with the op-by-op
route and with itself."""
import importlib

import pytest
import torch

from oracle import kernels as K
from oracle import ref_render as R
from tests import ray_grad_model as M
from tests.test_gpu_render import _close, _setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def _pose(g, B=1, rows=3):
    """B random camera poses: a rotation (QR of a Gaussian) and a translation near the origin."""
    q, _ = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))
    t = torch.randn(B, 3, 1, generator=g) * 0.2
    p = torch.cat([q, t], 2)
    if rows == 4:
        p = torch.cat([p, torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(B, 1, 4)], 1)
    return p.contiguous()


def _intrinsic(B, h, w):
    k = torch.tensor([[0.9 * w, 0.0, 0.5 * w], [0.0, 0.9 * w, 0.5 * h], [0.0, 0.0, 1.0]])
    return k.expand(B, 3, 3).contiguous()


# ---- ray generation ------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["b1_3x4", "b1_4x4", "bn_3x4", "bn_4x4", "view_3x4"])
def test_gen_rays_pose_gradient_matches_oracle(host, dev, case):
    g = torch.Generator().manual_seed(17)
    h, w, N = 12, 20, 240
    rows = 4 if case.endswith("4x4") else 3
    B = N if case.startswith("bn") else 1
    pose = _pose(g, B, rows)
    Kc = _intrinsic(B, h, w)
    if case.startswith("view"):
        pix = torch.arange(h * w)
        ij = torch.stack([pix // w, pix % w], 1)
    else:
        ij = torch.stack([torch.randint(0, h, (N,), generator=g), torch.randint(0, w, (N,), generator=g)], 1)
    wo = torch.randn(ij.shape[0], 3, generator=g)
    wd = torch.randn(ij.shape[0], 3, generator=g)

    p_ref = pose.clone().requires_grad_(True)
    o_ref, d_ref = R.get_rays_from_pose(p_ref, Kc, ij)
    ((o_ref * wo).sum() + (d_ref * wd).sum()).backward()

    grads = []
    for _ in range(2):
        if case.startswith("view"):
            p = pose[0].to(dev).requires_grad_(True)  # [3,4] through get_view_rays' unsqueeze
            o, d = host.get_view_rays(p, Kc[0].to(dev), h, w)
        else:
            p = pose.to(dev).requires_grad_(True)
            o, d = host.get_rays_from_pose(p, Kc.to(dev), ij.to(torch.int32).to(dev))
        torch.testing.assert_close(o.detach().cpu(), o_ref.detach(), rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(d.detach().cpu(), d_ref.detach(), rtol=1e-5, atol=1e-6)
        ((o * wo.to(dev)).sum() + (d * wd.to(dev)).sum()).backward()
        assert p.grad is not None, "pose.grad is undefined: ray generation has no backward"
        assert p.grad.shape == p.shape
        grads.append(p.grad.detach().cpu())
    ref = p_ref.grad if not case.startswith("view") else p_ref.grad[0]
    _close(grads[0], ref, 1e-5, 1e-5)
    assert torch.equal(grads[0], grads[1]), "the pose gradient must be the same bits run to run"
    if rows == 4:
        assert float(grads[0][..., 3, :].abs().max()) == 0.0


# ---- f2n_hash_rays_grad through the C ABI --------------------------------------------------------

def _field(L, F, T, disjoint, seed):
    g = torch.Generator().manual_seed(seed)
    stride = T * F if disjoint else T
    numel = max(T * L * F, stride * (L - 1) + T * F)
    table = torch.randn(numel, generator=g) * 0.1
    primes = []
    while len(primes) < 3 * L:
        v = int(torch.randint(1 << 28, 1 << 30, (1,), generator=g))
        if R._is_prime(v):
            primes.append(v)
    return dict(table16=K.cast_f16(table), numel=numel, stride=stride,
                primes=torch.tensor(primes, dtype=torch.int32).reshape(L, 3),
                bias=torch.rand(L, 3, generator=g) * 1000.0 + 100.0, mul=K.level_mul(L))


def _rays_and_samples(n_rays, seed, fld=None):
    """fld: samples whose cell a rounding of the contraction could decide (tests/ray_grad_model.py,
    `ambiguous`) get a new t until none is left -- no seed gives 4000 samples without one (1-3 % of
    them are), so the samples are redrawn and nothing is left out of a comparison."""
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n_rays, 3, generator=g) * 0.25
    d = torch.randn(n_rays, 3, generator=g) * 2.0
    lens = torch.randint(0, 200, (n_rays,), generator=g)
    lens[::7] = 0  # empty segments
    lens[1] = 64
    lens[2] = 65
    end = torch.cumsum(lens, 0)
    bounds = torch.stack([end - lens, end], 1).to(torch.int32).contiguous()
    n = int(end[-1])
    ray = torch.repeat_interleave(torch.arange(n_rays), lens)
    t = torch.rand(n, generator=g) * 3.0 + 0.01
    nhat = d / d.norm(dim=1, keepdim=True)
    pts = (o[ray] + nhat[ray] * t[:, None]).contiguous()
    for _ in range(100 if fld is not None else 0):
        amb = torch.from_numpy(M.ambiguous(fld, pts))
        if not bool(amb.any()):
            break
        t[amb] = torch.rand(int(amb.sum()), generator=g) * 3.0 + 0.01
        pts = (o[ray] + nhat[ray] * t[:, None]).contiguous()
    else:
        assert fld is None, "ambiguous samples left after 100 draws"
    return o, d, bounds, ray, t, pts


def _oracle_rays_grad(fld, L, F, T, o, d, ray, t, pts, x, g):
    """CPU composition: Q5 hash backward at the contracted points, the contraction's backward (the
    reference's ATen expression under autograd), per-ray sums, the normalisation's backward."""
    _, gx = K.hash_bwd(x, fld["table16"], fld["primes"], fld["bias"], fld["mul"], g, fld["numel"],
                       L, F, T, fld["stride"], 128.0, need_pts_grad=True)
    p = pts.clone().requires_grad_(True)
    norm = p.norm(2, dim=1, keepdim=True)
    mask = norm <= 1.0
    xc = p * mask + ~mask * (1 + 1.0 - 1.0 / norm) * p / norm
    (dp,) = torch.autograd.grad(xc, p, gx)
    n_rays = o.shape[0]
    d_o = torch.zeros(n_rays, 3).index_add_(0, ray, dp)
    m = torch.zeros(n_rays, 3).index_add_(0, ray, dp * t[:, None])
    dv = d.clone().requires_grad_(True)
    ((dv / torch.linalg.norm(dv, 2, -1, True)) * m).sum().backward()
    return d_o, dv.grad


@pytest.mark.parametrize("F", [1, 2, 4, 8])
@pytest.mark.parametrize("L,T,disjoint", [(16, 5000, False), (32, 5000, False), (16, 5000, True),
                                          (32, 1 << 12, True), (16, 1 << 12, False)])
def test_hash_rays_grad_matches_oracle(capi, dev, F, L, T, disjoint):
    """Against the float32 oracle composition at 5 % + 0.2 % of the largest element, and element by
    element against the float64 model of tests/ray_grad_model.py at twice its rounding bound (the
    cases built to corner the kernel are tests/test_gpu_ray_grad_f64.py)."""
    fld = dict(_field(L, F, T, disjoint, seed=F * 100 + L), L=L, F=F, T=T)
    n_rays = 40
    o, d, bounds, ray, t, pts = _rays_and_samples(n_rays, seed=L + F, fld=fld)
    n = pts.shape[0]
    gen = torch.Generator().manual_seed(3)
    g = torch.randn(n, L * F, generator=gen) * 5e-3
    to = lambda v: v.to(dev)
    pts_d = to(pts)
    x_d = torch.empty_like(pts_d)
    capi.call("contract_fwd", pts_d, x_d, n)  # the contracted points exactly as the encode forms them
    x = x_d.cpu()
    ref_o, ref_d = _oracle_rays_grad(fld, L, F, T, o, d, ray, t, pts, x, g)

    g_cm = to(g.t().contiguous())  # the renderer hands over channel-major storage
    outs = []
    for _ in range(2):
        d_o = torch.full((n_rays, 3), float("nan"), device=dev)
        d_d = torch.full((n_rays, 3), float("nan"), device=dev)
        capi.call("hash_rays_grad", pts_d, to(t), to(bounds), to(d), to(fld["table16"]),
                  to(fld["primes"]), to(fld["bias"]), to(fld["mul"]), g_cm, 1, n, d_o, d_d, n_rays,
                  L, F, T, fld["stride"], 128.0)
        torch.cuda.synchronize()
        outs.append((d_o.cpu(), d_d.cpu()))
    got_o, got_d = outs[0]
    empty = (bounds[:, 1] == bounds[:, 0])
    assert float(got_o[empty].abs().max()) == 0.0 and float(got_d[empty].abs().max()) == 0.0
    assert ref_o.abs().max() > 0
    # Q5 terms are f16-rounded and of both signs: compare against their own scale
    _close(got_o, ref_o, 5e-2, 2e-3)
    _close(got_d, ref_d, 5e-2, 2e-3)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    m = M.model(M.Inputs(fld, pts, t, bounds, d, g))
    assert m["finite"] and not M.ambiguous(fld, pts).any()
    r_o = float(M.ratio(got_o, m["d_o"], m["E"]["d_o"]).max())
    r_d = float(M.ratio(got_d, m["d_d"], m["E"]["d_d"]).max())
    print("\nlargest |err| / E: d_o %.3f, d_d %.3f" % (r_o, r_d))
    assert r_o <= M.BAR and r_d <= M.BAR, (r_o, r_d)


# ---- Renderer::render with fused_ray_grad --------------------------------------------------------

def _render(hr, dev, o, d, mode, emb, noise, bg, need_grad):
    to = lambda v: v.to(dev)
    o_g, d_g = to(o).requires_grad_(need_grad), to(d).requires_grad_(need_grad)
    if mode == "train":
        out = hr.render(o_g, d_g, to(emb), "train", to(noise), to(bg))
    else:
        out = hr.render(o_g, d_g, None, "validate")
    return o_g, d_g, out


def _loss(colors, depths):
    return colors.square().sum() + depths.sum() * 0.1


@pytest.mark.parametrize("dense", [0, 1])
@pytest.mark.parametrize("mode", ["validate", "train"])
def test_fused_ray_grad_matches_oracle(host, dev, dense, mode):
    """The setup of test_gpu_render.test_pose_gradient_path, on the fused path.  Whole renders against
    the oracle's own sampler roundings, hence the 5 % bar here and in the two tests below; the kernel
    itself is held to float64 element by element in tests/test_gpu_ray_grad_f64.py."""
    oracle, hr, o, d, noise, bg, gt, emb = _setup(host, 8, 2, 14, 64, 4.0 / 64, 24, 3.0, 11)
    o_r, d_r = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    if mode == "train":
        res = oracle.render(o_r, d_r, emb, R.TRAIN, noise, bg)
    else:
        res = oracle.render(o_r, d_r, None, R.VALIDATE)
    _loss(res.colors, res.depths).backward()
    hr.set_fused_ray_grad(True)
    hr.set_dense_first_pass(dense)
    o_g, d_g, (colors, depths, weights, idx) = _render(hr, dev, o, d, mode, emb, noise, bg, True)
    assert colors.grad_fn is not None
    _loss(colors, depths).backward()
    assert torch.equal(idx.cpu(), res.idx_start_end)
    _close(colors.detach().cpu(), res.colors.detach(), 1e-4)
    _close(o_g.grad.cpu(), o_r.grad, 5e-2, 2e-3)
    _close(d_g.grad.cpu(), d_r.grad, 5e-2, 2e-3)


@pytest.mark.parametrize("margin_min_samples", [0, 1 << 30])
def test_fused_ray_grad_speculative_dense_pass(host, dev, margin_min_samples):
    """The speculative dense first pass (the previous chunk kept every sample): the guess that is
    accepted on the density-margin flag (margin_min_samples 0) or after the exact scan (2^30)."""
    oracle, hr, o, d, noise, bg, gt, emb = _setup(host, 8, 2, 14, 64, 4.0 / 64, 24, -8.0, 13)
    o_r, d_r = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    res = oracle.render(o_r, d_r, None, R.VALIDATE)
    _loss(res.colors, res.depths).backward()
    hr.set_fused_ray_grad(True)
    hr.set_dense_first_pass(1)
    hr.set_speculate_dense(True)
    hr.set_margin_min_samples(margin_min_samples)
    _render(hr, dev, o, d, "validate", None, None, None, False)  # a chunk that keeps everything
    assert hr.last_kept_fraction == 1.0
    o_g, d_g, (colors, depths, weights, idx) = _render(hr, dev, o, d, "validate", None, None, None,
                                                      True)
    _loss(colors, depths).backward()
    assert hr.last_kept_fraction == 1.0
    assert torch.equal(idx.cpu(), res.idx_start_end)
    _close(colors.detach().cpu(), res.colors.detach(), 1e-4)
    _close(o_g.grad.cpu(), o_r.grad, 5e-2, 2e-3)
    _close(d_g.grad.cpu(), d_r.grad, 5e-2, 2e-3)


@pytest.mark.parametrize("dense", [0, 1])
@pytest.mark.parametrize("big", [False, True])
def test_fused_ray_grad_leaves_render_and_parameter_gradients(host, capi, dev, dense, big):
    """Rays that require grad change nothing else: the same colours, depths, weights and bounds bit
    for bit as the fused render of detached rays, and the same parameter gradients (d(enc) is handed
    on untouched).  The network gradients are float-atomic sums: within their run-to-run spread; the
    table gradient of a >= 65536-sample batch under BWD_PHASES = 1 (binned, exact): bit-equal."""
    if big:
        oracle, hr, o, d, noise, bg, gt, emb = _setup(host, 16, 2, 19, 128, 4.0 / 128, 1024, 0.0, 5)
    else:
        oracle, hr, o, d, noise, bg, gt, emb = _setup(host, 8, 2, 14, 64, 4.0 / 64, 24, 3.0, 11)
    hr.set_fused_ray_grad(True)
    hr.set_dense_first_pass(dense)
    hr.set_speculate_dense(False)
    runs = []
    with capi.option("BWD_PHASES", 1):
        for need_grad in (False, False, True):
            hr.zero_grad()
            o_g, d_g, out = _render(hr, dev, o, d, "train", emb, noise, bg, need_grad)
            _loss(out[0], out[1]).backward()
            runs.append(([v.detach().clone() for v in out],
                         {k: v.clone() for k, v in hr.grads().items() if v is not None}))
            if need_grad:
                assert d_g.grad is not None and float(d_g.grad.abs().max()) > 0
    (base, g0), (_, g1), (with_grad, g2) = runs
    if big:
        assert base[2].numel() >= 65536
    for a, b in zip(base, with_grad):
        assert torch.equal(a, b)
    assert set(g0) == set(g2)
    for k in g0:
        if k.endswith("feat_pool") and big:
            assert torch.equal(g0[k], g2[k]), k
            continue
        spread = float((g0[k] - g1[k]).abs().max())
        scale = float(g0[k].abs().max())
        diff = float((g0[k] - g2[k]).abs().max())
        assert diff <= max(4 * spread, 1e-5 * scale), (k, diff, spread, scale)


def test_fused_and_op_by_op_agree_at_reference_sampler(host, dev):
    """4096 rays x 1024 samples at step 1/256 (the localiser's sampler), VALIDATE."""
    oracle, hr, o, d, noise, bg, gt, emb = _setup(host, 16, 2, 19, 1024, 1.0 / 256, 4096, 5.0, 23)
    grads = {}
    for fused in (False, True):
        hr.set_fused_ray_grad(fused)
        hr.set_dense_first_pass(-1)
        o_g, d_g, (colors, depths, weights, idx) = _render(hr, dev, o, d, "validate", None, None,
                                                          None, True)
        _loss(colors, depths).backward()
        grads[fused] = (o_g.grad.cpu(), d_g.grad.cpu(), colors.detach().cpu(), idx.cpu())
    assert torch.equal(grads[False][3], grads[True][3])
    _close(grads[True][2], grads[False][2], 1e-4)
    # The Q5 point gradient is piecewise constant in the contracted point and jumps at cell faces.
    # When this was written the op-by-op route sampled with ATen ops (positions that differ from the
    # sampler kernel's in the last bit), so among 4 M samples a handful landed across a fine-level face
    # and moved their ray's gradient by a jump of about mul * feature * g: those few rays are allowed
    # outside the per-element bar, the gradient as a whole is not.  (It samples with the kernel now,
    # PtsSampler::get_samples_grad; the allowance stays as it was.)
    for got, ref in ((grads[True][0], grads[False][0]), (grads[True][1], grads[False][1])):
        scale = float(ref.abs().max())
        bad = (got - ref).abs() > 2e-3 * scale + 5e-2 * ref.abs()
        assert int(bad.sum()) <= ref.numel() // 1000, int(bad.sum())
        assert float((got - ref).norm() / ref.norm()) < 5e-3


# ---- render_image(pose) --------------------------------------------------------------------------

H, W, CHUNK = 16, 24, 128


def _view_setup(host, seed=29):
    oracle, hr, *_ = _setup(host, 8, 2, 14, 64, 4.0 / 64, 1, 3.0, seed)
    g = torch.Generator().manual_seed(seed)
    pose = _pose(g)[0]
    Kc = _intrinsic(1, H, W)[0]
    target = torch.rand(H, W, 3, generator=g)
    hr.set_pixel_tiles(8)
    return oracle, hr, pose, Kc, target


def _image_pose_grad(hr, dev, pose, Kc, target, fused, mode="backward", dense=0):
    hr.set_fused_ray_grad(fused)
    hr.set_dense_first_pass(dense)
    p = pose.to(dev).requires_grad_(True)
    colors, _ = hr.render_image(p, Kc.to(dev), H, W, CHUNK)
    loss = (colors - target.to(dev)).square().mean()
    if mode == "grad":
        (gp,) = torch.autograd.grad(loss, p)
        return gp.cpu()
    loss.backward()
    assert p.grad is not None, "pose.grad is undefined"
    return p.grad.cpu()


def test_render_image_pose_gradient(host, dev):
    oracle, hr, pose, Kc, target = _view_setup(host)
    # oracle chain: get_rays_from_pose -> Renderer.render (rays are independent: one chunk) -> clip
    p_ref = pose.clone().requires_grad_(True)
    pix = torch.arange(H * W)
    o, d = R.get_rays_from_pose(p_ref[None], Kc[None], torch.stack([pix // W, pix % W], 1))
    res = oracle.render(o, d, None, R.VALIDATE)
    img = res.colors.clip(0.0, 1.0).reshape(H, W, 3)
    (img - target).square().mean().backward()
    ref = p_ref.grad
    assert float(ref.abs().max()) > 0
    g_op = _image_pose_grad(hr, dev, pose, Kc, target, False)
    for dense in (0, 1):
        g_fused = _image_pose_grad(hr, dev, pose, Kc, target, True, dense=dense)
        _close(g_fused, g_op, 5e-2, 2e-3)
        _close(g_fused, ref, 5e-2, 2e-3)
    _close(g_op, ref, 5e-2, 2e-3)


@pytest.mark.parametrize("dense", [0, 1])
def test_frozen_field_gives_the_same_pose_gradient(host, dev, dense):
    oracle, hr, pose, Kc, target = _view_setup(host)
    hr.zero_grad()
    g_full = _image_pose_grad(hr, dev, pose, Kc, target, True, dense=dense)
    assert hr.grads()["scene_field.feat_pool"] is not None
    # torch.autograd.grad(loss, pose): no table gradient is formed or stored
    hr.zero_grad()
    g_only = _image_pose_grad(hr, dev, pose, Kc, target, True, mode="grad", dense=dense)
    assert hr.grads()["scene_field.feat_pool"] is None
    assert torch.equal(g_only, g_full)
    # the field frozen
    params = hr.named_parameters()
    try:
        for v in params.values():
            v.requires_grad_(False)
        hr.zero_grad()
        g_frozen = _image_pose_grad(hr, dev, pose, Kc, target, True, dense=dense)
        assert hr.grads()["scene_field.feat_pool"] is None
        assert torch.equal(g_frozen, g_full)
    finally:
        for k, v in params.items():
            if k != "scene_field.prim_pool":
                v.requires_grad_(True)


@pytest.mark.parametrize("fused", [False, True])
def test_adam_on_the_pose_moves_it(host, dev, fused):
    """Localizer::optimize_pose_by_differential (src/localizer.cpp:142-167): Adam on a [3,4] pose,
    render_image + mse_loss + backward; three steps of lr 1e-4 must change the pose."""
    oracle, hr, pose, Kc, target = _view_setup(host)
    hr.set_fused_ray_grad(fused)
    p = pose.to(dev).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=1e-4)
    for _ in range(3):
        opt.zero_grad()
        colors, _ = hr.render_image(p, Kc.to(dev), H, W, 1 << 16)
        loss = torch.nn.functional.mse_loss(colors, target.to(dev))
        loss.backward()
        assert p.grad is not None
        opt.step()
    moved = float((p.detach().cpu() - pose).abs().max())
    assert moved > 1e-5, moved
