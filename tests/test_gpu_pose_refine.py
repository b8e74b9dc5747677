"""Per-image pose refinement on the GPU: f2n_cam_pose_grad against float64 within the derived bound of
tests/pose_refine_model.py, f2n_pose_compose and its backward against the float64 matrix_exp
reference to one float32 ulp, and a training step whose rays come from a PoseRefiner: the same bits
as without it at zero corrections, a gradient that reaches delta, Adam steps that move it."""
import importlib

import numpy as np
import pytest
import torch

from tests import lens_model as lm
from tests import pose_refine_model as pm
from tests.test_gpu_pose_grad import H, W, _intrinsic, _pose
from tests.test_gpu_render import _close, _setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


# ---- f2n_cam_pose_grad ---------------------------------------------------------------------------

def _run_cam_pose_grad(capi, dev, K, dist, ij, d_o, d_d, cam_start, order, pose_ld, n, E):
    """Two runs from a d_poses full of 7.0 and a workspace full of NaN -> [E, pose_ld] float64."""
    t = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    f32, i32 = torch.float32, torch.int32
    # (one dummy element where there are no rays: the entry wants pointers)
    pad = lambda a, w: a if len(a) else np.zeros((1, w), dtype=a.dtype)
    args = (t(K, f32), t(dist, f32), t(pad(ij, 2), i32), t(pad(d_o, 3), f32), t(pad(d_d, 3), f32),
            t(cam_start, i32), t(order, i32))
    n_ws = capi.lib().cdll.f2n_cam_pose_grad_workspace_floats(n, E)
    outs = []
    for _ in range(2):
        d_poses = torch.full((E, pose_ld), 7.0, device=dev)
        ws = torch.full((n_ws,), float("nan"), device=dev)
        capi.call("cam_pose_grad", *args, d_poses, pose_ld, ws, n, E)
        torch.cuda.synchronize()
        outs.append(d_poses.cpu())
    assert torch.equal(outs[0], outs[1]), "the per-camera sums must be the same bits run to run"
    return outs[0].numpy().astype(np.float64)


def _check_sums(got, pose_ld, t64, cam_start, label):
    ref, mag = pm.sums_f64(t64, cam_start)
    tol = pm.tol(cam_start, mag)
    assert np.isfinite(got).all(), label
    err = np.abs(got[:, :12] - ref)
    ratio = np.divide(err, tol, out=np.zeros_like(err), where=tol > 0)
    print("%s: largest err/tol %.4f" % (label, ratio.max()))
    assert (err <= tol).all(), (label, float(ratio.max()))
    if pose_ld == 16:
        assert (got[:, 12:] == 0).all(), label
    return ref, tol


def _gen_dirs(capi, dev, K, dist, cam, ij):
    """v_r of distorted cameras: rays_d of f2n_gen_rays_dist under identity poses, which is v_r
    exactly (products with 0 and 1) -- an existing, tested kernel, not the code under test."""
    E, n = K.shape[0], ij.shape[0]
    eye = torch.eye(3, 4).expand(E, 3, 4).contiguous().to(dev)
    o = torch.empty(n, 3, device=dev)
    d = torch.empty(n, 3, device=dev)
    capi.call("gen_rays_dist", eye, 12, torch.as_tensor(K).to(dev), torch.as_tensor(dist).to(dev), E,
              torch.as_tensor(cam).to(dev), torch.as_tensor(ij).to(dev), 0, 1, o, d, n)
    torch.cuda.synchronize()
    return d.cpu().numpy()


@pytest.fixture(scope="module")
def case():
    c = pm.counts_case()
    c["K"] = np.tile(lm.intrinsic()[None], (c["E"], 1, 1))
    c["dist"] = np.asarray([lm.SETS[k % len(lm.SETS)] for k in range(c["E"])], dtype=np.float32)
    c["cam_start"] = pm.cam_bounds(c["cam"], c["E"])
    c["perm"] = np.random.default_rng(9).permutation(c["n"])
    return c


@pytest.mark.parametrize("pose_ld", [12, 16])
@pytest.mark.parametrize("lens", ["pinhole", "distorted"])
@pytest.mark.parametrize("shuffled", [False, True])
def test_cam_pose_grad_matches_float64(capi, dev, case, pose_ld, lens, shuffled):
    c = case
    cam, ij, d_o, d_d = c["cam"], c["ij"], c["d_o"], c["d_d"]
    order = None
    if shuffled:
        p = c["perm"]
        cam, ij, d_o, d_d = cam[p], ij[p], d_o[p], d_d[p]
        order = np.argsort(cam, kind="stable").astype(np.int32)
    dist = c["dist"] if lens == "distorted" else None
    v = _gen_dirs(capi, dev, c["K"], dist, cam, ij) if dist is not None else pm.pinhole_dirs32(
        ij, c["K"][cam])
    got = _run_cam_pose_grad(capi, dev, c["K"], dist, ij, d_o, d_d, c["cam_start"], order, pose_ld,
                             c["n"], c["E"])
    t64 = pm.terms(d_o, d_d, v, np.float64)
    if order is not None:
        t64 = t64[order]
    ref, _ = _check_sums(got, pose_ld, t64, c["cam_start"], "%s %s %d" % (lens, shuffled, pose_ld))
    cnt = np.diff(c["cam_start"])
    assert (got[cnt == 0] == 0).all() and (got[pm.ZERO_CAM] == 0).all()
    assert np.abs(ref).max() > 1e3  # the case is not trivially small


@pytest.mark.parametrize("n,E", [(70000, 1), (300, 5000), (0, 3)])
def test_cam_pose_grad_at_the_edges_of_the_partition(capi, dev, n, E):
    rng = np.random.default_rng(n + E)
    cam = np.sort(rng.integers(0, E, n)).astype(np.int32)
    ij = np.stack([rng.integers(0, lm.H, n), rng.integers(0, lm.W, n)], 1).astype(np.int32)
    d = (rng.standard_normal((n, 6)) * np.exp(3.0 * rng.standard_normal((n, 6)))).astype(np.float32)
    d_o, d_d = np.ascontiguousarray(d[:, :3]), np.ascontiguousarray(d[:, 3:])
    K = np.tile(lm.intrinsic()[None], (E, 1, 1))
    cam_start = pm.cam_bounds(cam, E)
    assert n == 0 or E > 1 or n > 64 * pm.PIECE
    for pose_ld in (12, 16):
        got = _run_cam_pose_grad(capi, dev, K, None, ij, d_o, d_d, cam_start, None, pose_ld, n, E)
        if n == 0:
            assert (got == 0).all()
            continue
        v = pm.pinhole_dirs32(ij, K[cam])
        _check_sums(got, pose_ld, pm.terms(d_o, d_d, v, np.float64), cam_start, "n %d E %d" % (n, E))
        assert (got[np.diff(cam_start) == 0] == 0).all()


def test_cam_pose_grad_agrees_with_gen_rays_bwd_per_ray(capi, dev, case):
    """f2n_gen_rays_bwd with one pose per ray, its [n,3,4] blocks summed per camera in float64."""
    c = case
    n, E = c["n"], c["E"]
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    per_ray = torch.full((n, 12), 7.0, device=dev)
    ws = torch.empty(capi.lib().cdll.f2n_gen_rays_bwd_workspace_floats(n), device=dev)
    capi.call("gen_rays_bwd", to(c["K"][c["cam"]]), n, to(c["ij"]), 0, 1, to(c["d_o"]), to(c["d_d"]),
              per_ray, 12, ws, n)
    torch.cuda.synchronize()
    t64 = per_ray.cpu().numpy().astype(np.float64)
    got = _run_cam_pose_grad(capi, dev, c["K"], None, c["ij"], c["d_o"], c["d_d"], c["cam_start"],
                             None, 12, n, E)
    _check_sums(got, 12, t64, c["cam_start"], "against gen_rays_bwd")


# ---- f2n_pose_compose ----------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [3, 4])
def test_pose_compose_and_backward_match_float64(capi, dev, rows):
    c = pm.compose_case(rows)
    E, pose_ld = c["E"], rows * 4
    base, delta, fixed, d_out = (torch.as_tensor(c[k]) for k in ("base", "delta", "fixed", "d_out"))
    d64 = delta.to(torch.float64).requires_grad_(True)
    ref = pm.compose_ref(base, d64, fixed)
    (ref_grad,) = torch.autograd.grad(ref, d64, d_out.to(torch.float64))
    runs = []
    for _ in range(2):
        out = torch.full((E, 3, 4), 7.0, device=dev)
        d_delta = torch.full((E, 6), 7.0, device=dev)
        capi.call("pose_compose", base.to(dev), pose_ld, delta.to(dev), fixed.to(dev), out, E)
        capi.call("pose_compose_bwd", base.to(dev), pose_ld, delta.to(dev), fixed.to(dev),
                  d_out.to(dev), d_delta, E)
        torch.cuda.synchronize()
        runs.append((out.cpu(), d_delta.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    out, d_delta = runs[0]
    # forward: one ulp of the rounded float64 value (f64 inside, so at most a double rounding)
    r64 = ref.detach().numpy()
    r32 = r64.astype(np.float32).astype(np.float64)
    assert (np.abs(out.numpy().astype(np.float64) - r32) <= pm.ulp32(r64)).all()
    Rn = out[:, :, :3].to(torch.float64)
    eye = torch.eye(3, dtype=torch.float64)
    assert float((Rn.transpose(1, 2) @ Rn - eye).abs().max()) <= 4 * pm.U
    # zero corrections and fixed cameras: the base rows, bit for bit
    keep = (delta.abs().sum(1) == 0) | (fixed != 0)
    assert int(keep.sum()) >= E // 3 + 1 and int((delta.abs().sum(1) == 0).sum()) >= 1
    assert torch.equal(out[keep], base[keep][:, :3, :])
    assert not torch.equal(out[~keep], base[~keep][:, :3, :])
    # no fixed list at all: the same for the cameras that are free
    out_free = torch.empty(E, 3, 4, device=dev)
    capi.call("pose_compose", base.to(dev), pose_ld, delta.to(dev), None, out_free, E)
    assert torch.equal(out_free.cpu()[fixed == 0], out[fixed == 0])
    # backward: one ulp of the float64 autograd value; fixed cameras exact zeros
    g64 = ref_grad.numpy()
    assert (np.abs(d_delta.numpy().astype(np.float64) - g64) <= pm.ulp32(g64)).all()
    assert float(d_delta[fixed != 0].abs().max()) == 0.0
    assert float(d_delta[fixed == 0].abs().min()) > 0.0


def test_pose_compose_bindings_carry_the_gradient(host, dev):
    c = pm.compose_case(3)
    base, fixed, d_out = (torch.as_tensor(c[k]).to(dev) for k in ("base", "fixed", "d_out"))
    delta = torch.as_tensor(c["delta"]).to(dev).requires_grad_(True)
    out = host.pose_compose(base, delta, fixed)
    (out * d_out).sum().backward()
    assert torch.equal(delta.grad, host.pose_compose_bwd(base, delta.detach(), fixed, d_out))


# ---- end to end ------------------------------------------------------------------------------------

N_CAMS, N_RAYS, NO_RAYS, FIXED = 8, 300, 5, 2


@pytest.fixture(scope="module")
def scene(host, dev):
    """The small Renderer of test_gpu_pose_grad._view_setup (L 8, F 2, T 2^14, S 64) with one
    embedding per camera, 8 cameras, 300 rays with given cameras and pixels; camera NO_RAYS gets
    none, camera FIXED is fixed."""
    oracle, hr, o, d, noise, bg, gt, emb = _setup(host, 8, 2, 14, 64, 4.0 / 64, N_RAYS, 3.0, 29,
                                                  E=N_CAMS)
    g = torch.Generator().manual_seed(31)
    base = _pose(g, N_CAMS)
    K = _intrinsic(N_CAMS, H, W)
    cam = torch.randint(0, N_CAMS - 1, (N_RAYS,), generator=g)
    cam = torch.where(cam >= NO_RAYS, cam + 1, cam).to(torch.int32)  # not sorted
    ij = torch.stack([torch.randint(0, H, (N_RAYS,), generator=g),
                      torch.randint(0, W, (N_RAYS,), generator=g)], 1).to(torch.int32)
    hr.set_fused_ray_grad(True)
    to = lambda x: x.to(dev)
    return dict(hr=hr, base=to(base), K=to(K), cam=to(cam), ij=to(ij), noise=to(noise), bg=to(bg),
                gt=to(gt))


def _step(s, o, d):
    s["hr"].zero_grad()
    loss, *_ = s["hr"].train_step(o, d, s["cam"], s["gt"], 1e-2, s["noise"], s["bg"], True)
    return loss.detach().cpu(), {k: v.detach().cpu().clone() for k, v in s["hr"].grads().items()
                                 if v is not None}


def test_training_step_through_the_refiner(host, dev, scene):
    s = scene
    refiner = host.PoseRefiner(s["base"])
    mask = torch.zeros(N_CAMS, dtype=torch.bool)
    mask[FIXED] = True
    refiner.set_fixed(mask.to(dev))
    assert torch.equal(refiner.poses().detach(), s["base"])
    # (a) zero corrections: the rays and the loss of a run without the refiner
    o, d, gt, cam = refiner.sample_random_rays(s["K"], H, W, N_RAYS, cam_idx=s["cam"], ij=s["ij"])
    assert gt is None and torch.equal(cam, s["cam"])
    assert o.requires_grad and d.requires_grad
    with torch.no_grad():
        o0, d0 = host.get_rays_from_cameras(s["base"], s["K"], s["cam"], s["ij"])
    assert torch.equal(o.detach(), o0) and torch.equal(d.detach(), d0)
    o_leaf, d_leaf = o0.clone().requires_grad_(True), d0.clone().requires_grad_(True)
    loss_leaf, grads_leaf = _step(s, o_leaf, d_leaf)
    assert o_leaf.grad is not None and float(d_leaf.grad.abs().max()) > 0
    refiner.zero_grad()
    loss, grads = _step(s, o, d)
    assert torch.equal(loss, loss_leaf), (float(loss), float(loss_leaf))
    # (b) delta.grad against the float64 chain from the leaf run's own ray gradients
    got = refiner.delta.grad
    assert got is not None, "delta.grad is undefined: the batch has no path back to its poses"
    got = got.cpu().numpy().astype(np.float64)
    order = np.argsort(s["cam"].cpu().numpy(), kind="stable")
    cam_sorted = s["cam"].cpu().numpy()[order]
    cam_start = pm.cam_bounds(cam_sorted, N_CAMS)
    v = pm.pinhole_dirs32(s["ij"].cpu().numpy(), s["K"].cpu().numpy()[s["cam"].cpu().numpy()])
    t64 = pm.terms(o_leaf.grad.cpu().numpy(), d_leaf.grad.cpu().numpy(), v, np.float64)[order]
    sums, mag = pm.sums_f64(t64, cam_start)
    tol = pm.tol(cam_start, mag)                                   # [E,12]
    base64 = s["base"].cpu()
    fixed = refiner.fixed.cpu()
    d0_64 = torch.zeros(N_CAMS, 6, dtype=torch.float64, requires_grad=True)
    ref_poses = pm.compose_ref(base64, d0_64, fixed)
    (ref,) = torch.autograd.grad(ref_poses, d0_64, torch.as_tensor(sums).reshape(N_CAMS, 3, 4))
    jac = torch.autograd.functional.jacobian(lambda x: pm.compose_ref(base64, x, fixed),
                                             torch.zeros(N_CAMS, 6, dtype=torch.float64))
    jac = torch.stack([jac[c, :, :, c, :] for c in range(N_CAMS)]).reshape(N_CAMS, 12, 6).abs()
    bound = torch.einsum("cek,ce->ck", jac, torch.as_tensor(tol)).numpy() + pm.ulp32(ref.numpy())
    err = np.abs(got - ref.numpy())
    print("delta.grad: largest err/bound %.4f" % float(np.max(err / np.maximum(bound, 1e-300))))
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
    with_rays = [c for c in range(N_CAMS) if c not in (NO_RAYS, FIXED)]
    assert (np.abs(got[with_rays]).max(1) > 0).all()
    assert (got[NO_RAYS] == 0).all() and (got[FIXED] == 0).all()
    # (c) the field's gradients are those of the leaf run (float-atomic sums: the tolerances that
    # test_gpu_render.py holds the same gradients to)
    assert set(grads) == set(grads_leaf) and "scene_field.feat_pool" in grads
    for k in grads:
        if k.endswith("feat_pool"):
            _close(grads[k], grads_leaf[k], 2e-3, 1e-3)
        else:
            _close(grads[k], grads_leaf[k], 1e-3, 1e-3)
    # (d) three Adam steps
    adam = refiner.make_adam(1e-3)
    assert adam.n_groups() == 1
    for _ in range(3):
        adam.zero_grad()
        o, d, _, _ = refiner.sample_random_rays(s["K"], H, W, N_RAYS, cam_idx=s["cam"], ij=s["ij"])
        _step(s, o, d)
        adam.step()
    delta = refiner.delta.detach().cpu()
    assert (delta[with_rays].abs().max(1).values > 0).all()
    assert float(delta[NO_RAYS].abs().max()) == 0.0 and float(delta[FIXED].abs().max()) == 0.0
    norms = refiner.correction_norms().cpu()
    assert norms.shape == (N_CAMS, 2)
    torch.testing.assert_close(norms[:, 0], delta[:, :3].norm(dim=1))
    poses = refiner.poses().detach().cpu()
    assert torch.equal(poses[FIXED], s["base"].cpu()[FIXED])
    assert not torch.equal(poses[with_rays[0]], s["base"].cpu()[with_rays[0]])


def test_refiner_draws_sorted_cameras_and_round_trips(host, dev, scene, tmp_path):
    s = scene
    refiner = host.PoseRefiner(s["base"])
    images = torch.rand(N_CAMS, H, W, 3, device=dev)
    o, d, gt, cam = refiner.sample_random_rays(s["K"], H, W, 257, images=images)
    assert o.shape == (257, 3) and gt.shape == (257, 3) and cam.dtype == torch.int32
    assert bool((cam[1:] >= cam[:-1]).all()) and int(cam.min()) >= 0 and int(cam.max()) < N_CAMS
    (o.sum() + (d * d).sum()).backward()
    assert refiner.delta.grad is not None and float(refiner.delta.grad.abs().max()) > 0
    # (e) save / load
    with torch.no_grad():
        refiner.delta.copy_(torch.randn(N_CAMS, 6, device=dev) * 0.01)
    mask = torch.zeros(N_CAMS, dtype=torch.int32, device=dev)
    mask[FIXED] = 1
    refiner.set_fixed(mask)
    path = str(tmp_path / "pose_refiner.pt")
    refiner.save(path)
    other = host.PoseRefiner(torch.zeros(N_CAMS, 3, 4, device=dev))
    other.load(path)
    assert torch.equal(other.delta, refiner.delta) and torch.equal(other.base, refiner.base)
    assert torch.equal(other.fixed, refiner.fixed) and int(other.fixed.sum()) == 1
    assert torch.equal(other.poses(), refiner.poses())
