"""Calibration refinement on the GPU: f2n_cam_intr_grad against the float64 terms of
tests/intr_refine_model.py within TERM_TOL per ray and within the derived bound per camera,
f2n_intr_compose and its backward against float64, get_rays_from_calibrated_cameras against today's
route and the C ABI, a training step whose rays come from an IntrinsicsRefiner (the same bits as
without it at gamma = 0, a gradient that reaches gamma, Adam steps that move the learned columns),
and the calibration recovered from rays alone."""
import importlib

import numpy as np
import pytest
import torch

from tests import intr_refine_model as im
from tests import lens_model as lm
from tests import pose_refine_model as pm
from tests.test_gpu_pose_grad import H, W
from tests.test_gpu_pose_refine import FIXED, N_CAMS, N_RAYS, NO_RAYS, _gen_dirs, scene  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def _dev(a, dev, dtype):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


def _poses(R, rows):
    """[E,rows,4] float32: the rotations, a translation that must not matter, row 3 of a [4,4]."""
    E = R.shape[0]
    t = np.linspace(-1.0, 1.0, 3 * E, dtype=np.float32).reshape(E, 3, 1)
    P = np.concatenate([R, t], 2)
    if rows == 4:
        P = np.concatenate([P, np.tile(np.array([[[0, 0, 0, 1]]], dtype=np.float32), (E, 1, 1))], 1)
    return np.ascontiguousarray(P.astype(np.float32))


def _run_cam_intr_grad(capi, dev, poses, K, dist, ij, d_d, cam_start, order, n, E):
    """Two runs from a d_intr full of 7.0 and a workspace full of NaN -> [E,8] float64."""
    f32, i32 = torch.float32, torch.int32
    pad = lambda a, w: a if len(a) else np.zeros((1, w), dtype=a.dtype)  # the entry wants pointers
    pose_ld = poses.shape[1] * 4
    args = (_dev(poses, dev, f32), pose_ld, _dev(K, dev, f32), _dev(dist, dev, f32),
            _dev(pad(ij, 2), dev, i32), _dev(pad(d_d, 3), dev, f32), _dev(cam_start, dev, i32),
            _dev(order, dev, i32))
    n_ws = capi.lib().cdll.f2n_cam_intr_grad_workspace_floats(n, E)
    outs = []
    for _ in range(2):
        d_intr = torch.full((E, 8), 7.0, device=dev)
        ws = torch.full((n_ws,), float("nan"), device=dev)
        capi.call("cam_intr_grad", *args, d_intr, ws, n, E)
        torch.cuda.synchronize()
        outs.append(d_intr.cpu())
    assert torch.equal(outs[0], outs[1]), "the per-camera sums must be the same bits run to run"
    return outs[0].numpy().astype(np.float64)


def _forward_xy(capi, dev, K, dist, cam, ij):
    """The forward's ideal point per ray, from existing kernels: f2n_gen_rays_dist under identity
    poses (test_gpu_pose_refine._gen_dirs), or the pinhole expression."""
    v = _gen_dirs(capi, dev, K, dist, cam, ij) if dist is not None else pm.pinhole_dirs32(ij, K[cam])
    return v[:, 0], -v[:, 1]


# ---- per-ray terms ---------------------------------------------------------------------------------

@pytest.mark.parametrize("which", range(6))
def test_cam_intr_grad_terms_match_float64(capi, dev, which):
    """One camera per ray (cam_start = arange): d_intr rows are the per-ray terms."""
    c = im.term_case(which)
    n = c["n"]
    K = np.tile(c["K"][None], (n, 1, 1))
    dist = np.tile(c["k"][None], (n, 1)) if which < 5 else None  # the zero set: a NULL table
    cam = np.arange(n, dtype=np.int32)
    x, y = _forward_xy(capi, dev, K, dist, cam, c["ij"])
    got = _run_cam_intr_grad(capi, dev, _poses(c["R"], 3), K, dist, c["ij"], c["d_d"],
                             np.arange(n + 1), None, n, n)
    t64, mag = im.ray_terms(c["ij"], c["K"], c["k"], x, y, c["R"], c["d_d"], np.float64)
    assert np.isfinite(got).all() and (mag > 0).all()
    ratio = np.abs(got - t64) / (im.TERM_TOL * mag)
    print("set %d: largest err / (TERM_TOL mag) per parameter %s" % (which, np.round(ratio.max(0), 3)))
    assert (ratio <= 1.0).all(), ratio.max(0)
    assert (np.abs(got).max(0) > 0).all()  # every column is fed


def test_zero_coefficient_rows_give_the_pinhole_bits(capi, dev):
    c = im.term_case(5)
    n = c["n"]
    K = np.tile(c["K"][None], (n, 1, 1))
    args = (_poses(c["R"], 3), K)
    rest = (c["ij"], c["d_d"], np.arange(n + 1), None, n, n)
    null = _run_cam_intr_grad(capi, dev, *args, None, *rest)
    zeros = _run_cam_intr_grad(capi, dev, *args, np.zeros((n, 4), dtype=np.float32), *rest)
    assert (null == zeros).all() and np.abs(null[:, 4:]).max() > 0


# ---- per-camera sums -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def case():
    c = pm.counts_case()
    c["K"] = np.tile(lm.intrinsic()[None], (c["E"], 1, 1))
    c["dist"] = np.asarray([lm.SETS[k % len(lm.SETS)] for k in range(c["E"])], dtype=np.float32)
    c["R"] = lm.rotations(c["E"], 13)
    c["cam_start"] = pm.cam_bounds(c["cam"], c["E"])
    c["perm"] = np.random.default_rng(9).permutation(c["n"])
    return c


def _check_sums(got, t64, mag, cam_start, label):
    ref, abs_sums = im.sums_f64(t64, cam_start)
    tol = im.sum_tol(cam_start, abs_sums, im.sums_f64(mag, cam_start)[0])
    assert np.isfinite(got).all(), label
    err = np.abs(got - ref)
    ratio = np.divide(err, tol, out=np.zeros_like(err), where=tol > 0)
    print("%s: largest err/tol %.4f" % (label, ratio.max()))
    assert (err <= tol).all(), (label, float(ratio.max()))
    return ref


@pytest.mark.parametrize("rows", [3, 4])
@pytest.mark.parametrize("lens", ["pinhole", "distorted"])
@pytest.mark.parametrize("shuffled", [False, True])
def test_cam_intr_grad_sums_match_float64(capi, dev, case, rows, lens, shuffled):
    c = case
    cam, ij, d_d = c["cam"], c["ij"], c["d_d"]
    order = None
    if shuffled:
        p = c["perm"]
        cam, ij, d_d = cam[p], ij[p], d_d[p]
        order = np.argsort(cam, kind="stable").astype(np.int32)
    dist = c["dist"] if lens == "distorted" else None
    x, y = _forward_xy(capi, dev, c["K"], dist, cam, ij)
    got = _run_cam_intr_grad(capi, dev, _poses(c["R"], rows), c["K"], dist, ij, d_d, c["cam_start"],
                             order, c["n"], c["E"])
    k = c["dist"][cam] if dist is not None else np.zeros((c["n"], 4), dtype=np.float32)
    t64, mag = im.ray_terms(ij, c["K"][cam], k, x, y, c["R"][cam], d_d, np.float64)
    if order is not None:
        t64, mag = t64[order], mag[order]
    ref = _check_sums(got, t64, mag, c["cam_start"], "%s %s %d" % (lens, shuffled, rows))
    cnt = np.diff(c["cam_start"])
    assert (got[cnt == 0] == 0).all() and (got[pm.ZERO_CAM] == 0).all()
    assert np.abs(ref).max() > 1e2  # the case is not trivially small


@pytest.mark.parametrize("n,E", [(70000, 1), (300, 5000), (0, 3)])
def test_cam_intr_grad_at_the_edges_of_the_partition(capi, dev, n, E):
    rng = np.random.default_rng(n + E)
    cam = np.sort(rng.integers(0, E, n)).astype(np.int32)
    ij = np.stack([rng.integers(0, lm.H, n), rng.integers(0, lm.W, n)], 1).astype(np.int32)
    d_d = (rng.standard_normal((n, 3)) * np.exp(3.0 * rng.standard_normal((n, 3)))).astype(np.float32)
    K = np.tile(lm.intrinsic()[None], (E, 1, 1))
    R = lm.rotations(8, 5)[np.arange(E) % 8]
    cam_start = pm.cam_bounds(cam, E)
    assert n == 0 or E > 1 or n > 64 * pm.PIECE
    for rows in (3, 4):
        got = _run_cam_intr_grad(capi, dev, _poses(R, rows), K, None, ij, d_d, cam_start, None, n, E)
        if n == 0:
            assert (got == 0).all()
            continue
        x, y = _forward_xy(capi, dev, K, None, cam, ij)
        t64, mag = im.ray_terms(ij, K[cam], np.zeros((n, 4), dtype=np.float32), x, y, R[cam], d_d,
                                np.float64)
        _check_sums(got, t64, mag, cam_start, "n %d E %d" % (n, E))
        assert (got[np.diff(cam_start) == 0] == 0).all()


# ---- f2n_intr_compose ----------------------------------------------------------------------------

def _compose_case(E, G, seed=3):
    rng = np.random.default_rng(seed + E + G)
    K = np.tile(lm.intrinsic()[None], (E, 1, 1)) * (1.0 + 0.1 * rng.random((E, 1, 1)))
    K[:, 2, 2] = 1.0
    K[:, 0, 1] = 0.25  # a skew entry: copied, not touched
    dist = np.asarray([lm.SETS[e % len(lm.SETS)] for e in range(E)], dtype=np.float32)
    gamma = (rng.standard_normal((G, 8)) * 0.05).astype(np.float32)
    group = rng.integers(0, G, E).astype(np.int32)
    if G >= 3:
        group[group == 1] = 0   # an empty group
        gamma[2] = 0.0          # a group whose correction is zero
    if E > 4:
        group[3] = -1           # a fixed image
        group[4] = -7
    return K.astype(np.float32), dist, gamma, group


def _run_compose(capi, dev, K, dist, gamma, group):
    E, G = K.shape[0], gamma.shape[0]
    f32, i32 = torch.float32, torch.int32
    out_K = torch.full((E, 3, 3), 7.0, device=dev)
    out_dist = torch.full((E, 4), 7.0, device=dev)
    capi.call("intr_compose", _dev(K, dev, f32), _dev(dist, dev, f32), _dev(gamma, dev, f32),
              _dev(group, dev, i32), out_K, out_dist, E, G)
    torch.cuda.synchronize()
    return out_K.cpu().numpy(), out_dist.cpu().numpy()


@pytest.mark.parametrize("E,G", [(1, 1), (65, 1), (65, 3), (65, 65)])
def test_intr_compose_and_backward_match_float64(capi, dev, E, G):
    K, dist, gamma, group = _compose_case(E, G)
    # zero gamma: the base rows, bit for bit
    zK, zD = _run_compose(capi, dev, K, dist, np.zeros_like(gamma), group)
    assert (zK.view(np.int32) == K.view(np.int32)).all() and (zD.view(np.int32) == dist.view(np.int32)).all()
    # random gamma: one float32 ulp of float64 (f64 inside, rounded once); the rest of K copied
    oK, oD = _run_compose(capi, dev, K, dist, gamma, group)
    rK, rD = im.compose64(K, dist, gamma, group)
    assert (np.abs(oK.astype(np.float64) - rK) <= pm.ulp32(rK)).all()
    assert (np.abs(oD.astype(np.float64) - rD) <= pm.ulp32(rD)).all()
    untouched = np.ones((3, 3), dtype=bool)
    untouched[0, 0] = untouched[1, 1] = untouched[0, 2] = untouched[1, 2] = False
    assert (oK[:, untouched] == K[:, untouched]).all()
    keep = (group < 0) | ~gamma[np.maximum(group, 0)].any(1)
    assert (oK[keep] == K[keep]).all() and (oD[keep] == dist[keep]).all()
    assert (oK[~keep][:, 0, 0] != K[~keep][:, 0, 0]).all()
    # no coefficient table: zeros
    nK, nD = _run_compose(capi, dev, K, None, gamma, group)
    assert (nK == oK).all()
    assert (np.abs(nD.astype(np.float64) - im.compose64(K, None, gamma, group)[1]) == 0).all()
    # backward
    rng = np.random.default_rng(E * 7 + G)
    d_K = rng.standard_normal((E, 3, 3)).astype(np.float32)
    d_dist = (rng.standard_normal((E, 4)) * np.exp(rng.standard_normal((E, 4)))).astype(np.float32)
    learn = np.array([1, 1, 0, 1, 1, 0, 1, 1], dtype=np.int32)
    f32, i32 = torch.float32, torch.int32

    def bwd(learn_, d_K_, d_dist_):
        runs = []
        for _ in range(2):
            d_gamma = torch.full((G, 8), 7.0, device=dev)
            capi.call("intr_compose_bwd", _dev(K, dev, f32), _dev(dist, dev, f32), _dev(gamma, dev, f32),
                      _dev(group, dev, i32), _dev(learn_, dev, i32), _dev(d_K_, dev, f32),
                      _dev(d_dist_, dev, f32), d_gamma, E, G)
            torch.cuda.synchronize()
            runs.append(d_gamma.cpu())
        assert torch.equal(runs[0], runs[1]), "the same bits run to run"
        return runs[0].numpy().astype(np.float64)

    for learn_, d_K_, d_dist_ in ((learn, d_K, d_dist), (None, d_K, d_dist), (None, None, d_dist),
                                  (None, d_K, None)):
        got = bwd(learn_, d_K_, d_dist_)
        ref, mag, cnt = im.compose_bwd64(K, gamma, group, learn_, d_K_, d_dist_)
        assert (np.abs(got - ref) <= im.compose_bwd_tol(ref, mag, cnt)).all()
        assert (got[cnt == 0] == 0).all()
        if learn_ is not None:
            assert (got[:, learn_ == 0] == 0).all() and np.abs(got[:, learn_ != 0]).max() > 0
        if d_K_ is None:
            assert (got[:, :4] == 0).all()
        if d_dist_ is None:
            assert (got[:, 4:] == 0).all()
    if G >= 3:
        assert cnt[1] == 0 and cnt.sum() == E - 2


# ---- host ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def batch(dev):
    g = np.random.default_rng(21)
    E, n = 5, 300
    R = lm.rotations(E, 21)
    t = (g.standard_normal((E, 3, 1)) * 0.2).astype(np.float32)
    cam = g.integers(0, E, n).astype(np.int32)
    cam[cam == 3] = 2  # camera 3 has no rays
    ij = np.stack([g.integers(0, lm.H, n), g.integers(0, lm.W, n)], 1).astype(np.int32)
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    return dict(E=E, n=n, poses=to(np.concatenate([R, t], 2)), K=to(np.tile(lm.intrinsic()[None], (E, 1, 1))),
                dist=to(np.asarray(lm.SETS, dtype=np.float32)), cam=to(cam), ij=to(ij),
                w_o=to(g.standard_normal((n, 3)).astype(np.float32)),
                w_d=to(g.standard_normal((n, 3)).astype(np.float32)), cam_np=cam)


def _calibrated(host, b, want, dist=True):
    leaf = lambda x, on: x.clone().requires_grad_(on)
    poses, K = leaf(b["poses"], "poses" in want), leaf(b["K"], "K" in want)
    D = leaf(b["dist"], "dist" in want) if dist else None
    o, d = host.get_rays_from_calibrated_cameras(poses, K, D, b["cam"], b["ij"])
    if want:
        ((o * b["w_o"]).sum() + (d * b["w_d"]).sum()).backward()
    return o.detach(), d.detach(), poses.grad, K.grad, None if D is None else D.grad


@pytest.mark.parametrize("lens", ["distorted", "pinhole"])
def test_calibrated_rays_and_their_gradients(host, capi, dev, batch, lens):
    b = batch
    D = b["dist"] if lens == "distorted" else None
    with torch.no_grad():
        o0, d0 = host.get_rays_from_cameras(b["poses"], b["K"], b["cam"], b["ij"], dist=D)
    p_old = b["poses"].clone().requires_grad_(True)
    o1, d1 = host.get_rays_from_cameras(p_old, b["K"], b["cam"], b["ij"], dist=D)
    ((o1 * b["w_o"]).sum() + (d1 * b["w_d"]).sum()).backward()
    o, d, gp, gK, gD = _calibrated(host, b, ("poses", "K", "dist"), dist=D is not None)
    assert torch.equal(o, o0) and torch.equal(d, d0), "the rays of get_rays_from_cameras"
    assert torch.equal(gp, p_old.grad), "poses.grad of today's route, bit for bit"
    # the C ABI on the same batch
    order = np.argsort(b["cam_np"], kind="stable").astype(np.int32)
    cam_start = pm.cam_bounds(b["cam_np"][order], b["E"])
    want = _run_cam_intr_grad(capi, dev, b["poses"].cpu().numpy(), b["K"].cpu().numpy(),
                              None if D is None else D.cpu().numpy(), b["ij"].cpu().numpy(),
                              b["w_d"].cpu().numpy(), cam_start, order, b["n"], b["E"])
    want = torch.as_tensor(want, dtype=torch.float32)
    gK = gK.cpu()
    assert torch.equal(torch.stack([gK[:, 0, 0], gK[:, 1, 1], gK[:, 0, 2], gK[:, 1, 2]], 1), want[:, :4])
    assert float(gK[:, 0, 1].abs().max()) == 0 and float(gK[:, 1, 0].abs().max()) == 0
    assert float(gK[:, 2].abs().max()) == 0 and float(want[[0, 1, 2, 4]].abs().min()) > 0
    assert float(want[3].abs().max()) == 0  # the camera without rays
    if D is not None:
        assert gD.shape == D.shape and torch.equal(gD.cpu(), want[:, 4:])
    else:
        assert gD is None


def test_gradients_are_formed_only_where_asked(host, batch):
    b = batch
    o0, d0, *_ = _calibrated(host, b, ())
    for want in (("K",), ("dist",), ("poses",), ("poses", "dist")):
        o, d, gp, gK, gD = _calibrated(host, b, want)
        assert torch.equal(o, o0) and torch.equal(d, d0)
        assert (gp is not None) == ("poses" in want), want
        assert (gK is not None) == ("K" in want), want
        assert (gD is not None) == ("dist" in want), want
    _, _, gp_all, gK_all, gD_all = _calibrated(host, b, ("poses", "K", "dist"))
    assert torch.equal(_calibrated(host, b, ("K",))[3], gK_all)
    assert torch.equal(_calibrated(host, b, ("dist",))[4], gD_all)
    assert torch.equal(_calibrated(host, b, ("poses",))[2], gp_all)


def test_intr_compose_bindings_carry_the_gradient(host, dev):
    K, dist, gamma, group = _compose_case(65, 3)
    to = lambda a: torch.as_tensor(a).to(dev)
    g = to(gamma).requires_grad_(True)
    learn = to(np.array([1, 0, 1, 1, 1, 1, 0, 1], dtype=np.int32))
    Kn, Dn = host.intr_compose(to(K), to(dist), g, to(group), learn)
    wK, wD = torch.randn_like(Kn), torch.randn_like(Dn)
    ((Kn * wK).sum() + (Dn * wD).sum()).backward()
    assert torch.equal(g.grad, host.intr_compose_bwd(to(K), to(dist), g.detach(), to(group), learn, wK, wD))
    assert float(g.grad[:, [1, 6]].abs().max()) == 0 and float(g.grad[0].abs().max()) > 0
    with pytest.raises(RuntimeError, match="group holds an entry"):
        host.intr_compose(to(K), to(dist), g, to(group) + 3, learn)


# ---- end to end ------------------------------------------------------------------------------------

def _step(host, s, o, d):
    s["hr"].zero_grad()
    out = s["hr"].train_step_supervised(o, d, s["cam"], s["gt"], host.RaySupervision(want_colors=True),
                                        1e-2, s["noise"], s["bg"], True)
    torch.cuda.synchronize()
    grads = {k: v.detach().cpu().clone() for k, v in s["hr"].grads().items() if v is not None}
    return out[0].detach().cpu(), out[5].detach().cpu(), grads


@pytest.fixture(scope="module")
def zero_gamma_runs(host, dev, scene):  # noqa: F811
    """One batch twice: (a) from PoseRefiner::sample_random_rays, (b) through an IntrinsicsRefiner at
    gamma = 0 on top of the same PoseRefiner."""
    s = scene
    poser = host.PoseRefiner(s["base"])
    mask = torch.zeros(N_CAMS, dtype=torch.bool)
    mask[FIXED] = True
    poser.set_fixed(mask.to(dev))
    calib = host.IntrinsicsRefiner(s["K"])
    o, d, _, _ = poser.sample_random_rays(s["K"], H, W, N_RAYS, cam_idx=s["cam"], ij=s["ij"])
    run_a = _step(host, s, o, d)
    delta_a = poser.delta.grad.detach().cpu().clone()
    poser.zero_grad()
    o1, d1, gt, cam = calib.sample_random_rays(poser.poses(), H, W, N_RAYS, cam_idx=s["cam"], ij=s["ij"])
    run_b = _step(host, s, o1, d1)
    return dict(calib=calib, rays_a=(o.detach(), d.detach()), rays_b=(o1.detach(), d1.detach()), gt=gt,
                cam=cam, run_a=run_a, run_b=run_b, delta_a=delta_a,
                delta_b=poser.delta.grad.detach().cpu().clone(),
                gamma_grad=None if calib.gamma.grad is None else calib.gamma.grad.detach().cpu().clone())


def test_training_step_through_both_refiners(host, dev, scene, zero_gamma_runs):  # noqa: F811
    s, z = scene, zero_gamma_runs
    fresh = host.IntrinsicsRefiner(s["K"])
    assert fresh.n_groups == 1 and fresh.gamma.shape == (1, 8)
    assert torch.equal(fresh.intrinsics().detach(), s["K"])
    assert float(fresh.dist().detach().abs().max()) == 0 and float(fresh.corrections().abs().max()) == 0
    # gamma = 0: the rays, the loss and the colours of the batch without the calibration refiner
    assert z["gt"] is None and torch.equal(z["cam"], s["cam"])
    assert torch.equal(z["rays_b"][0], z["rays_a"][0]) and torch.equal(z["rays_b"][1], z["rays_a"][1])
    (loss_a, colors_a, _), (loss_b, colors_b, _) = z["run_a"], z["run_b"]
    assert torch.equal(loss_b, loss_a) and torch.equal(colors_b, colors_a)
    assert float(z["delta_a"].abs().max()) > 0
    print("delta.grad: largest difference %.3e" % float((z["delta_b"] - z["delta_a"]).abs().max()))
    assert torch.equal(z["delta_b"], z["delta_a"]), "delta.grad is unchanged by the second refiner"
    g = z["gamma_grad"]
    assert g is not None, "gamma.grad is undefined: the batch has no path back to the calibration"
    assert bool(torch.isfinite(g).all()) and float(g.abs().min()) > 0
    calib = z["calib"]
    # (c) a few Adam steps move gamma in the learned columns only
    learned = [True, True, False, False, True, False, False, True]
    calib.set_learned(learned)
    assert calib.learn.cpu().tolist() == [int(x) for x in learned]
    adam = calib.make_adam(1e-3)
    assert adam.n_groups() == 1
    for _ in range(3):
        adam.zero_grad()
        o3, d3, _, _ = calib.sample_random_rays(s["base"], H, W, N_RAYS, cam_idx=s["cam"], ij=s["ij"])
        _step(host, s, o3, d3)
        adam.step()
    gamma = calib.gamma.detach().cpu()[0]
    keep = torch.tensor(learned)
    assert float(gamma[~keep].abs().max()) == 0 and float(gamma[keep].abs().min()) > 0
    corr = calib.corrections().cpu()
    assert corr.shape == (N_CAMS, 8) and float(corr[:, [0, 1, 4, 7]].abs().min()) > 0
    assert float(corr[:, [2, 3, 5, 6]].abs().max()) == 0
    # fixed images keep the base calibration
    fixed = torch.zeros(N_CAMS, dtype=torch.int32, device=dev)
    fixed[FIXED] = 1
    calib.set_fixed(fixed)
    Kn = calib.intrinsics().detach()
    assert torch.equal(Kn[FIXED], s["K"][FIXED]) and not torch.equal(Kn[0], s["K"][0])
    assert calib.group.cpu().tolist() == [-1 if e == FIXED else 0 for e in range(N_CAMS)]
    calib.set_fixed(torch.zeros_like(fixed))
    assert calib.group.cpu().tolist() == [0] * N_CAMS


@pytest.mark.parametrize("ray", [0, 1, 2])
def test_parameter_gradients_at_zero_gamma_are_those_without_the_refiner(host, dev, scene, ray):  # noqa: F811
    """Every parameter gradient of a step through both refiners at gamma = 0, bit for bit against the
    step on the same batch from PoseRefiner::sample_random_rays, with the loss and the colours.

    The batch is one ray.  The gradients of app_emb and of the two networks are float-atomic sums of
    the step itself (f2n_scatter_add_bwd, the shade backward), and a float sum is free of its order
    only while at most two addends meet in an element: one ray is at most 64 samples, which no kernel
    of the step spreads over more than two wavefronts.  On the 300 rays of
    test_training_step_through_both_refiners two calls of the SAME PoseRefiner step, with no
    calibration code in them, differ in these gradients by the last bit or two (app_emb 5.8e-11 to
    8.7e-11 of 4.6e-4, the networks up to 1.9e-9 of 6.3e-3; feat_pool, integer sums, 0), so a
    comparison there would measure that and not the refiner.  That the step repeats itself on this
    batch is asserted first, not assumed."""
    s = dict(scene)
    for k in ("cam", "ij", "gt", "noise", "bg"):
        s[k] = scene[k][ray:ray + 1].contiguous()
    poser = host.PoseRefiner(s["base"])
    calib = host.IntrinsicsRefiner(s["K"])

    def pose_only():
        poser.zero_grad()
        o, d, _, _ = poser.sample_random_rays(s["K"], H, W, 1, cam_idx=s["cam"], ij=s["ij"])
        return _step(host, s, o, d) + (poser.delta.grad.detach().cpu().clone(),)

    def both():
        poser.zero_grad()
        calib.zero_grad()
        o, d, _, _ = calib.sample_random_rays(poser.poses(), H, W, 1, cam_idx=s["cam"], ij=s["ij"])
        return _step(host, s, o, d) + (poser.delta.grad.detach().cpu().clone(),)

    def same(x, y, what):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]), what + ": loss or colours"
        assert set(x[2]) == set(y[2]) and "scene_field.feat_pool" in x[2] and "app_emb" in x[2]
        unequal = {k: float((x[2][k] - y[2][k]).abs().max()) for k in x[2] if not torch.equal(x[2][k], y[2][k])}
        assert not unequal, (what, unequal)
        assert torch.equal(x[3], y[3]), what + ": delta.grad"

    a = pose_only()
    same(pose_only(), a, "the PoseRefiner step against itself")
    same(both(), a, "through both refiners against the PoseRefiner step")
    assert all(float(g.abs().max()) > 0 for k, g in a[2].items() if not k.endswith("feat_pool"))
    assert float(a[3].abs().max()) > 0 and float(calib.gamma.grad.abs().max()) > 0


def test_refiner_draws_sorted_cameras_and_round_trips(host, dev, scene, tmp_path):  # noqa: F811
    s = scene
    group = torch.arange(N_CAMS, device=dev) % 3
    dist = torch.as_tensor(np.asarray([lm.SETS[e % 5] for e in range(N_CAMS)], dtype=np.float32)).to(dev)
    calib = host.IntrinsicsRefiner(s["K"], dist, group)
    assert calib.n_groups == 3 and calib.n_images == N_CAMS
    images = torch.rand(N_CAMS, H, W, 3, device=dev)
    o, d, gt, cam = calib.sample_random_rays(s["base"], H, W, 257, images=images)
    assert o.shape == (257, 3) and gt.shape == (257, 3) and cam.dtype == torch.int32
    assert bool((cam[1:] >= cam[:-1]).all()) and int(cam.min()) >= 0 and int(cam.max()) < N_CAMS
    assert d.requires_grad
    (o.sum() + (d * d).sum()).backward()  # the origins do not depend on the calibration
    assert calib.gamma.grad is not None and float(calib.gamma.grad.abs().min()) > 0
    with torch.no_grad():
        calib.gamma.copy_(torch.randn(3, 8, device=dev) * 0.01)
    calib.set_learned([True] * 4 + [False] * 4)
    path = str(tmp_path / "intrinsics_refiner.pt")
    calib.save(path)
    other = host.IntrinsicsRefiner(torch.zeros(N_CAMS, 3, 3, device=dev), None, group)
    other.load(path)
    for name in ("gamma", "base_K", "base_dist", "group", "learn"):
        assert torch.equal(getattr(other, name), getattr(calib, name)), name
    assert torch.equal(other.intrinsics(), calib.intrinsics()) and torch.equal(other.dist(), calib.dist())


def test_calibration_is_recovered_from_rays_on_the_device(host, dev):
    """tests/test_intr_refine_model_cpu.py's experiment through IntrinsicsRefiner and
    get_rays_from_calibrated_cameras: the same pixels, Adam settings and thresholds."""
    to = lambda a: torch.as_tensor(a).to(dev)
    K, D = to(im.REC_K[None].copy()), to(im.REC_DIST[None].copy())
    eye = torch.eye(3, 4, device=dev)[None].contiguous()
    calib, truth = host.IntrinsicsRefiner(K, D), host.IntrinsicsRefiner(K, D)
    with torch.no_grad():
        truth.gamma.copy_(to(im.REC_GAMMA.astype(np.float32))[None])
    every = np.stack(np.meshgrid(np.arange(im.REC_H), np.arange(im.REC_W), indexing="ij"), -1)
    every = to(every.reshape(-1, 2).astype(np.int32))
    pixels = to(np.stack([im.recovery_pixels(s) for s in range(im.REC_STEPS)]))
    cam0 = torch.zeros(im.REC_BATCH, dtype=torch.int32, device=dev)

    def loss_on(ij, cam):
        n = ij.shape[0]
        with torch.no_grad():
            want = truth.sample_random_rays(eye, im.REC_H, im.REC_W, n, cam_idx=cam, ij=ij)[1]
        got = calib.sample_random_rays(eye, im.REC_H, im.REC_W, n, cam_idx=cam, ij=ij)[1]
        return (got - want).square().sum(1).mean()

    cam_all = torch.zeros(every.shape[0], dtype=torch.int32, device=dev)
    with torch.no_grad():
        first = float(loss_on(every, cam_all))
    adam = calib.make_adam(im.REC_LR)
    for step in range(im.REC_STEPS):
        adam.zero_grad()
        loss_on(pixels[step], cam0).backward()
        adam.step()
    with torch.no_grad():
        last = float(loss_on(every, cam_all))
    off = calib.gamma.detach().cpu().numpy()[0].astype(np.float64) - im.REC_GAMMA
    print("loss %.3e -> %.3e (%.3g-fold), gamma - gamma* = %s" % (first, last, first / last,
                                                                  np.array2string(off, precision=4)))
    assert first / last >= 1e3
    assert abs(off[0]) < 0.01 and abs(off[1]) < 0.01
