"""Lens distortion (k1, k2, p1, p2) in ray generation on the GPU: f2n_gen_rays_dist,
f2n_gen_rays_dist_bwd and f2n_project_points against the float64 restatement of
tests/lens_model.py, with the tolerances derived there (TOL for an undistorted coordinate, PIX_TOL
for a projected pixel; both re-measured by tests/test_lens_cpu.py on the float32 restatement, never
on these kernels), and the host functions that pass `dist` through."""
import importlib

import numpy as np
import pytest
import torch

from tests import lens_model as M
from tests.test_gpu_render import _setup

pytestmark = pytest.mark.gpu

N = M.H * M.W
SET_IDS = ["set%d" % i for i in range(len(M.SETS))]


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


@pytest.fixture(scope="module")
def refs():
    """The float64 camera-frame directions of the five sets over the whole image, computed once."""
    ij, K = M.pixels(), M.intrinsic()
    return [M.reference_dirs(k, ij, K) for k in M.SETS]


@pytest.fixture(scope="module")
def general():
    return {rows: M.general_case(rows) for rows in (3, 4)}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _gen(capi, dev, entry, poses, pose_ld, K, dist, n_cams, cam, ij, first, width, n):
    o = torch.full((n, 3), float("nan"), device=dev)
    d = torch.full((n, 3), float("nan"), device=dev)
    if entry == "gen_rays":
        capi.call(entry, poses, pose_ld, K, n_cams, cam, ij, first, width, o, d, n)
    else:
        capi.call(entry, poses, pose_ld, K, dist, n_cams, cam, ij, first, width, o, d, n)
    torch.cuda.synchronize()
    return o, d


def _bwd(capi, dev, entry, K, dist, n_cams, ij, first, width, d_o, d_d, pose_ld, n):
    out = torch.full((n_cams, pose_ld), float("nan"), device=dev)
    ws = torch.empty(capi.lib().cdll.f2n_gen_rays_bwd_workspace_floats(n), device=dev)
    if entry == "gen_rays_bwd":
        capi.call(entry, K, n_cams, ij, first, width, d_o, d_d, out, pose_ld, ws, n)
    else:
        capi.call(entry, K, dist, n_cams, ij, first, width, d_o, d_d, out, pose_ld, ws, n)
    torch.cuda.synchronize()
    return out


def _modes(dev, rows=3):
    """The three addressing modes of f2n_gen_rays on the general case's cameras:
    (poses, pose_ld, K, dist-or-zeros-builder rows, n_cams, cam_idx, ij, first_pixel, width, n)."""
    c = M.general_case(rows)
    poses, K, cam, ij = (_t(c[k], dev) for k in ("poses", "K", "cam", "ij"))
    ld = rows * 4
    first = 2 * M.W + 3  # a view that starts inside a row
    return {
        "view": (poses[1:2].contiguous(), ld, K[1:2].contiguous(), 1, None, None, first, M.W, N - first),
        "cam_idx": (poses, ld, K, poses.shape[0], cam, ij, 0, 1, N),
        "per_ray": (poses[cam.long()].contiguous(), ld, K[cam.long()].contiguous(), N, None, ij, 0, 1, N),
    }


# ---- 1. zero coefficients change nothing ---------------------------------------------------------

@pytest.mark.parametrize("mode", ["view", "cam_idx", "per_ray"])
@pytest.mark.parametrize("rows", [3, 4])
def test_zero_coefficients_give_the_pinhole_bits(capi, dev, mode, rows):
    poses, ld, K, n_cams, cam, ij, first, width, n = _modes(dev, rows)[mode]
    want_o, want_d = _gen(capi, dev, "gen_rays", poses, ld, K, None, n_cams, cam, ij, first, width, n)
    assert bool(torch.isfinite(want_d).all())
    for dist in (None, torch.zeros(n_cams, 4, device=dev)):
        o, d = _gen(capi, dev, "gen_rays_dist", poses, ld, K, dist, n_cams, cam, ij, first, width, n)
        assert torch.equal(o, want_o) and torch.equal(d, want_d)
    if mode == "cam_idx":
        return  # the backward has no cam_idx
    g = torch.Generator().manual_seed(5)
    d_o, d_d = (torch.randn(n, 3, generator=g).to(dev) for _ in range(2))
    want = _bwd(capi, dev, "gen_rays_bwd", K, None, n_cams, ij, first, width, d_o, d_d, ld, n)
    assert bool(torch.isfinite(want).all())
    for dist in (None, torch.zeros(n_cams, 4, device=dev)):
        got = _bwd(capi, dev, "gen_rays_dist_bwd", K, dist, n_cams, ij, first, width, d_o, d_d, ld, n)
        assert torch.equal(got, want)


# ---- 2. identity rotation: the undistorted direction itself ---------------------------------------

@pytest.mark.parametrize("s", range(len(M.SETS)), ids=SET_IDS)
def test_identity_rotation_matches_float64(capi, dev, refs, s):
    t = torch.tensor([0.25, -0.5, 0.125])
    pose = torch.cat([torch.eye(3), t[:, None]], 1)[None].contiguous().to(dev)
    K = _t(M.intrinsic()[None], dev)
    dist = torch.tensor([M.SETS[s]], dtype=torch.float32, device=dev)
    ij = _t(M.pixels(), dev)
    v64 = refs[s]
    runs = {
        "view": _gen(capi, dev, "gen_rays_dist", pose, 12, K, dist, 1, None, None, 0, M.W, N),
        "ij": _gen(capi, dev, "gen_rays_dist", pose, 12, K, dist, 1, None, ij, 0, 1, N),
    }
    for name, (o, d) in runs.items():
        assert torch.equal(o.cpu(), t.expand(N, 3)), name
        d = d.cpu().double().numpy()
        assert bool((d[:, 2] == -1.0).all()), name
        ex = float(np.abs(d[:, 0] - v64[:, 0]).max())
        ey = float(np.abs(d[:, 1] - v64[:, 1]).max())  # rays_d[1] = -y, v64[1] = -y64
        print("set %d %s: |x - x64| = %.3g, |y - y64| = %.3g, TOL = %.3g" % (s, name, ex, ey, M.TOL))
        assert ex <= M.TOL and ey <= M.TOL, (name, ex, ey)
    assert torch.equal(runs["view"][1], runs["ij"][1])
    # the bound tells the cameras apart: pinhole rays miss it on this set
    _, pin = _gen(capi, dev, "gen_rays", pose, 12, K, None, 1, None, None, 0, M.W, N)
    miss = float(np.abs(pin.cpu().double().numpy()[:, :2] - v64[:, :2]).max())
    assert miss >= 0.0158 > M.TOL, miss


# ---- 3. a general pose, one camera per ray --------------------------------------------------------

def _dir_bound(c):
    """Per component a: TOL (|R a0| + |R a1|) + 4 u (|R a0 x| + |R a1 y| + |R a2|)."""
    R, v = np.abs(c["R"]), np.abs(c["v"])
    return (M.TOL * (R[:, :, 0] + R[:, :, 1])
            + 4 * M.U * (R[:, :, 0] * v[:, 0:1] + R[:, :, 1] * v[:, 1:2] + R[:, :, 2]))


@pytest.mark.parametrize("rows", [3, 4])
def test_general_pose_one_camera_per_ray(capi, dev, general, rows):
    c = general[rows]
    assert len(set(c["cam"].tolist())) == len(M.SETS)
    poses, K, dist, cam, ij = (_t(c[k], dev) for k in ("poses", "K", "dist", "cam", "ij"))
    o, d = _gen(capi, dev, "gen_rays_dist", poses, rows * 4, K, dist, poses.shape[0], cam, ij, 0, 1, N)
    assert np.array_equal(o.cpu().numpy().astype(np.float64), c["origins"])
    err = np.abs(d.cpu().double().numpy() - c["dirs"])
    bound = _dir_bound(c)
    print("rows %d: largest err / bound = %.3g" % (rows, float((err / bound).max())))
    assert bool((err <= bound).all()), float((err / bound).max())
    # a wrong stride would hand a ray another camera's coefficients: far outside the bound
    wrong = np.einsum("nab,nb->na", c["R"], M.reference_dirs(M.SETS[0], c["ij"], c["K"][0]))
    assert float((np.abs(wrong - c["dirs"]) / bound).max()) > 1e3
    # the per-ray tables (n_cams == n, no cam_idx) give the same bits
    idx = cam.long()
    o2, d2 = _gen(capi, dev, "gen_rays_dist", poses[idx].contiguous(), rows * 4, K[idx].contiguous(),
                  dist[idx].contiguous(), N, None, ij, 0, 1, N)
    assert torch.equal(o2, o) and torch.equal(d2, d)


# ---- 4. finite under abuse -------------------------------------------------------------------------

@pytest.mark.parametrize("coeffs", [(-5.0, 0.0, 0.0, 0.0), (-5.0, 3.0, 0.1, -0.1)])
def test_finite_under_abuse(capi, dev, coeffs):
    pose = torch.eye(4)[None, :3].contiguous().to(dev)
    K = _t(M.intrinsic()[None], dev)
    dist = torch.tensor([coeffs], dtype=torch.float32, device=dev)
    o, d = _gen(capi, dev, "gen_rays_dist", pose, 12, K, dist, 1, None, None, 0, M.W, N)
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(d).all())


# ---- 5. backward -----------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [3, 4])
@pytest.mark.parametrize("s", range(len(M.SETS)), ids=SET_IDS)
def test_backward_one_pose_matches_float64_sums(capi, dev, refs, s, rows):
    g = torch.Generator().manual_seed(11 + s)
    d_o, d_d = (torch.randn(N, 3, generator=g) for _ in range(2))
    K = _t(M.intrinsic()[None], dev)
    dist = torch.tensor([M.SETS[s]], dtype=torch.float32, device=dev)
    v64 = refs[s]
    go, gd = d_o.double().numpy(), d_d.double().numpy()
    terms = gd[:, :, None] * v64[:, None, :]               # [n, i, j]
    want = np.concatenate([terms.sum(0), go.sum(0)[:, None]], 1)
    any_order = N * M.U * np.concatenate([np.abs(terms).sum(0), np.abs(go).sum(0)[:, None]], 1)
    bound = any_order.copy()
    bound[:, :2] += M.TOL * np.abs(gd).sum(0)[:, None]     # x and y carry the solve's error
    runs = []
    for ij in (None, _t(M.pixels(), dev)):
        for _ in range(2):
            runs.append(_bwd(capi, dev, "gen_rays_dist_bwd", K, dist, 1, ij, 0, M.W if ij is None else 1,
                             d_o.to(dev), d_d.to(dev), rows * 4, N).cpu())
    for r in runs[1:]:
        assert torch.equal(r, runs[0])  # a fixed order: the same bits run to run, view and ij mode
    got = runs[0].double().numpy().reshape(rows, 4)
    err = np.abs(got[:3] - want)
    print("set %d: largest err / bound = %.3g" % (s, float((err / bound).max())))
    assert bool((err <= bound).all()), (err / bound).max()
    if rows == 4:
        assert bool((got[3] == 0.0).all())
    # pinhole directions would not pass
    K64 = M.intrinsic()
    xd, yd = M.normalised(M.pixels(), K64, np.float64)
    pin = (gd[:, :, None] * np.stack([xd, -yd], 1)[:, None, :]).sum(0)
    assert float((np.abs(pin - want[:, :2]) / bound[:, :2]).max()) > 1.0


@pytest.mark.parametrize("rows", [3, 4])
def test_backward_one_pose_per_ray(capi, dev, general, rows):
    c = general[rows]
    g = torch.Generator().manual_seed(13)
    d_o, d_d = (torch.randn(N, 3, generator=g) for _ in range(2))
    idx = _t(c["cam"], dev).long()
    K = _t(c["K"], dev)[idx].contiguous()
    dist = _t(c["dist"], dev)[idx].contiguous()
    got = _bwd(capi, dev, "gen_rays_dist_bwd", K, dist, N, _t(c["ij"], dev), 0, 1, d_o.to(dev),
               d_d.to(dev), rows * 4, N).cpu().double().numpy().reshape(N, rows, 4)
    go, gd = d_o.double().numpy(), d_d.double().numpy()
    want = gd[:, :, None] * c["v"][:, None, :]
    bound = M.U * np.abs(want)
    bound[:, :, :2] += M.TOL * np.abs(gd)[:, :, None]
    err = np.abs(got[:, :3, :3] - want)
    assert bool((err <= bound).all()), float((err / np.maximum(bound, 1e-300)).max())
    assert np.array_equal(got[:, :3, 3], go)
    if rows == 4:
        assert bool((got[:, 3] == 0.0).all())


# ---- 6. projection ---------------------------------------------------------------------------------

def test_projection_returns_to_the_pixel_centres(capi, dev):
    c = M.projection_case()
    n = c["points"].shape[0]
    poses, K, dist, cam, pts = (_t(c[k], dev) for k in ("poses", "K", "dist", "cam", "points"))
    pix = torch.full((n, 2), float("nan"), device=dev)
    valid = torch.full((n,), -1, dtype=torch.int32, device=dev)
    capi.call("project_points", pts, poses, 12, K, dist, poses.shape[0], cam, pix, valid, n)
    torch.cuda.synchronize()
    assert bool((valid == 1).all())
    got = pix.cpu().double().numpy()
    idx = c["cam"]
    p64, _ = M.project(c["points"], c["poses"][idx], c["K"][idx], c["dist"][idx], np.float64)
    e_model = float(np.abs(got - p64).max())
    e_centre = float(np.abs(got - c["centre"]).max())
    print("project: |gpu - f64| = %.3g, |gpu - centre| = %.3g, PIX_TOL = %.3g"
          % (e_model, e_centre, M.PIX_TOL))
    assert e_model <= M.PIX_TOL
    assert e_centre <= M.PIX_TOL
    # a pinhole projection of the same points lands pixels away
    pin = torch.empty_like(pix)
    capi.call("project_points", pts, poses, 12, K, None, poses.shape[0], cam, pin, valid, n)
    assert float((pin.cpu().double() - torch.from_numpy(c["centre"])).abs().max()) > 0.5
    # [4,4] poses, one camera per point: the same bits
    c4 = M.general_case(4)
    i = cam.long()
    pix4 = torch.empty_like(pix)
    capi.call("project_points", pts, _t(c4["poses"], dev)[i].contiguous(), 16, K[i].contiguous(),
              dist[i].contiguous(), n, None, pix4, valid, n)
    assert torch.equal(pix4, pix)
    # mirrored through the camera centre: behind it
    behind = (2 * c["poses"][idx][:, :3, 3] - c["points"]).astype(np.float32)
    capi.call("project_points", _t(behind, dev), poses, 12, K, dist, poses.shape[0], cam, pix, valid, n)
    torch.cuda.synchronize()
    assert bool((valid == 0).all()) and bool(torch.isfinite(pix).all())


# ---- 7. the host library ---------------------------------------------------------------------------

def test_host_ray_functions_pass_dist_through(host, capi, dev, general):
    c = general[3]
    s = 4
    pose = _t(c["poses"][2], dev)
    K = _t(M.intrinsic(), dev)
    dist = torch.tensor(M.SETS[s], dtype=torch.float32, device=dev)
    ij = _t(M.pixels(), dev)
    o, d = host.get_view_rays(pose, K, M.H, M.W, dist=dist)
    o2, d2 = host.get_rays_from_pose(pose[None], K[None], ij, dist=dist[None])
    want_o, want_d = _gen(capi, dev, "gen_rays_dist", pose[None].contiguous(), 12, K[None].contiguous(),
                          dist[None].contiguous(), 1, None, None, 0, M.W, N)
    assert torch.equal(o, o2) and torch.equal(d, d2)
    assert torch.equal(o, want_o) and torch.equal(d, want_d)
    pin_o, pin_d = host.get_view_rays(pose, K, M.H, M.W)
    assert not torch.equal(d, pin_d)
    zo, zd = host.get_view_rays(pose, K, M.H, M.W, dist=torch.zeros(1, 4, device=dev))
    assert torch.equal(zd, pin_d) and torch.equal(zo, pin_o)
    # the pose gradient under grad mode is the C-ABI backward
    g = torch.Generator().manual_seed(17)
    w_o, w_d = (torch.randn(N, 3, generator=g).to(dev) for _ in range(2))
    want = _bwd(capi, dev, "gen_rays_dist_bwd", K[None].contiguous(), dist[None].contiguous(), 1, None,
                0, M.W, w_o, w_d, 12, N).view(3, 4)
    p = pose.clone().requires_grad_(True)
    o, d = host.get_view_rays(p, K, M.H, M.W, dist=dist)
    ((o * w_o).sum() + (d * w_d).sum()).backward()
    assert p.grad is not None and torch.equal(p.grad, want)
    assert dist.grad is None and K.grad is None
    # one camera per ray, with a gradient to each pose
    idx = _t(c["cam"], dev).long()
    pp = _t(c["poses"], dev)[idx].clone().requires_grad_(True)
    o, d = host.get_rays_from_pose(pp, _t(c["K"], dev)[idx], ij, dist=_t(c["dist"], dev)[idx])
    ((o * w_o).sum() + (d * w_d).sum()).backward()
    want = _bwd(capi, dev, "gen_rays_dist_bwd", _t(c["K"], dev)[idx].contiguous(),
                _t(c["dist"], dev)[idx].contiguous(), N, ij, 0, 1, w_o, w_d, 12, N).view(N, 3, 4)
    assert torch.equal(pp.grad, want)
    # the training batch: each ray under its own image's coefficients
    torch.manual_seed(3)
    ro, rd, _, cam = host.sample_random_rays(_t(c["poses"], dev), _t(c["K"], dev), M.H, M.W, 512,
                                             dist=_t(c["dist"], dev))
    torch.manual_seed(3)
    po, pd, _, cam_p = host.sample_random_rays(_t(c["poses"], dev), _t(c["K"], dev), M.H, M.W, 512)
    assert torch.equal(cam, cam_p) and torch.equal(ro, po) and not torch.equal(rd, pd)
    # and back: the points of those rays project onto pixel centres under the same cameras
    i = cam.long()
    pix, valid = host.project_points((ro + 2.0 * rd).contiguous(), _t(c["poses"], dev)[i].contiguous(),
                                     _t(c["K"], dev)[i].contiguous(), dist=_t(c["dist"], dev)[i].contiguous())
    assert bool((valid == 1).all())
    frac = pix.cpu().double() - 0.5
    # (ray error TOL through fx, fy <= 42, on top of the projection's own tolerance)
    assert float((frac - frac.round()).abs().max()) <= M.PIX_TOL + 42 * M.TOL * 2


H_IMG, W_IMG = 24, 32


def _renderer(host, seed):
    _, hr, *_ = _setup(host, 8, 2, 14, 64, 4.0 / 64, 1, 3.0, seed)
    return hr


def _small_intrinsic():
    return torch.tensor([[0.9 * W_IMG, 0.0, 0.5 * W_IMG], [0.0, 0.9 * W_IMG, 0.5 * H_IMG],
                         [0.0, 0.0, 1.0]])


def test_render_image_with_dist(host, dev, general):
    hr = _renderer(host, 29)
    pose = _t(general[3]["poses"][1], dev)
    K = _small_intrinsic().to(dev)
    dist = torch.tensor(M.SETS[0], dtype=torch.float32, device=dev)
    o, d = host.get_view_rays(pose, K, H_IMG, W_IMG, dist=dist)
    hr.set_pixel_tiles(0)  # rows, the order of get_view_rays
    with torch.no_grad():
        # the renderer chooses its first pass from what the previous call kept: every call that is
        # compared follows a render of the same rays
        hr.render_all_rays(o, d, 1 << 16)
        direct, direct_depth = hr.render_all_rays(o, d, 1 << 16)
        colors, depths = hr.render_image(pose, K, H_IMG, W_IMG, 1 << 16, dist=dist)
        pinhole, _ = hr.render_image(pose, K, H_IMG, W_IMG, 1 << 16)
    assert colors.shape == (H_IMG, W_IMG, 3) and depths.shape == (H_IMG, W_IMG, 3)
    assert torch.equal(colors, direct.reshape(H_IMG, W_IMG, 3).clip(0.0, 1.0))
    assert torch.equal(depths, direct_depth.reshape(H_IMG, W_IMG, 1).repeat(1, 1, 3))
    assert not torch.equal(colors, pinhole)
    # positional calls keep their meaning
    with torch.no_grad():
        again, _ = hr.render_image(pose, K, H_IMG, W_IMG, 1 << 16, dist)
    assert again.shape == colors.shape


def test_localizer_uses_dist_params(host, dev, general):
    P, Kp = 6, 64
    coeffs = M.SETS[0]
    locs = {}
    for name, k in (("dist", coeffs), ("zero", (0.0, 0.0, 0.0, 0.0))):
        param = host.LocalizerParam()
        param.render_pixel_num = Kp
        param.dist_params = list(k)
        locs[name] = host.Localizer(param, _renderer(host, 31), _small_intrinsic().to(dev), H_IMG,
                                    W_IMG, torch.zeros(3).to(dev), 1.0)
    g = torch.Generator().manual_seed(31)
    base = _t(general[3]["poses"][0], dev)
    poses = host.perturb_poses(base, torch.randn(P, 6, generator=g).to(dev),
                               [0.02, 0.03, 0.05, 2.5, 1.5, 3.5])
    image = torch.rand(H_IMG, W_IMG, 3, generator=g).to(dev)
    pix = torch.randperm(H_IMG * W_IMG, generator=g)[:Kp]
    ij = torch.stack([pix // W_IMG, pix % W_IMG], 1).to(torch.int32).to(dev)
    K = locs["dist"].intrinsic
    dist = torch.tensor(coeffs, dtype=torch.float32, device=dev)
    o, d = locs["dist"].pose_rays(poses, ij)
    want_o, want_d = host.get_rays_from_poses(poses, K, ij, dist=dist)
    assert torch.equal(o, want_o) and torch.equal(d, want_d)
    zo, zd = locs["zero"].pose_rays(poses, ij)
    pin_o, pin_d = host.get_rays_from_poses(poses, K, ij)
    assert torch.equal(zd, pin_d) and not torch.equal(d, pin_d)
    w = {name: loc.evaluate_poses(poses, image, ij) for name, loc in locs.items()}
    for name in w:
        assert w[name].shape == (P,) and bool(torch.isfinite(w[name]).all()), name
    assert not torch.equal(w["dist"], w["zero"])
    # render_image: the distorted view, differentiable in the pose
    with torch.no_grad():
        img = locs["dist"].render_image(base)
        img0 = locs["zero"].render_image(base)
    assert img.shape == (H_IMG, W_IMG, 3) and not torch.equal(img, img0)
    steps = locs["dist"].optimize_pose_by_differential(base.clone(), image, 1)
    assert len(steps) == 1 and bool(torch.isfinite(steps[0]).all())
