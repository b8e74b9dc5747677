"""CPU-side checks of the lens-distortion entry points (f2n_gen_rays_dist, f2n_gen_rays_dist_bwd,
f2n_project_points): the numpy restatements of tests/lens_model.py invert each other, the two
tolerances the GPU tests use are re-measured here on the float32 restatement (never on a kernel), the
entries parse from the header, are exported and reject bad arguments before touching a GPU, and the
distortion columns of cams_meta.tsv come back from read_cams_meta unchanged."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import lens_model as M

NEW = ("f2n_gen_rays_dist", "f2n_gen_rays_dist_bwd", "f2n_project_points")


# ---- the restatements ------------------------------------------------------------------------------

def test_float64_restatement_round_trips():
    ij, K = M.pixels(), M.intrinsic()
    for k in M.SETS:
        xd, yd = M.normalised(ij, K, np.float64)
        x, y, det = M.undistort(k, xd, yd, np.float64, steps=30)
        bx, by = M.distort(k, x, y, np.float64)
        assert float(np.abs(bx - xd).max()) <= 1e-12 and float(np.abs(by - yd).max()) <= 1e-12, k
        assert float(det.min()) >= 0.47, (k, float(det.min()))  # far from a singular Jacobian
        # Newton is at round-off after 5 steps: 8 leave a margin
        x5, y5, _ = M.undistort(k, xd, yd, np.float64, steps=5)
        assert float(max(np.abs(x5 - x).max(), np.abs(y5 - y).max())) <= 1e-12, k
        # and the distortion matters: a pinhole direction is off by at least 0.0158 somewhere
        off = float(max(np.abs(xd - x).max(), np.abs(yd - y).max()))
        assert 0.0158 <= off <= 0.25, (k, off)


def test_tol_covers_f32_restatement():
    """TOL = 4 x (f32 restatement, 8 steps, against float64, 30 steps), rounded up to a power of two."""
    ij, K = M.pixels(), M.intrinsic()
    e32 = 0.0
    for k in M.SETS:
        v32 = M.camera_dirs(k, ij, K, np.float32)
        assert v32.dtype == np.float32
        v64 = M.reference_dirs(k, ij, K)
        e32 = max(e32, float(np.abs(v32.astype(np.float64) - v64)[:, :2].max()))
    print("E32 = %.4g, 4 E32 = %.4g, TOL = %.4g" % (e32, 4 * e32, M.TOL))
    assert e32 > 0
    assert 4 * e32 <= M.TOL
    assert M.pow2_ceil(4 * e32) == M.TOL == 2.0 ** -20


def test_pix_tol_covers_f32_restatement():
    """PIX_TOL by the same recipe on project(), on the points the GPU test projects."""
    c = M.projection_case()
    cam = c["cam"]
    args = (c["points"], c["poses"][cam], c["K"][cam], c["dist"][cam])
    p32, v32 = M.project(*args, np.float32)
    p64, v64 = M.project(*args, np.float64)
    assert p32.dtype == np.float32 and bool(v32.all()) and bool(v64.all())
    e = float(np.abs(p32.astype(np.float64) - p64).max())
    back = float(np.abs(p64 - c["centre"]).max())
    print("project: |f32 - f64| = %.4g, 4 x = %.4g, PIX_TOL = %.4g; |f64 - centre| = %.4g"
          % (e, 4 * e, M.PIX_TOL, back))
    assert e > 0
    assert 4 * e <= M.PIX_TOL
    assert M.pow2_ceil(4 * e) == M.PIX_TOL
    # the points are float32 roundings of points on the rays: their exact projection is the pixel
    # centre up to that rounding, well inside the tolerance
    assert back <= M.PIX_TOL / 4
    # a point behind its camera
    behind = (2 * c["poses"][cam][:, :3, 3] - c["points"]).astype(np.float32)
    _, vb = M.project(behind, *args[1:], np.float64)
    assert not bool(vb.any())


# ---- the C ABI -------------------------------------------------------------------------------------

def test_entry_points_parse_and_export(capi):
    decls = capi.parse_header()
    cdll = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert name in decls, name
        assert hasattr(cdll, name), name
    assert capi.lib().cdll.f2n_abi_version() == 2  # additions only
    # f2n_gen_rays with one more pointer, f2n_gen_rays_bwd with one more pointer
    for new, old in (("f2n_gen_rays_dist", "f2n_gen_rays"), ("f2n_gen_rays_dist_bwd", "f2n_gen_rays_bwd")):
        names_new = [n for _, n in decls[new][1]]
        names_old = [n for _, n in decls[old][1]]
        assert "dist" in names_new and [n for n in names_new if n != "dist"] == names_old, new


def _reject(fn, good, nulls, bads):
    for i in nulls:
        args = list(good)
        args[i] = None
        assert fn(*args) == -1, i
    for i, bad in bads:
        args = list(good)
        args[i] = bad
        assert fn(*args) == -1, (i, bad)


def test_bad_arguments_rejected_without_a_gpu(capi):
    c = capi.lib().cdll
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: validation answers first
    # f2n_gen_rays_dist(poses, pose_ld, K, dist, n_cams, cam_idx, ij, first_pixel, width, o, d, n, s)
    good = [fake, 12, fake, fake, 1, None, None, 0, 8, fake, fake, 64, None]
    _reject(c.f2n_gen_rays_dist, good, (0, 2, 9, 10),
            ((1, 9), (1, 0), (1, -12), (4, 0), (4, -1), (4, 5), (8, 0), (8, -3), (11, -1)))
    for dist in (fake, None):  # NULL dist is the pinhole camera, not an error
        args = list(good)
        args[3], args[11] = dist, 0
        assert c.f2n_gen_rays_dist(*args) == 0
    # f2n_gen_rays_dist_bwd(K, dist, n_cams, ij, first_pixel, width, d_o, d_d, d_poses, pose_ld, ws,
    #                       n, stream)
    good = [fake, fake, 1, None, 0, 8, fake, fake, fake, 12, fake, 64, None]
    _reject(c.f2n_gen_rays_dist_bwd, good, (0, 6, 7, 8, 10),
            ((2, 0), (2, -1), (2, 5), (4, -1), (5, 0), (9, 9), (9, 0), (11, -1)))
    for dist in (fake, None):
        args = list(good)
        args[1], args[11] = dist, 0
        assert c.f2n_gen_rays_dist_bwd(*args) == 0
    # f2n_project_points(points, poses, pose_ld, K, dist, n_cams, cam_idx, pix, valid, n, stream)
    good = [fake, fake, 16, fake, fake, 1, None, fake, fake, 64, None]
    _reject(c.f2n_project_points, good, (0, 1, 3, 7, 8),
            ((2, 9), (2, 0), (5, 0), (5, -1), (5, 5), (9, -1)))
    for dist in (fake, None):
        args = list(good)
        args[4], args[9] = dist, 0
        assert c.f2n_project_points(*args) == 0


def test_ray_kernels_have_no_scratch_or_spills(tmp_path):
    """rays.hip cross-compiled for gfx950 with the project's own flags: the pinhole kernel, its
    sibling with the Newton loop unrolled, and the projection."""
    build = importlib.import_module("f2-nerf_amd._build")
    cmd = [build.HIPCC, *build.HIP_FLAGS, "-I", build.INCLUDE_DIR, "-I", build.KERNEL_DIR,
           "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(build.KERNEL_DIR, "rays.hip"), "-o", str(tmp_path / "rays.o")]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    kernels, cur = {}, None
    for line in res.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            kernels[cur] = {}
            continue
        m = re.search(r"remark: ([^:\[]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if cur and m:
            kernels[cur][m.group(1).strip()] = int(m.group(2))
    for want in ("gen_rays_kernel", "gen_rays_dist_kernel", "project_points_kernel"):
        assert sum(want in k for k in kernels) == 1, (want, sorted(kernels))
    assert len(kernels) == 3, sorted(kernels)
    for name, r in kernels.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)


# ---- cams_meta.tsv ---------------------------------------------------------------------------------

def test_read_cams_meta_returns_the_distortion_columns(pkg, tmp_path):
    """27 numbers per image: pose 12, intrinsic 9, k1 k2 p1 p2, near far (src/dataset.cpp:59-63)."""
    H = pkg.load_host()
    g = torch.Generator().manual_seed(3)
    n = len(M.SETS)
    rows = torch.randn(n, 27, generator=g)
    rows[:, 21:25] = torch.tensor(M.SETS)
    path = tmp_path / "cams_meta.tsv"
    with open(path, "w") as f:
        f.write("\t".join("c%d" % i for i in range(27)) + "\n")
        for r in rows:
            f.write("\t".join(repr(float(v)) for v in r) + "\n")
    poses, intrinsics, dist, bounds = H.read_cams_meta(str(path))
    assert dist.shape == (n, 4) and dist.dtype == torch.float32 and dist.is_contiguous()
    assert torch.equal(dist, torch.tensor(M.SETS, dtype=torch.float32))
    assert float(dist.abs().max()) > 0
    assert torch.equal(poses.reshape(n, 12), rows[:, :12])
    assert torch.equal(intrinsics.reshape(n, 9), rows[:, 12:21])
    # fed on unchanged: the ray functions and the localiser take the rows as read (on a CPU they get
    # as far as the refusal to run without a GPU, not a complaint about the argument)
    pose, K = poses[0], intrinsics[0]
    for call in (lambda: H.get_view_rays(pose, K, 4, 6, dist=dist[0]),
                 lambda: H.get_rays_from_pose(poses[:1], intrinsics[:1],
                                              torch.zeros(3, 2, dtype=torch.int32), dist=dist[:1]),
                 lambda: H.sample_random_rays(poses, intrinsics, 4, 6, 8, dist=dist),
                 lambda: H.project_points(torch.zeros(3, 3), pose, K, dist=dist[0])):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()
    p = H.LocalizerParam()
    assert list(p.dist_params) == [0.0] * 4
    p.dist_params = [float(v) for v in dist[0]]
    assert list(p.dist_params) == [float(v) for v in dist[0]]
