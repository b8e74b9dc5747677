"""CPU-side checks of the localiser (f2n_perturb_poses, f2n_pose_scores, f2n_average_pose and the
Localizer class): the entries parse from the header and are exported, reject NULL and negative
arguments before touching a GPU, the class refuses CPU tensors, and the kernels compile for gfx950
with the project's own HIP flags without scratch and without float atomics.  Needs hipcc, not a GPU."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest
import torch

build = importlib.import_module("f2-nerf_amd._build")
SRC = os.path.join(build.KERNEL_DIR, "localizer.hip")
NEW = ("f2n_perturb_poses", "f2n_pose_scores", "f2n_average_pose")


def test_entry_points_parse_and_export(capi):
    decls = capi.parse_header()
    cdll = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert name in decls, name
        assert hasattr(cdll, name), name
    # additions only: the ABI version stays
    assert capi.lib().cdll.f2n_abi_version() == 2
    assert [t for t, _ in decls["f2n_perturb_poses"][1]].count(ctypes.c_float) == 6


def test_null_and_negative_arguments_rejected(capi):
    cdll = capi.lib().cdll
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: validation answers first
    # f2n_perturb_poses(pose, pose_ld, noise, 6 sigmas, poses, P, stream)
    good = [fake, 12, fake, .1, .1, .1, 1., 1., 1., fake, 8, None]
    for i in (0, 2, 9):
        args = list(good)
        args[i] = None
        assert cdll.f2n_perturb_poses(*args) == -1, i
    for i, bad in ((1, 9), (1, 0), (10, -1)):
        args = list(good)
        args[i] = bad
        assert cdll.f2n_perturb_poses(*args) == -1, (i, bad)
    # f2n_pose_scores(colors, image, ij, loss, weights, workspace, P, K, h, w, stream)
    good = [fake] * 6 + [8, 64, 24, 32, None]
    for i in range(6):
        args = list(good)
        args[i] = None
        assert cdll.f2n_pose_scores(*args) == -1, i
    for i, bad in ((6, -1), (7, -1), (7, 0), (8, 0), (8, -4), (9, 0), (9, -4)):
        args = list(good)
        args[i] = bad
        assert cdll.f2n_pose_scores(*args) == -1, (i, bad)
    # f2n_average_pose(poses, weights, pose_out, P, stream)
    good = [fake, fake, fake, 8, None]
    for i in range(3):
        args = list(good)
        args[i] = None
        assert cdll.f2n_average_pose(*args) == -1, i
    for bad in (-1, 0):
        assert cdll.f2n_average_pose(fake, fake, fake, bad, None) == -1, bad


def _cpu_localizer(H, resize_factor=2):
    r = H.Renderer(2, n_levels=2, log2_table=8, max_samples=8, device="cpu")
    p = H.LocalizerParam()
    p.resize_factor = resize_factor
    k = torch.tensor([[100.0, 0.0, 50.0], [0.0, 100.0, 40.0], [0.0, 0.0, 1.0]])
    return H.Localizer(p, r, k, 80, 100, torch.tensor([0.1, 0.2, 0.3]), 2.0), k


def test_param_defaults_and_resize(pkg):
    H = pkg.load_host()
    p = H.LocalizerParam()
    assert p.render_pixel_num == 256 and p.resize_factor == 1 and p.train_result_dir == ""
    for axis in "xyz":
        assert getattr(p, "noise_position_" + axis) == pytest.approx(0.025)
        assert getattr(p, "noise_rotation_" + axis) == pytest.approx(2.5)
    loc, k = _cpu_localizer(H)
    assert (loc.infer_height(), loc.infer_width(), loc.radius()) == (40, 50, 2.0)
    want = k / 2
    want[2, 2] = 1.0
    assert torch.equal(loc.intrinsic, want)
    assert k[0, 0] == 100.0  # the caller's tensor is not scaled in place
    # NeRF x <- world y, y <- z, z <- x; positions over the radius, rotations in degrees
    p.noise_position_x, p.noise_position_y, p.noise_position_z = 0.1, 0.2, 0.3
    p.noise_rotation_x, p.noise_rotation_y, p.noise_rotation_z = 1.0, 2.0, 3.0
    r = H.Renderer(2, n_levels=2, log2_table=8, max_samples=8, device="cpu")
    loc = H.Localizer(p, r, k, 80, 100, torch.zeros(3), 4.0)
    assert loc.noise_sigmas(2.0) == pytest.approx([0.1, 0.15, 0.05, 4.0, 6.0, 2.0])


def test_construction_from_a_train_result_dir(pkg, tmp_path):
    """inference_params.yaml + checkpoints/latest/renderer.pt, as a training run leaves them."""
    H = pkg.load_host()
    p = H.LocalizerParam()
    p.train_result_dir = str(tmp_path)
    p.resize_factor = 2
    with pytest.raises(RuntimeError, match="Failed to open"):
        H.Localizer(p)
    k = torch.tensor([[120.0, 0.0, 64.0], [0.0, 110.0, 48.0], [0.0, 0.0, 1.0]])
    H.save_inference_params(str(tmp_path), 3, 96, 128, k, torch.tensor([0.5, -0.25, 2.0]), 3.5)
    with pytest.raises(Exception):  # the parameters are there, the checkpoint is not
        H.Localizer(p)
    os.makedirs(tmp_path / "checkpoints" / "latest")
    H.manual_seed(11)
    trained = H.Renderer(3)  # the reference's compile-time configuration, on the default device
    trained.save(str(tmp_path / "checkpoints" / "latest" / "renderer.pt"))
    loc = H.Localizer(p)
    assert (loc.infer_height(), loc.infer_width(), loc.radius()) == (48, 64, 3.5)
    want = k / 2
    want[2, 2] = 1.0
    assert torch.equal(loc.intrinsic.cpu(), want)
    got, ref = loc.renderer.named_parameters(), trained.named_parameters()
    assert set(got) == set(ref)
    for name in ref:
        assert torch.equal(got[name], ref[name]), name


def test_no_cpu_implementation(pkg):
    H = pkg.load_host()
    loc, _ = _cpu_localizer(H)
    pose, image = torch.eye(4)[:3].contiguous(), torch.zeros(40, 50, 3)
    ij = torch.zeros(4, 2, dtype=torch.int32)
    calls = [
        lambda: loc.render_image(pose),
        lambda: loc.evaluate_poses(pose[None], image),
        lambda: loc.evaluate_poses_full(pose[None], image, ij),
        lambda: loc.pose_rays(pose[None], ij),
        lambda: loc.optimize_pose_by_random_search(pose, image, 4, 1.0),
        lambda: loc.random_search(pose, image, 4, 1.0, torch.zeros(4, 6)),
        lambda: loc.optimize_pose_by_differential(pose.clone(), image, 1),
        lambda: loc.world2camera(torch.eye(4)),
        lambda: loc.camera2world(pose),
        lambda: H.Localizer.calc_average_pose([(pose, 1.0)]),
        lambda: H.Localizer.calc_average_pose(pose[None], torch.ones(1)),
        lambda: H.perturb_poses(pose, torch.zeros(4, 6), [0.0] * 6),
        lambda: H.pose_scores(torch.zeros(1, 4, 3), image, ij),
        lambda: H.average_pose(pose[None], torch.ones(1)),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()
            pytest.fail("call %d did not raise" % i)


def _resource_usage(tmp_path):
    cmd = [build.HIPCC, *build.HIP_FLAGS, "-I", build.INCLUDE_DIR, "-I", build.KERNEL_DIR,
           "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", SRC,
           "-o", str(tmp_path / "localizer.o")]
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
    return kernels


def test_kernels_have_no_scratch_or_spills(tmp_path):
    if not os.path.exists(build.HIPCC) and shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: the build needs it too")
    kernels = _resource_usage(tmp_path)
    for want in ("perturb_poses_kernel", "pose_loss_kernel", "pose_weights_kernel",
                 "average_pose_kernel"):
        assert sum(want in k for k in kernels) == 1, (want, sorted(kernels))
    assert len(kernels) == 4, sorted(kernels)
    for name, r in kernels.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0 and r.get("AGPRs Spill", 0) == 0, (name, r)
        assert r.get("SGPRs Spill", 0) == 0, (name, r)


def test_source_has_no_float_atomics():
    text = open(SRC).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    assert not re.search(r"\batomic\w*\s*\(|\bunsafeAtomic\w*|__hip_atomic|__atomic_", text), \
        "the localiser kernels sum in a fixed order: no atomics of any kind"
