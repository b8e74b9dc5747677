"""CPU-side checks of the calibration-refinement entry points (f2n_cam_intr_grad, f2n_intr_compose,
f2n_intr_compose_bwd): the ABI, the validation before any HIP work, the workspace size and the
kernels' resource usage.  Cross-compiled for gfx950; needs hipcc, not a GPU."""
import ctypes
import importlib
import os
import shutil

import pytest

from tests import test_pose_refine_cpu as pose_cpu

build = importlib.import_module("f2-nerf_amd._build")
SRC = os.path.join(build.KERNEL_DIR, "intr_refine.hip")
NEW = ("f2n_cam_intr_grad", "f2n_cam_intr_grad_workspace_floats", "f2n_intr_compose",
       "f2n_intr_compose_bwd")
INVALID = -1


def test_entry_points_parse_and_export(capi):
    decls = capi.parse_header()
    cdll = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert name in decls, name
        assert hasattr(cdll, name), name
    assert capi.lib().cdll.f2n_abi_version() == 2
    ret, params = decls["f2n_cam_intr_grad_workspace_floats"]
    assert ret is ctypes.c_int64 and [t for t, _ in params] == [ctypes.c_int64, ctypes.c_int64]
    assert [n for _, n in decls["f2n_cam_intr_grad"][1]] == [
        "poses", "pose_ld", "intrinsics", "dist", "ij", "d_rays_d", "cam_start", "order", "d_intr",
        "workspace", "n", "n_cams", "stream"]
    assert [n for _, n in decls["f2n_intr_compose"][1]] == [
        "base_K", "base_dist", "gamma", "group", "out_K", "out_dist", "n_images", "n_groups", "stream"]
    assert [n for _, n in decls["f2n_intr_compose_bwd"][1]] == [
        "base_K", "base_dist", "gamma", "group", "learn", "d_K", "d_dist", "d_gamma", "n_images",
        "n_groups", "stream"]


@pytest.mark.parametrize("n,E", [(0, 1), (1, 1), (1024, 1), (1025, 3), (70000, 1), (300, 5000)])
def test_workspace_is_positive_and_bounded(capi, n, E):
    got = capi.lib().cdll.f2n_cam_intr_grad_workspace_floats(n, E)
    assert got > 0 and got % 8 == 0
    assert got <= 8 * (-(-n // 1024) + E)


# f2n_cam_intr_grad(poses, pose_ld, K, dist, ij, d_d, cam_start, order, d_intr, ws, n, n_cams, stream)
def _grad_args():
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: validation answers first
    return [fake, 12, fake, None, fake, fake, fake, None, fake, fake, 64, 3, None]


# f2n_intr_compose(base_K, base_dist, gamma, group, out_K, out_dist, n_images, n_groups, stream)
def _compose_args():
    fake = ctypes.c_void_p(0x1000)
    return [fake, None, fake, fake, fake, fake, 5, 2, None]


# f2n_intr_compose_bwd(base_K, base_dist, gamma, group, learn, d_K, d_dist, d_gamma, n_images,
#                      n_groups, stream)
def _compose_bwd_args():
    fake = ctypes.c_void_p(0x1000)
    return [fake, None, fake, fake, None, None, None, fake, 5, 2, None]


def test_null_and_negative_arguments_rejected(capi):
    cdll = capi.lib().cdll
    for fn, good, ptrs, bads in (
            (cdll.f2n_cam_intr_grad, _grad_args(), (0, 2, 4, 5, 6, 8, 9),
             ((1, 9), (1, 0), (1, 15), (10, -1), (11, 0), (11, -4), (10, 1 << 31))),
            (cdll.f2n_intr_compose, _compose_args(), (0, 2, 3, 4, 5),
             ((6, -1), (7, 0), (7, -3), (6, 1 << 31), (7, 1 << 31))),
            (cdll.f2n_intr_compose_bwd, _compose_bwd_args(), (0, 2, 3, 7),
             ((8, -1), (9, 0), (9, -3), (8, 1 << 31), (9, 1 << 31)))):
        for i in ptrs:
            args = list(good)
            args[i] = None
            assert fn(*args) == INVALID, (fn.__name__, i)
        for i, bad in bads:
            args = list(good)
            args[i] = bad
            assert fn(*args) == INVALID, (fn.__name__, i, bad)


def test_two_faults_answer_before_anything_is_launched(capi):
    """Pointers, then counts, then pose_ld: an inconsistent call stays a rejection whichever fault is
    looked at first, and a compose over no images does nothing and launches nothing."""
    cdll = capi.lib().cdll
    for fn, good, faults in (
            (cdll.f2n_cam_intr_grad, _grad_args(), ({4: None, 1: 9}, {10: -1, 1: 9}, {5: None, 11: 0})),
            (cdll.f2n_intr_compose, _compose_args(), ({0: None, 7: 0}, {6: -1, 7: 0}, {6: 0, 7: 0},
                                                      {5: None, 6: 0})),
            (cdll.f2n_intr_compose_bwd, _compose_bwd_args(), ({7: None, 9: 0}, {8: -1, 9: 0},
                                                              {8: 0, 9: 0}))):
        for f in faults:
            args = list(good)
            for i, bad in f.items():
                args[i] = bad
            assert fn(*args) == INVALID, (fn.__name__, f)
    args = _compose_args()
    args[6] = 0
    assert cdll.f2n_intr_compose(*args) == 0


def test_kernels_have_no_scratch_or_spills(tmp_path, monkeypatch):
    if not os.path.exists(build.HIPCC) and shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: the build needs it too")
    monkeypatch.setattr(pose_cpu, "SRC", SRC)  # the recipe of test_pose_refine_cpu.py, on this file
    kernels = pose_cpu._resource_usage(tmp_path)
    for want in ("cam_intr_grad_piece_kernel", "cam_intr_grad_final_kernel", "intr_compose_kernel",
                 "intr_compose_bwd_kernel"):
        assert sum(want in k for k in kernels) == 1, (want, sorted(kernels))
    assert len(kernels) == 4, sorted(kernels)
    for name, r in kernels.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0 and r.get("AGPRs Spill", 0) == 0, (name, r)
        assert r.get("SGPRs Spill", 0) == 0, (name, r)
