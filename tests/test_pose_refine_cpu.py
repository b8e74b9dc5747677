"""CPU-side checks of the pose-refinement entry points (f2n_cam_pose_grad, f2n_pose_compose,
f2n_pose_compose_bwd): the ABI, the validation order, the kernels' resource usage, the float64
reference of the correction, and the bound that tests/test_gpu_pose_refine.py holds the per-camera
sums to -- shown here to be neither violated by a float32 restatement nor idle against three wrong
partitions.  Cross-compiled for gfx950; needs hipcc, not a GPU.

Measured here (the restatement, never the kernel): largest |f32 - f64| / tol_c over the 40-camera case
with d_rays = randn * exp(3 randn): 0.293 in either order (a one-ray camera: the product's rounding
against gamma(3)); over the cameras of 1000 rays and more 0.0072 in serial order and 0.0020 in the
kernel's piece / stride order (test_bound_holds_for_f32_restatements prints them)."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import lens_model as lm
from tests import pose_refine_model as pm

build = importlib.import_module("f2-nerf_amd._build")
SRC = os.path.join(build.KERNEL_DIR, "pose_refine.hip")
NEW = ("f2n_cam_pose_grad", "f2n_cam_pose_grad_workspace_floats", "f2n_pose_compose",
       "f2n_pose_compose_bwd")
INVALID = -1


# ---- ABI -------------------------------------------------------------------------------------------

def test_entry_points_parse_and_export(capi):
    decls = capi.parse_header()
    cdll = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert name in decls, name
        assert hasattr(cdll, name), name
    assert capi.lib().cdll.f2n_abi_version() == 2
    ret, params = decls["f2n_cam_pose_grad_workspace_floats"]
    assert ret is ctypes.c_int64 and [t for t, _ in params] == [ctypes.c_int64, ctypes.c_int64]
    assert [n for _, n in decls["f2n_cam_pose_grad"][1]] == [
        "intrinsics", "dist", "ij", "d_rays_o", "d_rays_d", "cam_start", "order", "d_poses",
        "pose_ld", "workspace", "n", "n_cams", "stream"]


def test_library_still_does_not_import_getenv(capi):
    syms = subprocess.run(["nm", "-D", "--undefined-only", capi.LIB_PATH], capture_output=True,
                          text=True).stdout
    assert "getenv" not in syms


@pytest.mark.parametrize("n,E", [(0, 1), (1, 1), (1024, 1), (1025, 3), (70000, 1), (300, 5000),
                                 (1 << 20, 24)])
def test_workspace_is_positive_and_bounded(capi, n, E):
    got = capi.lib().cdll.f2n_cam_pose_grad_workspace_floats(n, E)
    assert got > 0 and got % 12 == 0
    assert got <= 12 * (-(-n // 1024) + E)


# f2n_cam_pose_grad(K, dist, ij, d_o, d_d, cam_start, order, d_poses, pose_ld, ws, n, n_cams, stream)
def _grad_args():
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: validation answers first
    return [fake, None, fake, fake, fake, fake, None, fake, 12, fake, 64, 3, None]


# f2n_pose_compose(base, pose_ld, delta, fixed, out, n_cams, stream)
def _compose_args():
    fake = ctypes.c_void_p(0x1000)
    return [fake, 12, fake, None, fake, 5, None]


# f2n_pose_compose_bwd(base, pose_ld, delta, fixed, d_out, d_delta, n_cams, stream)
def _compose_bwd_args():
    fake = ctypes.c_void_p(0x1000)
    return [fake, 16, fake, None, fake, fake, 5, None]


def test_null_and_negative_arguments_rejected(capi):
    cdll = capi.lib().cdll
    for fn, good, ptrs, bads in (
            (cdll.f2n_cam_pose_grad, _grad_args(), (0, 2, 3, 4, 5, 7, 9),
             ((8, 9), (8, 0), (8, 15), (10, -1), (11, 0), (11, -4), (10, 1 << 31))),
            (cdll.f2n_pose_compose, _compose_args(), (0, 2, 4), ((1, 9), (1, 0), (5, -1))),
            (cdll.f2n_pose_compose_bwd, _compose_bwd_args(), (0, 2, 4, 5),
             ((1, 13), (1, -12), (6, -1)))):
        for i in ptrs:
            args = list(good)
            args[i] = None
            assert fn(*args) == INVALID, (fn.__name__, i)
        for i, bad in bads:
            args = list(good)
            args[i] = bad
            assert fn(*args) == INVALID, (fn.__name__, i, bad)


def test_two_faults_answer_before_anything_is_launched(capi):
    """Pointers, then counts, then pose_ld.  Every status is INVALID_ARG, so the order shows in what a
    call with no rays or no cameras does: pose_ld is looked at before the n_cams == 0 return of the
    compose entries, and a bad pose_ld with a null pointer or a negative count stays a rejection."""
    cdll = capi.lib().cdll
    for fn, good, faults in (
            (cdll.f2n_cam_pose_grad, _grad_args(), ({2: None, 8: 9}, {10: -1, 8: 9}, {3: None, 11: 0})),
            (cdll.f2n_pose_compose, _compose_args(), ({0: None, 1: 9}, {5: -1, 1: 9}, {5: 0, 1: 9},
                                                      {4: None, 5: 0})),
            (cdll.f2n_pose_compose_bwd, _compose_bwd_args(), ({5: None, 1: 9}, {6: -1, 1: 9},
                                                              {6: 0, 1: 9}, {4: None, 6: 0}))):
        for f in faults:
            args = list(good)
            for i, bad in f.items():
                args[i] = bad
            assert fn(*args) == INVALID, (fn.__name__, f)
    # no cameras and nothing else wrong: nothing to do, and nothing launched
    args = _compose_args()
    args[5] = 0
    assert cdll.f2n_pose_compose(*args) == 0


def _resource_usage(tmp_path):
    cmd = [build.HIPCC, *build.HIP_FLAGS, "-I", build.INCLUDE_DIR, "-I", build.KERNEL_DIR,
           "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", SRC,
           "-o", str(tmp_path / "pose_refine.o")]
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
    for want in ("cam_pose_grad_piece_kernel", "cam_pose_grad_final_kernel", "pose_compose_kernel",
                 "pose_compose_bwd_kernel"):
        assert sum(want in k for k in kernels) == 1, (want, sorted(kernels))
    assert len(kernels) == 4, sorted(kernels)
    for name, r in kernels.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0 and r.get("AGPRs Spill", 0) == 0, (name, r)
        assert r.get("SGPRs Spill", 0) == 0, (name, r)


# ---- the compose reference -------------------------------------------------------------------------

def test_matrix_exp_reference_agrees_with_closed_form_rodrigues():
    rng = np.random.default_rng(11)
    worst = 0.0
    for th in (1e-9, 1e-6, 1e-4, 1e-3, 0.1, 1.0, 2.0, 3.1):
        for _ in range(4):
            axis = rng.standard_normal(3)
            w = th * axis / np.linalg.norm(axis)
            got = torch.linalg.matrix_exp(pm.hat(torch.tensor(w)[None]))[0].numpy()
            worst = max(worst, float(np.abs(got - pm.rodrigues(w)).max()))
    print("matrix_exp vs Rodrigues, |omega| up to 3.1: %.2e" % worst)
    assert worst <= 4e-15
    z = torch.zeros(1, 3, dtype=torch.float64)
    assert torch.equal(torch.linalg.matrix_exp(pm.hat(z))[0], torch.eye(3, dtype=torch.float64))


def test_matrix_exp_gradient_is_finite_at_zero_and_is_the_generator():
    base = torch.eye(3, 4, dtype=torch.float64)[None]
    delta = torch.zeros(1, 6, dtype=torch.float64, requires_grad=True)
    out = pm.compose_ref(base, delta)
    g = torch.zeros(1, 3, 4, dtype=torch.float64)
    g[0, 2, 1], g[0, 0, 3] = 1.0, 2.0  # d R'[2][1] / d omega_x = 1 at the identity
    (d,) = torch.autograd.grad(out, delta, g)
    assert torch.isfinite(d).all()
    assert torch.allclose(d, torch.tensor([[1.0, 0, 0, 2.0, 0, 0]], dtype=torch.float64), atol=1e-15)


# ---- the bound for the per-camera sums -------------------------------------------------------------

@pytest.fixture(scope="module")
def heavy():
    c = pm.counts_case(heavy=True)
    v = pm.pinhole_dirs32(c["ij"], lm.intrinsic())
    cs = pm.cam_bounds(c["cam"], c["E"])
    t64 = pm.terms(c["d_o"], c["d_d"], v, np.float64)
    ref, mag = pm.sums_f64(t64, cs)
    return dict(c=c, cs=cs, t32=pm.terms(c["d_o"], c["d_d"], v, np.float32), ref=ref,
                tol=pm.tol(cs, mag))


def test_case_has_the_counts_that_matter():
    assert len(pm.COUNTS) == 40 and pm.COUNTS[0] == 0 and pm.COUNTS[-1] == 0
    assert set((0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 3000)) <= set(
        pm.COUNTS)
    cs = pm.cam_bounds(pm.counts_case()["cam"], 40)
    spans = [len(pm.runs_of(cs, c)) for c in range(40)]
    assert max(spans) >= 4 and spans.count(2) >= 3  # cameras across one and across several pieces
    # both ways of summing a run, on both sides of the threshold
    lens = {e - s for c in range(40) for s, e in pm.runs_of(cs, c)}
    assert {pm.LANE_RUN - 1, pm.LANE_RUN} <= lens or (min(lens) < pm.LANE_RUN <= max(lens))


def test_bound_holds_for_f32_restatements(heavy):
    worst = {}
    for name, fn in (("serial", pm.sums32_serial), ("pieces", pm.sums32_pieces)):
        got = fn(heavy["t32"], heavy["cs"]).astype(np.float64)
        err = np.abs(got - heavy["ref"])
        assert (err <= heavy["tol"]).all(), name
        ratio = np.divide(err, heavy["tol"], out=np.zeros_like(err), where=heavy["tol"] > 0)
        worst[name] = float(ratio.max())
        worst[name + ", 1000 rays and more"] = float(ratio[np.diff(heavy["cs"]) >= 1000].max())
        empty = np.diff(heavy["cs"]) == 0
        assert (got[empty] == 0).all() and (got[pm.ZERO_CAM] == 0).all()
    print("largest err/tol of the f32 restatements:", worst)
    # not idle either: a float32 sum does use a visible part of it
    assert max(worst.values()) > 1e-2


@pytest.mark.parametrize("mutant", [pm.mutant_dropped_piece, pm.mutant_full_last_stride,
                                    pm.mutant_boundary_ray])
def test_bound_rejects_wrong_partitions(mutant):
    """Float64 sums over a wrong partition must leave the bound in at least one element of every
    camera whose rays the mutation touches.

    The data are of one sign and within a factor of two (1 <= |d| < 2), so a mutation moves an
    element fed by d_rays_o by at least 1 per ray it adds or drops, and cancellation cannot hide it.
    With the heavy-tailed gradients of the main case a single ray can lie orders of magnitude below
    ANY summation bound of its camera, which says nothing about the partition.  A camera is eligible
    up to 2048 rays: tol <= gamma(cnt + 2) * 2 cnt < 1 needs cnt (cnt + 2) < 2^23, cnt <= 2895; past
    that a worst-case float32 bound cannot see one ray, whatever the code does."""
    c = pm.counts_case(heavy=False)
    v = pm.pinhole_dirs32(c["ij"], lm.intrinsic())
    cs = pm.cam_bounds(c["cam"], c["E"])
    t64 = pm.terms(c["d_o"], c["d_d"], v, np.float64)
    ref, mag = pm.sums_f64(t64, cs)
    tol = pm.tol(cs, mag)
    got, touched = mutant(t64, cs)
    cnt = np.diff(cs)
    elig = [k for k in touched if cnt[k] <= 2048 and k != pm.ZERO_CAM]
    assert len(elig) >= 3, (mutant.__name__, touched)
    for k in elig:
        assert (np.abs(got[k] - ref[k]) > tol[k]).any(), (mutant.__name__, k, int(cnt[k]))
    # and the unmutated float64 sums are, of course, inside
    assert (np.abs(pm.sums_f64(t64, cs)[0] - ref) <= tol).all()
