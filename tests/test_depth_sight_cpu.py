"""The depth-supervision entries without a GPU: f2n_depth_sight_fwd / _bwd and f2n_depth_splat are
declared, exported and cited, their ctypes prototypes come out of the header as written, every
argument check answers before any HIP work, the kernels compile for gfx950 without scratch or LDS, and
the host operators refuse CPU tensors."""
import ctypes
import importlib
import os
import re
import subprocess

import pytest
import torch

ENTRIES = ("f2n_depth_sight_fwd", "f2n_depth_sight_bwd", "f2n_depth_splat")
INVALID, UNSUPPORTED, OK = -1, -3, 0


def test_entries_are_declared_exported_and_cited(capi):
    decls = capi.parse_header()
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert decls["f2n_depth_sight_fwd"][1] == [
        (P, "weights"), (P, "t"), (P, "dt"), (P, "idx"), (P, "z"), (F, "eps"), (P, "out"),
        (I, "n_rays"), (P, "stream")]
    assert decls["f2n_depth_sight_bwd"][1] == [
        (P, "weights"), (P, "t"), (P, "dt"), (P, "idx"), (P, "z"), (F, "eps"), (P, "d_out"),
        (P, "dw"), (I, "n_rays"), (P, "stream")]
    assert decls["f2n_depth_splat"][1] == [
        (P, "points"), (P, "cam_idx"), (P, "poses"), (I, "pose_ld"), (P, "intrinsics"), (P, "dist"),
        (L, "n_cams"), (I, "h"), (I, "w"), (P, "depth"), (L, "n"), (P, "stream")]
    # the prototypes capi.py hands to ctypes are these
    lib = capi.lib()
    for name in ENTRIES:
        fn = getattr(lib.cdll, name)
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == [t for t, _ in decls[name][1]]
    assert lib.cdll.f2n_abi_version() == 2                 # entries added, nothing else changed
    text = open(capi.HEADER).read()
    pos = text.index("f2n_depth_sight_fwd(")
    assert text.index("f2n_weight_dist_bwd(") < pos < text.index("scatter (row A9)")
    flat = " ".join(text[text.rindex("/*", 0, pos):pos].split())
    for words in ("reference has NO such kernel", "src/CustomOps/CustomOps.cu:13-67",
                  "src/main_functions/train_manager.cpp:80-93", "WRITES ZEROS", "receive no gradient",
                  "the same bits on every run", "finite and > 0"):
        assert words in flat, words
    pos = text.index("f2n_depth_splat(")
    assert text.index("f2n_project_points(") < pos
    flat = " ".join(text[text.rindex("/*", 0, pos):pos].split())
    for words in ("src/rays.cpp:7-28", "not the z-depth", "does not depend on the order of arrival",
                  "two launches give the same bits", "every element written", "never used as an address"):
        assert words in flat, words


def test_depth_sight_argument_validation_without_gpu(capi):
    c = capi.lib().cdll
    fake = 0x1000                                          # never dereferenced
    fwd, bwd = c.f2n_depth_sight_fwd, c.f2n_depth_sight_bwd
    # (weights, t, dt, idx, z, eps, out, n_rays, stream)
    good = [fake, fake, fake, fake, fake, 0.05, fake, 4, None]
    for i, bad in ((3, None), (4, None), (6, None), (7, -1), (5, -1e-3), (5, float("nan")),
                   (5, float("inf")), (5, -float("inf"))):
        args = list(good)
        args[i] = bad
        assert fwd(*args) == INVALID, (i, bad)
    assert fwd(None, None, None, None, None, 0.0, None, 0, None) == INVALID   # required even when empty
    for eps in (0.0, 0.05):
        args = list(good)
        args[5], args[7] = eps, 0
        assert fwd(*args) == OK                            # no rays: nothing is launched
    # (weights, t, dt, idx, z, eps, d_out, dw, n_rays, stream)
    good = [fake, fake, fake, fake, fake, 0.05, fake, fake, 4, None]
    for i, bad in ((3, None), (4, None), (6, None), (7, None), (8, -1), (5, -1.0), (5, float("nan")),
                   (5, float("inf"))):
        args = list(good)
        args[i] = bad
        assert bwd(*args) == INVALID, (i, bad)
    args = list(good)
    args[8] = 0
    assert bwd(*args) == OK


def test_depth_splat_argument_validation_without_gpu(capi):
    fn = capi.lib().cdll.f2n_depth_splat
    fake = 0x1000
    # (points, cam_idx, poses, pose_ld, intrinsics, dist, n_cams, h, w, depth, n, stream)
    good = [fake, fake, fake, 12, fake, None, 2, 6, 8, fake, 100, None]
    for i, bad in ((0, None), (2, None), (4, None), (9, None), (10, -1), (6, 0), (6, -2), (7, 0),
                   (7, -6), (8, 0), (8, -1), (3, 9), (3, 0)):
        args = list(good)
        args[i] = bad
        assert fn(*args) == INVALID, (i, bad)
    args = list(good)
    args[1] = None                                         # no cam_idx: n_cams must be 1 or n
    assert fn(*args) == INVALID
    for n_cams, h, w in ((1, 1 << 16, 1 << 15), (2, 1 << 15, 1 << 15), (1 << 31, 1, 1),
                         (3, 46341, 46341), ((1 << 31) - 1, 2, 1)):
        args = list(good)
        args[6], args[7], args[8] = n_cams, h, w
        assert fn(*args) == UNSUPPORTED, (n_cams, h, w)    # h * w * n_cams >= 2^31


def test_depth_kernels_have_no_scratch_no_lds_no_spills(tmp_path):
    """depth_sight.hip and depth_splat.hip cross-compiled for gfx950 with the project's own flags."""
    build = importlib.import_module("f2-nerf_amd._build")
    want = {"depth_sight.hip": ("depth_sight_fwd_kernel", "depth_sight_bwd_kernel"),
            "depth_splat.hip": ("depth_splat_kernel", "depth_finish_kernel")}
    for src, names in want.items():
        cmd = [build.HIPCC, *build.HIP_FLAGS, "-I", build.INCLUDE_DIR, "-I", build.KERNEL_DIR,
               "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(build.KERNEL_DIR, src), "-o", str(tmp_path / (src + ".o"))]
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
        for name in names:
            assert sum(name in k for k in kernels) == 1, (name, sorted(kernels))
        assert len(kernels) == len(names), sorted(kernels)
        for name, r in kernels.items():
            print("  %s: %s" % (name, r))
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("LDS Size") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
            assert r.get("VGPRs") <= 64, (name, r)         # eight waves per SIMD: nothing to hide behind


def test_kernel_header_fixes_the_evaluation_order():
    build = importlib.import_module("f2-nerf_amd._build")
    text = open(os.path.join(build.KERNEL_DIR, "depth_sight.hip")).read()
    head = " ".join(text[:text.index("#include")].split())
    for words in ("EVALUATION ORDER", "fmaf(w, w, e)", "fmaf(w, m, d)", "fmaf(c2, m, base)",
                  "ascending order", "reconverged", "wave_sum", "-ffp-contract=off"):
        assert words in head, words
    body = text[text.index("#include"):]
    assert "atomic" not in body and "__shared__" not in body


def test_host_ops_refuse_cpu_tensors(pkg):
    H = pkg.load_host()
    w = torch.ones(4)
    idx = torch.tensor([[0, 4]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        H.depth_sight(w, w, w, idx, torch.ones(1), 0.1)
    pose = torch.eye(4)[:3].unsqueeze(0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        H.splat_depth(torch.zeros(3, 3), torch.zeros(3, dtype=torch.int32), pose,
                      torch.eye(3).unsqueeze(0), None, 4, 6)
    # gather_depth is index arithmetic (ATen only): it runs wherever its tensors live
    maps = torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(2, 3, 4)
    cam = torch.tensor([1, 0, 1], dtype=torch.int32)
    ij = torch.tensor([[2, 3], [0, 0], [1, 2]], dtype=torch.int32)
    assert torch.equal(H.gather_depth(maps, cam, ij), maps[cam.long(), ij[:, 0].long(), ij[:, 1].long()])
    # an index outside the maps in any one component is "no return", never another pixel or camera
    # (row 3 of a 3-row map would otherwise read row 0 of the next camera, column 4 the next row)
    cam = torch.tensor([0, 0, 2, -1, 1, 1, 0], dtype=torch.int32)
    ij = torch.tensor([[3, 0], [0, 4], [0, 0], [1, 1], [-1, 2], [2, -1], [2, 3]], dtype=torch.int32)
    assert H.gather_depth(maps, cam, ij).tolist() == [0.0] * 6 + [float(maps[0, 2, 3])]
    o = H.DepthLossOptions(empty=0.1, near=0.2, expected=0.3, eps=0.05)
    assert (round(o.empty, 6), round(o.near, 6), round(o.expected, 6), round(o.eps, 6)) == (
        0.1, 0.2, 0.3, 0.05)
    d = H.DepthLossOptions()
    assert (d.empty, d.near, d.expected, d.eps) == (0.0, 0.0, 0.0, 0.0)
