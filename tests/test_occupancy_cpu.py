"""CPU-side checks of the occupancy-bitfield entry points (f2n_occ_update, f2n_occ_lookup,
f2n_density_march_occ, f2n_sample_compact_occ): they parse from the header, are exported, reject bad
arguments before touching a GPU, every instantiation of their kernels compiles, with the project's
own HIP flags, without scratch or spills, and a grid class in the host module leaves the Renderer's
parameters (the checkpoint layout) alone.  Cross-compiled for gfx950; needs hipcc, not a GPU."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest

build = importlib.import_module("f2-nerf_amd._build")
NEW = ("f2n_occ_update", "f2n_occ_lookup", "f2n_density_march_occ", "f2n_sample_compact_occ")


def test_entry_points_parse_and_export(capi):
    decls = capi.parse_header()
    for name in NEW:
        assert name in decls, name
    cdll = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert hasattr(cdll, name), name
    # the additions are backward-compatible: the ABI version stays
    assert capi.lib().cdll.f2n_abi_version() == 2
    assert [n for _, n in decls["f2n_occ_lookup"][1]] == ["pts", "n", "bits", "G", "out", "stream"]
    assert decls["f2n_occ_lookup"][1][1][0] is ctypes.c_int64


def test_every_entry_cites_the_reference_site_it_alters(capi):
    text = open(capi.HEADER).read()
    start = text.index("occupancy bitfield")
    section = text[start:text.index("ray order", start)]
    for site in ("src/renderer.cpp:58-90", "src/points_sampler.cpp:20-64",
                 "src/main_functions/train_manager.cpp:102"):
        assert site in section, site


FAKE = ctypes.c_void_p(0x1000)  # never dereferenced: validation answers first
BAD_G = (0, -128, 16, 31, 48, 100, 512)


def test_lookup_arguments_rejected(capi):
    fn = capi.lib().cdll.f2n_occ_lookup
    good = [FAKE, 10, FAKE, 128, FAKE, None]
    for i in (0, 2, 4):
        args = list(good)
        args[i] = None
        assert fn(*args) == -1, i
    args = list(good)
    args[1] = -1
    assert fn(*args) == -1
    for G in BAD_G:
        args = list(good)
        args[3] = G
        assert fn(*args) == -1, G
    assert fn(None, 0, None, 64, None, None) == 0  # nothing to do is not an error


def test_update_arguments_rejected(capi):
    fn = capi.lib().cdll.f2n_occ_update
    # (table, primes, bias, mul, w0, b0, probe_u, density, bits, G, L, F, T, level_stride,
    #  density_shift, threshold, decay, stream)
    good = [FAKE] * 6 + [None, FAKE, FAKE, 128, 16, 2, 1 << 19, 1 << 19, 3.0, 1.0, 0.95, None]
    for i in (0, 1, 2, 3, 4, 5, 7, 8):
        args = list(good)
        args[i] = None
        assert fn(*args) == -1, i
    for G in BAD_G:
        args = list(good)
        args[9] = G
        assert fn(*args) == -1, G
    for i, bad in ((10, 0), (10, 33), (12, 0), (13, -2), (13, 3), (16, -0.5)):
        args = list(good)
        args[i] = bad
        assert fn(*args) == -1, (i, bad)
    for F in (0, 3, 16):
        args = list(good)
        args[11] = F
        assert fn(*args) == -3, F


def test_march_and_compact_arguments_rejected(capi):
    cdll = capi.lib().cdll
    # f2n_density_march_occ(rays_o, rays_d, noise, table, primes, bias, mul, w0, b0, bits, G, kept,
    #                       len, n_rays, S, step, L, F, T, level_stride, t_thresh, shift, stream)
    good = [FAKE, FAKE, None] + [FAKE] * 7 + [128, FAKE, FAKE, 4, 1024, 1.0 / 256, 16, 2, 1 << 19,
                                              1 << 19, 1e-4, 3.0, None]
    for i in (0, 1, 3, 4, 5, 6, 7, 8, 9, 11, 12):
        args = list(good)
        args[i] = None
        assert cdll.f2n_density_march_occ(*args) == -1, i
    for i, bad in ((13, -1), (14, 0), (16, 0), (16, 33), (18, 0), (19, -2), (19, 3)):
        args = list(good)
        args[i] = bad
        assert cdll.f2n_density_march_occ(*args) == -1, (i, bad)
    for G in BAD_G:
        args = list(good)
        args[10] = G
        assert cdll.f2n_density_march_occ(*args) == -1, G
    for F in (0, 3, 16):
        args = list(good)
        args[17] = F
        assert cdll.f2n_density_march_occ(*args) == -3, F
    # f2n_sample_compact_occ(rays_o, rays_d, noise, bounds, len, bits, G, pts, dirs, dt, t, n_rays, S,
    #                        step, stream)
    good = [FAKE, FAKE, None, FAKE, FAKE, FAKE, 128, FAKE, FAKE, FAKE, FAKE, 4, 1024, 1.0 / 256, None]
    for i in (0, 1, 3, 4, 5):
        args = list(good)
        args[i] = None
        assert cdll.f2n_sample_compact_occ(*args) == -1, i
    for i, bad in ((11, -1), (12, 0)):
        args = list(good)
        args[i] = bad
        assert cdll.f2n_sample_compact_occ(*args) == -1, (i, bad)
    for G in BAD_G:
        args = list(good)
        args[6] = G
        assert cdll.f2n_sample_compact_occ(*args) == -1, G


def test_two_faults_answer_with_the_first_check(capi):
    """Two bad arguments at once: the status is that of the check an entry makes first.  The order and
    the codes are each entry's own (the shared field-argument check covers only L < 1, T < 1, a negative
    stride, F outside {1, 2, 4, 8} and a stride that is no multiple of F, in that order)."""
    INVALID, UNSUPPORTED = -1, -3
    cdll = capi.lib().cdll
    odd = (1 << 19) + 1
    # f2n_occ_update: G and the level count first, then the field arguments, then the pointers
    good = [FAKE] * 6 + [None, FAKE, FAKE, 128, 16, 2, 1 << 19, 1 << 19, 3.0, 1.0, 0.95, None]
    for faults, want in (({10: 0, 11: 3}, INVALID), ({10: 33, 11: 3}, INVALID), ({12: 0, 11: 3}, INVALID),
                         ({9: 100, 11: 3}, INVALID), ({11: 3, 13: odd}, UNSUPPORTED),
                         ({0: None, 11: 3}, UNSUPPORTED), ({10: 33, 13: odd}, INVALID),
                         ({0: None, 10: 33}, INVALID), ({10: 64, 11: 1}, INVALID)):
        args = list(good)
        for i, bad in faults.items():
            args[i] = bad
        assert cdll.f2n_occ_update(*args) == want, faults
    # f2n_density_march_occ: counts, level count and G first, then the field arguments, then n_rays == 0
    # and the pointers
    good = [FAKE, FAKE, None] + [FAKE] * 7 + [128, FAKE, FAKE, 4, 1024, 1.0 / 256, 16, 2, 1 << 19,
                                              1 << 19, 1e-4, 3.0, None]
    for faults, want in (({13: -1, 17: 3}, INVALID), ({16: 0, 17: 3}, INVALID), ({16: 33, 17: 3}, INVALID),
                         ({18: 0, 17: 3}, INVALID), ({14: 0, 17: 3}, INVALID), ({10: 100, 17: 3}, INVALID),
                         ({17: 3, 19: odd}, UNSUPPORTED), ({3: None, 17: 3}, UNSUPPORTED),
                         ({16: 33, 19: odd}, INVALID), ({3: None, 16: 33}, INVALID),
                         ({13: -1, 16: 33}, INVALID), ({16: 64, 17: 1}, INVALID),
                         ({13: 0, 17: 3}, UNSUPPORTED), ({13: 0, 19: odd}, INVALID)):
        args = list(good)
        for i, bad in faults.items():
            args[i] = bad
        assert cdll.f2n_density_march_occ(*args) == want, faults


def _resource_usage(tmp_path, name):
    src = os.path.join(build.KERNEL_DIR, name)
    cmd = [build.HIPCC, *build.HIP_FLAGS, "-I", build.INCLUDE_DIR, "-I", build.KERNEL_DIR,
           "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", str(tmp_path / (name + ".o"))]
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


def _assert_clean(kernels, names):
    for name in names:
        r = kernels[name]
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0 and r.get("AGPRs Spill", 0) == 0, (name, r)
        assert r.get("SGPRs Spill", 0) == 0, (name, r)


ALL_SHAPES = {(f, p) for f in "1248" for p in "01"}  # F in {1, 2, 4, 8} x power-of-two T or not


def test_kernels_have_no_scratch_or_spills(tmp_path):
    if not os.path.exists(build.HIPCC) and shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: the build needs it too")
    kernels = _resource_usage(tmp_path, "occupancy.hip")
    update = [k for k in kernels if "occ_update_kernel" in k]
    assert {re.search(r"kernelILi(\d)ELb(\d)", k).groups() for k in update} == ALL_SHAPES
    lookup = [k for k in kernels if "occ_lookup_kernel" in k]
    assert len(lookup) == 1, lookup
    _assert_clean(kernels, update + lookup)

    kernels = _resource_usage(tmp_path, "sampler.hip")
    march = [k for k in kernels if "density_march_occ_kernel" in k]
    assert {re.search(r"kernelILi(\d)ELb(\d)", k).groups() for k in march} == ALL_SHAPES
    compact = [k for k in kernels if "sample_compact_occ_kernel" in k]
    assert len(compact) == 1, compact
    _assert_clean(kernels, march + compact)


def test_no_scalar_memory_writes_in_the_new_kernels(tmp_path):
    """The bitfield is written with ordinary vector stores from plain C++: the device code of the two
    translation units holds no scalar store, scalar atomic or scalar-cache write-back."""
    for name in ("occupancy.hip", "sampler.hip"):
        src = os.path.join(build.KERNEL_DIR, name)
        out = tmp_path / (name + ".s")
        cmd = [build.HIPCC, *build.HIP_FLAGS, "-I", build.INCLUDE_DIR, "-I", build.KERNEL_DIR,
               "--offload-device-only", "-S", src, "-o", str(out)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert res.returncode == 0, res.stdout[-4000:]
        asm = out.read_text()
        pattern = r"^\s*s_(?:buffer_|scratch_)?(?:st" + r"ore|atom" + r"ic)|^\s*s_dcache_(?:wb|discard)"
        assert not re.search(pattern, asm, flags=re.M), name


def test_grid_class_leaves_renderer_parameters_alone(pkg):
    H = pkg.load_host()
    assert hasattr(H, "OccupancyGrid") and hasattr(H.Renderer, "set_occupancy")
    r = H.Renderer(4, device="cpu")
    before = {k: tuple(v.shape) for k, v in r.named_parameters().items()}
    grid = H.OccupancyGrid(32, device="cpu")
    assert grid.resolution == 32 and tuple(grid.words.shape) == (32 ** 3 // 32,)
    assert bool(grid.bits().all()) and grid.fraction() == 1.0   # fresh: nothing is skipped
    r.set_occupancy(grid)
    assert {k: tuple(v.shape) for k, v in r.named_parameters().items()} == before
    assert set(before) == {
        "app_emb", "scene_field.feat_pool", "scene_field.prim_pool", "scene_field.bias_pool",
        "scene_field.mlp.weight", "scene_field.mlp.bias", "shader.mlp.0.weight", "shader.mlp.0.bias",
        "shader.mlp.2.weight", "shader.mlp.2.bias"}
    r.set_occupancy(None)
    assert r.occupancy is None
    for bad in (0, 16, 48, 512):
        with pytest.raises(Exception):
            H.OccupancyGrid(bad, device="cpu")


def test_set_bits_and_bits_round_trip_on_the_host(pkg):
    import torch

    H = pkg.load_host()
    grid = H.OccupancyGrid(32, device="cpu")
    g = torch.Generator().manual_seed(3)
    want = torch.rand(32, 32, 32, generator=g) < 0.5
    grid.set_bits(want)
    assert torch.equal(grid.bits(), want)
    # bit i = (cz*G + cy)*G + cx in bit (i & 31) of word (i >> 5)
    one = torch.zeros(32, 32, 32, dtype=torch.bool)
    one[3, 5, 31] = True
    grid.set_bits(one)
    i = (3 * 32 + 5) * 32 + 31
    words = grid.words.to(torch.int64) & 0xFFFFFFFF
    assert int(words[i >> 5]) == 1 << (i & 31) and int(words.ne(0).sum()) == 1
    assert abs(grid.fraction() - 1.0 / 32 ** 3) < 1e-12
