"""The one-kernel inference render (render_rays.hip, f2n_render_rays) without a GPU: every
instantiation the launcher can reach compiles, with the project's own HIP flags, without scratch or
spills and within a CU's LDS; the set of instantiations is exactly the set the launcher dispatches to;
and the C ABI rejects bad arguments before any HIP work.  Cross-compiled for gfx950; needs hipcc."""
import importlib
import os
import re
import shutil
import subprocess

import pytest

build = importlib.import_module("f2-nerf_amd._build")
SRC = os.path.join(build.KERNEL_DIR, "render_rays.hip")
MAX_LEVELS = 32


def _dispatched():
    """(C, F, pow2 T) as the launcher's switch reaches them: C = L * F in {8, 16, 32, 64}, F in
    {1, 2, 4, 8}, L = C / F at most F2N_MAX_LEVELS.  The grid is a kernel argument, not a template
    parameter: one instantiation serves both."""
    return {(str(c), str(f), p) for c in (8, 16, 32, 64) for f in (1, 2, 4, 8) if c // f <= MAX_LEVELS
            for p in ("0", "1")}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(build.HIPCC) and shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: the build needs it too")
    out = tmp_path_factory.mktemp("render_rays") / "render_rays.o"
    cmd = [build.HIPCC, *build.HIP_FLAGS, "-I", build.INCLUDE_DIR, "-I", build.KERNEL_DIR,
           "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", SRC, "-o", str(out)]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    found, cur = {}, None
    for line in res.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            found[cur] = {}
            continue
        m = re.search(r"remark: ([^:\[]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if cur and m:
            found[cur][m.group(1).strip()] = int(m.group(2))
    # render_rays_kernel<C, F, POW2>
    return {re.search(r"kernelILi(\d+)ELi(\d)ELb(\d)EE", k).groups(): (k, v)
            for k, v in found.items() if "render_rays_kernelI" in k}


def test_header_level_cap_is_the_one_assumed_here(capi):
    text = open(capi.HEADER).read()
    assert int(re.search(r"#define\s+F2N_MAX_LEVELS\s+(\d+)", text).group(1)) == MAX_LEVELS


def test_instantiations_are_exactly_the_dispatched_ones(kernels):
    assert set(kernels) == _dispatched(), sorted(kernels)
    assert len(kernels) == 30


def test_no_scratch_no_spills_lds_within_a_cu(kernels):
    for key, (name, r) in kernels.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0 and r.get("AGPRs Spill", 0) == 0, (name, r)
        assert r.get("LDS Size") <= 163840, (name, r)


def test_occupancy_is_the_documented_one(kernels):
    # 8-wave workgroups; C <= 32 fits two per CU in LDS and 128 registers (four waves
    # per SIMD), C = 64 one per CU (two waves per SIMD)
    for (c, f, p), (name, r) in kernels.items():
        regs = r.get("VGPRs", 0) + r.get("AGPRs", 0)
        if c == "64":
            assert regs <= 256 and r.get("Occupancy") >= 2, (name, r)
        else:
            assert regs <= 128 and r.get("LDS Size") <= 81920 and r.get("Occupancy") >= 4, (name, r)


def _call(c, n_rays=4, S=64, L=16, F=2, T=1 << 19, stride=None, G=0, ptr=1 << 20, occ=None, emb=None,
          img=None, null=()):
    """f2n_render_rays with fake, aligned, non-null pointers: every call here is rejected (or is the
    empty launch) before the pointers could be used."""
    import ctypes

    names = ["rays_o", "rays_d", "noise", "table", "primes", "bias", "mul", "w_h", "b_h", "w1", "b1",
             "w2", "b2"]
    a = [None if n in null or n == "noise" else ptr for n in names]
    a += [emb, img, occ, G]
    a += [None if n in null else ptr for n in ("bg", "colors", "depths", "last_trans", "kept")]
    a += [None, n_rays, S, ctypes.c_float(1.0 / 64), L, F, T, T * F if stride is None else stride,
          ctypes.c_float(1e-4), ctypes.c_float(3.0), ctypes.c_float(1e-2), None]
    return c.f2n_render_rays(*a)


def test_argument_validation_without_gpu(capi):
    OK, INVALID, UNSUPPORTED = 0, -1, -3
    c = capi.lib().cdll
    assert "f2n_render_rays" in capi.parse_header()
    assert c.f2n_abi_version() == 2
    assert _call(c, n_rays=0) == OK                      # nothing to do: no launch
    assert _call(c, n_rays=0, S=100) == OK               # any S >= 1 is valid
    # widths and channel counts the matrix-core network does not cover
    for L, F in ((16, 3), (16, 16), (2, 5)):
        assert _call(c, n_rays=0, L=L, F=F) == UNSUPPORTED, (L, F)
    for L, F in ((3, 2), (16, 8), (1, 4), (12, 2), (64, 1), (5, 1)):
        assert _call(c, n_rays=0, L=L, F=F) == UNSUPPORTED, (L, F)
    for L, F in ((8, 1), (4, 2), (16, 2), (8, 8), (32, 1), (32, 2), (16, 4), (1, 8)):
        assert _call(c, n_rays=0, L=L, F=F) == OK, (L, F)
    # negative counts, S < 1, L < 1
    assert _call(c, n_rays=-1) == INVALID
    assert _call(c, S=0) == INVALID
    assert _call(c, L=0) == INVALID
    assert _call(c, T=0) == INVALID
    assert _call(c, stride=-2) == INVALID
    assert _call(c, stride=(1 << 19) * 2 + 1) == INVALID   # not a multiple of F
    # null required pointers
    for name in ("rays_o", "rays_d", "table", "primes", "bias", "mul", "w_h", "b_h", "w1", "b1", "w2",
                 "b2", "bg", "colors", "depths", "last_trans", "kept"):
        assert _call(c, null=(name,)) == INVALID, name
    # the embedding and the image ids come together
    assert _call(c, emb=1 << 20) == INVALID
    assert _call(c, img=1 << 20) == INVALID
    assert _call(c, emb=(1 << 20) + 4, img=1 << 20) == INVALID     # rows are read as float4
    # a grid needs a power-of-two resolution in 32..256; without a grid G is ignored
    for G in (0, 16, 48, 100, 512, -64):
        assert _call(c, occ=1 << 20, G=G) == INVALID, G
        assert _call(c, n_rays=0, occ=1 << 20, G=G) == INVALID, G
        assert _call(c, n_rays=0, occ=None, G=G) == OK, G
    for G in (32, 64, 128, 256):
        assert _call(c, n_rays=0, occ=1 << 20, G=G) == OK, G
    # ---- two faults at once: the first check's status (F and the width before the stride's
    # divisibility, the level cap as "unsupported", all of them before the pointers)
    odd = (1 << 19) * 2 + 1
    for kw, want in ((dict(n_rays=-1, F=3), INVALID), (dict(L=0, F=3), INVALID), (dict(T=0, F=3), INVALID),
                     (dict(S=0, F=3), INVALID), (dict(F=3, stride=odd), UNSUPPORTED),
                     (dict(L=33, F=3), UNSUPPORTED), (dict(L=33, stride=odd), UNSUPPORTED),
                     (dict(L=3, stride=odd), UNSUPPORTED), (dict(L=64, F=1), UNSUPPORTED),
                     (dict(L=64, F=1, stride=-2), INVALID), (dict(null=("table",), F=3), UNSUPPORTED),
                     (dict(null=("table",), L=33), UNSUPPORTED), (dict(n_rays=-1, L=33), INVALID),
                     (dict(occ=1 << 20, G=100, F=3), UNSUPPORTED)):
        assert _call(c, **kw) == want, kw
