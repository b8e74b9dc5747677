"""The eight-rays-per-wavefront head and the resumed tail of the one-pass render (render_rays_head.hip:
f2n_render_rays_head, f2n_render_rays_tail, f2n_render_rays_state_bytes) without a GPU: every
instantiation the launchers can reach compiles, with the project's own HIP flags, without scratch or
spills and within a CU's LDS; the sets of instantiations are exactly the dispatched ones; and the C ABI
rejects bad arguments -- the n_head and state rules among them -- before any HIP work.  Cross-compiled
for gfx950; needs hipcc.  (The occupancy reached is recorded in DESIGN section 5, not fixed here.)"""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest

build = importlib.import_module("f2-nerf_amd._build")
SRC = os.path.join(build.KERNEL_DIR, "render_rays_head.hip")
MAX_LEVELS = 32


def _dispatched():
    """(C, F, pow2 T) as both launchers' switches reach them: the set of f2n_render_rays."""
    return {(str(c), str(f), p) for c in (8, 16, 32, 64) for f in (1, 2, 4, 8) if c // f <= MAX_LEVELS
            for p in ("0", "1")}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(build.HIPCC) and shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: the build needs it too")
    out = tmp_path_factory.mktemp("render_rays_head") / "render_rays_head.o"
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
    # render_rays_{head,tail}_kernel<C, F, POW2>
    by_kind = {"head": {}, "tail": {}, "other": {}}
    for k, v in found.items():
        m = re.search(r"render_rays_(head|tail)_kernelILi(\d+)ELi(\d)ELb(\d)EE", k)
        if m:
            by_kind[m.group(1)][m.groups()[1:]] = (k, v)
        else:
            by_kind["other"][k] = v
    return by_kind


def test_instantiations_are_exactly_the_dispatched_ones(kernels):
    assert set(kernels["head"]) == _dispatched(), sorted(kernels["head"])
    assert set(kernels["tail"]) == _dispatched(), sorted(kernels["tail"])
    assert len(kernels["head"]) == 30 and len(kernels["tail"]) == 30
    assert not kernels["other"], sorted(kernels["other"])


def test_no_scratch_no_spills_lds_within_a_cu(kernels):
    for kind in ("head", "tail"):
        for key, (name, r) in kernels[kind].items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("AGPRs Spill", 0) == 0, (name, r)
            assert r.get("LDS Size") <= 163840, (name, r)


def _call(c, entry, n_rays=4, S=128, L=16, F=2, T=1 << 19, stride=None, G=0, ptr=1 << 20, occ=None,
          emb=None, img=None, null=(), n_head=64, state=1 << 20):
    """An entry with fake, aligned, non-null pointers: every call here is rejected (or is the empty
    launch) before the pointers could be used."""
    names = ["rays_o", "rays_d", "noise", "table", "primes", "bias", "mul", "w_h", "b_h", "w1", "b1",
             "w2", "b2"]
    a = [None if n in null or n == "noise" else ptr for n in names]
    a += [emb, img, occ, G]
    a += [None if n in null else ptr for n in ("bg", "colors", "depths", "last_trans", "kept")]
    a += [None, n_rays, S, ctypes.c_float(1.0 / 64), L, F, T, T * F if stride is None else stride,
          ctypes.c_float(1e-4), ctypes.c_float(3.0), ctypes.c_float(1e-2), n_head, state, None]
    return getattr(c, entry)(*a)


def test_header_declares_the_entries_and_the_version_stays(capi):
    decls = capi.parse_header()
    for name in ("f2n_render_rays_head", "f2n_render_rays_tail", "f2n_render_rays_state_bytes"):
        assert name in decls, name
    head, tail = decls["f2n_render_rays_head"][1], decls["f2n_render_rays_tail"][1]
    assert [n for _, n in head] == [n for _, n in tail]
    assert [n for _, n in head][-3:] == ["n_head", "state", "stream"]
    # the arguments of f2n_render_rays, then n_head and state, then the stream
    assert [n for _, n in head][:-3] == [n for _, n in decls["f2n_render_rays"][1]][:-1]
    assert capi.lib().cdll.f2n_abi_version() == 2
    text = open(capi.HEADER).read()
    i = text.index("int64_t f2n_render_rays_state_bytes")
    doc = text[text.rindex("/*", 0, i):i]
    for site in ("src/renderer.cpp:33-123", "src/renderer.cpp:125-151", "src/localizer.cpp:172"):
        assert site in doc, site


def test_state_bytes(capi):
    c = capi.lib().cdll
    assert c.f2n_render_rays_state_bytes(0) == 0
    assert c.f2n_render_rays_state_bytes(1) == 64          # at most 64 bytes per ray
    assert c.f2n_render_rays_state_bytes(65536) == 64 * 65536
    assert c.f2n_render_rays_state_bytes((1 << 31) - 1) == 64 * ((1 << 31) - 1)   # no 32-bit overflow
    assert c.f2n_render_rays_state_bytes(-1) < 0


@pytest.mark.parametrize("entry", ["f2n_render_rays_head", "f2n_render_rays_tail"])
def test_argument_validation_without_gpu(capi, entry):
    OK, INVALID, UNSUPPORTED = 0, -1, -3
    c = capi.lib().cdll
    call = lambda **kw: _call(c, entry, **kw)
    assert call(n_rays=0) == OK                            # nothing to do: no launch
    assert call(n_rays=0, S=100) == OK
    # ---- n_head: a multiple of 64, or >= S
    for S, n_head in ((128, 64), (192, 128), (1024, 960), (100, 64), (128, 128), (128, 129), (100, 100),
                      (64, 64), (1, 1), (50, 77), (128, 1 << 30)):
        assert call(n_rays=0, S=S, n_head=n_head) == OK, (S, n_head)
    for S, n_head in ((128, 0), (128, -1), (128, -64), (128, 1), (128, 63), (128, 65), (128, 100),
                      (128, 127), (1024, 1000), (100, 99), (100, 8)):
        assert call(n_rays=0, S=S, n_head=n_head) == INVALID, (S, n_head)
        assert call(S=S, n_head=n_head) == INVALID, (S, n_head)
    # ---- state: needed when a ray can outlive the head, 16-byte aligned
    assert call(n_rays=0, S=128, n_head=64, state=None) == INVALID
    assert call(S=128, n_head=64, state=None) == INVALID
    assert call(n_rays=0, S=128, n_head=128, state=None) == OK        # whole rays: no state
    assert call(n_rays=0, S=100, n_head=1 << 30, state=None) == OK
    assert call(n_rays=0, S=128, n_head=64, state=(1 << 20) + 4) == INVALID
    # ---- everything f2n_render_rays checks
    for L, F in ((16, 3), (16, 16), (2, 5), (3, 2), (16, 8), (1, 4), (12, 2), (64, 1), (5, 1)):
        assert call(n_rays=0, L=L, F=F) == UNSUPPORTED, (L, F)
    for L, F in ((8, 1), (4, 2), (16, 2), (8, 8), (32, 1), (32, 2), (16, 4), (1, 8)):
        assert call(n_rays=0, L=L, F=F) == OK, (L, F)
    assert call(n_rays=-1) == INVALID
    assert call(S=0) == INVALID
    assert call(L=0) == INVALID
    assert call(T=0) == INVALID
    assert call(stride=-2) == INVALID
    assert call(stride=(1 << 19) * 2 + 1) == INVALID       # not a multiple of F
    for name in ("rays_o", "rays_d", "table", "primes", "bias", "mul", "w_h", "b_h", "w1", "b1", "w2",
                 "b2", "bg", "colors", "depths", "last_trans", "kept"):
        assert call(null=(name,)) == INVALID, name
    assert call(emb=1 << 20) == INVALID
    assert call(img=1 << 20) == INVALID
    assert call(emb=(1 << 20) + 4, img=1 << 20) == INVALID  # rows are read as float4
    for G in (0, 16, 48, 100, 512, -64):
        assert call(occ=1 << 20, G=G) == INVALID, G
        assert call(n_rays=0, occ=1 << 20, G=G) == INVALID, G
        assert call(n_rays=0, occ=None, G=G) == OK, G
    for G in (32, 64, 128, 256):
        assert call(n_rays=0, occ=1 << 20, G=G) == OK, G
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
        assert call(**kw) == want, kw
