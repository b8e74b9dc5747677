"""f2n_hash_pts_grad_exact and f2n_hash_rays_grad_exact (enc_grad.hip) without a GPU: they parse from
the header with a citation, are exported, answer bad arguments with the documented status before any
HIP work (the siblings' checks, in the siblings' order: f2n_hash_bwd's and f2n_hash_rays_grad's), and
every instantiation the dispatcher reaches compiles with the project's own HIP flags without scratch,
spills or LDS.  Cross-compiled for gfx950; needs hipcc, not a GPU."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest

build = importlib.import_module("f2-nerf_amd._build")
SRC = os.path.join(build.KERNEL_DIR, "enc_grad.hip")
NEW = ("f2n_hash_pts_grad_exact", "f2n_hash_rays_grad_exact")
OK, INVALID, UNSUPPORTED = 0, -1, -3
FAKE = ctypes.c_void_p(0x1000)        # never dereferenced: validation answers first
T = 1 << 14


def _pts_args(**kw):
    """f2n_hash_pts_grad_exact(pts, table, primes, bias, mul, g, ld_p, ld_c, pts_grad, n, L, F, T,
    level_stride, stream)"""
    a = dict(pts=FAKE, table=FAKE, primes=FAKE, bias=FAKE, mul=FAKE, g=FAKE, ld_p=32, ld_c=1, out=FAKE,
             n=8, L=16, F=2, T=T, stride=T, stream=None)
    a.update(kw)
    return list(a.values())


def _rays_args(**kw):
    """f2n_hash_rays_grad_exact(pts, t, bounds, rays_d, table, primes, bias, mul, g, ld_p, ld_c, d_o, d_d,
    n_rays, L, F, T, level_stride, stream)"""
    a = dict(pts=FAKE, t=FAKE, bounds=FAKE, rays_d=FAKE, table=FAKE, primes=FAKE, bias=FAKE, mul=FAKE,
             g=FAKE, ld_p=1, ld_c=1 << 10, d_o=FAKE, d_d=FAKE, n=4, L=16, F=2, T=T, stride=T, stream=None)
    a.update(kw)
    return list(a.values())


ENTRIES = [("f2n_hash_pts_grad_exact", _pts_args, ("pts", "table", "primes", "bias", "mul", "g", "out")),
           ("f2n_hash_rays_grad_exact", _rays_args,
            ("pts", "t", "bounds", "rays_d", "table", "primes", "bias", "mul", "g", "d_o", "d_d"))]


def test_entry_points_parse_export_and_cite(capi):
    decls = capi.parse_header()
    cdll = ctypes.CDLL(capi.LIB_PATH)
    text = open(capi.HEADER).read()
    for name in NEW:
        assert name in decls and hasattr(cdll, name), name
        pos = text.index(name + "(")
        block = text[text.rindex("/*", 0, pos):pos]
        assert "src/hash_3d_anchored.cu:25-93" in block, name      # the forward being differentiated
        assert "src/hash_3d_anchored.cu:138-143" in block, name    # the form it replaces
        assert "NOT quirk Q5" in block, name
    assert capi.lib().cdll.f2n_abi_version() == 2                   # the additions leave the ABI version
    rays, q5 = decls["f2n_hash_rays_grad_exact"][1], decls["f2n_hash_rays_grad"][1]
    assert rays == [p for p in q5 if p[1] != "grad_scale"]         # f2n_hash_rays_grad's, without grad_scale
    src = open(SRC).read()
    assert "f2n_dispatch_field(" in src and re.search(r"atomic\w*\s*\(", src, re.I) is None
    assert src.count("density_grad_level<F, POW2>(") == 1 and "#include \"density_grad.hiph\"" in src


@pytest.mark.parametrize("name,args,ptrs", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_argument_validation_without_gpu(capi, name, args, ptrs):
    fn = getattr(capi.lib().cdll, name)
    assert fn(*args(n=0)) == OK                                     # the empty call: no launch
    for L, F in ((1, 1), (4, 8), (32, 2), (32, 8), (5, 4), (16, 1)):
        assert fn(*args(n=0, L=L, F=F, stride=T * F)) == OK, (L, F)
    assert fn(*args(n=0, T=12289, stride=2 * 12289)) == OK
    for p in ptrs:
        assert fn(*args(**{p: None})) == INVALID, p
        assert fn(*args(n=0, **{p: None})) == INVALID, p            # the siblings check pointers first
    assert fn(*args(n=-1)) == INVALID
    assert fn(*args(ld_p=-1)) == INVALID and fn(*args(ld_c=-1)) == INVALID
    for F in (0, 3, 5, 16):
        assert fn(*args(F=F)) == UNSUPPORTED, F
    assert fn(*args(L=0)) == INVALID and fn(*args(L=33)) == INVALID
    assert fn(*args(T=0)) == INVALID
    assert fn(*args(stride=-2)) == INVALID
    assert fn(*args(F=4, stride=T + 2)) == INVALID                  # no multiple of F
    assert fn(*args(F=4, table=ctypes.c_void_p(0x1002))) == INVALID  # a row is one load of 2 F bytes
    # two faults at once: the first check's status -- pointers, counts, F, the rest of the field
    assert fn(*args(n=-1, F=3)) == INVALID
    assert fn(*args(L=0, F=3)) == UNSUPPORTED and fn(*args(F=3, stride=T + 1)) == UNSUPPORTED
    assert fn(*args(table=None, F=3)) == INVALID


def test_every_instantiation_compiles_without_scratch(tmp_path):
    if not os.path.exists(build.HIPCC) and shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: the build needs it too")
    cmd = [build.HIPCC, *build.HIP_FLAGS, "-I", build.INCLUDE_DIR, "-I", build.KERNEL_DIR,
           "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", SRC, "-o",
           str(tmp_path / "enc_grad.o")]
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
    seen = set()
    for name, r in found.items():
        m = re.search(r"hash_(pts|rays)_grad_exact_kernelILi(\d)ELb(\d)EE", name)
        assert m, "a kernel the dispatcher does not know: " + name
        seen.add(m.groups())
        assert r.get("ScratchSize") == 0 and r.get("LDS Size", 0) == 0, (name, r)
        assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0 and r.get("AGPRs", 0) == 0, (name, r)
    assert seen == {(k, str(f), p) for k in ("pts", "rays") for f in (1, 2, 4, 8) for p in ("0", "1")}
