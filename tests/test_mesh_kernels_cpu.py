"""f2n_density_lattice (density_lattice.hip) and f2n_mesh_count / f2n_mesh_emit (mesh.hip) without a
GPU: every instantiation compiles with the project's own HIP flags without scratch, spills or LDS, the
lattice kernel's instantiations are exactly the dispatched ones, registers and occupancy are those
DESIGN section 5 documents, and the C ABI rejects bad arguments before any HIP work.  Cross-compiled for
gfx950; needs hipcc."""
import importlib
import os
import re
import shutil
import subprocess

import pytest

build = importlib.import_module("f2-nerf_amd._build")
OK, INVALID, UNSUPPORTED = 0, -1, -3

# VGPRs (no AGPRs) and waves per SIMD from hipcc's resource remarks
LATTICE = {("1", "1"): (37, 8), ("1", "0"): (38, 8), ("2", "1"): (37, 8), ("2", "0"): (38, 8),
           ("4", "1"): (48, 8), ("4", "0"): (49, 8), ("8", "1"): (64, 8), ("8", "0"): (65, 7)}
MESH = {"mesh_count": (22, 8), "mesh_emit": (46, 8)}


def _remarks(tmp, stem):
    if not os.path.exists(build.HIPCC) and shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: the build needs it too")
    src = os.path.join(build.KERNEL_DIR, stem + ".hip")
    cmd = [build.HIPCC, *build.HIP_FLAGS, "-I", build.INCLUDE_DIR, "-I", build.KERNEL_DIR,
           "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
           str(tmp / (stem + ".o"))]
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
    return found


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mesh_kernels")
    lattice = {}
    for name, r in _remarks(tmp, "density_lattice").items():
        m = re.search(r"density_lattice_kernelILi(\d)ELb(\d)EE", name)
        assert m, "a kernel the dispatcher does not know: " + name
        lattice[(m.group(1), m.group(2))] = (name, r)
    mesh = {}
    for name, r in _remarks(tmp, "mesh").items():
        m = re.search(r"\d+(mesh_count|mesh_emit)_kernelE", name)
        assert m, "an unexpected kernel: " + name
        mesh[m.group(1)] = (name, r)
    return lattice, mesh


def test_instantiations_are_exactly_the_dispatched_ones(kernels):
    """f2n_dispatch_field: F in {1, 2, 4, 8} x (T a power of two or not); one mapping, L an argument"""
    lattice, mesh = kernels
    assert set(lattice) == {(str(f), p) for f in (1, 2, 4, 8) for p in ("0", "1")}
    assert set(mesh) == {"mesh_count", "mesh_emit"}


def test_no_scratch_no_spills(kernels):
    for inst in kernels:
        for name, r in inst.values():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("AGPRs Spill", 0) == 0, (name, r)
            assert r.get("SGPRs Spill") == 0, (name, r)
            assert r.get("LDS Size", 0) == 0, (name, r)


def test_registers_and_occupancy_are_the_documented_ones(kernels):
    for inst, documented in zip(kernels, (LATTICE, MESH)):
        for key, (name, r) in inst.items():
            vgprs, waves = documented[key]
            assert r.get("AGPRs", 0) == 0, (name, r)
            assert r.get("VGPRs") == vgprs, (name, r)
            assert r.get("Occupancy") == waves, (name, r)


def test_design_documents_these_figures():
    text = open(os.path.join(build.REPO_DIR, "DESIGN.md")).read()
    at = text.index("f2n_density_lattice, f2n_mesh_count and f2n_mesh_emit")
    block = text[at:at + 8000]
    for f in ("1", "2", "4", "8"):
        cell = "%d / %d" % (LATTICE[(f, "1")][0], LATTICE[(f, "0")][0])
        assert cell in block, (f, cell)
    for entry, (vgprs, waves) in MESH.items():
        assert "%s_kernel | %d | %d" % (entry, vgprs, waves) in block, entry


def _lattice(c, dims=(5, 6, 7), step=(0.1, 0.1, 0.1), L=16, F=2, T=1 << 14, stride=None, ptr=1 << 20, null=()):
    """f2n_density_lattice with fake, aligned, non-null pointers: every call here is rejected before the
    pointers could be used"""
    a = [None if k in null else ptr for k in ("table", "primes", "bias", "mul", "w0", "b0", "logit")]
    if "table_odd" in null:
        a[0] = ptr + 2
    return c.f2n_density_lattice(*a, -1.0, -1.0, -1.0, *step, *dims, L, F, T, T if stride is None else stride, None)


def test_lattice_argument_validation_without_gpu(capi):
    c = capi.lib().cdll
    assert {"f2n_density_lattice", "f2n_mesh_count", "f2n_mesh_emit"} <= set(capi.parse_header())
    assert c.f2n_abi_version() == 2
    for dims in ((1, 6, 7), (5, 1, 7), (5, 6, 1), (0, 6, 7), (-3, 6, 7), (1 << 16, 1 << 15, 2), (2048, 1024, 1024)):
        assert _lattice(c, dims=dims) == INVALID, dims
    for step in ((0.0, 0.1, 0.1), (0.1, -0.1, 0.1), (0.1, 0.1, float("nan"))):
        assert _lattice(c, step=step) == INVALID, step
    assert _lattice(c, L=0) == INVALID and _lattice(c, T=0) == INVALID and _lattice(c, stride=-2) == INVALID
    assert _lattice(c, F=4, stride=(1 << 14) + 2) == INVALID
    for F in (0, 3, 5, 16):
        assert _lattice(c, F=F) == UNSUPPORTED, F
    assert _lattice(c, L=33) == UNSUPPORTED
    for name in ("table", "primes", "bias", "mul", "w0", "b0", "logit"):
        assert _lattice(c, null=(name,)) == INVALID, name
    assert _lattice(c, F=4, null=("table_odd",)) == INVALID
    # two faults at once: the lattice, then f2n_field_args_status, then the level cap, then the pointers
    for kw, want in ((dict(dims=(1, 6, 7), F=3), INVALID), (dict(step=(0.0, 1.0, 1.0), L=33), INVALID),
                     (dict(L=0, F=3), INVALID), (dict(L=33, F=3), UNSUPPORTED),
                     (dict(L=33, F=2, stride=(1 << 14) + 1), INVALID), (dict(L=33, null=("w0",)), UNSUPPORTED),
                     (dict(F=3, null=("logit",)), UNSUPPORTED)):
        assert _lattice(c, **kw) == want, kw


def _emit(c, V=10, T=10, dims=(5, 6, 7), step=(0.1, 0.1, 0.1), ptr=1 << 20, null=()):
    a = [None if k in null else ptr for k in ("values", "mask", "voff", "toff", "vertices", "triangles")]
    return c.f2n_mesh_emit(*a, V, T, -1.0, -1.0, -1.0, *step, 0.0, *dims, None)


def test_mesh_argument_validation_without_gpu(capi):
    c = capi.lib().cdll
    ptr = 1 << 20
    for dims in ((1, 6, 7), (5, 1, 7), (5, 6, 1), (2048, 1024, 1024)):
        assert c.f2n_mesh_count(ptr, ptr, ptr, ptr, *dims, 0.0, None) == INVALID, dims
        assert _emit(c, dims=dims) == INVALID, dims
    for k in range(4):
        a = [ptr] * 4
        a[k] = None
        assert c.f2n_mesh_count(*a, 5, 6, 7, 0.0, None) == INVALID, k
    assert _emit(c, V=0, T=0) == OK and _emit(c, V=0, T=0, null=("vertices", "triangles", "values")) == OK
    assert _emit(c, V=-1) == INVALID and _emit(c, T=-1) == INVALID
    assert _emit(c, V=0, T=4) == INVALID and _emit(c, V=4, T=0) == INVALID
    assert _emit(c, V=1 << 31) == UNSUPPORTED and _emit(c, T=((1 << 31) + 2) // 3) == UNSUPPORTED
    assert _emit(c, V=(1 << 31) - 1, T=((1 << 31) - 1) // 3, null=("voff",)) == INVALID     # the largest accepted
    assert _emit(c, step=(0.1, 0.0, 0.1)) == INVALID
    for name in ("values", "mask", "voff", "toff", "vertices", "triangles"):
        assert _emit(c, null=(name,)) == INVALID, name


def test_no_cpu_implementation(pkg):
    import torch

    H = pkg.load_host()
    field = H.Hash3DAnchored(n_levels=2, n_channels=2, log2_table=8, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        H.density_lattice(field, (-1.0, -1.0, -1.0), (0.5, 0.5, 0.5), (5, 5, 5))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        H.marching_tets(torch.zeros(3, 3, 3), 0.0, (-1.0, -1.0, -1.0), (0.5, 0.5, 0.5))
    r = H.Renderer(2, n_levels=2, log2_table=8, max_samples=8, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        H.extract_mesh(r, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (5, 5, 5), 1.0)
    assert H.DENSITY_SHIFT == 3.0
