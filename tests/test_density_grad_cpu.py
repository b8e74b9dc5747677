"""f2n_density_grad and f2n_ray_normals (density_grad.hip) without a GPU: the C ABI rejects bad
arguments before any HIP work, every instantiation the dispatcher reaches compiles with the project's
own HIP flags without scratch or spills, the set of instantiations is exactly the dispatched one, and
the registers and occupancy are those DESIGN section 5 documents.  Cross-compiled for gfx950; needs
hipcc."""
import importlib
import os
import re
import shutil
import subprocess

import pytest

build = importlib.import_module("f2-nerf_amd._build")
SRC = os.path.join(build.KERNEL_DIR, "density_grad.hip")
OK, INVALID, UNSUPPORTED = 0, -1, -3

# VGPRs (no AGPRs) and waves per SIMD from hipcc's resource remarks, (F, pow2 T)
DOCUMENTED = {
    "density_grad": {("1", "1"): (44, 8), ("1", "0"): (45, 8), ("2", "1"): (44, 8), ("2", "0"): (45, 8),
                     ("4", "1"): (53, 8), ("4", "0"): (54, 8), ("8", "1"): (71, 7), ("8", "0"): (68, 7)},
    "ray_normals": {("1", "1"): (54, 8), ("1", "0"): (56, 8), ("2", "1"): (54, 8), ("2", "0"): (56, 8),
                    ("4", "1"): (63, 8), ("4", "0"): (64, 8), ("8", "1"): (78, 6), ("8", "0"): (79, 6)},
}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(build.HIPCC) and shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: the build needs it too")
    out = tmp_path_factory.mktemp("density_grad") / "density_grad.o"
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
    out = {}
    for name, r in found.items():
        m = re.search(r"(density_grad|ray_normals)_kernelILi(\d)ELb(\d)EE", name)
        assert m, "a kernel the dispatcher does not know: " + name
        out.setdefault(m.group(1), {})[(m.group(2), m.group(3))] = (name, r)
    return out


def test_instantiations_are_exactly_the_dispatched_ones(kernels):
    """f2n_dispatch_field: F in {1, 2, 4, 8} x (T a power of two or not); L is a kernel argument"""
    want = {(str(f), p) for f in (1, 2, 4, 8) for p in ("0", "1")}
    assert set(kernels) == {"density_grad", "ray_normals"}
    for entry, inst in kernels.items():
        assert set(inst) == want, (entry, sorted(inst))


def test_no_scratch_no_spills(kernels):
    for entry, inst in kernels.items():
        for key, (name, r) in inst.items():
            assert r.get("ScratchSize") == 0, (name, r)
            assert r.get("VGPRs Spill") == 0 and r.get("AGPRs Spill", 0) == 0, (name, r)
            assert r.get("SGPRs Spill") == 0, (name, r)
            assert r.get("LDS Size", 0) == 0, (name, r)


def test_registers_and_occupancy_are_the_documented_ones(kernels):
    for entry, inst in kernels.items():
        for key, (name, r) in inst.items():
            vgprs, waves = DOCUMENTED[entry][key]
            assert r.get("AGPRs", 0) == 0, (name, r)
            assert r.get("VGPRs") == vgprs, (name, r)
            assert r.get("Occupancy") == waves, (name, r)


def test_design_documents_these_figures():
    text = open(os.path.join(build.REPO_DIR, "DESIGN.md")).read()
    at = text.index("f2n_density_grad and f2n_ray_normals")
    block = text[at:at + 6000]
    for entry, inst in DOCUMENTED.items():
        for f in ("1", "2", "4", "8"):
            cell = "%d / %d" % (inst[(f, "1")][0], inst[(f, "0")][0])
            assert cell in block, (entry, f, cell)


def _grad(c, n=8, L=16, F=2, T=1 << 14, stride=None, ptr=1 << 20, null=()):
    """f2n_density_grad with fake, aligned, non-null pointers: every call here is rejected (or is the
    empty launch) before the pointers could be used."""
    a = [None if k in null else ptr for k in ("pts", "table", "primes", "bias", "mul", "w0", "grad")]
    if "table_odd" in null:
        a[1] = ptr + 2
    return c.f2n_density_grad(*a, n, L, F, T, T if stride is None else stride, None)


def _normals(c, n_rays=8, L=16, F=2, T=1 << 14, stride=None, ptr=1 << 20, null=()):
    a = [None if k in null else ptr
         for k in ("pts", "bounds", "weights", "table", "primes", "bias", "mul", "w0", "normals")]
    if "table_odd" in null:
        a[3] = ptr + 2
    return c.f2n_ray_normals(*a, n_rays, L, F, T, T if stride is None else stride, None)


@pytest.mark.parametrize("call,ptrs", [
    (_grad, ("pts", "table", "primes", "bias", "mul", "w0", "grad")),
    (_normals, ("pts", "bounds", "weights", "table", "primes", "bias", "mul", "w0", "normals"))],
    ids=["density_grad", "ray_normals"])
def test_argument_validation_without_gpu(capi, call, ptrs):
    c = capi.lib().cdll
    assert {"f2n_density_grad", "f2n_ray_normals"} <= set(capi.parse_header())
    assert c.f2n_abi_version() == 2
    count = "n" if call is _grad else "n_rays"
    empty = {count: 0}
    assert call(c, **empty) == OK                                   # nothing to do: no launch
    assert call(c, **empty, null=ptrs) == OK                        # ... whatever the pointers
    for L, F in ((1, 1), (4, 8), (32, 2), (32, 8), (5, 4), (16, 1)):  # any L up to the cap, any of the four F
        assert call(c, **empty, L=L, F=F) == OK, (L, F)
    assert call(c, **empty, T=12289, stride=2 * 12289) == OK and call(c, **empty, T=1, stride=2) == OK
    assert call(c, **{count: -1}) == INVALID
    assert call(c, L=0) == INVALID
    assert call(c, T=0) == INVALID
    assert call(c, stride=-2) == INVALID
    assert call(c, F=4, stride=(1 << 14) + 2) == INVALID            # not a multiple of F
    for F in (0, 3, 5, 16):
        assert call(c, F=F) == UNSUPPORTED, F
    assert call(c, L=33) == UNSUPPORTED and call(c, **empty, L=33) == UNSUPPORTED
    for name in ptrs:
        assert call(c, null=(name,)) == INVALID, name
    assert call(c, F=4, null=("table_odd",)) == INVALID             # a row is one load of 2 F bytes
    # two faults at once: the first check's status -- the count, then f2n_field_args_status (L, T and
    # the stride's sign; F; the stride's divisibility), then the level cap, then the pointers
    for kw, want in ((dict(F=3, **{count: -1}), INVALID), (dict(L=0, F=3), INVALID), (dict(T=0, F=3), INVALID),
                     (dict(F=3, stride=(1 << 14) + 1), UNSUPPORTED), (dict(L=33, F=3), UNSUPPORTED),
                     (dict(L=33, F=2, stride=(1 << 14) + 1), INVALID), (dict(L=33, null=("pts",)), UNSUPPORTED),
                     (dict(F=3, null=("pts",)), UNSUPPORTED), (dict(L=33, **{count: -1}), INVALID)):
        assert call(c, **kw) == want, kw


def test_no_cpu_implementation(pkg):
    """Hash3DAnchored.density_grad and a render with normals on refuse CPU tensors like every operator"""
    import torch

    H = pkg.load_host()
    field = H.Hash3DAnchored(n_levels=2, n_channels=2, log2_table=8, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        field.density_grad(torch.ones(3, 3))
    r = H.Renderer(2, n_levels=2, log2_table=8, max_samples=8, device="cpu")
    assert not r.normals
    r.set_normals(True)
    assert r.normals
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        r.render_all_rays_with_normals(torch.zeros(3, 3), torch.ones(3, 3), 2)
    assert r.normals                      # the call restores what it found, an exception included
    r.set_normals(False)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        r.render_all_rays_with_normals(torch.zeros(3, 3), torch.ones(3, 3), 2)
    assert not r.normals
