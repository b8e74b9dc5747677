"""The matrix-core shade backward's two-wave form keeps its occupancy: every production
instantiation of shade_bwd_mfma_kernel at 16-sample tiles x 2 per stride compiles, with the
project's own HIP flags, to 2 waves per SIMD without scratch or spills and within a CU's LDS.
Cross-compiled for gfx950; needs hipcc, not a GPU."""
import importlib
import os
import re
import shutil
import subprocess

import pytest

build = importlib.import_module("f2-nerf_amd._build")
SRC = os.path.join(build.KERNEL_DIR, "shade_mfma.hip")


def _resource_usage(tmp_path):
    cmd = [build.HIPCC, *build.HIP_FLAGS, "-I", build.INCLUDE_DIR, "-I", build.KERNEL_DIR,
           "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", SRC,
           "-o", str(tmp_path / "shade_mfma.o")]
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


def test_shade_bwd_two_waves_per_simd(tmp_path):
    if not os.path.exists(build.HIPCC) and shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: the build needs it too")
    kernels = _resource_usage(tmp_path)
    # shade_bwd_mfma_kernel<C, V, WIDE, TS = 2>: mangled template arguments ...ILi<C>ELi<V>ELb<W>ELi2EE
    two_wave = {k: v for k, v in kernels.items()
                if re.search(r"shade_bwd_mfma_kernelILi\d+ELi\dELb\dELi2EE", k)}
    shapes = {re.search(r"kernelILi(\d+)ELi\dELb(\d)", k).groups() for k in two_wave}
    assert shapes == {(c, w) for c in ("8", "16", "32", "64") for w in ("0", "1")}, sorted(shapes)
    for name, r in two_wave.items():
        assert r.get("Occupancy") == 2, (name, r)
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0 and r.get("AGPRs Spill", 0) == 0, (name, r)
        assert r.get("VGPRs", 0) + r.get("AGPRs", 0) <= 256, (name, r)
        assert r.get("LDS Size") <= 163840, (name, r)
