"""hash_fwd_raytile_kernel with both corner orders in it (F2N_OPT_GATHER_PAIRED) keeps what it had with
one: every instantiation compiles, with the project's own HIP flags, without scratch or spills, and
its registers leave the occupancy to its LDS -- three workgroups (of one wave per SIMD) per CU at
F = 2 with 32-sample tiles, the benchmark's form.  Cross-compiled for gfx950 and read from the code
object's resource usage; needs hipcc, not a GPU."""
import importlib
import os
import re
import shutil
import subprocess

import pytest

build = importlib.import_module("f2-nerf_amd._build")
SRC = os.path.join(build.KERNEL_DIR, "hash_grid.hip")
LDS_PER_CU = 163840
# registers per lane: the parent's 32-sample-tile kernels took 73 and its 16-sample-tile ones 40-54
# (F = 8); 128 is what four waves per SIMD allow, more than the LDS ever admits here
MAX_VGPRS = 128


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(build.HIPCC) and shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: the build needs it too")
    out = tmp_path_factory.mktemp("hash_raytile") / "hash_grid.o"
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
    return {re.search(r"kernelILi(\d+)ELb(\d)ELi(\d+)EE", k).groups(): (k, v)
            for k, v in found.items() if "hash_fwd_raytile_kernelI" in k}


def test_every_instantiation_is_there(kernels):
    assert set(kernels) == {(f, p, s) for f in "1248" for p in "01" for s in ("16", "32")}, sorted(kernels)


def test_no_scratch_and_occupancy_left_to_the_lds(kernels):
    for (f, p2, s), (name, r) in kernels.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0 and r.get("AGPRs Spill", 0) == 0, (name, r)
        assert r.get("VGPRs", 0) + r.get("AGPRs", 0) <= MAX_VGPRS, (name, r)
        by_lds = min(LDS_PER_CU // r["LDS Size"], 8)        # workgroups per CU = waves per SIMD
        assert r.get("Occupancy") == by_lds, (name, r, by_lds)


def test_benchmark_form_holds_three_workgroups_per_cu(kernels):
    for p2 in "01":
        name, r = kernels[("2", p2, "32")]
        assert r.get("Occupancy") == 3, (name, r)
        assert r.get("VGPRs", 0) <= 80, (name, r)           # the parent's 73, with a little room
