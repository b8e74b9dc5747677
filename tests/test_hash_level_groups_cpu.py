"""f2n_hash_fwd_raytile_groups and hash_fwd_raytile_kernel_groups without a GPU: the entry is declared and
exported, answers invalid calls before any HIP work, the default schedule is what the header's rule
says, and every instantiation of the kernel compiles for gfx950 with the project's own flags without
scratch or spills, at no more than 128 registers and with as many workgroups per CU as its LDS admits --
no fewer than hash_fwd_raytile_kernel of the same (F, POW2, SAMPLES), three for the benchmark's form.
Read from the code object's resource usage as tests/test_hash_raytile_occupancy_cpu.py reads it."""
import importlib
import os
import re
import shutil
import subprocess

import pytest

build = importlib.import_module("f2-nerf_amd._build")
SRC = os.path.join(build.KERNEL_DIR, "hash_grid.hip")
LDS_PER_CU = 163840
MAX_VGPRS = 128
INVALID, UNSUPPORTED = -1, -3
FORMS = {(f, p, s) for f in "1248" for p in "01" for s in ("16", "32")}


def test_entry_is_declared_and_exported(capi):
    decls = capi.parse_header()
    ret, params = decls["f2n_hash_fwd_raytile_groups"]
    _, old = decls["f2n_hash_fwd_raytile"]
    # the same arguments, the mask before the stream
    assert [n for _, n in params] == [n for _, n in old[:-1]] + ["group_starts", "stream"]
    assert params[-2][0] is capi._CTYPES["uint32_t"]
    assert "f2n_hash_raytile_default_groups" in decls
    cdll = capi.lib().cdll
    assert hasattr(cdll, "f2n_hash_fwd_raytile_groups") and cdll.f2n_abi_version() == 2


def test_invalid_calls_are_answered_before_any_hip_work(capi):
    fn = capi.lib().cdll.f2n_hash_fwd_raytile_groups
    fake = 0x1000
    # (pts, table, primes, bias, mul, out_cm, n_rays, S, L, F, T, level_stride, group_starts, stream)
    good = [fake] * 6 + [130, 32, 16, 2, 1 << 12, 1 << 12, 0xfc41, None]
    for i in range(6):
        args = list(good)
        args[i] = None
        assert fn(*args) == INVALID, i
    for faults, want in (({7: 24}, UNSUPPORTED),              # S % 16 != 0
                         ({7: 8}, UNSUPPORTED),
                         ({12: 1 << 16}, INVALID),            # a group that opens at level L
                         ({12: 0x80000001}, INVALID),
                         ({8: 5, 12: 0x21}, INVALID),         # bit 5 at L = 5
                         ({8: 33}, UNSUPPORTED),              # more than 32 levels
                         ({8: 33, 12: 0}, UNSUPPORTED),
                         ({8: 0}, INVALID),
                         ({9: 3}, UNSUPPORTED),               # F
                         ({6: -1}, INVALID)):
        args = list(good)
        for i, bad in faults.items():
            args[i] = bad
        assert fn(*args) == want, faults
    for mask in (0, 1, 0xfc41, 0xffff):                       # no rays: nothing to launch
        args = list(good)
        args[6], args[12] = 0, mask
        assert fn(*args) == 0, mask


FEW_TILES = 1024


def _rule(L, tiles):
    """the header's rule, position = l / (L - 1).  From FEW_TILES tiles on: the levels below 2/3 one
    group, the levels from 2/3 on two to a group, counted from the first of them.  Fewer tiles: the
    levels below 2/5 one group, from 2/5 to below 2/3 a second, every level from 2/3 on its own."""
    fine = [l for l in range(1, L) if 3 * l >= 2 * (L - 1)]
    if tiles >= FEW_TILES:
        return 1 | sum(1 << l for l in fine[::2])
    middle = [l for l in range(1, L) if 5 * l >= 2 * (L - 1) and l not in fine]
    return 1 | sum(1 << l for l in fine + middle[:1])


def test_default_schedule_is_the_documented_rule(capi):
    fn = capi.lib().cdll.f2n_hash_raytile_default_groups
    for tiles in (0, 1, FEW_TILES - 1, FEW_TILES, 1 << 40):
        assert fn(1, tiles) == 0b1
        assert fn(2, tiles) == 0b11
    assert fn(16, 4096) == fn(16, FEW_TILES) == 0x5401        # 0-9, 10-11, 12-13, 14-15
    assert fn(16, 256) == fn(16, FEW_TILES - 1) == 0xfc41     # 0-5, 6-9, 10, 11, 12, 13, 14, 15
    assert fn(5, 4096) == 0b01001                             # 0-2, 3-4
    assert fn(5, 256) == 0b11101                              # 0-1, 2, 3, 4
    header = open(capi.HEADER).read()
    assert "0x5401" in header and "0xfc41" in header and "tiles >= %d" % FEW_TILES in header
    for L in range(1, 33):
        for tiles in (0, 256, FEW_TILES - 1, FEW_TILES, 4096):
            assert fn(L, tiles) == _rule(L, tiles), (L, tiles)
    assert fn(0, 4096) == INVALID and fn(33, 4096) == UNSUPPORTED and fn(16, -1) == INVALID


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(build.HIPCC) and shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: the build needs it too")
    out = tmp_path_factory.mktemp("hash_level_groups") / "hash_grid.o"
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

    def by_form(marker):
        return {re.search(marker + r"ILi(\d+)ELb(\d)ELi(\d+)EE", k).groups(): (k, v)
                for k, v in found.items() if marker + "I" in k}

    return by_form("hash_fwd_raytile_kernel_groups"), by_form("hash_fwd_raytile_kernel")


def test_every_instantiation_is_there(kernels):
    groups, parent = kernels
    assert set(groups) == FORMS, sorted(groups)
    assert set(parent) == FORMS, sorted(parent)


def test_no_scratch_and_occupancy_left_to_the_lds(kernels):
    groups, parent = kernels
    for form, (name, r) in groups.items():
        assert r.get("ScratchSize") == 0, (name, r)
        assert r.get("VGPRs Spill") == 0 and r.get("AGPRs Spill", 0) == 0, (name, r)
        assert r.get("SGPRs Spill", 0) == 0, (name, r)
        assert r.get("VGPRs", 0) + r.get("AGPRs", 0) <= MAX_VGPRS, (name, r)
        by_lds = min(LDS_PER_CU // r["LDS Size"], 8)        # workgroups per CU = waves per SIMD
        assert r.get("Occupancy") == by_lds, (name, r, by_lds)
        assert r["Occupancy"] >= parent[form][1]["Occupancy"], (name, r, parent[form])


def test_benchmark_form_holds_three_workgroups_per_cu(kernels):
    groups, _ = kernels
    for p2 in "01":
        name, r = groups[("2", p2, "32")]
        assert r.get("Occupancy") == 3, (name, r)
