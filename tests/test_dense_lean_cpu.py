"""The lean dense first pass without a GPU: the new sampler kernel (sample_dense_kernel) compiles, with
the project's own HIP flags, without scratch or spills and at no lower occupancy than the kernel it
replaces; the per-ray direction row of the ray-uniform network kernels is a scalar argument -- no
instantiation was added and every one still compiles clean at the occupancy of its form (the register
and occupancy bars themselves stay in tests/test_shade_rays_occupancy_cpu.py); the new C entries
answer null or negative arguments as their siblings do; the option is a 0 / 1 switch.
Cross-compiled for gfx950; needs hipcc, not a GPU."""
import importlib
import os
import re
import shutil
import subprocess

import pytest

build = importlib.import_module("f2-nerf_amd._build")
INVALID, UNSUPPORTED, OK = -1, -3, 0
FAKE = 0x1000          # a non-null pointer for calls that are rejected, or have no rays, before a launch


def _resource_usage(tmp, name):
    if not os.path.exists(build.HIPCC) and shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: the build needs it too")
    src = os.path.join(build.KERNEL_DIR, name)
    flags = [f for f in build.HIP_FLAGS if f not in build.HIP_FLAGS_DROP.get(name, ())]
    cmd = [build.HIPCC, *flags, "-I", build.INCLUDE_DIR, "-I", build.KERNEL_DIR, "--offload-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp / (name + ".o"))]
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


def _no_scratch(name, r):
    assert r.get("ScratchSize") == 0, (name, r)
    assert r.get("VGPRs Spill") == 0 and r.get("AGPRs Spill", 0) == 0, (name, r)


def test_sampler_kernel_compiles_clean(tmp_path):
    k = _resource_usage(tmp_path, "sampler.hip")
    dense = [(n, r) for n, r in k.items() if "sample_dense_kernel" in n]
    old = [(n, r) for n, r in k.items() if "sample_rays_kernel" in n]
    assert len(dense) == 1 and len(old) == 1, sorted(k)
    (name, r), (_, r_old) = dense[0], old[0]
    _no_scratch(name, r)
    assert r.get("LDS Size") == 0, (name, r)
    assert r.get("Occupancy") >= r_old.get("Occupancy"), (r, r_old)


def test_network_kernels_take_the_direction_row_as_an_argument(tmp_path):
    k = _resource_usage(tmp_path, "shade_mfma.hip")
    fwd_re, bwd_re = r"kernelILi(\d+)ELb(\d)ELi(\d+)EE", r"kernelILi(\d+)ELi(\d)ELb(\d)ELi(\d)EE"

    def by_args(marker, pattern):
        return {re.search(pattern, n).groups(): (n, r) for n, r in k.items() if marker in n}

    rays_fwd, twin_fwd = by_args("shade_fwd_mfma_rays_kernelI", fwd_re), by_args("shade_fwd_mfma_kernelI", fwd_re)
    rays_bwd, twin_bwd = by_args("shade_bwd_mfma_rays_kernelI", bwd_re), by_args("shade_bwd_mfma_kernelI", bwd_re)
    # no kernel of its own for the per-ray row, and no instantiation the per-sample kernels lack
    assert rays_fwd and rays_bwd and not [n for n in k if "raydirs" in n]
    for rays, twins in ((rays_fwd, twin_fwd), (rays_bwd, twin_bwd)):
        for args, (n, r) in rays.items():
            _no_scratch(n, r)
            # the occupancy of the per-sample-dirs kernel of the same template arguments
            assert args in twins, (n, sorted(twins))
            assert r.get("Occupancy") >= twins[args][1].get("Occupancy"), (n, r, twins[args][1])


def test_new_entries_validate_arguments_like_their_siblings(capi):
    """Every call here has a fault or no rays: nothing is launched."""
    c = capi.lib().cdll
    # f2n_sample_dense(rays_o, rays_d, noise, noise_row, noise_affine, x, dt, t, bounds, ray_dirs,
    #                  n_rays, S, step, stream) beside f2n_sample_rays
    good = [FAKE, FAKE, None, None, 0, FAKE, FAKE, FAKE, FAKE, FAKE, 4, 128, 1.0 / 32, None]
    assert c.f2n_sample_rays(None, None, None, None, None, None, None, None, -1, 8, 0.1, None) == INVALID
    for faults in ({10: -1}, {11: 0}, {4: 2}, {4: -1}, {0: None}, {1: None}, {5: None}, {6: None},
                   {7: None}, {8: None}, {9: None}, {10: 1 << 24, 11: 1 << 10}):
        args = list(good)
        for i, bad in faults.items():
            args[i] = bad
        assert c.f2n_sample_dense(*args) == INVALID, faults
    for empty in ({10: 0}, {10: 0, 0: None, 5: None}):
        args = list(good)
        for i, bad in empty.items():
            args[i] = bad
        assert c.f2n_sample_dense(*args) == OK, empty
        assert c.f2n_sample_rays(None, None, None, None, None, None, None, None, 0, 8, 0.1, None) == OK

    # f2n_shade_fwd_raydirs / f2n_shade_bwd_raydirs beside f2n_shade_fwd_rays / f2n_shade_bwd_rays
    fwd_good = [FAKE, 32, FAKE, None] + [FAKE] * 6 + [None, FAKE, FAKE, 4, 64, None]
    bwd_good = [FAKE, 32, FAKE, None] + [FAKE] * 6 + [None] + [FAKE] * 9 + [None, 4, 64, None]
    cases = (({13: -1}, {14: 96}, {14: 0}, {0: None}, {2: None}, {4: None}, {11: None}, {12: None}),
             ({21: -1}, {22: 96}, {22: 0}, {0: None}, {2: None}, {4: None}, {11: None}, {13: None},
              {14: None}, {3: FAKE, 10: FAKE}))          # (an embedding without its gradient)
    for (lean, sibling), good_args, faults_list, c_at, n_at in (
            ((c.f2n_shade_fwd_raydirs, c.f2n_shade_fwd_rays), fwd_good, cases[0], 1, 13),
            ((c.f2n_shade_bwd_raydirs, c.f2n_shade_bwd_rays), bwd_good, cases[1], 1, 21)):
        for faults in faults_list:
            args = list(good_args)
            for i, bad in faults.items():
                args[i] = bad
            assert lean(*args) == sibling(*args) == INVALID, faults
        args = list(good_args)
        args[c_at] = 24                                    # no matrix-core tiling for this width
        assert lean(*args) == sibling(*args) == UNSUPPORTED
        args = list(good_args)
        args[n_at] = 0                                     # no rays: nothing to do
        assert lean(*args) == sibling(*args) == OK
        args = list(good_args)
        args[n_at], args[n_at + 1] = 1 << 20, 1 << 10      # 2^30 samples: beyond the 32-bit offsets
        assert lean(*args) == sibling(*args) == UNSUPPORTED


def test_dense_lean_option_is_a_switch(capi):
    keys = capi.option_keys()
    assert keys["DENSE_LEAN"] == 12 and max(keys.values()) == 12
    c = capi.lib().cdll
    assert c.f2n_get_option(12) == 0                       # the lean route is the default
    with capi.option("DENSE_LEAN", 1):
        assert c.f2n_get_option(12) == 1
    assert c.f2n_get_option(12) == 0
    assert c.f2n_set_option(12, 2) == INVALID and c.f2n_set_option(13, 0) == INVALID
