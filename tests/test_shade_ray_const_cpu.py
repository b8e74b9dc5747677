"""The per-ray constant of the ray-uniform network kernels, without a GPU: the three C entries are
declared and exported and answer null pointers and negative counts before any HIP work; every
instantiation of the kernels that load the constant (shade_fwd_mfma_rays_kernel_const,
shade_bwd_mfma_rays_kernel_const) compiles, with the project's own HIP flags, without scratch or
spills, within the registers of its form -- forward 128 at four waves per SIMD, backward 256 at two
waves per SIMD and 512 at one -- and in no more registers than the kernel of the same template
arguments that forms the constant itself.  Cross-compiled for gfx950; needs hipcc, not a GPU."""
import ctypes
import re

import pytest

from tests.test_dense_lean_cpu import FAKE, INVALID, OK, UNSUPPORTED, _no_scratch, _resource_usage

WIDTHS = ("8", "16", "32", "64")
ENTRIES = ("f2n_shade_ray_const", "f2n_shade_fwd_rays_const", "f2n_shade_bwd_rays_const")


def test_entries_are_declared_and_exported(capi):
    decls = capi.parse_header()
    assert set(ENTRIES) <= set(decls)
    cdll = ctypes.CDLL(capi.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(cdll, name), name
    # (ray_dirs, w1, b1, ray_const, n_rays, stream)
    assert [n for _, n in decls[ENTRIES[0]][1]] == ["ray_dirs", "w1", "b1", "ray_const", "n_rays", "stream"]
    # the forward takes the buffer where f2n_shade_fwd_raydirs takes the directions; the backward both
    fwd = [n for _, n in decls[ENTRIES[1]][1]]
    bwd = [n for _, n in decls[ENTRIES[2]][1]]
    assert fwd == ["ray_const" if n == "ray_dirs" else n for _, n in decls["f2n_shade_fwd_raydirs"][1]]
    twin = [n for _, n in decls["f2n_shade_bwd_raydirs"][1]]
    assert bwd == twin[:3] + ["ray_const"] + twin[3:]
    text = open(capi.HEADER).read()
    assert re.search(r"#define\s+F2N_SHADE_RAY_CONST_FLOATS\s+80\b", text)


def test_entries_validate_before_any_hip_work(capi):
    """Every call here has a fault or no rays: nothing is launched."""
    c = capi.lib().cdll
    good = [FAKE, FAKE, FAKE, FAKE, 4, None]
    for faults in ({4: -1}, {0: None}, {1: None}, {2: None}, {3: None}, {3: FAKE + 4}):
        args = list(good)
        for i, bad in faults.items():
            args[i] = bad
        assert c.f2n_shade_ray_const(*args) == INVALID, faults
    assert c.f2n_shade_ray_const(None, None, None, None, 0, None) == OK
    # (enc_cm, C, ray_const, ray_img, w_h, b_h, w1, b1, w2, b2, app_emb, logit, rgb, n_rays, S, stream)
    fwd_good = [FAKE, 32, FAKE, None] + [FAKE] * 6 + [None, FAKE, FAKE, 4, 64, None]
    # (enc_cm, C, ray_dirs, ray_const, ray_img, w_h .. b2, app_emb, d_logit, d_rgb, d_enc_cm, g_w_h ..
    #  g_b2, g_app_emb, n_rays, S, stream)
    bwd_good = [FAKE, 32, FAKE, FAKE, None] + [FAKE] * 6 + [None] + [FAKE] * 9 + [None, 4, 64, None]
    cases = ((c.f2n_shade_fwd_rays_const, fwd_good, 13,
              ({13: -1}, {14: 96}, {14: 0}, {0: None}, {2: None}, {4: None}, {11: None}, {12: None},
               {2: FAKE + 4})),
             (c.f2n_shade_bwd_rays_const, bwd_good, 22,
              ({22: -1}, {23: 96}, {23: 0}, {0: None}, {2: None}, {3: None}, {5: None}, {12: None},
               {14: None}, {15: None}, {3: FAKE + 4}, {4: FAKE, 11: FAKE})))   # (an embedding without its gradient)
    for fn, good_args, n_at, faults_list in cases:
        for faults in faults_list:
            args = list(good_args)
            for i, bad in faults.items():
                args[i] = bad
            assert fn(*args) == INVALID, faults
        args = list(good_args)
        args[1] = 24                                       # no matrix-core tiling for this width
        assert fn(*args) == UNSUPPORTED
        args = list(good_args)
        args[n_at] = 0                                     # no rays: nothing to do
        assert fn(*args) == OK
        args = list(good_args)
        args[n_at], args[n_at + 1] = 1 << 20, 1 << 10      # 2^30 samples: beyond the 32-bit offsets
        assert fn(*args) == UNSUPPORTED


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return _resource_usage(tmp_path_factory.mktemp("shade_ray_const"), "shade_mfma.hip")


def _regs(r):
    return r.get("VGPRs", 0) + r.get("AGPRs", 0)


def _by_args(kernels, marker, pattern):
    return {re.search(pattern, n).groups(): (n, r) for n, r in kernels.items() if marker in n}


def test_forward_fits_four_waves_per_simd(kernels):
    # <C, WIDE, W>: W = 16 the production form, 12 the one with 64-bit row offsets, 8 and 12 the
    # measurement forms of F2N_OPT_SHADE_VARIANT
    pat = r"kernel_constILi(\d+)ELb(\d)ELi(\d+)EE"
    new = _by_args(kernels, "shade_fwd_mfma_rays_kernel_constI", pat)
    old = _by_args(kernels, "shade_fwd_mfma_rays_kernelI", r"kernelILi(\d+)ELb(\d)ELi(\d+)EE")
    assert set(new) == set(old) and {k for k in new if k[2] == "16"} == {(c, "0", "16") for c in WIDTHS}
    for args, (name, r) in new.items():
        _no_scratch(name, r)
        assert r.get("LDS Size") <= 163840, (name, r)
        if args[2] == "16":
            assert _regs(r) <= 128 and r.get("Occupancy") >= 4, (name, r)
        assert r.get("Occupancy") >= old[args][1].get("Occupancy"), (name, r, old[args][1])
        assert _regs(r) <= _regs(old[args][1]), (name, r, old[args][1])


def test_backward_fits_both_forms(kernels):
    # <C, V, WIDE, TS>: the instantiations of the forming kernel, one for one (C = 64 with 64-bit row
    # offsets has no two-wave form there either)
    pat = r"kernel_constILi(\d+)ELi(\d)ELb(\d)ELi(\d)EE"
    new = _by_args(kernels, "shade_bwd_mfma_rays_kernel_constI", pat)
    old = _by_args(kernels, "shade_bwd_mfma_rays_kernelI", r"kernelILi(\d+)ELi(\d)ELb(\d)ELi(\d)EE")
    assert new and set(new) == set(old), (sorted(new), sorted(old))
    for args, (name, r) in new.items():
        _no_scratch(name, r)
        assert r.get("LDS Size") <= 163840, (name, r)
        if args[3] == "2":
            assert _regs(r) <= 256 and r.get("Occupancy") == 2, (name, r)
        else:
            assert _regs(r) <= 512 and r.get("Occupancy") == 1, (name, r)
        assert _regs(r) <= _regs(old[args][1]), (name, r, old[args][1])


def test_constant_kernel_is_small(kernels):
    k = [(n, r) for n, r in kernels.items() if "shade_ray_const_kernel" in n]
    assert len(k) == 1, sorted(kernels)
    name, r = k[0]
    _no_scratch(name, r)
    assert r.get("LDS Size") == 0 and _regs(r) <= 64, (name, r)
