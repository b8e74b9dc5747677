"""Argument validation of the learned background's entries (f2n_envmap_fwd, f2n_envmap_bwd,
f2n_envmap_grad_apply) and their size query: every call here has a fault or no work, so nothing is
launched and no GPU is needed."""
import re

INVALID, OK = -1, 0
FAKE = 0x1000


def _sweep(fn, good, cases):
    for faults, want in cases:
        args = list(good)
        for i, bad in faults.items():
            args[i] = bad
        assert fn(*args) == want, faults


def test_texels_and_shift(capi):
    c = capi.lib().cdll
    assert c.f2n_envmap_texels(2) == 24 and c.f2n_envmap_texels(5) == 150
    assert c.f2n_envmap_texels(128) == 6 * 128 * 128 and c.f2n_envmap_texels(4096) == 6 * 4096 * 4096
    for bad in (1, 0, -1, -4096, 4097, (1 << 31) - 1, -(1 << 31)):
        assert c.f2n_envmap_texels(bad) == 0
    # the fixed-point shift is a constant of the header, and the model's
    from tests import envmap_model as em

    text = open(capi.HEADER).read()
    assert int(re.search(r"#define\s+F2N_ENVMAP_SHIFT\s+(\d+)", text).group(1)) == em.SHIFT == 48


def test_envmap_fwd_validates_before_any_hip_work(capi):
    fn = capi.lib().cdll.f2n_envmap_fwd
    # (dirs, tex, R, bg, n_rays, stream)
    good = [FAKE, FAKE, 8, FAKE, 0, None]
    assert fn(*good) == OK                                   # no rays: nothing launched
    _sweep(fn, good, (
        ({2: 2}, OK), ({2: 4096}, OK),
        # no rays does not excuse a bad argument
        ({0: None}, INVALID), ({1: None}, INVALID), ({3: None}, INVALID),
        ({2: 1}, INVALID), ({2: 0}, INVALID), ({2: -8}, INVALID), ({2: 4097}, INVALID),
        ({4: -1}, INVALID), ({4: -(1 << 31)}, INVALID),
        # ... and a fault is answered before the launch whatever the ray count
        ({4: 64, 0: None}, INVALID), ({4: 64, 1: None}, INVALID), ({4: 64, 3: None}, INVALID),
        ({4: 64, 2: 1}, INVALID), ({4: 64, 2: 4097}, INVALID)))


def test_envmap_bwd_validates_before_any_hip_work(capi):
    fn = capi.lib().cdll.f2n_envmap_bwd
    # (dirs, bg, d_bg, R, acc, flags, n_rays, stream)
    good = [FAKE, FAKE, FAKE, 8, FAKE, FAKE, 0, None]
    assert fn(*good) == OK
    _sweep(fn, good, (
        ({3: 2}, OK), ({3: 4096}, OK),
        ({0: None}, INVALID), ({1: None}, INVALID), ({2: None}, INVALID), ({4: None}, INVALID),
        ({5: None}, INVALID), ({3: 1}, INVALID), ({3: 0}, INVALID), ({3: -2}, INVALID),
        ({3: 4097}, INVALID), ({6: -1}, INVALID),
        ({6: 64, 0: None}, INVALID), ({6: 64, 1: None}, INVALID), ({6: 64, 2: None}, INVALID),
        ({6: 64, 4: None}, INVALID), ({6: 64, 5: None}, INVALID), ({6: 64, 3: 1}, INVALID),
        ({6: 64, 3: 4097}, INVALID)))


def test_envmap_grad_apply_validates_before_any_hip_work(capi):
    fn = capi.lib().cdll.f2n_envmap_grad_apply
    # (acc, R, d_tex, accumulate, stream): there is no count that could be zero, so every call
    # here carries a fault
    good = [FAKE, 8, FAKE, 0, None]
    _sweep(fn, good, (
        ({0: None}, INVALID), ({2: None}, INVALID), ({1: 1}, INVALID), ({1: 0}, INVALID),
        ({1: -8}, INVALID), ({1: 4097}, INVALID), ({3: 2}, INVALID), ({3: -1}, INVALID),
        ({3: 1, 0: None}, INVALID), ({3: 1, 1: 4097}, INVALID)))
