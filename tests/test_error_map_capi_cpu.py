"""Argument validation of the error map's entries (f2n_mask_cell_counts, f2n_error_map_accum,
f2n_error_map_apply, f2n_error_cdf, f2n_draw_pixels_guided) and the size query: every call here has
a fault or no work, so nothing is launched and no GPU is needed."""
INVALID, OK = -1, 0
FAKE = 0x1000
NAN = float("nan")
# (E, h, w, gh, gw) faults shared by the entries that take the geometry
GEOMETRY_FAULTS = (
    dict(E=0), dict(E=-1), dict(h=0), dict(w=0), dict(h=-37), dict(gh=0), dict(gw=0), dict(gh=-1),
    dict(gh=38), dict(gw=71),                                   # more cells than pixels
    dict(E=1 << 12, h=64, w=64, gh=64, gw=64),                  # n_cells = 2^24
    dict(E=(1 << 24) - 1, gh=2, gw=1),                          # n_cells just below 2^25
    dict(h=46341, w=46341),                                     # h*w >= 2^31
    dict(h=1 << 16, w=1 << 15),                                 # h*w = 2^31
    dict(E=1 << 10, h=1 << 13, w=1 << 13),                      # E*h*w = 2^36
    dict(E=(1 << 31) - 1, h=(1 << 31) - 1, w=(1 << 31) - 1),    # no overflow on the way
)


def _sweep(fn, good, cases):
    for faults, want in cases:
        args = list(good)
        for i, bad in faults.items():
            args[i] = bad
        assert fn(*args) == want, faults


def _geometry_cases(index):
    """GEOMETRY_FAULTS as _sweep cases; index: position of E, h, w, gh, gw in the argument list"""
    return tuple(({index[k]: v for k, v in f.items()}, INVALID) for f in GEOMETRY_FAULTS)


def test_error_cdf_workspace_words(capi):
    q = capi.lib().cdll.f2n_error_cdf_workspace_words
    assert q(1) == 1 and q(2048) == 1 and q(2049) == 2
    assert q(7 * 37 * 70) == 9 and (7 * 37 * 70) % 2048 != 0     # the GPU tests' second shape
    assert q(200 * 32 * 32) == 100 and q((1 << 24) - 1) == 8192
    assert q(0) == 0 and q(-5) == 0 and q(1 << 24) == 0


def test_mask_cell_counts_validates_before_any_hip_work(capi):
    fn = capi.lib().cdll.f2n_mask_cell_counts
    # (bits, E, h, w, gh, gw, counts, stream)
    good = [FAKE, 3, 37, 70, 5, 8, FAKE, None]
    idx = dict(E=1, h=2, w=3, gh=4, gw=5)
    _sweep(fn, good, (({6: None}, INVALID), ({0: None, 6: None}, INVALID)) + _geometry_cases(idx))


def test_error_map_accum_validates_before_any_hip_work(capi):
    fn = capi.lib().cdll.f2n_error_map_accum
    # (colors, gt, alpha, bg, ray_weight, cam, ij, n, E, h, w, gh, gw, acc_sum, acc_cnt, stream)
    good = [FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 16, 3, 37, 70, 5, 8, FAKE, FAKE, None]
    idx = dict(E=8, h=9, w=10, gh=11, gw=12)
    _sweep(fn, good, (
        ({0: None}, INVALID), ({1: None}, INVALID), ({5: None}, INVALID), ({6: None}, INVALID),
        ({13: None}, INVALID), ({14: None}, INVALID), ({7: -1}, INVALID),
        ({3: None}, INVALID),                                   # alpha without bg
        ({7: 0}, OK), ({7: 0, 2: None, 3: None, 4: None}, OK),
        # no rays does not excuse a bad argument
        ({7: 0, 0: None}, INVALID), ({7: 0, 3: None}, INVALID), ({7: 0, 11: 38}, INVALID),
        ({7: 0, 14: None}, INVALID)) + _geometry_cases(idx))


def test_error_map_apply_validates_before_any_hip_work(capi):
    fn = capi.lib().cdll.f2n_error_map_apply
    # (value, acc_sum, acc_cnt, n_cells, decay, stream)
    good = [FAKE, FAKE, FAKE, 120, 0.5, None]
    _sweep(fn, good, (
        ({0: None}, INVALID), ({1: None}, INVALID), ({2: None}, INVALID), ({3: 0}, INVALID),
        ({3: -1}, INVALID), ({3: 1 << 24}, INVALID), ({4: -0.01}, INVALID), ({4: 1.01}, INVALID),
        ({4: NAN}, INVALID), ({4: float("inf")}, INVALID)))


def test_error_cdf_validates_before_any_hip_work(capi):
    fn = capi.lib().cdll.f2n_error_cdf
    # (value, counts, n_cells, cdf, partial, stream)
    good = [FAKE, FAKE, 120, FAKE, FAKE, None]
    _sweep(fn, good, (
        ({0: None}, INVALID), ({1: None}, INVALID), ({3: None}, INVALID), ({4: None}, INVALID),
        ({2: 0}, INVALID), ({2: -7}, INVALID), ({2: 1 << 24}, INVALID)))


def test_draw_pixels_guided_validates_before_any_hip_work(capi):
    fn = capi.lib().cdll.f2n_draw_pixels_guided
    # (bits, counts, value, cdf, n_valid, E, h, w, gh, gw, seed_lo, seed_hi, attempts,
    #  uniform_fraction, cam, ij, tries, ray_weight, n, stream)
    good = [FAKE, FAKE, FAKE, FAKE, FAKE, 3, 37, 70, 5, 8, 1, 2, 32, 0.25, FAKE, FAKE, FAKE, FAKE, 16,
            None]
    idx = dict(E=5, h=6, w=7, gh=8, gw=9)
    _sweep(fn, good, (
        ({1: None}, INVALID), ({2: None}, INVALID), ({3: None}, INVALID), ({4: None}, INVALID),
        ({14: None}, INVALID), ({15: None}, INVALID), ({16: None}, INVALID), ({17: None}, INVALID),
        ({18: -1}, INVALID), ({12: 0}, INVALID), ({12: -1}, INVALID), ({12: 65}, INVALID),
        ({13: -0.25}, INVALID), ({13: 1.5}, INVALID), ({13: NAN}, INVALID),
        ({18: 0}, OK), ({18: 0, 0: None}, OK),                  # bits are optional
        ({18: 0, 12: 1, 13: 0.0}, OK), ({18: 0, 12: 64, 13: 1.0}, OK),
        # no rays does not excuse a bad argument
        ({18: 0, 12: 65}, INVALID), ({18: 0, 13: NAN}, INVALID), ({18: 0, 3: None}, INVALID),
        ({18: 0, 8: 38}, INVALID)) + _geometry_cases(idx))
