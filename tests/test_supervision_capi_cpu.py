"""Argument validation of masked training's entries (f2n_mask_pack, f2n_draw_pixels_masked,
f2n_loss_sup_fwd) and their size queries: every call here has a fault or no work, so nothing is
launched and no GPU is needed."""
INVALID, OK = -1, 0
FAKE = 0x1000


def _sweep(fn, good, cases):
    for faults, want in cases:
        args = list(good)
        for i, bad in faults.items():
            args[i] = bad
        assert fn(*args) == want, faults


def test_mask_sizes(capi):
    c = capi.lib().cdll
    assert c.f2n_mask_words(3, 5, 70) == 33 and c.f2n_mask_pack_workspace_words(3, 5, 70) == 5
    assert c.f2n_mask_words(1, 1, 32) == 1 and c.f2n_mask_words(1, 1, 33) == 2
    assert c.f2n_mask_words(200, 1080, 1920) == 200 * 1080 * 1920 // 32      # 52 MB of bits
    # one partial per workgroup of 256 pixels, 2^20 workgroups at the most
    assert c.f2n_mask_pack_workspace_words(1, 1 << 14, 1 << 14) == 1 << 20
    assert c.f2n_mask_pack_workspace_words(1, 1 << 14, (1 << 14) - 1) == (1 << 20) - 64
    assert c.f2n_mask_pack_workspace_words(200, 1080, 1920) == 1 << 20
    assert c.f2n_mask_words(1 << 10, 1 << 13, 1 << 13) == 0                  # 2^36 pixels: too many
    assert c.f2n_mask_words((1 << 10) - 1, 1 << 13, 1 << 13) == ((1 << 36) - (1 << 26)) // 32
    assert c.f2n_mask_words((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1) == 0  # no overflow on the way
    for bad in ((0, 5, 70), (3, 0, 70), (3, 5, 0), (-1, 5, 70), (3, -5, 70), (3, 5, -70)):
        assert c.f2n_mask_words(*bad) == 0 and c.f2n_mask_pack_workspace_words(*bad) == 0


def test_mask_pack_validates_before_any_hip_work(capi):
    fn = capi.lib().cdll.f2n_mask_pack
    # (mask, E, h, w, words, count, partial, stream)
    good = [FAKE, 3, 5, 70, FAKE, FAKE, FAKE, None]
    _sweep(fn, good, (
        ({0: None}, INVALID), ({4: None}, INVALID), ({5: None}, INVALID), ({6: None}, INVALID),
        ({1: 0}, INVALID), ({2: 0}, INVALID), ({3: 0}, INVALID), ({1: -3}, INVALID),
        ({2: -5}, INVALID), ({3: -70}, INVALID),
        ({1: 1 << 10, 2: 1 << 13, 3: 1 << 13}, INVALID),
        ({1: (1 << 31) - 1, 2: (1 << 31) - 1, 3: (1 << 31) - 1}, INVALID)))


def test_draw_pixels_masked_validates_before_any_hip_work(capi):
    fn = capi.lib().cdll.f2n_draw_pixels_masked
    # (bits, E, h, w, seed_lo, seed_hi, attempts, cam, ij, tries, n, stream)
    good = [FAKE, 3, 5, 70, 1, 2, 32, FAKE, FAKE, FAKE, 16, None]
    _sweep(fn, good, (
        ({0: None}, INVALID), ({7: None}, INVALID), ({8: None}, INVALID), ({9: None}, INVALID),
        ({10: -1}, INVALID), ({1: 0}, INVALID), ({2: 0}, INVALID), ({3: 0}, INVALID),
        ({1: -1}, INVALID), ({1: 1 << 10, 2: 1 << 13, 3: 1 << 13}, INVALID),
        ({6: 0}, INVALID), ({6: -1}, INVALID), ({6: 65}, INVALID),
        ({10: 0}, OK), ({10: 0, 6: 1}, OK), ({10: 0, 6: 64}, OK),
        # no rays does not excuse a bad argument
        ({10: 0, 6: 65}, INVALID), ({10: 0, 0: None}, INVALID), ({10: 0, 2: 0}, INVALID)))


def test_loss_sup_validates_before_any_hip_work(capi):
    c = capi.lib().cdll
    assert c.f2n_loss_sup_workspace_floats(1) == 5 and c.f2n_loss_sup_workspace_floats(256) == 5
    assert c.f2n_loss_sup_workspace_floats(257) == 10 and c.f2n_loss_sup_workspace_floats(0) == 5
    fn = c.f2n_loss_sup_fwd
    # (colors, gt, var, ray_weight, alpha, opacity, bg, n_rays, var_weight, opacity_weight,
    #  d_colors, d_var, d_opacity, partial, out6, stream)
    good = [FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0, 0.3, 0.7, FAKE, FAKE, FAKE, FAKE, FAKE, None]
    # n_rays == 0 is invalid like f2n_loss_fwd's, so every call below answers before a launch
    assert fn(*good) == INVALID
    live = list(good)
    live[7] = 64
    _sweep(fn, live, (
        ({0: None}, INVALID), ({1: None}, INVALID), ({2: None}, INVALID), ({10: None}, INVALID),
        ({11: None}, INVALID), ({13: None}, INVALID), ({14: None}, INVALID), ({7: -4}, INVALID),
        ({6: None}, INVALID),                      # alpha without bg
        ({5: None}, INVALID),                      # alpha and an opacity weight without the opacity
        ({12: None}, INVALID)))                    # alpha and opacity without d_opacity
