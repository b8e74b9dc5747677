"""Argument validation of the camera-visibility entries (f2n_occ_mark_rays, f2n_occ_dilate,
f2n_occ_count_add, f2n_occ_count_bits): every call here has a fault or no work, so nothing is launched
and no GPU is needed."""
INVALID, OK = -1, 0
FAKE, OTHER = 0x1000, 0x2000
NAN, INF = float("nan"), float("inf")
BAD_G = (0, -32, 16, 31, 48, 100, 512, 1 << 20)


def _sweep(fn, good, cases):
    for faults, want in cases:
        args = list(good)
        for i, bad in faults.items():
            args[i] = bad
        assert fn(*args) == want, faults


def test_header_declares_the_entries(capi):
    decls = capi.parse_header()
    assert [n for _, n in decls["f2n_occ_mark_rays"][1]] == [
        "poses", "pose_ld", "intrinsics", "dist", "cam_first", "n_cams", "h", "w", "pixel_stride",
        "mask_bits", "n_steps", "step", "bits", "G", "stream"]
    assert [n for _, n in decls["f2n_occ_dilate"][1]] == ["in", "out", "G", "stream"]
    assert [n for _, n in decls["f2n_occ_count_add"][1]] == ["bits", "count", "G", "stream"]
    assert [n for _, n in decls["f2n_occ_count_bits"][1]] == ["count", "min_count", "bits", "G", "stream"]


def test_mark_rays_validates_before_any_hip_work(capi):
    fn = capi.lib().cdll.f2n_occ_mark_rays
    # (poses, pose_ld, intrinsics, dist, cam_first, n_cams, h, w, pixel_stride, mask_bits, n_steps,
    #  step, bits, G, stream); n_cams = 0: a call that passes validation launches nothing
    good = [FAKE, 12, FAKE, FAKE, 0, 0, 12, 20, 1, FAKE, 96, 1.0 / 32, FAKE, 32, None]
    assert fn(*good) == OK
    _sweep(fn, good, (
        ({0: None}, INVALID), ({2: None}, INVALID), ({12: None}, INVALID),       # null tables, null bits
        ({1: 0}, INVALID), ({1: 9}, INVALID), ({1: 15}, INVALID), ({1: 24}, INVALID),
        ({6: 0}, INVALID), ({6: -3}, INVALID), ({7: 0}, INVALID), ({7: -1}, INVALID),
        ({8: 0}, INVALID), ({8: -2}, INVALID),
        ({10: 0}, INVALID), ({10: -1}, INVALID), ({10: 65537}, INVALID), ({10: 1 << 30}, INVALID),
        ({4: -1}, INVALID), ({5: -1}, INVALID),
        ({11: 0.0}, INVALID), ({11: -0.01}, INVALID), ({11: NAN}, INVALID), ({11: INF}, INVALID),
        ({11: -INF}, INVALID),
        # what is optional or at a limit
        ({3: None}, OK), ({9: None}, OK), ({3: None, 9: None}, OK), ({1: 16}, OK),
        ({10: 1}, OK), ({10: 65536}, OK), ({8: 1 << 20}, OK), ({4: 1 << 20}, OK),
        ({6: 1, 7: 1}, OK), ({11: 1e-30}, OK), ({11: 1e30}, OK),
        ({13: 64}, OK), ({13: 128}, OK), ({13: 256}, OK))
        + tuple(({13: g}, INVALID) for g in BAD_G))


def test_dilate_validates_before_any_hip_work(capi):
    fn = capi.lib().cdll.f2n_occ_dilate
    # (in, out, G, stream): there is no empty call, so only faults are tried
    good = [FAKE, OTHER, 32, None]
    _sweep(fn, good, (
        ({0: None}, INVALID), ({1: None}, INVALID), ({0: None, 1: None}, INVALID),
        ({1: FAKE}, INVALID), ({0: OTHER}, INVALID))                             # in == out
        + tuple(({2: g}, INVALID) for g in BAD_G))


def test_count_entries_validate_before_any_hip_work(capi):
    add = capi.lib().cdll.f2n_occ_count_add
    # (bits, count, G, stream)
    _sweep(add, [FAKE, OTHER, 32, None], (
        ({0: None}, INVALID), ({1: None}, INVALID)) + tuple(({2: g}, INVALID) for g in BAD_G))
    to_bits = capi.lib().cdll.f2n_occ_count_bits
    # (count, min_count, bits, G, stream)
    _sweep(to_bits, [FAKE, 1, OTHER, 32, None], (
        ({0: None}, INVALID), ({2: None}, INVALID)) + tuple(({3: g}, INVALID) for g in BAD_G))
