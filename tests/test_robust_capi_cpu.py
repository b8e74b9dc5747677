"""Argument validation of f2n_robust_weights and its size query: every call here has a fault, so
nothing is launched and no GPU is needed."""
import math

INVALID = -1
FAKE = 0x1000


def _sweep(fn, good, cases):
    for faults in cases:
        args = list(good)
        for i, bad in faults.items():
            args[i] = bad
        assert fn(*args) == INVALID, faults


def test_workspace_query(capi):
    ws = capi.lib().cdll.f2n_robust_workspace_words
    for n in (1, 9, 256, 4096, 65536, (1 << 24) - 1):
        assert ws(n) >= 8 + n + 2 * (n // 9)             # header, a word per ray, two per 3 x 3 patch
        assert capi.robust_workspace_words(n) == ws(n)
    for bad in (0, -1, 1 << 24, (1 << 24) + 1, 2 ** 31 - 1, -2 ** 31):
        assert ws(bad) == 0


def test_robust_weights_validates_before_any_hip_work(capi):
    fn = capi.lib().cdll.f2n_robust_weights
    # (colors, target, ray_weight, n_rays, P, nbhd, quantile, box_thresh, nbhd_thresh, weight_out,
    #  omega_out, stats4, workspace, stream): a call with one fault never reaches a launch, so the
    #  fake pointers are never dereferenced
    nan = math.nan
    for good in ([FAKE, FAKE, FAKE, 512, 16, 8, 0.5, 0.5, 0.6, FAKE, FAKE, FAKE, FAKE, None],
                 [FAKE, FAKE, None, 100, 0, 8, 1.0, 0.0, 1.0, FAKE, None, FAKE, FAKE, None]):
        _sweep(fn, good, (
            {0: None}, {1: None}, {9: None}, {11: None}, {12: None},
            {3: 0}, {3: -1}, {3: 1 << 24}, {3: 2 ** 31 - 1},
            {6: 0.0}, {6: -0.5}, {6: 1.0000001}, {6: 2.0}, {6: nan}, {6: math.inf},
            {7: -1e-6}, {7: 1.0000001}, {7: nan}, {8: -1e-6}, {8: 1.0000001}, {8: nan},
            {4: -1}, {4: 1}, {4: 2}, {4: 65}, {4: 1 << 16}))
    patches = [FAKE, FAKE, FAKE, 512, 16, 8, 0.5, 0.5, 0.6, FAKE, FAKE, FAKE, FAKE, None]
    _sweep(fn, patches, (
        {3: 511}, {3: 513}, {3: 255}, {4: 3}, {4: 11}, {4: 64},      # n_rays % P^2 != 0
        {5: 0}, {5: -1}, {5: 17}, {5: 1 << 20},                      # nbhd outside 1 .. P
        {3: 9, 4: 3, 5: 4}, {3: 4096, 4: 64, 5: 65}))
