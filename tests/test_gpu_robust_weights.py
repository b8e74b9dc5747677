"""f2n_robust_weights (robust_mask.hip) against tests/robust_model.py: labels, weights, counts and the
bits of T, all with array_equal -- the rule is integers after a float32 residual whose order is fixed,
so there is no tolerance.  Shapes: the smallest at which each part can go wrong -- the wave edge (63,
64, 65), the stride of the selecting workgroup (1023, 1025, 2049), patches of 3 (the smallest), 11 and
13 (odd, edge blocks of 3 and 5), 16 (one workgroup pass) and 64 (the largest: 16 pixels per lane)."""
import importlib

import numpy as np
import pytest
import torch

from tests import robust_model as M

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def _data(n, seed, distinct=None):
    g = np.random.default_rng(seed)
    colors, target = g.random((n, 3), dtype=F32), g.random((n, 3), dtype=F32)
    if distinct is not None:                     # residuals drawn from `distinct` values only
        target[:] = 0
        colors[:] = 0
        colors[:, 0] = g.choice(np.array([0.125, 0.25, 0.5, 0.75], dtype=F32)[:distinct], size=n)
    return colors, target


def _run(capi, dev, colors, target, m=None, **kw):
    w, o, s = capi.robust_weights(torch.from_numpy(colors).to(dev), torch.from_numpy(target).to(dev),
                                  None if m is None else torch.from_numpy(m).to(dev), **kw)
    torch.cuda.synchronize()
    return w.cpu().numpy(), o.cpu().numpy(), s.cpu().numpy()


def _check(capi, dev, colors, target, m=None, **kw):
    want = M.robust_weights(colors, target, m, **kw)
    w, o, s = _run(capi, dev, colors, target, m, **kw)
    assert np.array_equal(o, want["omega"]), kw
    assert np.array_equal(w.view(np.uint32), want["weight"].view(np.uint32)), kw
    assert np.array_equal(s.view(np.uint32), want["stats"].view(np.uint32)), (kw, s, want["stats"])
    return want


@pytest.mark.parametrize("n", (1, 63, 64, 65, 1023, 1025, 2049))
def test_scattered_rays(capi, dev, n):
    colors, target = _data(n, n)
    for q in (0.5, 0.3, 1.0):
        want = _check(capi, dev, colors, target, quantile=q)
        assert want["omega"].sum() == want["k"]          # distinct residuals: exactly k inliers
    m = (np.random.default_rng(n + 1).random(n) > 0.3).astype(F32) * F32(0.5)
    _check(capi, dev, colors, target, m, quantile=0.5)


@pytest.mark.parametrize("shape", ((1, 3), (1, 11), (2, 13), (3, 16), (1, 64)), ids=lambda s: "%dx%d" % s)
def test_patches(capi, dev, shape):
    n_patches, P = shape
    n = n_patches * P * P
    colors, target = _data(n, P)
    # a coherent blob of large residuals in the first patch, and isolated ones
    blob = np.zeros((n_patches, P, P), dtype=bool)
    blob[0, :max(P // 2, 2), :max(P // 2, 2)] = True
    blob[-1, P - 1, P - 1] = True
    colors[blob.reshape(-1)] += 1.0
    seen = set()
    for nbhd in sorted({min(8, P), P, 1}):
        for q in (0.5, 0.8):
            want = _check(capi, dev, colors, target, P=P, nbhd=nbhd, quantile=q)
            seen.add((want["W"] & ~want["w0"]).any())
    if P >= 11:
        assert True in seen                              # the box restored something somewhere
    m = (np.random.default_rng(P + 1).random(n) > 0.2).astype(F32)
    _check(capi, dev, colors, target, m, P=P, nbhd=min(8, P), quantile=0.6, box_thresh=0.7,
           nbhd_thresh=0.9)
    _check(capi, dev, colors, target, m, P=P, nbhd=min(8, P), quantile=0.2, box_thresh=0.0,
           nbhd_thresh=1.0)
    _check(capi, dev, colors, target, m, P=P, nbhd=min(8, P), quantile=0.2, box_thresh=1.0,
           nbhd_thresh=0.0)


def test_ties_and_equal_residuals(capi, dev):
    for n, P in ((1025, 0), (2 * 169, 13)):
        colors, target = _data(n, 7, distinct=4)
        for q in (0.1, 0.26, 0.5, 0.74, 0.99):
            want = _check(capi, dev, colors, target, P=P, nbhd=min(8, max(P, 1)), quantile=q)
            assert want["w0"].sum() > want["k"]          # the ties at T came along
        colors, target = _data(n, 8, distinct=1)         # every residual equal
        for q in (0.01, 0.5, 1.0):
            want = _check(capi, dev, colors, target, P=P, nbhd=min(8, max(P, 1)), quantile=q)
            assert want["omega"].all() and want["T"] == F32(0.125) * F32(0.125)


def test_rank_at_both_ends(capi, dev):
    colors, target = _data(1025, 9)
    lo = _check(capi, dev, colors, target, quantile=1e-6)
    hi = _check(capi, dev, colors, target, quantile=1.0)
    almost = _check(capi, dev, colors, target, quantile=0.9999)
    assert lo["k"] == 1 and lo["omega"].sum() == 1 and lo["T"] == lo["eps"].min()
    assert hi["k"] == 1025 and hi["omega"].all() and almost["k"] == 1025


def test_ray_weights(capi, dev):
    n_patches, P = 3, 16
    n = n_patches * P * P
    colors, target = _data(n, 10)
    g = np.random.default_rng(11)
    scattered = np.where(g.random(n) > 0.25, g.random(n, dtype=F32) + F32(0.5), F32(0)).astype(F32)
    one_patch = np.ones(n, dtype=F32)
    one_patch[P * P:2 * P * P] = 0
    negzero = scattered.copy()
    negzero[::7] = F32(-0.0)                                 # -0 == 0: not considered, weight +0
    for m in (scattered, one_patch, negzero, np.zeros(n, dtype=F32)):
        for kw in (dict(P=P, nbhd=8), dict(P=0)):
            want = _check(capi, dev, colors, target, m, quantile=0.5, **kw)
            assert not want["omega"][m == 0].any() and want["stats"][1] == (m != 0).sum()
    zero = _check(capi, dev, colors, target, np.zeros(n, dtype=F32), P=P, nbhd=8)
    assert not zero["stats"].any() and not zero["weight"].view(np.uint32).any()


def test_non_finite_colours(capi, dev):
    n_patches, P = 2, 11
    n = n_patches * P * P
    colors, target = _data(n, 12)
    colors[3] = np.nan
    colors[40, 1] = np.inf
    colors[100] = (3e19, 3e19, 0)                            # the residual overflows
    target[101, 2] = -np.inf
    for kw in (dict(P=P, nbhd=8), dict(P=0)):
        for q in (0.5, 1.0):
            want = _check(capi, dev, colors, target, quantile=q, **kw)
            assert not want["w0"][[3, 40, 100, 101]].any()
        assert np.isinf(want["T"]) and want["stats"][2] == n - 4
    # on rays with m = 0 the colours are not read: the outputs stay finite and equal to the clean run
    m = np.ones(n, dtype=F32)
    m[[3, 40, 100, 101]] = 0
    clean = colors.copy()
    clean[[3, 40, 100, 101]] = 0
    clean_target = target.copy()
    clean_target[101] = 0
    for kw in (dict(P=P, nbhd=8), dict(P=0)):
        a = _run(capi, dev, colors, target, m, quantile=0.5, **kw)
        b = _run(capi, dev, clean, clean_target, m, quantile=0.5, **kw)
        assert all(np.array_equal(x, y) and np.isfinite(x).all() for x, y in zip(a, b))
        _check(capi, dev, colors, target, m, quantile=0.5, **kw)


def test_two_runs_give_the_same_bits(capi, dev):
    colors, target = _data(3 * 256, 13, distinct=4)
    for kw in (dict(P=16, nbhd=8), dict(P=0)):
        a = _run(capi, dev, colors, target, quantile=0.5, **kw)
        b = _run(capi, dev, colors, target, quantile=0.5, **kw)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_host_entry_and_graph_capture(host, dev):
    """host.robust_weights equals the model, and one capture of it on a side stream -- a single chain
    of launches, no parallel branches -- replayed twice on inputs changed in place equals the eager
    bits: nothing in it is read on the host"""
    n_patches, P = 2, 16
    n = n_patches * P * P
    opt = host.RobustLoss(quantile=0.5, patch=P)
    sets = [_data(n, 20 + i) for i in range(3)]
    ms = [(np.random.default_rng(30 + i).random(n) > 0.2).astype(F32) for i in range(3)]
    colors, target, m = (torch.from_numpy(x).to(dev) for x in (sets[0][0], sets[0][1], ms[0]))
    eager = []
    for (c, t), mm in zip(sets, ms):
        w, o, s = host.robust_weights(torch.from_numpy(c).to(dev), torch.from_numpy(t).to(dev), opt,
                                      torch.from_numpy(mm).to(dev))
        want = M.robust_weights(c, t, mm, P=P, nbhd=8, quantile=0.5)
        assert np.array_equal(o.cpu().numpy(), want["omega"])
        assert np.array_equal(w.cpu().numpy(), want["weight"])
        assert np.array_equal(s.cpu().numpy(), want["stats"])
        eager.append((w.clone(), o.clone(), s.clone()))
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        out = host.robust_weights(colors, target, opt, m)
    for i in (1, 2):
        colors.copy_(torch.from_numpy(sets[i][0]))
        target.copy_(torch.from_numpy(sets[i][1]))
        m.copy_(torch.from_numpy(ms[i]))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, eager[i]))
    # off-patch options: a quantile of 1 or more keeps every considered ray
    w, o, s = host.robust_weights(colors, target, host.RobustLoss(), m)
    assert torch.equal(w, m) and float(s[1]) == float(m.sum())
