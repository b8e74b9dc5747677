"""The line-of-sight depth losses on the GPU: f2n_depth_sight_fwd / _bwd through the C ABI and the
autograd op host.depth_sight, element by element against the float64 model of
tests/depth_sight_model.py within its bound tol = u (len_r M_sum + K_SIGHT M_op).  The layouts hold rays
of 0, 1, 2, 63, 64, 65, 129 and 200 samples, tiling and with gaps, contiguous and thinned, and for each
length a target in front of every sample, behind every sample, on a sample, on the boundary between
the first two strides, with a sample on the band's edge, and z in {0, negative, NaN, +inf}; each with
eps = 0 and eps = 0.03."""
import importlib

import numpy as np
import pytest
import torch

from tests import depth_sight_model as dm
from tests import ragged_cases as rc

pytestmark = pytest.mark.gpu

CASES = [(name, variant, eps) for name in dm.LAYOUTS for variant in dm.T_VARIANTS
         for eps in dm.EPS_VALUES]


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def _report(lay, case, got, ref, what):
    """print the figures, then assert"""
    for name, (ratio, _) in dm.ratios(lay, case, got, ref).items():
        print("  %s %s: largest (err/u - len M_sum)/M_op = %.3f (K = %g)" % (
            what, name, float(ratio.max()), dm.K_SIGHT))
    rc.assert_no_failures(dm.sight_failures(lay, case, got, ref), what)


def _launch(capi, dev, lay, case, weights=None):
    w = (case["weights"] if weights is None else weights).to(dev)
    t, dt, z, d_out = (case[k].to(dev) for k in ("t", "dt", "z", "d_out"))
    bounds = lay.bounds.to(dev)
    out = torch.full((lay.n_rays, 3), rc.SENTINEL, device=dev)
    dw = torch.full((lay.n_total,), rc.SENTINEL, device=dev)
    capi.call("depth_sight_fwd", w, t, dt, bounds, z, case["eps"], out, lay.n_rays)
    capi.call("depth_sight_bwd", w, t, dt, bounds, z, case["eps"], d_out, dw, lay.n_rays)
    return out, dw


# ---- kernels through the C ABI --------------------------------------------------------------------

@pytest.mark.parametrize("name,variant,eps", CASES)
def test_kernels_per_element(capi, dev, name, variant, eps):
    lay, case, ref = dm.shared(name, variant, eps)
    runs = [_launch(capi, dev, lay, case) for _ in range(2)]
    # two launches: equal bits (NaN-free outputs, so torch.equal compares them all)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    got = dict(out=runs[0][0].cpu().numpy(), dw=runs[0][1].cpu().numpy())
    # sentinels outside the ranges survive, invalid rays hold exact zeros, the rest is within the
    # bound: all in sight_failures.  The corner values, spelled out once more:
    z = case["z"].numpy()
    for r in range(lay.n_rays):
        if lay.kind[r] in dm.INVALID_KINDS:
            assert (got["out"][r] == 0).all()
            assert (got["dw"][int(lay.start[r]):int(lay.end[r])] == 0).all()
        elif lay.len[r] == 0:
            assert got["out"][r, 0] == 0 and got["out"][r, 1] == 1
            assert got["out"][r, 2] == np.float32(z[r]) * np.float32(z[r])
    if name == "gaps":
        assert (got["dw"][~lay.inside] == rc.SENTINEL).all() and (~lay.inside).sum() > rc.WAVE
    _report(lay, case, got, ref, "%s %s eps=%g" % (name, variant, eps))


def test_no_rays_is_ok_and_writes_nothing(capi, dev):
    out = torch.full((6,), rc.SENTINEL, device=dev)
    z = torch.ones(4, device=dev)
    idx = torch.zeros(1, 2, dtype=torch.int32, device=dev)
    capi.call("depth_sight_fwd", z, z, z, idx, z, 0.1, out, 0)
    capi.call("depth_sight_bwd", z, z, z, idx, z, 0.1, z, out, 0)
    assert bool((out == rc.SENTINEL).all())


def test_nan_weight_spoils_only_its_own_ray(capi, dev):
    lay, case, ref = dm.shared("gaps", "thinned", dm.EPS_VALUES[1])
    clean_out, clean_dw = _launch(capi, dev, lay, case)
    r = next(i for i in range(lay.n_rays) if lay.len[i] == 129 and lay.kind[i] == "inside")
    s, e = int(lay.start[r]), int(lay.end[r])
    w = case["weights"].clone()
    w[s + 70] = float("nan")                               # in the second stride
    out, dw = _launch(capi, dev, lay, case, weights=w)
    others = torch.ones(lay.n_rays, dtype=torch.bool)
    others[r] = False
    assert torch.equal(out[others], clean_out[others])
    outside = torch.ones(lay.n_total, dtype=torch.bool)
    outside[s:e] = False
    assert torch.equal(dw[outside], clean_dw[outside])
    # the expected depth sums every sample: NaN, and with it every dw of the ray
    assert bool(torch.isnan(out[r, 2])) and bool(torch.isnan(dw[s:e]).all())


# ---- the autograd op ------------------------------------------------------------------------------

class _DropGrad(torch.autograd.Function):
    """identity whose backward hands on no gradient at all"""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return None


def test_autograd_op(host, capi, dev):
    lay, case, ref = dm.shared("gaps", "thinned", dm.EPS_VALUES[1])
    k_out, k_dw = _launch(capi, dev, lay, case)
    t, dt, z, d_out = (case[k].to(dev) for k in ("t", "dt", "z", "d_out"))
    bounds = lay.bounds.to(dev)
    w = case["weights"].to(dev).requires_grad_(True)
    t_req, dt_req, z_req = (v.clone().requires_grad_(True) for v in (t, dt, z))
    out = host.depth_sight(w, t_req, dt_req, bounds, z_req, case["eps"])
    assert out.shape == (lay.n_rays, 3) and torch.equal(out, k_out)
    (out * d_out).sum().backward()
    assert t_req.grad is None and dt_req.grad is None and z_req.grad is None
    # the gradient is the kernel's output inside the ranges and the op's zero fill outside
    inside = torch.from_numpy(lay.inside).to(dev)
    assert torch.equal(w.grad[inside], k_dw[inside]) and not bool(w.grad[~inside].any())
    got = dict(out=out.detach().cpu().numpy(), dw=np.where(lay.inside, w.grad.cpu().numpy(),
                                                           np.float32(rc.SENTINEL)))
    _report(lay, case, got, ref, "host.depth_sight")

    # an undefined upstream gradient stays undefined (lean gradients: the default) ...
    w2 = case["weights"].to(dev).requires_grad_(True)
    terms = host.depth_sight(w2, t, dt, bounds, z, case["eps"])
    (_DropGrad.apply(terms).sum() + (w2 * 2.0).sum()).backward()
    assert torch.equal(w2.grad, torch.full_like(w2, 2.0))
    # ... and is a zero where the nodes are asked to materialise them
    with capi.option("DENSE_LEAN", 1):
        w3 = case["weights"].to(dev).requires_grad_(True)
        terms = host.depth_sight(w3, t, dt, bounds, z, case["eps"])
        (_DropGrad.apply(terms).sum() + (w3 * 2.0).sum()).backward()
    assert torch.equal(w3.grad, w2.grad)

    # non-contiguous views of the weights and of the targets
    pair = torch.stack([case["weights"], torch.rand(lay.n_total)], 1).to(dev).requires_grad_(True)
    z_pair = torch.stack([z, torch.rand_like(z)], 1)
    out_view = host.depth_sight(pair[:, 0], t, dt, bounds, z_pair[:, 0], case["eps"])
    assert not pair[:, 0].is_contiguous() and not z_pair[:, 0].is_contiguous()
    assert torch.equal(out_view, out)
    (out_view * d_out).sum().backward()
    assert torch.equal(pair.grad[:, 0], w.grad) and not bool(pair.grad[:, 1].any())

    # eps is checked: negative or not finite is an error, not a launch
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="f2n_depth_sight_fwd"):
            host.depth_sight(w.detach(), t, dt, bounds, z, bad)
