"""f2n_loss_sup_fwd (loss_sup.hip) against the float64 model of tests/supervision_model.py: the six
outputs and the three gradients within bounds counted from the kernel's stated evaluation order, at
the ray counts around the 256-thread block edge and in a multi-block tree, for every combination of
null and non-null ray_weight, alpha and opacity weight, with exact zeros among the weights, a batch
whose weights are all zero, and through host.train_loss_sup.

Largest error-to-bound ratios seen on an MI355X are recorded in NOTES.md section 32."""
import importlib

import numpy as np
import pytest
import torch

from tests import supervision_model as sm

pytestmark = pytest.mark.gpu

CASES = [(n, wk, al, ow) for n in sm.LOSS_SIZES for wk in (None, "mixed") for al in (False, True)
         for ow in (0.0, sm.OPACITY_WEIGHT)]
CASES += [(n, "allzero", True, sm.OPACITY_WEIGHT) for n in sm.LOSS_SIZES]


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def _dev(case, key, dev):
    return None if case[key] is None else torch.from_numpy(case[key].copy()).to(dev)


def _call(capi, dev, case, ow, with_opacity):
    """one f2n_loss_sup_fwd; every output buffer carries GUARD sentinels past its end"""
    n = case["var"].shape[0]
    t = {k: _dev(case, k, dev) for k in ("colors", "gt", "var", "ray_weight", "alpha", "opacity", "bg")}
    if not with_opacity:
        t["opacity"] = None
    if t["alpha"] is None:
        t["bg"] = None
    with_op = t["alpha"] is not None and with_opacity
    full = lambda k: torch.full((k + sm.GUARD,), sm.SENTINEL, device=dev)
    d_colors, d_var, d_op, out = full(3 * n), full(n), full(n), full(6)
    n_ws = capi.lib().cdll.f2n_loss_sup_workspace_floats(n)
    assert n_ws == 5 * -(-n // sm.LOSS_BLOCK)
    partial = full(n_ws)
    capi.call("loss_sup_fwd", t["colors"], t["gt"], t["var"], t["ray_weight"], t["alpha"], t["opacity"],
              t["bg"], n, sm.VAR_WEIGHT, ow, d_colors, d_var, d_op if with_op else None, partial, out)
    torch.cuda.synchronize()
    for buf, used in ((d_colors, 3 * n), (d_var, n), (d_op, n if with_op else 0), (out, 6), (partial, n_ws)):
        assert bool((buf[used:] == sm.SENTINEL).all()), "guard overwritten"
    got = dict(out=out[:6].cpu().numpy(), d_colors=d_colors[:3 * n].reshape(n, 3).cpu().numpy(),
               d_var=d_var[:n].cpu().numpy())
    if with_op:
        got["d_opacity"] = d_op[:n].cpu().numpy()
    return got


def _same_bits(a, b):
    return a.keys() == b.keys() and all(
        np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)


@pytest.mark.parametrize("n,weight_kind,with_alpha,ow", CASES)
def test_loss_sup_per_element(capi, dev, n, weight_kind, with_alpha, ow):
    case = sm.loss_case(n, weight_kind, with_alpha)
    with_opacity = ow != 0.0                # the opacity is handed over exactly when it is weighted
    ref = sm.loss_ref(case, sm.VAR_WEIGHT, ow, with_opacity)
    got = _call(capi, dev, case, ow, with_opacity)
    assert _same_bits(got, _call(capi, dev, case, ow, with_opacity))      # deterministic sums
    fails, worst = sm.loss_failures(ref, got)
    print("[supervision] loss_sup n=%d weights=%s alpha=%s ow=%g max err/bound: %s" % (
        n, weight_kind, with_alpha, ow, "  ".join("%s %.4g" % kv for kv in sorted(worst.items()))))
    assert not fails, "\n".join(fails)
    assert not np.isnan(got["out"]).any()   # the NaN colour of a masked ray went nowhere
    if weight_kind == "allzero":
        assert not got["out"].view(np.int32).any()
        assert all(not got[k].view(np.int32).any() for k in got if k != "out")
    if not (with_alpha and with_opacity):
        assert got["out"][3] == 0.0 and "d_opacity" not in got


@pytest.mark.parametrize("n", sm.LOSS_SIZES)
def test_opacity_given_but_not_weighted(capi, dev, n):
    """alpha and opacity with opacity_weight == 0: the term is reported, its gradient is exactly 0"""
    case = sm.loss_case(n, "mixed", True)
    ref = sm.loss_ref(case, sm.VAR_WEIGHT, 0.0, True)
    got = _call(capi, dev, case, 0.0, True)
    fails, _ = sm.loss_failures(ref, got)
    assert not fails, "\n".join(fails)
    assert not got["d_opacity"].any()
    assert n == 1 or got["out"][3] > 0.0


@pytest.mark.parametrize("n", [1, 257])
def test_train_loss_sup_with_upstream_factor(host, dev, n):
    """host.train_loss_sup: the same outputs, and an upstream factor reaches the three gradients"""
    factor = 4.0
    for weight_kind, with_alpha in ((None, False), ("mixed", True), ("allzero", True)):
        case = sm.loss_case(n, weight_kind, with_alpha)
        colors = _dev(case, "colors", dev).requires_grad_(True)
        var = _dev(case, "var", dev).requires_grad_(True)
        opacity = _dev(case, "opacity", dev).requires_grad_(True)
        stats = host.train_loss_sup(
            colors, _dev(case, "gt", dev), var, opacity=opacity, ray_weight=_dev(case, "ray_weight", dev),
            alpha=_dev(case, "alpha", dev), bg_color=_dev(case, "bg", dev) if with_alpha else None,
            var_loss_weight=sm.VAR_WEIGHT, opacity_weight=sm.OPACITY_WEIGHT)
        (stats[0] * factor).backward()
        ref = sm.loss_ref(case, sm.VAR_WEIGHT, sm.OPACITY_WEIGHT, True)
        got = dict(out=stats.detach().cpu().numpy(), d_colors=colors.grad.cpu().numpy() / factor,
                   d_var=var.grad.cpu().numpy() / factor)
        if with_alpha:
            got["d_opacity"] = opacity.grad.cpu().numpy() / factor
        else:
            assert opacity.grad is None or not bool(opacity.grad.any())
        # (a power of two: the factor and the division above are exact)
        fails, _ = sm.loss_failures(ref, got)
        assert not fails, "n=%d %s: %s" % (n, weight_kind, "\n".join(fails))
