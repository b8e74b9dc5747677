"""f2n_loss_fwd (loss.hip) against train_manager's formula in float64 (tests/step_tail_cases.py): the
four outputs within the any-order bound of their sums, both gradients element by element, at the ray
counts where the partial and the finish kernel change path (one block, 255 / 256 / 257 partials), with
exact zeros, errors far below the sqrt floor, a NaN colour, and through host.train_loss."""
import importlib

import numpy as np
import pytest
import torch

from tests import step_tail_cases as st

pytestmark = pytest.mark.gpu

CASES = [(n, kind) for n in st.LOSS_SIZES for kind in st.LOSS_KINDS]


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def _call(capi, dev, case, weight):
    """one f2n_loss_fwd; every output buffer carries GUARD sentinels past its end"""
    n = case["var"].shape[0]
    colors, gt, var = (torch.from_numpy(case[k]).to(dev) for k in ("colors", "gt", "var"))
    d_colors = torch.full((3 * n + st.GUARD,), st.SENTINEL, device=dev)
    d_var = torch.full((n + st.GUARD,), st.SENTINEL, device=dev)
    out4 = torch.full((4 + st.GUARD,), st.SENTINEL, device=dev)
    n_ws = capi.lib().cdll.f2n_loss_workspace_floats(n)
    assert n_ws == 3 * -(-n // st.LOSS_BLOCK)
    partial = torch.full((n_ws + st.GUARD,), st.SENTINEL, device=dev)
    capi.call("loss_fwd", colors, gt, var, n, weight, d_colors, d_var, partial, out4)
    torch.cuda.synchronize()
    for buf, used in ((d_colors, 3 * n), (d_var, n), (out4, 4), (partial, n_ws)):
        assert bool((buf[used:] == st.SENTINEL).all()), "guard overwritten"
    return dict(out4=out4[:4].cpu().numpy(), d_colors=d_colors[:3 * n].reshape(n, 3).cpu().numpy(),
                d_var=d_var[:n].cpu().numpy())


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)


@pytest.mark.parametrize("n,kind", CASES)
def test_loss_fwd_per_element(capi, dev, n, kind):
    case = st.loss_case(n, kind)
    worst = {}
    for w in st.LOSS_WEIGHTS:
        got = _call(capi, dev, case, w)
        assert _same_bits(got, _call(capi, dev, case, w))                # deterministic sums
        fails, wst = st.loss_failures(case, st.loss_ref(n, kind, w), got)
        for k, x in wst.items():
            worst[k] = max(worst.get(k, -np.inf), x)
        st.assert_none(fails, "n=%d %s w=%g" % (n, kind, w))
    print("[step-tail] loss n=%d %s max err/bound: %s" % (
        n, kind, "  ".join("%s %.4g" % (k, worst[k]) for k in st.LOSS_OUT + ("d_colors", "d_var"))))


@pytest.mark.parametrize("n,ray", [(1, 0), (257, 256), (65537, 300), (65537, 65536)])
def test_loss_fwd_nan_colour(capi, dev, n, ray):
    case = {k: a.copy() for k, a in st.loss_case(n, "mixed").items()}
    case["colors"][ray, 2] = np.nan
    got = _call(capi, dev, case, 0.3)
    st.assert_none(st.loss_nan_failures(got, ray, 2), "n=%d ray=%d" % (n, ray))


@pytest.mark.parametrize("n", [1, 257, 65537])
def test_train_loss_with_upstream_factor(host, dev, n):
    """host.train_loss: the same outputs, and an upstream factor reaches both gradients"""
    factor = 3.0
    for kind, w in (("mixed", 0.3), ("spike", 1e-2), ("zero", 0.0)):
        case = st.loss_case(n, kind)
        colors = torch.from_numpy(case["colors"]).to(dev).requires_grad_(True)
        var = torch.from_numpy(case["var"]).to(dev).requires_grad_(True)
        stats = host.train_loss(colors, torch.from_numpy(case["gt"]).to(dev), var, w)
        (stats[0] * factor).backward()
        got = dict(out4=stats.detach().cpu().numpy(), d_colors=colors.grad.cpu().numpy(),
                   d_var=var.grad.cpu().numpy())
        fails, worst = st.loss_failures(case, st.loss_ref(n, kind, w), got, factor=factor)
        print("[step-tail] train_loss n=%d %s w=%g max err/bound: d_colors %.4g  d_var %.4g" % (
            n, kind, w, worst["d_colors"], worst["d_var"]))
        st.assert_none(fails, "train_loss n=%d %s w=%g" % (n, kind, w))
