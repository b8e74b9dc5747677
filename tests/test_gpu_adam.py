"""Fused Adam (f2n_adam_step / FusedAdam) against torch.optim.Adam with the reference's settings
(betas 0.9/0.99, eps 1e-15; weight decay 1e-6 on everything but the table), and the f16 shadow of the
hash table it emits against an RNE cast of the updated master.  Below those: one step at a time
against the float64 rule of tests/step_tail_cases.py, element by element within its bounds, at the
sizes where the launch takes another path (the float4 tail, the grid-stride passes past P) and
through FusedAdam on the reference's full-size table."""
import importlib

import numpy as np
import pytest
import torch

from tests import step_tail_cases as tail

pytestmark = pytest.mark.gpu


def test_adam_step_kernel_vs_torch(capi, dev):
    g = torch.Generator().manual_seed(0)
    for n, wd in ((100003, 0.0), (4096, 1e-6), (7, 1e-2)):
        p0 = torch.randn(n, generator=g) * 0.1
        ref_p = p0.clone().requires_grad_(True)
        opt = torch.optim.Adam([ref_p], lr=1e-2, betas=(0.9, 0.99), eps=1e-15, weight_decay=wd)
        p = p0.to(dev)
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        shadow = torch.empty(n, dtype=torch.int16, device=dev)
        for step in range(1, 5):
            grad = torch.randn(n, generator=g) * 1e-3
            grad[::5] = 0.0
            ref_p.grad = grad.clone()
            opt.step()
            capi.call("adam_step", p, grad.to(dev), m, v, shadow, n, 1e-2, 0.9, 0.99, 1e-15, wd, step)
            torch.testing.assert_close(p.cpu(), ref_p.detach(), rtol=2e-5, atol=1e-7)
            assert torch.equal(shadow.view(torch.float16), p.to(torch.float16))
        st = opt.state[ref_p]
        torch.testing.assert_close(m.cpu(), st["exp_avg"], rtol=1e-5, atol=1e-9)
        torch.testing.assert_close(v.cpu(), st["exp_avg_sq"], rtol=1e-5, atol=1e-12)


def test_fused_adam_optimizer_matches_torch_adam(dev):
    H = importlib.import_module("f2-nerf_amd").load_host()
    rens = []
    for _ in range(2):
        H.manual_seed(3)
        rens.append(H.Renderer(3, n_levels=4, log2_table=12, max_samples=64, step=4.0 / 64))
    a, b = rens
    for k, v in a.named_parameters().items():
        assert torch.equal(v, b.named_parameters()[k])
    opt_a, opt_b = a.make_adam(1e-2), b.make_fused_adam(1e-2)
    assert opt_a.n_groups() == opt_b.n_groups() == 4
    g = torch.Generator().manual_seed(1)
    o = (torch.randn(64, 3, generator=g) * 0.2).to(dev)
    d = torch.randn(64, 3, generator=g).to(dev)
    emb = torch.randint(0, 3, (64,), generator=g).to(torch.int32).to(dev)
    gt = torch.rand(64, 3, generator=g).to(dev)
    noise = (torch.rand(64, 64, generator=g) + 0.5).to(dev)
    bg = torch.rand(64, 3, generator=g).to(dev)
    for it in range(4):
        losses = []
        for ren, opt in ((a, opt_a), (b, opt_b)):
            opt.zero_grad()
            loss, _, _, _ = ren.train_step(o, d, emb, gt, 1e-2, noise, bg, True)
            losses.append(float(loss))
            opt.step()
        assert abs(losses[0] - losses[1]) <= 2e-5 * abs(losses[0]), (it, losses)
        # the table's f16 shadow is already the cast of the updated master, without a cast pass
        f = b.scene_field
        assert torch.equal(f.table_f16(), f.feat_pool.detach().to(torch.float16))
    pa, pb = a.named_parameters(), b.named_parameters()
    # Adam normalises every update to ~lr, so an entry whose gradient is rounding noise (the two
    # pipelines sum float atomics in different orders) may move differently: compare in aggregate.
    for k in pa:
        if pa[k].dtype == torch.float32:
            diff = (pb[k] - pa[k]).abs()
            tol = 2e-6 + 2e-4 * pa[k].abs()
            assert float((diff > tol).float().mean()) < 1e-3, k
            assert float(diff.norm() / (pa[k].norm() + 1e-12)) < 1e-4, k
    assert losses[0] < 1e9 and losses[0] == losses[0]


# ---- one step against float64, element by element (tests/step_tail_cases.py) ----------------------

def _guarded(a, dev):
    return torch.from_numpy(tail.with_guard(a)).to(dev)


def _run_step(capi, dev, case, step, wd, with_shadow):
    """one f2n_adam_step on guarded copies of the case -> got dict of numpy arrays"""
    n = case["p"].shape[0]
    p, g, m, v = (_guarded(case[k], dev) for k in ("p", "g", "m", "v"))
    g_before = g.clone()
    shadow = torch.full((n + tail.GUARD,), tail.SENTINEL_H, dtype=torch.int16, device=dev) if with_shadow else None
    capi.call("adam_step", p, g, m, v, shadow, n, tail.LR, tail.BETA1, tail.BETA2, tail.EPS, wd, step)
    torch.cuda.synchronize()
    assert torch.equal(g, g_before)                          # the gradient is read, never written
    got = dict(p=p.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy(), shadow=None)
    if with_shadow:
        got["shadow"] = shadow.cpu().numpy().view(np.uint16)
    return got


def _check_step(capi, dev, n, step, wd, worst):
    case = tail.adam_case(n, wd)
    got = _run_step(capi, dev, case, step, wd, True)         # adam_step_kernel<true>
    plain = _run_step(capi, dev, case, step, wd, False)      # adam_step_kernel<false>
    fails, w = tail.adam_failures(case, step, wd, got, plain)
    for k in w:
        worst[k] = max(worst.get(k, -np.inf), w[k])
    tail.assert_none(fails, "n=%d step=%d wd=%g" % (n, step, wd))
    # the plain run on its own too: same bounds, its guards intact
    tail.assert_none(tail.adam_failures(case, step, wd, plain)[0], "n=%d step=%d wd=%g, no shadow" % (n, step, wd))


@pytest.mark.parametrize("n", tail.SMALL_SIZES)
def test_adam_step_per_element_small(capi, dev, n):
    worst = {}
    for step in tail.STEPS:
        for wd in tail.WDS:
            _check_step(capi, dev, n, step, wd, worst)
    print("[step-tail] adam n=%d max err/bound: m %.4g  v %.4g  p %.4g (the part K_P scales: %.4g)" % (
        n, worst["m"], worst["v"], worst["p"], worst["p_update"]))


@pytest.mark.parametrize("n", tail.BIG_SIZES)
def test_adam_step_per_element_past_one_pass(capi, dev, n):
    """P - 1 .. 4 P: the last pass's tail, the second to fourth grid-stride passes"""
    step, wd = tail.BIG_PAIRS[n]
    worst = {}
    _check_step(capi, dev, n, step, wd, worst)
    print("[step-tail] adam n=%d (step %d, wd %g) max err/bound: m %.4g  v %.4g  p %.4g (the part K_P scales: %.4g)" % (
        n, step, wd, worst["m"], worst["v"], worst["p"], worst["p_update"]))


# the groups of Renderer::optim_param_groups and their weight decay
_GROUP_WD = (("scene_field.feat_pool", 0.0), ("scene_field.mlp.", 1e-6), ("shader.mlp.", 1e-6), ("app_emb", 1e-6))


def _group_wd(name):
    for prefix, wd in _GROUP_WD:
        if name.startswith(prefix):
            return wd
    return None


def test_fused_adam_full_size_table_per_element(dev):
    """FusedAdam on the reference's table (16 levels of 2^19 entries x 2 = 4 P elements), gradients
    from a 64-ray train_step.  Before each step p and grad are read; after it every element of every
    parameter is compared with the float64 step, which carries m and v (and what the kernel's f32 m,
    v may be off by) in float64 from step 1.  Elements whose gradient has been zero so far must keep
    their bits.  A fourth step at lr / 10 is held to the same bound."""
    H = importlib.import_module("f2-nerf_amd").load_host()
    H.manual_seed(7)
    ren = H.Renderer(3, n_levels=16, log2_table=19, max_samples=64, step=4.0 / 64)
    opt = ren.make_fused_adam(tail.LR)
    assert opt.n_groups() == 4
    params = ren.named_parameters()
    assert params["scene_field.feat_pool"].numel() == 4 * tail.P
    g = torch.Generator().manual_seed(1)
    o = (torch.randn(64, 3, generator=g) * 0.2).to(dev)
    d = torch.randn(64, 3, generator=g).to(dev)
    emb = torch.randint(0, 3, (64,), generator=g).to(torch.int32).to(dev)
    gt = torch.rand(64, 3, generator=g).to(dev)
    noise = (torch.rand(64, 64, generator=g) + 0.5).to(dev)
    bg = torch.rand(64, 3, generator=g).to(dev)
    state = {}
    field = ren.scene_field
    for it in range(1, 5):
        lr = tail.LR if it < 4 else tail.LR / 10
        if it == 4:
            opt.set_lr(lr)
        opt.zero_grad()
        ren.train_step(o, d, emb, gt, 1e-2, noise, bg, True)
        torch.cuda.synchronize()
        grads = ren.grads()
        before = {k: v.detach().clone() for k, v in params.items()}
        grad = {k: (None if v is None else v.detach().clone()) for k, v in grads.items()}
        opt.step()
        torch.cuda.synchronize()
        moved_total = 0
        for name, p in params.items():
            wd = _group_wd(name)
            flat_after, flat_before = p.detach().reshape(-1), before[name].reshape(-1)
            if wd is None or grad[name] is None:             # in no group, or nothing to step on
                assert torch.equal(flat_after, flat_before), name
                continue
            gflat = grad[name].reshape(-1)
            n = flat_after.numel()
            s = state.setdefault(name, dict(step=0, live=torch.zeros(n, dtype=torch.bool, device=dev),
                                            m=np.zeros(n), v=np.zeros(n), dm=np.zeros(n), dv=np.zeros(n)))
            s["step"] += 1
            s["live"] |= gflat != 0
            if wd != 0:
                s["live"][:] = True
            quiet = ~s["live"]                                # g = m = v = 0, wd = 0: nothing moves
            assert torch.equal(flat_after.view(torch.int32)[quiet], flat_before.view(torch.int32)[quiet]), name
            idx_dev = torch.nonzero(s["live"]).reshape(-1)
            idx = idx_dev.cpu().numpy()
            p0, g0, p1 = (t[idx_dev].cpu().numpy() for t in (flat_before, gflat, flat_after))
            r = tail.adam_ref(p0, g0, s["m"][idx], s["v"][idx], s["step"], wd, lr)
            tm, tv, tp, parts = tail.adam_tol(r, dm_in=s["dm"][idx], dv_in=s["dv"][idx])
            err = np.abs(p1.astype(np.float64) - r["P"])
            ratio = float((err / tp).max())
            moved = float(np.abs(p1.astype(np.float64) - p0).max())
            print("[step-tail] FusedAdam step %d lr %g %s: %d live of %d, max err/bound %.4g (the part K_P scales: "
                  "%.4g), largest move %.3g" % (it, lr, name, idx.size, n, ratio,
                                                tail.p_update_ratio(err, r, parts), moved))
            bad = np.flatnonzero(~(err <= tp))
            assert bad.size == 0, (name, it, idx[bad[:4]], err[bad[:4]], tp[bad[:4]])
            moved_total += int((p1 != p0).sum())
            s["m"][idx], s["v"][idx], s["dm"][idx], s["dv"][idx] = r["M"], r["V"], tm, tv
            if name == "scene_field.feat_pool":
                assert idx.size > 1000
                sh = field.table_f16().reshape(-1)
                assert (sh[idx_dev].view(torch.int16).cpu().numpy().view(np.uint16) == tail.f16_rne_bits(p1)).all()
        assert moved_total > 1000
        # the whole f16 working copy is the RNE cast of the stored master
        assert torch.equal(field.table_f16(), field.feat_pool.detach().to(torch.float16))
