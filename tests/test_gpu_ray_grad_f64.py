"""The gradient of the hash encoding with respect to the rays -- f2n_hash_rays_grad (the fused route)
and f2n_hash_bwd's point gradient + f2n_contract_bwd (the op-by-op route), with f2n_contract_fwd --
against the float64 restatement of tests/ray_grad_model.py, level by level and ray by ray: equal as
numbers where one level carries the gradient (no free order, nothing to round differently), and
|got - f64| <= 2 E everywhere else, with E the worst-case rounding bound counted there from the kernels'
code.  The bound's own checks are tests/test_ray_grad_model_cpu.py.  Each test prints the largest
|err| / E per output (-s): how much of the room the kernels use."""
import functools

import numpy as np
import pytest
import torch

from tests import ray_grad_model as M

pytestmark = pytest.mark.gpu

F2N_E_INVALID_ARG, F2N_E_UNSUPPORTED = -1, -3
CASES = M.cases()
LEVEL_CASES = [c for c in CASES if c.layer == "level"]
RAY_CASES = [c for c in CASES if c.layer != "level"]


@functools.lru_cache(maxsize=None)
def _case(c):
    """inputs and float64 model of one case, built once and shared (read only)"""
    return M.build_case(c)


def _device(inp, dev):
    fld = inp.fld
    d = {k: fld[k].to(dev) for k in ("table16", "primes", "bias", "mul")}
    d.update(pts=inp.pts.to(dev), t=inp.t.to(dev), bounds=inp.bounds.to(dev), rays_d=inp.rays_d.to(dev),
             g=inp.g.to(dev))
    return d


def _rays_grad(capi, dev, inp, d, g, ld_point, ld_chan, fill=float("nan")):
    fld, n_rays = inp.fld, inp.bounds.shape[0]
    d_o = torch.full((n_rays, 3), fill, device=dev)
    d_d = torch.full((n_rays, 3), fill, device=dev)
    capi.call("hash_rays_grad", d["pts"], d["t"], d["bounds"], d["rays_d"], d["table16"], d["primes"], d["bias"],
              d["mul"], g, ld_point, ld_chan, d_o, d_d, n_rays, fld["L"], fld["F"], fld["T"], fld["stride"],
              M.GRAD_SCALE)
    return d_o.cpu(), d_d.cpu()


def _pts_grad(capi, dev, inp, d, x, g, ld_point, ld_chan, tg):
    """f2n_hash_bwd's point gradient at the contracted points x, into a buffer prefilled with 7.0"""
    fld, n = inp.fld, x.shape[0]
    pg = torch.full((n, 3), 7.0, device=dev)
    capi.call("hash_bwd", x, d["table16"], d["primes"], d["bias"], d["mul"], g, ld_point, ld_chan, tg, pg, n,
              fld["L"], fld["F"], fld["T"], fld["stride"], M.GRAD_SCALE)
    return pg.cpu()


class _Report:
    """collects |err| / E per (route, output); every miss is named at the end"""

    def __init__(self, c):
        self.c, self.lines, self.misses = c, [], []

    def hold(self, route, key, got, ref, E):
        got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
        r = M.ratio(got, ref, E)
        worst = float(r.max()) if r.size else 0.0
        self.lines.append("  %-34s %-5s %.3f" % (route, key, worst))
        if not worst <= M.BAR:
            at = [int(i) for i in np.unravel_index(int(np.argmax(r)), r.shape)]
            self.misses.append("%s: %s%s |err|/E = %g (got %r, f64 %r, E %g)" % (
                route, key, at, worst, float(got[tuple(at)]), float(ref[tuple(at)]), float(E[tuple(at)])))

    def close(self):
        print("\n%s: largest |err| / E\n%s" % (M.case_id(self.c), "\n".join(self.lines)))
        assert not self.misses, "%s: outside 2 E:\n%s" % (M.case_id(self.c), "\n".join(self.misses))


# ---- 1. one level at a time: equal as numbers ------------------------------------------------------------

@pytest.mark.parametrize("c", LEVEL_CASES, ids=M.case_id)
def test_one_level_at_a_time_is_exact(capi, dev, c):
    """Single-sample rays inside the unit ball, the gradient in the channels of one level: the level's
    float32 sum in the kernels' own order is the whole result of both routes (the contraction is the
    identity, every other add is onto a zero)."""
    inp, m, _ = _case(c)
    fld = inp.fld
    L, F, n = fld["L"], fld["F"], inp.pts.shape[0]
    d = _device(inp, dev)
    tg = torch.zeros(fld["numel"], device=dev)
    wrong = []
    for l in range(L):
        g = torch.zeros_like(d["g"])
        g[:, l * F:(l + 1) * F] = d["g"][:, l * F:(l + 1) * F]
        want = m["level_f32"][:, l]
        d_o, _ = _rays_grad(capi, dev, inp, d, g, L * F, 1)
        pg = _pts_grad(capi, dev, inp, d, d["pts"], g, L * F, 1, tg)
        for route, got in (("hash_rays_grad d_o", d_o.numpy()), ("hash_bwd pts_grad", pg.numpy())):
            bad = int((got != want).sum())       # compared as numbers: NaN != anything, -0 == 0
            if bad:
                wrong.append("%s, level %d: %d of %d elements differ" % (route, l, bad, want.size))
    assert float(np.abs(m["level_f32"]).max()) > 0
    assert not wrong, "%s:\n%s" % (M.case_id(c), "\n".join(wrong))


# ---- 2.-4. all levels: fixed radii, one hot sample per ray, dense rays, ray counts -----------------------

@pytest.mark.parametrize("c", RAY_CASES, ids=M.case_id)
def test_rays_grad_within_bound(capi, dev, c):
    """Both routes stage by stage: contract_fwd -> x, hash_bwd -> G at the model's float32 contracted
    points, contract_bwd given float32(G) -> dp, and hash_rays_grad -> d_o, d_d."""
    inp, m, _ = _case(c)
    fld = inp.fld
    L, F, n = fld["L"], fld["F"], inp.pts.shape[0]
    d = _device(inp, dev)
    rep = _Report(c)
    g_cm = d["g"].t().contiguous()

    d_o, d_d = _rays_grad(capi, dev, inp, d, g_cm, 1, n)
    rep.hold("hash_rays_grad", "d_o", d_o, m["d_o"], m["E"]["d_o"])
    rep.hold("hash_rays_grad", "d_d", d_d, m["d_d"], m["E"]["d_d"])
    empty = (inp.bounds[:, 1] == inp.bounds[:, 0]).numpy()
    assert float(np.abs(d_o.numpy()[empty]).sum()) == 0.0 and float(np.abs(d_d.numpy()[empty]).sum()) == 0.0

    x = torch.full((n, 3), 7.0, device=dev)
    capi.call("contract_fwd", d["pts"], x, n)
    rep.hold("contract_fwd", "x", x, m["x"], m["E"]["x"])

    tg = torch.zeros(fld["numel"], device=dev)
    pg = _pts_grad(capi, dev, inp, d, torch.from_numpy(m["x32"]).to(dev), g_cm, 1, n, tg)
    rep.hold("hash_bwd", "G", pg, m["G"], m["E"]["G"])

    G32 = torch.from_numpy(m["G"]).float()
    dp_ref, dp_E = M.contract_bwd_model(inp.pts, G32.double().numpy(), np.zeros((n, 3)))
    dp = torch.full((n, 3), 7.0, device=dev)
    capi.call("contract_bwd", d["pts"], G32.to(dev), dp, n)
    rep.hold("contract_bwd(float32 G)", "dp", dp, dp_ref, dp_E)

    if c.layer == "points":
        # the |p| == 0 sample poisons its own ray and no other of its workgroup
        _, at = M.fixed_points()
        nan_o, nan_d = torch.isnan(d_o).all(1), torch.isnan(d_d).all(1)
        assert bool(nan_o[at]) and bool(nan_d[at]) and int(nan_o.sum()) == 1 and int(nan_d.sum()) == 1
        assert bool(torch.isnan(x.cpu()[at]).all()) and bool(torch.isnan(dp.cpu()[at]).all())
        assert not bool(torch.isnan(d_o).any(1)[[at - 1, at + 1, at + 2]].any())
    rep.close()


# ---- 5. layouts ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [c for c in CASES if c.layer == "dense"], ids=M.case_id)
def test_gradient_layouts(capi, dev, c):
    """channel-major, point-major and a padded point stride: the same bits from hash_rays_grad (its
    order is fixed), hash_bwd's point gradient within 2 E in each"""
    inp, m, _ = _case(c)
    fld = inp.fld
    L, F, n = fld["L"], fld["F"], inp.pts.shape[0]
    d = _device(inp, dev)
    rep = _Report(c)
    padded = torch.full((n, L * F + 3), float("nan"), device=dev)
    padded[:, :L * F] = d["g"]
    layouts = [("channel-major", d["g"].t().contiguous(), 1, n), ("point-major", d["g"], L * F, 1),
               ("padded point stride", padded, L * F + 3, 1)]
    tg = torch.zeros(fld["numel"], device=dev)
    x32 = torch.from_numpy(m["x32"]).to(dev)
    first = None
    for name, g, ld_point, ld_chan in layouts:
        d_o, d_d = _rays_grad(capi, dev, inp, d, g, ld_point, ld_chan)
        if first is None:
            first = (d_o, d_d)
            rep.hold(name, "d_o", d_o, m["d_o"], m["E"]["d_o"])
            rep.hold(name, "d_d", d_d, m["d_d"], m["E"]["d_d"])
        assert torch.equal(d_o, first[0]) and torch.equal(d_d, first[1]), name
        rep.hold(name + ", hash_bwd", "G", _pts_grad(capi, dev, inp, d, x32, g, ld_point, ld_chan, tg), m["G"],
                 m["E"]["G"])
    rep.close()


# ---- 6. entry checks -------------------------------------------------------------------------------------

def test_entry_checks(capi, dev):
    c = [c for c in CASES if c.layer == "count"][1]
    inp, m, _ = _case(c)
    fld = inp.fld
    L, F, T, n, n_rays = fld["L"], fld["F"], fld["T"], inp.pts.shape[0], inp.bounds.shape[0]
    d = _device(inp, dev)
    g_cm = d["g"].t().contiguous()
    fn = capi.lib().cdll.f2n_hash_rays_grad
    d_o = torch.full((n_rays, 3), 7.0, device=dev)
    d_d = torch.full((n_rays, 3), 7.0, device=dev)

    def status(table=d["table16"], rays=n_rays, F_=F, stride=fld["stride"], scale=M.GRAD_SCALE):
        args = (d["pts"], d["t"], d["bounds"], d["rays_d"], table, d["primes"], d["bias"], d["mul"], g_cm, 1, n,
                d_o, d_d, rays, L, F_, T, stride, scale)
        st = fn(*[capi._ptr(a) for a in args], capi.current_stream())
        torch.cuda.synchronize()
        return st

    assert status(rays=0) == 0
    assert status(scale=100.0) == F2N_E_INVALID_ARG        # not a power of two
    assert status(scale=0.0) == F2N_E_INVALID_ARG
    assert status(F_=3, stride=3 * T) == F2N_E_UNSUPPORTED
    assert status(table=d["table16"][1:]) == F2N_E_INVALID_ARG      # a row of F f16 is loaded whole
    assert float((d_o - 7.0).abs().max()) == 0.0 and float((d_d - 7.0).abs().max()) == 0.0, "written to"
    assert status() == 0
    a = (d_o.cpu().clone(), d_d.cpu().clone())
    d_o.fill_(7.0)
    d_d.fill_(7.0)
    assert status() == 0
    assert torch.equal(d_o.cpu(), a[0]) and torch.equal(d_d.cpu(), a[1])
    assert float(M.ratio(a[0], m["d_o"], m["E"]["d_o"]).max()) <= M.BAR
