"""f2n_hash_pts_grad_exact and f2n_hash_rays_grad_exact over the C ABI against the float64 model of
tests/enc_grad_model.py: |got - f64| <= 2 E per element with E the rounding bound counted there from
density_grad.hiph and ray_grad_model's per-ray counts, NaN where the model is NaN, equal as numbers where
E = 0.  The bound's own checks are tests/test_enc_grad_model_cpu.py.  Each test prints the largest
|err| / E (-s)."""
import numpy as np
import pytest
import torch

from tests import enc_grad_model as M

pytestmark = pytest.mark.gpu

CASES = M.cases()
SENTINEL = -12345.0


def _field(b, dev):
    return {k: b.fld[k].to(dev) for k in ("table16", "primes", "bias", "mul")}


def _lay(b, g, dev):
    """g [n, C] in the case's layout -> (device tensor, g_ld_point, g_ld_chan)"""
    n, C = g.shape
    if b.case.chan_major:
        return g.t().contiguous().to(dev), 1, n
    return g.contiguous().to(dev), C, 1


def _pts_grad(capi, dev, b, d, x, g):
    fld, n = b.fld, x.shape[0]
    gd, ld_p, ld_c = _lay(b, g, dev)
    out = torch.full((n, 3), SENTINEL, device=dev)
    capi.call("hash_pts_grad_exact", x.to(dev).contiguous(), d["table16"], d["primes"], d["bias"], d["mul"], gd,
              ld_p, ld_c, out, n, fld["L"], fld["F"], fld["T"], fld["stride"])
    return out


def _rays_grad(capi, dev, b, d, g):
    fld, n_rays = b.fld, b.bounds.shape[0]
    gd, ld_p, ld_c = _lay(b, g, dev)
    d_o = torch.full((n_rays, 3), SENTINEL, device=dev)
    d_d = torch.full((n_rays, 3), SENTINEL, device=dev)
    capi.call("hash_rays_grad_exact", b.pts.to(dev), b.t.to(dev), b.bounds.to(dev), b.rays_d.to(dev),
              d["table16"], d["primes"], d["bias"], d["mul"], gd, ld_p, ld_c, d_o, d_d, n_rays, fld["L"],
              fld["F"], fld["T"], fld["stride"])
    return d_o, d_d


def _hold(c, key, got, ref, E):
    got = got.cpu().numpy()
    r = M.ratio(got, ref, E)
    worst = float(r.max()) if r.size else 0.0
    print("\n%s: largest |err| / E of %s %.3f" % (M.case_id(c), key, worst))
    if not worst <= M.BAR:
        at = tuple(int(i) for i in np.unravel_index(int(np.argmax(r)), r.shape))
        raise AssertionError("%s: %s%s |err|/E = %g (got %r, f64 %r, E %g)" % (
            M.case_id(c), key, list(at), worst, float(got[at]), float(ref[at]), float(E[at])))


def _bits(*ts):
    return [t.view(torch.int32) for t in ts]


@pytest.mark.parametrize("c", CASES, ids=M.case_id)
def test_pts_grad_exact_within_bound(capi, dev, c):
    """the per-point entry at the contracted float32 points of every case; every element written; the
    same bits on a second run"""
    b = M.build_case(c)
    d = _field(b, dev)
    x = torch.from_numpy(b.x32)
    got = _pts_grad(capi, dev, b, d, x, b.g)
    assert not bool((got == SENTINEL).any())
    _hold(c, "pts_grad", got, b.mp["G"], b.mp["E_G"])
    assert torch.equal(got, _pts_grad(capi, dev, b, d, x, b.g))
    assert bool((_pts_grad(capi, dev, b, d, x, torch.zeros_like(b.g)) == 0).all())


@pytest.mark.parametrize("c", CASES, ids=M.case_id)
def test_rays_grad_exact_within_bound(capi, dev, c):
    """the ray entry against the model, then against the float64 recomposition of its sibling's output"""
    b = M.build_case(c)
    d = _field(b, dev)
    d_o, d_d = _rays_grad(capi, dev, b, d, b.g)
    assert not bool((d_o == SENTINEL).any()) and not bool((d_d == SENTINEL).any())     # empty rays included
    _hold(c, "d_o", d_o, b.d_o, b.E_o)
    _hold(c, "d_d", d_d, b.d_d, b.E_d)
    # the same bits on every run (compared as bits: the NaN ray is equal to itself)
    again = _rays_grad(capi, dev, b, d, b.g)
    assert all(torch.equal(p, q) for p, q in zip(_bits(d_o, d_d), _bits(*again)))
    length = (b.bounds[:, 1] - b.bounds[:, 0]).numpy()
    empty = torch.from_numpy(length == 0)
    assert bool((d_o.cpu()[empty] == 0).all()) and bool((d_d.cpu()[empty] == 0).all())
    # the origin sample poisons its own ray and no other
    bad = [b.nan_ray] if c.origin else []
    assert torch.nonzero(torch.isnan(d_o).any(1)).flatten().tolist() == bad
    assert torch.nonzero(torch.isnan(d_d).any(1)).flatten().tolist() == bad
    # a zero gradient gives exact zeros (the origin's ray apart: NaN)
    z_o, z_d = _rays_grad(capi, dev, b, d, torch.zeros_like(b.g))
    keep = torch.ones(len(length), dtype=torch.bool)
    keep[bad] = False
    assert bool((z_o.cpu()[keep] == 0).all()) and bool((z_d.cpu()[keep] == 0).all())

    # ... and f2n_hash_pts_grad_exact's OWN output at the points f2n_contract_fwd forms (contract_point,
    # the function the ray kernel calls), taken through the Jacobian and the sums in float64: what is left
    # between the two kernels is the Jacobian and the per-ray part, E_G = 0
    n = b.pts.shape[0]
    x = torch.empty(n, 3, device=dev)
    capi.call("contract_fwd", b.pts.to(dev), x, n)
    x = torch.nan_to_num(x, nan=0.0)                                # the origin: any finite cell
    G = _pts_grad(capi, dev, b, d, x, b.g).cpu().numpy().astype(np.float64)
    dp, E_dp = M.contract_bwd_model(b.pts, G, np.zeros_like(G))
    r_o, E_o, r_d, E_d = M.rays_model(b.bounds, b.t, dp, E_dp, b.rays_d)
    _hold(c, "d_o vs own pts_grad", d_o, r_o, E_o)
    _hold(c, "d_d vs own pts_grad", d_d, r_d, E_d)


@pytest.mark.parametrize("c", CASES[:len(M.SHAPES)], ids=M.case_id)
def test_the_q5_kernel_cannot_pass(capi, dev, c):
    """f2n_hash_rays_grad itself on the same inputs: the device counterpart of the Q5 mutant of
    tests/test_enc_grad_model_cpu.py.  Every ray with a sample (the origin's apart) leaves the bar."""
    b = M.build_case(c)
    fld, n_rays = b.fld, b.bounds.shape[0]
    d = _field(b, dev)
    gd, ld_p, ld_c = _lay(b, b.g, dev)
    d_o = torch.full((n_rays, 3), SENTINEL, device=dev)
    d_d = torch.full((n_rays, 3), SENTINEL, device=dev)
    capi.call("hash_rays_grad", b.pts.to(dev), b.t.to(dev), b.bounds.to(dev), b.rays_d.to(dev), d["table16"],
              d["primes"], d["bias"], d["mul"], gd, ld_p, ld_c, d_o, d_d, n_rays, fld["L"], fld["F"], fld["T"],
              fld["stride"], 128.0)
    length = (b.bounds[:, 1] - b.bounds[:, 0]).numpy()
    live = (length > 0) & ~np.isnan(b.d_o).any(1)
    out = (M.ratio(d_o, b.d_o, b.E_o) > M.BAR).any(1) | (M.ratio(d_d, b.d_d, b.E_d) > M.BAR).any(1)
    assert live.sum() >= 6 and out[live].all(), (M.case_id(c), int((~out[live]).sum()), int(live.sum()))


@pytest.mark.parametrize("c", CASES[:len(M.SHAPES)], ids=M.case_id)
def test_uniform_rows_are_f2n_density_grad(capi, dev, c):
    """grad_out rows all equal to w0.  Inside the unit ball the contracted point is the raw one and the
    per-point entry is f2n_density_grad bit for bit: the same device function in the same order.  For
    all radii the ray entry's d_o is the float64 sum of f2n_density_grad's rows within the per-ray part
    of the bound (E_dp = 0), and d_d likewise."""
    b = M.build_case(c)
    fld, n = b.fld, b.pts.shape[0]
    d = _field(b, dev)
    w0 = fld["w0"]
    g = w0[None].expand(n, -1).contiguous()
    dens = torch.full((n, 3), SENTINEL, device=dev)
    capi.call("density_grad", b.pts.to(dev), d["table16"], d["primes"], d["bias"], d["mul"], w0.to(dev), dens, n,
              fld["L"], fld["F"], fld["T"], fld["stride"])
    nrm = b.pts.norm(dim=1)
    inside = (nrm < 1) & (nrm > 0)
    assert int(inside.sum()) >= 100
    got = _pts_grad(capi, dev, b, d, b.pts[inside], g[inside])
    assert torch.equal(got, dens[inside.to(dev)])
    d_o, d_d = _rays_grad(capi, dev, b, d, g)
    rows = dens.cpu().numpy().astype(np.float64)
    r_o, E_o, r_d, E_d = M.rays_model(b.bounds, b.t, rows, np.zeros_like(rows), b.rays_d)
    _hold(c, "d_o vs density_grad", d_o, r_o, E_o)
    _hold(c, "d_d vs density_grad", d_d, r_d, E_d)
