"""f2n_density_grad and f2n_ray_normals over the C ABI against the float64 model of
tests/density_grad_model.py: |got - f64| <= 2 E per element with E the rounding bound counted there from
density_grad.hiph, NaN where the model is NaN, equal as numbers where E = 0.  The bound's own checks are
tests/test_density_grad_model_cpu.py.  Each test prints the largest |err| / E (-s)."""
import numpy as np
import pytest
import torch

from tests import density_grad_model as M

pytestmark = pytest.mark.gpu

CASES = M.cases()
RAY_CASES = [c for c in CASES if c.kind == "rays"]
SENTINEL = -12345.0


def _field(b, dev):
    return {k: b.fld[k].to(dev) for k in ("table16", "primes", "bias", "mul", "w0")}


def _grad(capi, dev, b, d):
    fld, n = b.fld, b.pts.shape[0]
    out = torch.full((n, 3), SENTINEL, device=dev)
    capi.call("density_grad", b.pts.to(dev), d["table16"], d["primes"], d["bias"], d["mul"], d["w0"], out, n,
              fld["L"], fld["F"], fld["T"], fld["stride"])
    return out


def _normals(capi, dev, b, d):
    fld, n_rays = b.fld, b.bounds.shape[0]
    out = torch.full((n_rays, 3), SENTINEL, device=dev)
    capi.call("ray_normals", b.pts.to(dev), b.bounds.to(dev), b.weights.to(dev), d["table16"], d["primes"],
              d["bias"], d["mul"], d["w0"], out, n_rays, fld["L"], fld["F"], fld["T"], fld["stride"])
    return out


def _hold(c, key, got, ref, E):
    got = got.cpu().numpy()
    r = M.ratio(got, ref, E)
    worst = float(r.max()) if r.size else 0.0
    print("\n%s: largest |err| / E of %s %.3f" % (M.case_id(c), key, worst))
    if not worst <= M.BAR:
        at = tuple(int(i) for i in np.unravel_index(int(np.argmax(r)), r.shape))
        raise AssertionError("%s: %s%s |err|/E = %g (got %r, f64 %r, E %g)" % (
            M.case_id(c), key, list(at), worst, float(got[at]), float(ref[at]), float(E[at])))


@pytest.mark.parametrize("c", CASES, ids=M.case_id)
def test_density_grad_within_bound(capi, dev, c):
    """every case's points, rays' samples included; every output element written"""
    b = M.build_case(c)
    got = _grad(capi, dev, b, _field(b, dev))
    assert not bool((got == SENTINEL).any())
    _hold(c, "grad", got, b.m["g"], b.m["E_g"])
    if c.tag == "w0zero":
        assert bool((got == 0).all())


@pytest.mark.parametrize("c", RAY_CASES, ids=M.case_id)
def test_ray_normals_within_bound(capi, dev, c):
    b = M.build_case(c)
    d = _field(b, dev)
    got = _normals(capi, dev, b, d)
    assert not bool((got == SENTINEL).any())                       # empty rays included
    _hold(c, "normals", got, b.m["N"], b.m["E_N"])
    # the same bits on every run (compared as bits: the NaN ray is equal to itself)
    assert torch.equal(got.view(torch.int32), _normals(capi, dev, b, d).view(torch.int32))
    length = (b.bounds[:, 1] - b.bounds[:, 0]).numpy()
    assert bool((got.cpu()[torch.from_numpy(length == 0)] == 0).all())
    if c.tag == "w0zero":
        assert bool((got == 0).all())
    if c.tag == "nan":
        assert torch.isnan(got).any(1).cpu().tolist() == [False, True, False, False, False]

    # ... and the float64 sum of w n^ formed from f2n_density_grad's OWN output: what is left between
    # the two kernels is the normalisation and the sum, whose bound is E_N with E_g = 0
    g = _grad(capi, dev, b, d).cpu().numpy().astype(np.float64)
    nh, E_nh = M.normal_model(g, np.zeros_like(g))
    N, E_N = M.ray_model(b.bounds, b.weights, nh, E_nh)
    _hold(c, "normals vs own grad", got, N, E_N)

    # property: the length of N_r is at most the ray's opacity, |N_r| <= sum_k w_k (1 + 8 u); rays
    # with a NaN sample apart
    w = np.zeros(b.bounds.shape[0])
    np.add.at(w, np.repeat(np.arange(b.bounds.shape[0]), length), b.weights.numpy().astype(np.float64))
    norm = np.linalg.norm(got.cpu().numpy().astype(np.float64), axis=1)
    fin = np.isfinite(norm)
    assert (norm[fin] <= w[fin] * (1 + 8 * M.U)).all()
