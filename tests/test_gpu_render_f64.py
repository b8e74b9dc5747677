"""The one-pass inference render -- f2n_render_rays, f2n_render_rays_head + f2n_render_rays_tail at every
n_head, and the head alone -- against the float64 model of tests/render_model.py, ray by ray: kept and
len equal to the model's, |got - f64| <= 2 E for colours, depths and last_trans with E the worst-case
rounding bound counted there from the kernels' code, equality where E = 0 (no kept, occupied sample:
colors == bg, last_trans == 1, depths == 0), and the routes' counts equal among themselves on every ray.
The bound's own checks are tests/test_render_model_cpu.py.

The model's per-sample inputs come from the op-by-op kernels on the device (f2n_sample_rays,
f2n_contract_fwd, f2n_hash_fwd), which are held elsewhere; the one-pass kernels claim to form the same
samples and encodings in bits whatever their stride width (sampler.hiph), so this is a test of that claim
as well -- to the resolution of the outputs.  A sample that differs in one bit can flip an f16 encoding
value and move that sample's logit by |w| ulp16, which is a few times E_logit; through a per-ray output
such a flip stays inside the bound or near it (render_model.INFORMATIONAL, f16_ulp: measured on the CPU,
below 0.5 E where the logit moves most, 0.66-2.86 E at the opaque second sample of a two-sample ray, below
0.3 E at the most opaque sample of the other cases), so one flipped value is not something this module
can see; a stride that reads another
sample's row, or another ray's, is.

render_model.sources_differ keeps the two sources honest: the device's t, dt, points and directions
differ from the CPU oracle's only as test_sample_rays allows, its contracted points lie within 2 E of
ray_grad_model's float64 contraction, and its encoding rows are the bits of K.hash_fwd at its own
contracted points (the bar of test_hash_fwd_parity); the share of encoding values that differ between
the sources is printed.  The cases' conditions -- ambiguity cap, required lengths, weight
behind every link -- are asserted again on the device's inputs, from the model alone.

Each case prints the largest |err| / E per output and route (-s): the figures of NOTES.md section 27."""
import time

import numpy as np
import pytest
import torch

from tests import render_model as M
from tests.test_gpu_occupancy import _pack
from tests.test_gpu_render_rays import _render_rays_raw
from tests.test_gpu_render_rays_head import _head_raw

pytestmark = pytest.mark.gpu

CASES = M.cases()


def _device_inputs(inp, dev):
    f = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.fld.items()}
    net = {k: v.to(dev) for k, v in inp.P.items()}
    to = lambda x: None if x is None else x.to(dev)
    img = None if inp.img is None else torch.from_numpy(inp.img.astype(np.int32)).to(dev)
    words = None if inp.occ is None else _pack(torch.from_numpy(inp.occ)).to(dev)
    return f, net, to(inp.o), to(inp.d), to(inp.noise), img, to(inp.bg), words


def _device_samples(capi, dev, inp, f, o, d, noise):
    """the op-by-op route's per-sample inputs: f2n_sample_rays, f2n_contract_fwd, f2n_hash_fwd (rows)"""
    c = inp.case
    n, S, C = c.n_rays, c.S, c.C
    N = n * S
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
    pts, dirs, dt, t, x, enc = nan(N, 3), nan(N, 3), nan(N), nan(N), nan(N, 3), nan(N, C)
    bounds = torch.zeros(n, 2, dtype=torch.int32, device=dev)
    capi.call("sample_rays", o, d, noise, pts, dirs, dt, t, bounds, n, S, inp.step)
    capi.call("contract_fwd", pts, x, N)
    capi.call("hash_fwd", x, f["table16"], f["primes"], f["bias"], f["mul"], enc, C, 1, None, N, f["L"], f["F"],
              f["T"], f["stride"])
    h = lambda a, *shape: a.cpu().numpy().reshape(shape)
    return M.Samples(h(t, n, S), h(dt, n, S), h(x, n, S, 3), h(enc, n, S, C), h(dirs, n, S, 3)[:, 0].copy(),
                     h(pts, n, S, 3))


def _named(out):
    return dict(zip(("colors", "depths", "last_trans", "kept", "len"), (x.cpu() for x in out)))


@pytest.mark.parametrize("c", CASES, ids=M.case_id)
def test_routes_within_bound(capi, dev, c):
    t0 = time.time()
    inp, smp_cpu, m_cpu = M.build_case(c)
    S, n = c.S, c.n_rays
    f, net, o, d, noise, img, bg, words = _device_inputs(inp, dev)
    G = M.G_OCC if words is not None else 0
    smp = _device_samples(capi, dev, inp, f, o, d, noise)
    share, largest = M.sources_differ(inp.fld, smp_cpu, smp)
    m = M.model(inp, smp)
    M.check_conditions(c, m)          # from the model alone, on the device's inputs
    n_amb = int(m["ambiguous"].sum())

    outs = {}
    with capi.option("GATHER_PAIRED", c.paired):
        outs["one-ray"] = _named(_render_rays_raw(capi, f, net, o, d, noise, S, inp.step, words, G, img, bg))
        for n_head in M.heads(S):
            route = "head-whole" if n_head >= S else "head-%d" % n_head
            if n_head == 64 and S == 64:
                route = "head-64=S"
            outs[route] = _named(_head_raw(capi, f, net, o, d, noise, S, inp.step, n_head, words, G, img, bg))
    torch.cuda.synchronize()

    lines, misses = [], []
    first = outs["one-ray"]
    for route, got in outs.items():
        # the routes agree in their counts on every ray, the ambiguous ones included
        assert torch.equal(got["kept"], first["kept"]) and torch.equal(got["len"], first["len"]), (c.name, route)
        fails = M.failures(got, m)
        r = M.ratios(got, m)
        lines.append("  %-12s %s  %d misses" % (route, "  ".join("%s %.3f" % kv for kv in r.items()), len(fails)))
        misses += ["%s: %s" % (route, x) for x in fails]
    print("\n%s (seed %d): %d ambiguous of %d; encodings that differ from the CPU oracle's: %.3g %% (largest "
          "%.3g); %.1f s\n%s" % (c.name, inp.seed, n_amb, n, 100 * share, largest,
                                 time.time() - t0, "\n".join(lines)))
    assert not misses, "%s: %d misses:\n%s" % (c.name, len(misses), "\n".join(misses[:12]))
    if c.occ == "empty":
        for got in outs.values():
            assert torch.equal(got["colors"], inp.bg) and bool((got["last_trans"] == 1).all())
            assert bool((got["depths"] == 0).all()) and int(got["kept"].abs().sum()) == 0
            assert bool((got["len"] == S).all())


def test_state_is_written_whole_and_a_final_ray_is_left_alone(capi, dev):
    """Entry behaviour the existing files do not hold: after the head at n_head = 64 every ray's pending
    word is 0 or 1 -- 1 exactly for the rays still alive at sample 64 (len >= 64: a ray that keeps all
    of the head's last stride is handed on, and the tail finds its end) --, and the tail leaves the
    outputs of the rays that ended in the head as the head wrote them."""
    c = [c for c in CASES if c.name == "len-C8-S100"][0]
    inp, _, _ = M.build_case(c)
    S, n = c.S, c.n_rays
    f, net, o, d, noise, img, bg, words = _device_inputs(inp, dev)
    m = M.model(inp, _device_samples(capi, dev, inp, f, o, d, noise))
    args = lambda outs, state: (o, d, noise, f["table16"], f["primes"], f["bias"], f["mul"], net["w_h"], net["b_h"],
                                net["w1"], net["b1"], net["w2"], net["b2"], net["emb"], img, None, 0, bg, *outs, n, S,
                                inp.step, f["L"], f["F"], f["T"], f["stride"], 1e-4, 3.0, 1e-2, 64, state)
    fresh = lambda: (torch.full((n, 3), float("nan"), device=dev), torch.full((n,), float("nan"), device=dev),
                     torch.full((n,), float("nan"), device=dev), torch.full((n,), -1, dtype=torch.int32, device=dev),
                     torch.full((n,), -1, dtype=torch.int32, device=dev))
    state = torch.full((16 * n,), float("nan"), device=dev)
    head = fresh()
    capi.call("render_rays_head", *args(head, state))
    pending = state.view(torch.int32).reshape(n, 16)[:, 0].cpu().numpy()
    clear = ~m["ambiguous"]
    assert set(pending.tolist()) <= {0, 1}
    assert np.array_equal(pending[clear] == 1, m["len"][clear] >= 64)
    done = torch.from_numpy(pending == 0)
    assert bool(torch.isnan(head[0].cpu()[~done]).all()) and bool((head[3].cpu()[~done] == -1).all())
    assert bool(torch.isfinite(head[0].cpu()[done]).all())
    both = tuple(x.clone() for x in head)
    capi.call("render_rays_tail", *args(both, state))
    for a, b in zip(both, head):
        assert torch.equal(a.cpu()[done], b.cpu()[done])
    assert bool(torch.isfinite(both[0]).all()) and bool((both[3] >= 0).all())
