"""Every route of the per-sample network kernels (f2n_shade_fwd, f2n_shade_bwd, f2n_shade_fwd_rays,
f2n_shade_bwd_rays) against the float64 restatement of tests/shade_model.py, element by element:
|got - f64| <= 2 E with E the worst-case rounding bound counted there from the kernels' code (exactly 0
where E = 0).  The bound's own checks are tests/test_shade_model_cpu.py.  Each test prints the largest
|err| / E per route and output (-s): how much of the room the kernels use."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from tests import shade_model as M

pytestmark = pytest.mark.gpu

CASES = M.cases()
FWD_CASES = [c for c in CASES if c.kind != "bwd"]
BWD_CASES = [c for c in CASES if c.kind != "fwd"]
W_KEYS = ("w_h", "b_h", "w1", "b1", "w2", "b2")


@functools.lru_cache(maxsize=None)
def _case(c):
    """inputs and float64 model of one case, built once and shared (read only)"""
    return M.build_case(c)


@contextlib.contextmanager
def _options(capi, **opts):
    with contextlib.ExitStack() as stack:
        for name, value in opts.items():
            stack.enter_context(capi.option(name, value))
        yield


class _Report:
    """collects |err| / E per (route, output); every miss is named at the end"""

    def __init__(self, c, m):
        self.c, self.m, self.lines, self.misses = c, m, [], []

    def hold(self, route, got, factor=1.0):
        """got: {output: tensor shaped as the model's}; factor 2: after a second, accumulating call"""
        parts = []
        for key, value in got.items():
            ref, E = factor * self.m[key], factor * self.m["E"][key]
            r = M.ratio(value.detach().cpu(), ref, E)
            if key == "d_enc":       # samples with an ambiguous ReLU are not compared, here only
                r = torch.where(self.m["keep"][:, None], r, torch.zeros_like(r))
            worst = float(r.max())
            parts.append("%s %.3f" % (key, worst))
            if not worst <= M.BAR:
                at = [int(i) for i in np.unravel_index(int(torch.argmax(r)), tuple(r.shape))]
                self.misses.append("%s: %s%s |err|/E = %g" % (route, key, at, worst))
        self.lines.append("  %-28s %s" % (route + ("" if factor == 1.0 else " x%d" % factor), ", ".join(parts)))

    def close(self):
        print("\n%s: largest |err| / E\n%s" % (M.case_id(self.c), "\n".join(self.lines)))
        assert not self.misses, "%s: outside 2 E:\n%s" % (M.case_id(self.c), "\n".join(self.misses))


def _device(inp, dev):
    dv = lambda t: None if t is None else t.to(dev).contiguous()
    d = {k: dv(v) for k, v in inp.P.items()}
    d.update(enc_cm=dv(inp.enc.t()), dirs=dv(inp.dirs), img=dv(inp.img), ray_img=dv(inp.ray_img),
             d_logit=dv(inp.d_logit), d_rgb=dv(inp.d_rgb))
    if inp.img is None:
        d["emb"] = None
    return d


def _weights(d):
    return tuple(d[k] for k in W_KEYS) + (d["emb"],)


def _forward(capi, dev, inp, d, want_pre):
    """one forward call into buffers prefilled with 7.0 -> {output: tensor shaped as the model's}"""
    n = inp.n
    logit = torch.full((n,), 7.0, device=dev)
    rgb = torch.full((n, 3), 7.0, device=dev)
    pre_cm = torch.full((64, n), 7.0, device=dev) if want_pre else None
    if inp.S:
        capi.call("shade_fwd_rays", d["enc_cm"], inp.C, d["dirs"], d["ray_img"], *_weights(d), logit, rgb,
                  inp.n_rays, inp.S)
    else:
        capi.call("shade_fwd", d["enc_cm"], inp.C, d["dirs"], d["img"], *_weights(d), logit, rgb, pre_cm, n)
    out = {"logit": logit, "rgb": rgb}
    if want_pre:
        out["pre"] = pre_cm.t()
    return out, pre_cm


@pytest.mark.parametrize("c", FWD_CASES, ids=M.case_id)
def test_shade_forward_routes(capi, dev, c):
    inp, m = _case(c)
    d = _device(inp, dev)
    rep = _Report(c, m)
    if c.kind == "rays":
        rep.hold("shade_fwd_rays", _forward(capi, dev, inp, d, False)[0])
    else:
        for variant in (0, 2, 3):     # four, two, three waves per SIMD
            with _options(capi, SHADE_FWD=0, SHADE_VARIANT=variant):
                rep.hold("mfma variant %d + pre_cm" % variant, _forward(capi, dev, inp, d, True)[0])
        with _options(capi, SHADE_FWD=1):
            rep.hold("vector + pre_cm", _forward(capi, dev, inp, d, True)[0])
            rep.hold("vector", _forward(capi, dev, inp, d, False)[0])
        with _options(capi, SHADE_FWD=0, SHADE_VARIANT=0):
            rep.hold("mfma", _forward(capi, dev, inp, d, False)[0])
    rep.close()


def _backward_twice(capi, dev, inp, d, pre_cm, rep, route):
    """two accumulating calls: d_enc (prefilled with 7.0, rewritten each time) and the parameter
    gradients after the first, the same at twice the bound after the second"""
    n, C = inp.n, inp.C
    keys = W_KEYS + (("emb",) if inp.img is not None else ())
    G = {k: torch.zeros_like(d[k]) for k in keys}
    g_all = tuple(G[k] for k in W_KEYS) + (G.get("emb"),)
    for call in (1, 2):
        d_enc = torch.full((C, n), 7.0, device=dev)
        if inp.S:
            capi.call("shade_bwd_rays", d["enc_cm"], C, d["dirs"], d["ray_img"], *_weights(d), d["d_logit"],
                      d["d_rgb"], d_enc, *g_all, inp.n_rays, inp.S)
        else:
            capi.call("shade_bwd", d["enc_cm"], C, d["dirs"], d["img"], *_weights(d), d["d_logit"], d["d_rgb"],
                      d_enc, *g_all, pre_cm, n)
        rep.hold(route if call == 1 else route + ", call 2", {"d_enc": d_enc.t()})
        rep.hold(route, {"g_" + k: G[k] for k in keys}, factor=float(call))


@pytest.mark.parametrize("c", BWD_CASES, ids=M.case_id)
def test_shade_backward_routes(capi, dev, c):
    inp, m = _case(c)
    d = _device(inp, dev)
    rep = _Report(c, m)
    if c.kind == "rays":
        for waves in (1, 2, 3):
            with _options(capi, SHADE_BWD_WAVES=waves):
                _backward_twice(capi, dev, inp, d, None, rep, "shade_bwd_rays waves %d" % waves)
    else:
        for waves, variant in ((1, 0), (1, 1), (2, 0), (3, 0)):   # one wave mixed / fenced, two fenced / mixed
            with _options(capi, SHADE_BWD=0, SHADE_BWD_WAVES=waves, SHADE_VARIANT=variant):
                _backward_twice(capi, dev, inp, d, None, rep, "mfma waves %d variant %d" % (waves, variant))
        with _options(capi, SHADE_FWD=0, SHADE_VARIANT=0):
            pre_cm = _forward(capi, dev, inp, d, True)[1]
        with _options(capi, SHADE_BWD=1):
            _backward_twice(capi, dev, inp, d, None, rep, "vector, recomputed")
            _backward_twice(capi, dev, inp, d, pre_cm, rep, "vector, saved pre_cm")
    rep.close()
