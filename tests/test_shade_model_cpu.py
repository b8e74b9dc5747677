"""tests/shade_model.py on the CPU: the closed-form float64 gradients against autograd, the bound
against an independent float32 evaluation (not too tight), the cap on ambiguous samples, and changes
a wrong kernel could make that the bound must reject (it has teeth).  Run with -s for the figures."""
import functools

import pytest
import torch

from oracle import kernels as K
from tests import shade_model as M

FWD = ("logit", "pre", "rgb")
CASES = M.cases()


@functools.lru_cache(maxsize=None)
def _built(c):
    return M.build_case(c)


def _compose(inp, sh, dtype):
    """The op-by-op torch composition of tests/test_gpu_shade.py::_reference in `dtype`, gradients by
    autograd -> dict keyed as the model's outputs."""
    enc = inp.enc.detach().clone().to(dtype).requires_grad_(True)
    P = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in inp.P.items()}
    h = enc @ P["w_h"].t() + P["b_h"]
    logit = h[:, 0]
    X = torch.cat([torch.ones_like(h[:, :1]), h[:, 1:]], 1)
    if inp.img is not None:
        X = X + P["emb"][inp.img.long()]
    X = torch.cat([X, sh.to(dtype)], 1)
    pre = X @ P["w1"].t() + P["b1"]
    o = torch.relu(pre) @ P["w2"].t() + P["b2"]
    rgb = (1 + 2 * 1e-3) / (1 + torch.exp(-o)) - 1e-3
    out = {"logit": logit.detach(), "pre": pre.detach(), "rgb": rgb.detach()}
    ((logit * inp.d_logit.to(dtype)).sum() + (rgb * inp.d_rgb.to(dtype)).sum()).backward()
    out["d_enc"] = enc.grad
    for k in M.GRAD_KEYS:
        if k != "emb" or inp.img is not None:
            out["g_" + k] = P[k].grad
    return out


def _outputs(c, m):
    keys = list(FWD)
    if c.kind != "fwd":
        keys += ["d_enc"] + ["g_" + k for k in M.GRAD_KEYS if k != "emb" or c.with_emb]
    return keys


def _share_outside(got, m, key):
    rows = m["keep"] if key == "d_enc" else None
    r = M.ratio(got, m[key], m["E"][key], rows)
    return float((r > M.BAR).double().mean())


@pytest.mark.parametrize("c", [c for c in CASES if c.kind != "fwd" and (c.n == 64 * 9 + 17 or c.kind == "rays")],
                         ids=M.case_id)
def test_closed_form_matches_autograd(c):
    """float64 autograd through the same expressions (the model's own SH values, its float32
    constants): every closed-form gradient within 1e-12 of its element's A."""
    inp, m = _built(c)
    enc = inp.enc.detach().double().requires_grad_(True)
    P = {k: v.detach().double().requires_grad_(True) for k, v in inp.P.items()}
    h = enc @ P["w_h"].t() + P["b_h"]
    X = torch.cat([torch.ones_like(h[:, :1]), h[:, 1:]], 1)
    if inp.img is not None:
        X = X + P["emb"][inp.img.long()]
    X = torch.cat([X, M.sh16(inp.dirs)[0]], 1)
    pre = X @ P["w1"].t() + P["b1"]
    rgb = M.C32 * torch.sigmoid(torch.relu(pre) @ P["w2"].t() + P["b2"]) - M.EPS32
    ((h[:, 0] * inp.d_logit.double()).sum() + (rgb * inp.d_rgb.double()).sum()).backward()
    got = {"d_enc": enc.grad}
    got.update({"g_" + k: P[k].grad for k in M.GRAD_KEYS if k != "emb" or c.with_emb})
    for key in ("logit", "pre", "rgb"):
        got[key] = {"logit": h[:, 0], "pre": pre, "rgb": rgb}[key].detach()
    for key, v in got.items():
        excess = (v - m[key]).abs() - 1e-12 * m["A"][key]
        assert float(excess.max()) <= 0, (key, float(excess.max()))


@pytest.mark.parametrize("c", CASES, ids=M.case_id)
def test_bound_admits_float32_composition(c):
    """Another order of operations, an independent SH (the oracle's): inside BAR * E everywhere, and
    no case leaves out more than MAX_AMBIGUOUS of its samples (build_case asserts it)."""
    inp, m = _built(c)
    assert m["ambiguous_share"] <= M.MAX_AMBIGUOUS
    assert c.n > 65 or bool(m["keep"].all())
    got = _compose(inp, K.sh_encode(inp.dirs, 4), torch.float32)
    line = []
    for key in _outputs(c, m):
        r = M.ratio(got[key], m[key], m["E"][key], m["keep"] if key == "d_enc" else None)
        worst = float(r.max()) if r.numel() else 0.0
        line.append("%s %.3f" % (key, worst))
        assert worst <= M.BAR, (M.case_id(c), key, worst)
    print("\n%s: ambiguous %.3f %%; max |err|/E: %s" % (M.case_id(c), 100 * m["ambiguous_share"], ", ".join(line)))


def test_zero_bound_means_zero():
    """Rows whose d_logit and d_rgb are zero have E = 0 in d_enc: the value must be exactly 0."""
    c = [c for c in CASES if c.kind == "edge"][0]
    inp, m = _built(c)
    dead = (inp.d_logit == 0) & (inp.d_rgb == 0).all(1)
    assert int(dead.sum()) >= 50
    assert float(m["E"]["d_enc"][dead].max()) == 0.0 and float(m["d_enc"][dead].abs().max()) == 0.0
    r = M.ratio(torch.full_like(m["d_enc"], 1e-30), m["d_enc"], m["E"]["d_enc"])
    assert bool(torch.isinf(r[dead]).all())


def test_edge_case_saturates():
    c = [c for c in CASES if c.kind == "edge"][0]
    _, m = _built(c)
    top = float(m["o"].abs().max())
    print("\nedge case: max |o| = %.2f" % top)
    assert 15.0 <= top <= 30.0


# ---- the bound has teeth: each change must put >= 1 % of the compared elements of each output it is
# checked on outside BAR * E, at one shape at least

TEETH_SHAPES = [c for c in CASES if c.n == 64 * 9 + 17 or c.tag in ("run5", "run1") or c.kind == "bwd"
                or (c.kind == "rays" and c.S == 128)]


def _first_of_run_takes_previous(img):
    img2 = img.clone()
    starts = torch.nonzero(img[1:] != img[:-1]).flatten() + 1
    img2[starts] = img[starts - 1]
    return img2


def _denc_f16(inp, m):
    """d_enc rounded to f16"""
    return {"d_enc": m["d_enc"].half().double()}


def _w1_11bit(inp, m):
    """pre with w1 rounded to an 11-bit significand (f16's; |w1| lies far inside its range)"""
    return {"pre": m["X"] @ inp.P["w1"].half().double().t() + inp.P["b1"].double()}


def _rgb_unwidened(inp, m):
    """rgb = sigmoid(o) - eps, without the (1 + 2 eps)"""
    return {"rgb": torch.sigmoid(m["o"]) - M.EPS32}


KY31_CHANGES = {"ky31": 5e-5, "ky31 by one unit": 1e-5}      # 0.45704580 -> 0.45709580 / 0.45705580


@functools.lru_cache(maxsize=None)
def _remodelled(c, what):
    inp, _ = _built(c)
    if what in KY31_CHANGES:
        return M.model(inp, consts=dict(M.SH_CONSTS, kY31=M.SH_CONSTS["kY31"] + KY31_CHANGES[what]))
    return M.model(inp._replace(img=_first_of_run_takes_previous(inp.img)))


def _ky31(inp, m, c, what="ky31"):
    """kY31 changed in its fifth significant digit (4 -> 9)"""
    m2 = _remodelled(c, what)
    return {"pre": m2["pre"], "g_w1[:, 16:]": m2["g_w1"]}


def _emb_row(inp, m, c):
    """the first sample of every id run takes the previous sample's embedding row"""
    if inp.img is None:
        return None
    m2 = _remodelled(c, "emb")
    return {"g_emb": m2["g_emb"], "rgb": m2["rgb"]}


def _b1_drops_stride_end(inp, m):
    """d b1 without the last sample of every 64-sample stride"""
    return {"g_b1": m["d_hid"][torch.arange(inp.n) % 64 != 63].sum(0)}


TEETH = [(_denc_f16, "d_enc"), (_w1_11bit, "pre"), (_rgb_unwidened, "rgb"), (_ky31, "pre"),
         (_ky31, "g_w1[:, 16:]"), (_emb_row, "g_emb"), (_emb_row, "rgb"), (_b1_drops_stride_end, "g_b1")]


@pytest.mark.parametrize("change,output", TEETH, ids=["%s-%s" % (f.__name__[1:], o) for f, o in TEETH])
def test_bound_rejects(change, output):
    """As run, the share outside the bound at the best shape: d_enc in f16 16.2 % (C = 16; 3.9 % at
    C = 32, n = 134 405; 1.0 % at C = 64), w1 at 11 bits 94 %, rgb unwidened 100 %, the embedding row
    100 % of d emb and 99.9 % of rgb (runs of 1), d b1 97 %, kY31 47 % of pre and 1.6 % of
    d w1[:, 16:] (two of its 16 columns move; ray-uniform form, C = 8).

    kY31 moved by ONE unit of that digit (4 -> 5, printed, not asserted) reaches 0.84 % of pre at best
    and nothing of d w1, and no bound of this kind can do better.  On pre two of 33 terms move by
    2.2e-5 of themselves against gamma(33) = 2.0e-6 of all 33: only the tail of the weights gets there.
    On d w1 an element moves by 2.2e-5 |G| <= 2.2e-5 sum |a| |b|, while sum E_a |b| alone is about
    1e-4 sum |a| |b|: E_a / |a| is the relative error of d_o, which the interval rule takes from
    E_o ~ 15 E_pre."""
    key = "g_w1" if output.startswith("g_w1") else output
    best = 0.0
    for c in TEETH_SHAPES:
        inp, m = _built(c)
        got = change(inp, m, c) if change in (_ky31, _emb_row) else change(inp, m)
        if got is None:
            continue
        r = M.ratio(got[output], m[key], m["E"][key], m["keep"] if key == "d_enc" else None)
        if output == "g_w1[:, 16:]":
            r = r[:, 16:]
        share = float((r > M.BAR).double().mean())
        print("\n%s, %s at %s: %.2f %% outside the bound" % (change.__doc__, output, M.case_id(c), 100 * share))
        best = max(best, share)
        if change is _ky31:
            one = M.ratio(_ky31(inp, m, c, "ky31 by one unit")[output], m[key], m["E"][key])
            one = one[:, 16:] if output == "g_w1[:, 16:]" else one
            print("   by one unit of that digit: %.2f %%" % (100 * float((one > M.BAR).double().mean())))
    assert best >= 0.01, (change.__doc__, output, best)
