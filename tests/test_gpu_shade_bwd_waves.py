"""Matrix-core shade backward at two waves per SIMD in 32-sample strides (F2N_OPT_SHADE_BWD_WAVES =
2, the default from 1.5 M samples per launch; 3 with unfenced phases) against the one-wave,
64-sample-stride form (= 1) on the same inputs: the data gradient d_enc bit for bit (the per-sample
chain is the same), the parameter gradients within the rounding bound of summing the same terms in
another order."""
import pytest
import torch

from oracle import kernels as K

pytestmark = pytest.mark.gpu

E = 5


def _inputs(C, n, with_emb, img_run, seed):
    g = torch.Generator().manual_seed(seed)
    enc = (torch.randn(n, C, generator=g) * 0.1).to(torch.float16).float()
    dirs = torch.randn(n, 3, generator=g)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    img = (torch.arange(n) // img_run % E).to(torch.int32) if with_emb else None
    P = {"w_h": torch.randn(16, C, generator=g) * 0.3, "b_h": torch.randn(16, generator=g) * 0.1,
         "w1": torch.randn(64, 32, generator=g) * 0.3, "b1": torch.randn(64, generator=g) * 0.1,
         "w2": torch.randn(3, 64, generator=g) * 0.3, "b2": torch.randn(3, generator=g) * 0.1,
         "emb": torch.randn(E, 16, generator=g) * 0.1}
    d_logit = torch.randn(n, generator=g)
    d_rgb = torch.randn(n, 3, generator=g)
    return enc, dirs, img, P, d_logit, d_rgb


def _run_both(capi, dev, C, n, with_emb, img_run, calls=1, arms=(2, 1)):
    """shade_bwd under each F2N_OPT_SHADE_BWD_WAVES value of `arms` on the same inputs"""
    enc, dirs, img, P, d_logit, d_rgb = _inputs(C, n, with_emb, img_run, C * 7919 + n)
    dv = lambda t: t.to(dev).contiguous()
    enc_cm, dirs_d, d_logit_d, d_rgb_d = dv(enc.t()), dv(dirs), dv(d_logit), dv(d_rgb)
    Pd = {k: dv(v) for k, v in P.items()}
    img_d = dv(img) if with_emb else None
    emb = Pd["emb"] if with_emb else None
    out = {}
    try:
        capi.set_option("SHADE_BWD", 0)
        for waves in arms:
            capi.set_option("SHADE_BWD_WAVES", waves)
            G = {k: torch.zeros_like(v) for k, v in Pd.items()}
            d_encs = []
            for _ in range(calls):
                d_enc = torch.full((C, n), 7.0, device=dev)  # must be overwritten
                capi.call("shade_bwd", enc_cm, C, dirs_d, img_d, Pd["w_h"], Pd["b_h"], Pd["w1"],
                          Pd["b1"], Pd["w2"], Pd["b2"], emb, d_logit_d, d_rgb_d, d_enc, G["w_h"],
                          G["b_h"], G["w1"], G["b1"], G["w2"], G["b2"],
                          G["emb"] if with_emb else None, None, n)
                d_encs.append(d_enc)
            torch.cuda.synchronize()
            out[waves] = (d_encs, G)
    finally:
        capi.set_option("SHADE_BWD_WAVES", 0)
    out["inputs"] = (enc, dirs, img, P, d_logit, d_rgb, calls)
    return out


def _abs_terms_f64(enc, dirs, img, P, d_logit, d_rgb, calls):
    """Per parameter-gradient element, the sum over samples of |term| (float64, CPU): every order in
    which a kernel adds the same float32 terms lands within D * 2^-24 * this of the exact sum, D the
    number of roundings on the longest path of a term (SH basis from the oracle, then widened)."""
    P = {k: v.double() for k, v in P.items()}
    enc = enc.double()
    h = enc @ P["w_h"].t() + P["b_h"]
    X16 = torch.cat([torch.ones_like(h[:, :1]), h[:, 1:]], 1)
    if img is not None:
        X16 = X16 + P["emb"][img.long()]
    X = torch.cat([X16, K.sh_encode(dirs, 4).double()], 1)
    pre = X @ P["w1"].t() + P["b1"]
    hid = torch.relu(pre)
    sg = torch.sigmoid(hid @ P["w2"].t() + P["b2"])
    d_o = (d_rgb.double() * (1 + 2e-3) * sg * (1 - sg)).abs()
    d_hid = ((d_o @ P["w2"].abs()) * (pre > 0)).abs()  # |d_o W2| <= |d_o| |W2|
    d_X = d_hid @ P["w1"][:, :16].abs()
    d_h = d_X.clone()
    d_h[:, 0] = d_logit.double().abs()
    A = {"w2": d_o.t() @ hid, "b2": d_o.sum(0), "w1": d_hid.t() @ X.abs(), "b1": d_hid.sum(0),
         "w_h": d_h.t() @ enc.abs(), "b_h": d_h.sum(0)}
    if img is not None:
        A["emb"] = torch.zeros_like(P["emb"]).index_add_(0, img.long(), d_X)
    return {k: calls * v for k, v in A.items()}


def _check(out, with_emb, arms=(2, 1)):
    """d_enc bit for bit; each parameter-gradient element of the two forms within the worst-case
    rounding bound of two float32 sums of the same terms in different orders (fixed in advance, not
    a statistical tolerance).  Roundings on a term's path, at most: one per sample a wave handles
    (n / 1024 + 64: at least 1024 waves share the strides, or one stride per wave), 64 for the
    product and the lane, quarter and k-step sums of its stride, 8 for the workgroup meet, 256 float
    atomics (one per workgroup); the embedding gradient adds one atomic per sample where ids change
    inside a stride and one per wave otherwise: n + 2048."""
    (d_new, G_new), (d_old, G_old) = out[arms[0]], out[arms[1]]
    for a, b in zip(d_new, d_old):
        assert torch.equal(a, b), "d_enc differs: %g" % float((a - b).abs().max())
    inputs = out["inputs"]
    n, calls = inputs[0].shape[0], inputs[-1]
    A = _abs_terms_f64(*inputs)
    for k in ("w_h", "b_h", "w1", "b1", "w2", "b2") + (("emb",) if with_emb else ()):
        D = (n // 1024 + 64) + 64 + 8 + 256 + ((n + 2048) if k == "emb" else 0)
        # two sums, each within D u sum|t| of the exact one; x2 for the float32 terms against the
        # float64 ones they are bounded by, x calls for accumulating calls
        tol = 2 * 2 * calls * D * 2.0 ** -24 * A[k]
        diff = (G_new[k].cpu().double() - G_old[k].cpu().double()).abs()
        bad = diff > tol
        assert not bool(bad.any()), (k, int(bad.sum()), float((diff - tol).max()))


@pytest.mark.parametrize("C", [8, 16, 32, 64])
@pytest.mark.parametrize("n", [1, 31, 33, 64 * 9 + 17, 64 * 2100 + 5])
@pytest.mark.parametrize("with_emb", [True, False])
def test_shade_bwd_two_waves_matches_one_wave(capi, dev, C, n, with_emb):
    _check(_run_both(capi, dev, C, n, with_emb, img_run=37), with_emb)


@pytest.mark.parametrize("C", [8, 32])
def test_shade_bwd_two_waves_accumulates(capi, dev, C):
    """A second call adds to the parameter gradients and rewrites d_enc."""
    out = _run_both(capi, dev, C, 64 * 300 + 9, True, img_run=37, calls=2)
    _check(out, True)
    assert torch.equal(out[2][0][0], out[2][0][1])


@pytest.mark.parametrize("C", [16, 32])
@pytest.mark.parametrize("n", [33, 64 * 2100 + 5])
def test_shade_bwd_two_waves_mixed_phases(capi, dev, C, n):
    """F2N_OPT_SHADE_BWD_WAVES = 3: the two-wave form with the phases of a stride not fenced."""
    arms = (3, 1)
    _check(_run_both(capi, dev, C, n, True, img_run=37, arms=arms), True, arms=arms)


@pytest.mark.parametrize("img_run", [1, 5, 13, 16, 31])
def test_shade_bwd_two_waves_image_changes(capi, dev, img_run):
    """Image ids that change inside a 32-sample stride, and runs that span strides: the embedding
    gradient is flushed on every change of id."""
    _check(_run_both(capi, dev, 32, 64 * 40 + 21, True, img_run=img_run), True)

