"""The float64 model of tests/density_grad_model.py, checked without a GPU: (i) it is the gradient of
the forward's interpolant (central differences), (ii) a float32 restatement in the kernel's order stays
inside the bound, (iii) the bound rejects wrong formulas, (iv) the generator reaches its input
conditions with nothing left out.

Eligibility in (iii).  Every mutant must leave 2 E on EVERY eligible sample or ray.  Eligibility is decided
from the inputs and the float64 model alone:
  per sample                the term the mutation changes, taken by itself in float64 and carried to the
                            raw frame through the contraction's (linear) Jacobian, exceeds TERM_OVER_E = 4
                            times the sample's bound E_g in some component.  The term: q5 -- Q5's vector
                            minus the gradient; flip -- twice the flipped component; no_mul -- the
                            level's contribution times (1 - 1 / mul_l); swap -- the level's contribution
                            with the channels reversed minus the one as it is (F >= 2 only; both at the
                            middle and the finest level); identity_jac -- G - J G, samples with
                            |p| > 1.01 only.  A sample whose changed term lies inside its own rounding
                            cannot tell the two formulas apart and is not eligible.
  no_weight, no_norm, plus_g   rays with at least one sample and no NaN sample
  drop_last_stride          such rays whose length is no multiple of 64
Every mutant must find at least 50 eligible samples (60 rays), and at least half of the samples it
can change at all, so that the rule is never met by leaving everything out."""
import numpy as np
import pytest
import torch

from tests import density_grad_model as M

CASES = M.cases()
POINT_CASES = [c for c in CASES if c.kind == "points"]
RAY_CASES = [c for c in CASES if c.kind == "rays"]
# one case per (F, L) is enough for the CPU-side checks that cost a model evaluation per mutant
MUTANT_POINT_CASES = [c for c in POINT_CASES if c.tag == "n200" and c.T == 1 << 14 and not c.disjoint]


TERM_OVER_E = 4.0


def _outside(ratio):
    return (ratio > M.BAR).any(1)


@pytest.mark.parametrize("c", MUTANT_POINT_CASES, ids=M.case_id)
def test_model_is_the_gradient_of_the_interpolant(c):
    """(i) central differences of the forward's float64 restatement, h = 1e-6 cell units of the finest
    level, inside one cell: in the contracted frame against G, every axis; and g against G through
    central differences of the contraction, inside and outside the ball."""
    b = M.build_case(c)
    fld, m = b.fld, b.m
    w0 = fld["w0"].numpy()
    ok = ~m["zero"]
    x, feat = m["x"][ok], m["feat"][ok]
    h = 1e-6 / float(fld["mul"][-1])
    scale = np.abs(m["G"][ok]).max(1)
    for ax in range(3):
        e = np.zeros(3)
        e[ax] = h
        fd = (M.interpolant(fld, feat, x, w0, e) - M.interpolant(fld, feat, x, w0, -e)) / (2 * h)
        assert np.abs(fd - m["G"][ok, ax]).max() <= 1e-6 * scale.max(), (M.case_id(c), ax)
        assert (np.abs(fd - m["G"][ok, ax]) <= 1e-6 * np.maximum(scale, 1e-30) + 1e-9 * scale.max()).all()
    # raw frame, by the chain rule: the contraction's own central differences (relative step 1e-5:
    # truncation 1e-10, cancellation 1e-11) times G against g, inside and outside the ball
    p = b.pts.numpy().astype(np.float64)[ok]

    def contract(q):
        n = np.linalg.norm(q, axis=1, keepdims=True)
        return np.where(n <= 1.0, q, (2.0 - 1.0 / n) * q / n)

    nrm = np.linalg.norm(p, axis=1)
    use = np.abs(nrm - 1.0) > 1e-3          # a step across |p| = 1 would straddle the two branches
    G = m["G"][ok]
    for ax in range(3):
        e = np.zeros_like(p)
        e[:, ax] = 1e-5 * nrm
        col = (contract(p + e) - contract(p - e)) / (2 * e[:, ax:ax + 1])      # d x_i / d p_ax
        fd, size = (col * G).sum(1), (np.abs(col) * np.abs(G)).sum(1)
        err = np.abs(fd - m["g"][ok, ax])
        assert (err[use] <= 1e-6 * size[use]).all(), (M.case_id(c), ax, float((err / size)[use].max()))
    assert (nrm > 1.0).any() and (nrm < 1.0).any()


def _f32_grad(fld, pts, w0):
    """density_grad.hiph in float32 numpy, operation for operation -> g [n, 3] float32"""
    f = np.float32
    L, F, stride = fld["L"], fld["F"], fld["stride"]
    p = pts.numpy().astype(f)
    x = M.contract_f32(pts)
    zero = np.isnan(x).any(1)
    x[zero] = 0
    rows = M.corner_rows(fld, x)
    tab = fld["table16"].numpy().view(np.float16)
    w0 = np.asarray(w0, dtype=f).reshape(L, F)
    g = np.zeros((p.shape[0], 3), dtype=f)

    def fma(a, b, c):
        return (a.astype(np.float64) * np.asarray(b, dtype=np.float64) + c.astype(np.float64)).astype(f)

    for l in range(L):
        mul, bias = f(float(fld["mul"][l])), fld["bias"][l].numpy().astype(f)
        pos = fma(x, mul, np.broadcast_to(bias, x.shape))
        fr = pos - np.floor(pos)
        cm = f(1) - fr
        feat = tab[stride * l + rows[:, l, :, None] * F + np.arange(F)].astype(f)      # [n, 8, F]
        s = feat[:, :, 0] * w0[l, 0]
        for k in range(1, F):
            s = fma(feat[:, :, k], w0[l, k], s)
        for ax in range(3):
            a, b = M._OTHER[ax]
            wg = (cm[:, a] * cm[:, b], cm[:, a] * fr[:, b], fr[:, a] * cm[:, b], fr[:, a] * fr[:, b])
            t = None
            for j, (hi, lo) in enumerate(M._PAIRS[ax]):
                d = s[:, hi] - s[:, lo]
                t = d * wg[j] if t is None else fma(d, wg[j], t)
            g[:, ax] = fma(t, mul, g[:, ax])
    n2 = fma(p[:, 2], p[:, 2], fma(p[:, 1], p[:, 1], p[:, 0] * p[:, 0]))
    nrm = np.sqrt(n2)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = f(1) / nrm
        ja = (f(2) - inv) * inv
        da = (f(2) * inv - f(2)) * inv * inv * inv
        pg = fma(p[:, 2], g[:, 2], fma(p[:, 1], g[:, 1], p[:, 0] * g[:, 0]))
        cc = da * pg
        out = np.stack([fma(cc, p[:, a], ja * g[:, a]) for a in range(3)], 1)
    out = np.where((nrm <= 1)[:, None], g, out)
    out[nrm == 0] = np.nan
    return out


def _f32_rays(bounds, weights, g):
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        ln = np.sqrt((g[:, 2].astype(np.float64) * g[:, 2] + (g[:, 1].astype(np.float64) * g[:, 1] + (g[:, 0] * g[:, 0]).astype(f)).astype(f)).astype(f))
        nh = -g / ln[:, None]
    nh[(g == 0).all(1)] = 0
    b = bounds.numpy()
    w = weights.numpy().astype(f)
    out = np.zeros((b.shape[0], 3), dtype=f)
    for r, (s, e) in enumerate(b):
        lanes = np.zeros((64, 3), dtype=f)
        for c in range(s, e, 64):
            k = min(64, e - c)
            lanes[:k] = (w[c:c + k, None].astype(np.float64) * nh[c:c + k] + lanes[:k]).astype(f)
        acc = f(0) * lanes[0]
        for lane in range(64):              # an order of our own: any order lies within the bound
            acc = acc + lanes[lane]
        out[r] = acc
    return out


@pytest.mark.parametrize("c", CASES, ids=M.case_id)
def test_float32_restatement_stays_within_the_bound(c):
    """(ii) and (iv): the kernel's operations in float32 numpy against the float64 model, and the
    generator's input conditions with nothing left out."""
    b = M.build_case(c)
    amb, flat = M.conditions(b)
    assert amb == 0 and flat == 0, (M.case_id(c), amb, flat)
    assert b.redrawn < 0.5
    g32 = _f32_grad(b.fld, b.pts, b.fld["w0"].numpy())
    r = M.ratio(g32, b.m["g"], b.m["E_g"])
    worst = float(r.max())
    if c.kind == "rays":
        N32 = _f32_rays(b.bounds, b.weights, g32)
        rn = M.ratio(N32, b.m["N"], b.m["E_N"])
        worst = max(worst, float(rn.max()))
        if c.tag == "w0zero":
            assert (b.m["N"] == 0).all() and (b.m["E_N"] == 0).all() and (b.m["g"] == 0).all()
        if c.tag == "nan":
            bad = np.isnan(b.m["N"]).any(1)
            assert bad.tolist() == [False, True, False, False, False]
    print("\n%s: largest |err| / E of the float32 restatement %.3f" % (M.case_id(c), worst))
    assert worst <= M.BAR, (M.case_id(c), worst)
    if c.tag in ("n200", "n1000"):
        assert np.isnan(b.m["g"]).any(1).sum() == 1            # the origin, and it alone
        assert b.m["pos_min"] < 0                              # Q1: negative pt at the fine levels


@pytest.mark.parametrize("c", MUTANT_POINT_CASES, ids=M.case_id)
def test_bound_rejects_wrong_gradients(c):
    """(iii), per sample"""
    b = M.build_case(c)
    fld, m = b.fld, b.m
    finite = ~m["zero"]
    nrm = np.linalg.norm(b.pts.numpy().astype(np.float64), axis=1)
    muts = ["q5", ("flip", 0), ("flip", 1), ("flip", 2), ("no_mul", fld["L"] // 2), ("no_mul", fld["L"] - 1), "identity_jac"]
    if fld["F"] >= 2:
        muts += [("swap", fld["L"] // 2), ("swap", fld["L"] - 1)]
    for mut in muts:
        mm = M.point_model(fld, b.pts, mut=mut)
        if mut == "identity_jac":
            can, term = finite & (nrm > 1.01), m["G"] - m["g"]
        else:        # the changed term in the contracted frame, through the Jacobian on its own
            can = finite
            term = M.contract_bwd_model(b.pts, mm["G"] - m["G"], np.zeros_like(m["G"]))[0]
        with np.errstate(invalid="ignore"):
            elig = can & (np.abs(term) > TERM_OVER_E * m["E_g"]).any(1)
        assert elig.sum() >= 50 and elig.sum() >= 0.5 * can.sum(), (M.case_id(c), mut, int(elig.sum()), int(can.sum()))
        out = _outside(M.ratio(mm["g"], m["g"], m["E_g"]))[elig]
        assert out.all(), (M.case_id(c), mut, int((~out).sum()), int(elig.sum()))


@pytest.mark.parametrize("c", [c for c in RAY_CASES if c.tag == "mixed130"], ids=M.case_id)
def test_bound_rejects_wrong_rays(c):
    """(iii), per ray"""
    b = M.build_case(c)
    m = b.m
    length = (b.bounds[:, 1] - b.bounds[:, 0]).numpy()
    for mut in ("no_weight", "no_norm", "plus_g", "drop_last_stride"):
        nh, E_nh = M.normal_model(m["g"], m["E_g"], mut)
        N, _ = M.ray_model(b.bounds, b.weights, nh, E_nh, mut)
        elig = length > 0
        if mut == "drop_last_stride":
            elig = elig & (length % 64 != 0)
        assert elig.sum() >= 60
        out = _outside(M.ratio(N, m["N"], m["E_N"]))[elig]
        assert out.all(), (M.case_id(c), mut, int((~out).sum()))


def test_cases_cover_what_they_claim(capi):
    for c in CASES:          # every case is one the C ABI accepts (checked before any HIP work: n = 0)
        b = M.build_case(c)
        stride = b.fld["stride"]
        assert stride == (c.T * c.F if c.disjoint else c.T)
        assert capi.lib().cdll.f2n_density_grad(None, None, None, None, None, None, None, 0, c.L, c.F, c.T,
                                                stride, None) == 0, M.case_id(c)
    assert {c.F for c in CASES} == {1, 2, 4, 8} and {c.L for c in CASES} == {4, 16, 32}
    assert {(c.F, c.L) for c in CASES if c.L == 32} == {(2, 32)}
    assert {c.T for c in CASES} == {1 << 14, 12289} and {c.disjoint for c in CASES} == {False, True}
    assert {int(c.tag[1:]) for c in POINT_CASES} == {1, 63, 64, 65, 200, 1000}
    b = M.build_case([c for c in RAY_CASES if c.tag == "mixed130"][0])
    length = (b.bounds[:, 1] - b.bounds[:, 0]).tolist()
    assert len(length) == 130 and set(length) == set(M.SEG_LENGTHS)
    assert M.build_case([c for c in RAY_CASES if c.tag == "one"][0]).bounds.shape[0] == 1
    assert torch.equal(M.build_case([c for c in RAY_CASES if c.tag == "w0zero"][0]).fld["w0"],
                       torch.zeros(32))
