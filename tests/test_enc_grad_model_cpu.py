"""The float64 model of tests/enc_grad_model.py, checked without a GPU: (i) it is the gradient of the
forward's interpolant with per-sample weights (central differences), (ii) with every row of g equal to
w0 it is density_grad_model.point_model, (iii) a float32 restatement in the kernels' order stays inside
the bound, (iv) the bound rejects wrong formulas -- the Q5 form the existing kernels compute among them,
(v) the case builder terminates with every case full.

Eligibility in (iv), density_grad_model's own rule.  Every mutant must leave 2 E on EVERY eligible sample
or ray, must find at least 50 of them, and at least half of those it can change at all.  Decided from
the inputs and the float64 model alone:
  per sample   the term the mutation changes, by itself in float64 and carried to the raw frame through
               the contraction's (linear) Jacobian, exceeds TERM_OVER_E = 4 times the sample's bound E_dp
               in some component.  It can change: every finite sample (swap_chan: F >= 2 only;
               identity_jac: |p| > 1.01 only).
  per ray      the same of d_o or d_d against E_o, E_d.  It can change: drop_last_stride -- rays whose
               length is no multiple of 64, no_t -- rays with a sample; rays without a NaN sample."""
import numpy as np
import pytest
import torch

from tests import density_grad_model as D
from tests import enc_grad_model as M

CASES = M.cases()
PER_SHAPE = CASES[:len(M.SHAPES)]                      # every (F, L) once
WIDE = [c for c in CASES if c.n_rays == M.WIDE]
TERM_OVER_E = 4.0


def _outside(r):
    return (r > M.BAR).any(1)


@pytest.mark.parametrize("c", PER_SHAPE, ids=M.case_id)
def test_model_is_the_gradient_of_the_interpolant(c):
    """(i) central differences of sum_c g[p, c] enc[p, c], h = 1e-6 cell units of the finest level, the
    step added to the fractions, inside one cell: every axis, 1e-6 relative
    (test_density_grad_model_cpu.py's).  With g = w0 in every row the generalised interpolant is
    density_grad_model's."""
    b = M.build_case(c)
    fld, ms = b.fld, b.ms
    ok = ~ms["zero"]
    x, feat, g = ms["x"][ok], ms["feat"][ok], b.g.numpy()[ok]
    h = 1e-6 / float(fld["mul"][-1])
    scale = np.abs(ms["G"][ok]).max(1)
    for ax in range(3):
        e = np.zeros(3)
        e[ax] = h
        fd = (M.interpolant(fld, feat, x, g, e) - M.interpolant(fld, feat, x, g, -e)) / (2 * h)
        err = np.abs(fd - ms["G"][ok, ax])
        assert (err <= 1e-6 * np.maximum(scale, 1e-300)).all(), (M.case_id(c), ax, float((err / scale).max()))
    w0 = fld["w0"].numpy()
    rows = np.broadcast_to(w0, (x.shape[0], w0.shape[0]))
    assert np.array_equal(M.interpolant(fld, feat, x, rows), D.interpolant(fld, feat, x, w0))


@pytest.mark.parametrize("c", PER_SHAPE, ids=M.case_id)
def test_uniform_rows_give_the_density_model(c):
    """(ii) g[p, :] = w0 for every p: values and bounds of density_grad_model.point_model"""
    b = M.build_case(c)
    w0 = b.fld["w0"]
    g = w0[None].expand(b.pts.shape[0], -1).contiguous()
    got, want = M.sample_model(b.fld, b.pts, g), D.point_model(b.fld, b.pts)
    for mine, theirs in (("G", "G"), ("E_G", "E_G"), ("dp", "g"), ("E_dp", "E_g")):
        assert np.array_equal(got[mine], want[theirs], equal_nan=True), (M.case_id(c), mine)


# ---- (iii) the kernels' operations in float32 numpy ---------------------------------------------------------

def _fma(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
            + np.asarray(c, dtype=np.float64)).astype(np.float32)


def _f32_levels(fld, x, g):
    """enc_grad_levels (density_grad_level per level) at float32 contracted points x -> G [n, 3] float32"""
    f = np.float32
    L, F, stride = fld["L"], fld["F"], fld["stride"]
    rows = M.corner_rows(fld, x)
    tab = fld["table16"].numpy().view(np.float16)
    g = g.numpy().astype(f).reshape(-1, L, F)
    G = np.zeros((x.shape[0], 3), dtype=f)
    for l in range(L):
        mul, bias = f(float(fld["mul"][l])), fld["bias"][l].numpy().astype(f)
        pos = _fma(x, mul, np.broadcast_to(bias, x.shape))
        fr = pos - np.floor(pos)
        cm = f(1) - fr
        feat = tab[stride * l + rows[:, l, :, None] * F + np.arange(F)].astype(f)      # [n, 8, F]
        s = feat[:, :, 0] * g[:, l, None, 0]
        for k in range(1, F):
            s = _fma(g[:, l, None, k], feat[:, :, k], s)
        for ax in range(3):
            a, b = M._OTHER[ax]
            wg = (cm[:, a] * cm[:, b], cm[:, a] * fr[:, b], fr[:, a] * cm[:, b], fr[:, a] * fr[:, b])
            t = None
            for j, (hi, lo) in enumerate(M._PAIRS[ax]):
                d = s[:, hi] - s[:, lo]
                t = d * wg[j] if t is None else _fma(d, wg[j], t)
            G[:, ax] = _fma(mul, t, G[:, ax])
    return G


def _f32_jacobian(pts, G):
    f = np.float32
    p = pts.numpy().astype(f)
    nrm = np.sqrt(_fma(p[:, 2], p[:, 2], _fma(p[:, 1], p[:, 1], p[:, 0] * p[:, 0])))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = f(1) / nrm
        ja = (f(2) - inv) * inv
        da = (f(2) * inv - f(2)) * inv * inv * inv
        pg = _fma(p[:, 2], G[:, 2], _fma(p[:, 1], G[:, 1], p[:, 0] * G[:, 0]))
        cc = da * pg
        out = np.stack([_fma(cc, p[:, a], ja * G[:, a]) for a in range(3)], 1)
    out = np.where((nrm <= 1)[:, None], G, out)
    out[nrm == 0] = np.nan
    return out


def _f32_rays(bounds, t, dp, rays_d):
    """the strided loop, a lane sum in an order of our own (any order lies within the bound), the epilogue"""
    f = np.float32
    b, tt, q = bounds.numpy(), t.numpy().astype(f), rays_d.numpy().astype(f)
    d_o = np.zeros((b.shape[0], 3), dtype=f)
    d_d = np.zeros((b.shape[0], 3), dtype=f)
    for r, (s, e) in enumerate(b):
        lo, lm = np.zeros((64, 3), dtype=f), np.zeros((64, 3), dtype=f)
        for c in range(s, e, 64):
            k = min(64, e - c)
            lo[:k] = lo[:k] + dp[c:c + k]
            lm[:k] = _fma(tt[c:c + k, None], dp[c:c + k], lm[:k])
        o, m = f(0) * lo[0], f(0) * lm[0]
        for lane in range(64):
            o, m = o + lo[lane], m + lm[lane]
        dn = np.sqrt(_fma(q[r, 2], q[r, 2], _fma(q[r, 1], q[r, 1], q[r, 0] * q[r, 0])))
        nv = q[r] / dn
        nm = _fma(nv[2], m[2], _fma(nv[1], m[1], nv[0] * m[0]))
        d_o[r] = o
        d_d[r] = (m - nv * nm) / dn
    return d_o, d_d


@pytest.mark.parametrize("c", CASES, ids=M.case_id)
def test_float32_restatement_stays_within_the_bound(c):
    """(iii) and (v): both entries' operations in float32 numpy against the float64 model; the builder's
    input conditions with nothing left out; NaN in the origin's own ray and no other"""
    b = M.build_case(c)
    assert int(M.ambiguous(b.fld, b.pts).sum()) == 0 and int(M.ambiguous_at(b.fld, b.x32).sum()) == 0
    assert b.redrawn < 0.5
    n = b.pts.shape[0]
    assert n == sum(M.lengths_of(c.n_rays)) and b.g.shape == (n, c.L * c.F)
    worst = {}
    Gp = _f32_levels(b.fld, b.x32, b.g)
    worst["pts"] = float(M.ratio(Gp, b.mp["G"], b.mp["E_G"]).max())
    x = M.contract_f32(b.pts)
    x[np.isnan(x).any(1)] = 0
    G = _f32_levels(b.fld, x, b.g)
    dp = _f32_jacobian(b.pts, G)
    worst["dp"] = float(M.ratio(dp, b.ms["dp"], b.ms["E_dp"]).max())
    d_o, d_d = _f32_rays(b.bounds, b.t, dp, b.rays_d)
    worst["d_o"] = float(M.ratio(d_o, b.d_o, b.E_o).max())
    worst["d_d"] = float(M.ratio(d_d, b.d_d, b.E_d).max())
    print("\n%s: largest |err| / E of the float32 restatement %s" % (M.case_id(c), worst))
    assert max(worst.values()) <= M.BAR, (M.case_id(c), worst)
    bad = np.isnan(b.d_o).any(1)
    assert np.array_equal(bad, np.isnan(b.d_d).any(1))
    assert np.nonzero(bad)[0].tolist() == ([b.nan_ray] if c.origin else [])
    assert np.nonzero(np.isnan(b.ms["dp"]).any(1))[0].tolist() == ([b.nan_at] if c.origin else [])
    length = (b.bounds[:, 1] - b.bounds[:, 0]).numpy()
    assert (b.d_o[length == 0] == 0).all() and (b.E_o[length == 0] == 0).all()
    assert (b.d_d[length == 0] == 0).all() and (b.E_d[length == 0] == 0).all()


# ---- (iv) mutants ---------------------------------------------------------------------------------------------

def _sample_mutants(fld):
    L = fld["L"]
    muts = ["q5", "q5_quarter", ("swap_w", 0), ("swap_w", 1), ("swap_w", 2), ("no_mul", L // 2), ("no_mul", L - 1),
            "g_f16", "identity_jac"]
    if fld["F"] >= 2:
        muts.append("swap_chan")
    return muts


def _check_samples(c, mut):
    b = M.build_case(c)
    ms = b.ms
    finite = ~ms["zero"]
    nrm = np.linalg.norm(b.pts.numpy().astype(np.float64), axis=1)
    mm = M.sample_model(b.fld, b.pts, b.g, mut)
    if mut == "identity_jac":
        can, term = finite & (nrm > 1.01), ms["G"] - ms["dp"]
    else:
        can = finite
        term = M.contract_bwd_model(b.pts, mm["G"] - ms["G"], np.zeros_like(ms["G"]))[0]
    with np.errstate(invalid="ignore"):
        elig = can & (np.abs(term) > TERM_OVER_E * ms["E_dp"]).any(1)
    assert elig.sum() >= 50 and elig.sum() >= 0.5 * can.sum(), (M.case_id(c), mut, int(elig.sum()), int(can.sum()))
    out = _outside(M.ratio(mm["dp"], ms["dp"], ms["E_dp"]))[elig]
    assert out.all(), (M.case_id(c), mut, int((~out).sum()), int(elig.sum()))


@pytest.mark.parametrize("c", PER_SHAPE, ids=M.case_id)
def test_bound_rejects_the_q5_form(c):
    """The form the existing kernels compute (f2n_hash_rays_grad, f2n_hash_bwd's pts_grad), even without
    their f16 roundings, and a quarter of it: neither can pass for the encoding's derivative."""
    _check_samples(c, "q5")
    _check_samples(c, "q5_quarter")


@pytest.mark.parametrize("c", PER_SHAPE, ids=M.case_id)
def test_bound_rejects_wrong_sample_gradients(c):
    for mut in _sample_mutants(M.build_case(c).fld)[2:]:
        _check_samples(c, mut)


@pytest.mark.parametrize("c", WIDE, ids=M.case_id)
def test_bound_rejects_wrong_ray_sums(c):
    b = M.build_case(c)
    length = (b.bounds[:, 1] - b.bounds[:, 0]).numpy()
    clean = ~np.isnan(b.d_o).any(1)
    for mut in ("drop_last_stride", "no_t"):
        d_o, _, d_d, _ = M.rays_model(b.bounds, b.t, b.ms["dp"], b.ms["E_dp"], b.rays_d, mut)
        can = clean & (length > 0)
        if mut == "drop_last_stride":
            can = can & (length % 64 != 0)
        elig = can & ((np.abs(d_o - b.d_o) > TERM_OVER_E * b.E_o).any(1)
                      | (np.abs(d_d - b.d_d) > TERM_OVER_E * b.E_d).any(1))
        assert elig.sum() >= 50 and elig.sum() >= 0.5 * can.sum(), (M.case_id(c), mut, int(elig.sum()), int(can.sum()))
        out = (_outside(M.ratio(d_o, b.d_o, b.E_o)) | _outside(M.ratio(d_d, b.d_d, b.E_d)))[elig]
        assert out.all(), (M.case_id(c), mut, int((~out).sum()))
        if mut == "no_t":           # t enters m only
            assert np.array_equal(d_o, b.d_o)


def test_cases_cover_what_they_claim(capi):
    null = [None] * 7
    for c in CASES:          # every case is one the C ABI accepts (f2n_density_grad checks the field first)
        stride = c.T * c.F if c.disjoint else c.T
        assert M.build_case(c).fld["stride"] == stride
        assert capi.lib().cdll.f2n_density_grad(*null, 0, c.L, c.F, c.T, stride, None) == 0, M.case_id(c)
    assert {(c.F, c.L) for c in CASES} == set(M.SHAPES)
    assert {c.T for c in CASES} == {1 << 14, 12289} and {c.disjoint for c in CASES} == {False, True}
    for F in (1, 2, 4, 8):   # both POW2 instantiations of every F
        assert {c.T for c in CASES if c.F == F} == {1 << 14, 12289}, F
    assert {c.chan_major for c in CASES} == {False, True}
    assert sum(c.origin for c in CASES) >= 1
    for c in CASES:
        assert set(M.lengths_of(c.n_rays)) == set(M.SEG_LENGTHS)
    b = M.build_case(CASES[0])
    nrm = b.pts.norm(dim=1)
    assert (nrm < 1).sum() > 100 and (nrm > 1).sum() > 100
    for v in M.R.D_NORMS:
        assert torch.isclose(b.rays_d.norm(dim=1), torch.tensor(v), rtol=1e-5).any(), v
    assert sum(M.build_case(c).pts.shape[0] for c in CASES) < 12000
    assert torch.equal(M.build_case(CASES[0]).g, M.build_case(CASES[0]).g)
