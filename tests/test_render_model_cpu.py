"""The power of tests/test_gpu_render_f64.py, checked without a GPU: the float64 model of
tests/render_model.py against a plain float64 composition of the oracle's ops, and against
ragged_cases' closed forms and autograd for its Jacobian; the oracle's f32 composition inside the
bound on every case; every mutant caught on every case it applies to (the f16 ulp, which a ray's outputs
cannot show, held at its sample's logit instead); and mutants the bar of the
existing render tests, _close(a, b, 1e-4), lets through on those tests' inputs while the bound catches
them.  The cases' conditions (ambiguity cap, required lengths, weight behind every link) are asserted
by build_case from the model alone."""
import numpy as np
import pytest
import torch

from oracle import kernels as K
from oracle import ref_render as R
from tests import ragged_cases as rc
from tests import render_model as M
from tests import shade_model as sm
from tests.test_gpu_fused import _composite_oracle
from tests.test_gpu_occupancy import _rays
from tests.test_gpu_render_rays import _raw_network
from tests.util import _raw_field

CASES = M.cases()
SMALL = [c for c in CASES if c.mode != "short"]


def _list(m):
    """the ragged list of a model's kept, occupied samples -> (ray index, sample index, int32 bounds)"""
    ri, ki = np.nonzero(m["use"])
    cum = np.cumsum(m["kept"])
    idx = torch.from_numpy(np.stack([cum - m["kept"], cum], 1).astype(np.int32))
    return ri, ki, idx


def _network_torch(inp, smp, ri, ki, dtype):
    """the network of shade.hip as plain torch ops in `dtype` on samples (ri, ki) -> head logit, rgb"""
    P = {k: v.to(dtype) for k, v in inp.P.items()}
    enc = torch.from_numpy(smp.enc[ri, ki]).to(dtype)
    dirs = torch.from_numpy(smp.dirs[ri])
    h = enc @ P["w_h"].t() + P["b_h"]
    X = torch.cat([torch.ones_like(h[:, :1]), h[:, 1:]], 1)
    if inp.img is not None:
        X = X + P["emb"][torch.from_numpy(inp.img[ri]).long()]
    sh = sm.sh16(dirs)[0] if dtype == torch.float64 else K.sh_encode(dirs.contiguous(), 4)
    hid = torch.relu(torch.cat([X, sh.to(dtype)], 1) @ P["w1"].t() + P["b1"])
    o = hid @ P["w2"].t() + P["b2"]
    if dtype == torch.float64:
        return h[:, 0], sm.C32 / (1.0 + torch.exp(-o)) - sm.EPS32
    eps = torch.tensor(1e-3)
    return h[:, 0], (1.0 + 2.0 * eps) / (1.0 + torch.exp(-o)) - eps


def _flex_sum64(val, ri, n):
    shape = (n,) + tuple(val.shape[1:])
    return torch.zeros(shape, dtype=torch.float64).index_add_(0, torch.from_numpy(ri), val)


def _flex_scan64(val, idx):
    """FlexAccumulateSum(include_this = False) in float64 (the oracle's C ops are float32 only)"""
    out = torch.zeros_like(val)
    for s, e in idx.tolist():
        out[s:e] = torch.cumsum(val[s:e], 0) - val[s:e]
    return out


def _composition64(inp, smp, hl=None):
    """the oracle's ops, composed in float64 without the model: chain, keep decision, network,
    compositing (renderer.cpp:58-118 with R.TruncExp and float64 flex sums)"""
    n, S, C = smp.enc.shape
    dt, t = torch.from_numpy(smp.dt).double(), torch.from_numpy(smp.t).double()
    logit0 = torch.from_numpy(smp.enc).double() @ inp.P["w_h"][0].double() + inp.P["b_h"][0].double()
    occ = torch.ones(n, S, dtype=torch.bool) if inp.occ is None else torch.from_numpy(
        inp.occ[M._cells(smp.x.reshape(-1, 3), M.G_OCC)].reshape(n, S))
    sec = R.TruncExp.apply(logit0 - M.DENSITY_SHIFT) * dt * occ
    acc = torch.cumsum(sec, 1) - sec
    pos = (torch.exp(-acc) > float(np.float32(M.T_THRESH))).long().cumprod(1).bool()
    use = pos & occ
    ri, ki = np.nonzero(use.numpy())
    kept = use.sum(1).numpy()
    cum = np.cumsum(kept)
    idx = torch.from_numpy(np.stack([cum - kept, cum], 1).astype(np.int32))
    net_hl, rgb = _network_torch(inp, smp, ri, ki, torch.float64)
    hl = net_hl if hl is None else hl
    sec2 = R.TruncExp.apply(hl - M.DENSITY_SHIFT) * dt[ri, ki]
    w = torch.exp(-_flex_scan64(sec2, idx)) * (1.0 - torch.exp(-sec2))
    Tl = torch.exp(-_flex_sum64(sec2, ri, n))
    colors = _flex_sum64(w[:, None] * rgb, ri, n) + Tl[:, None] * inp.bg.double()
    depths = _flex_sum64(w * (t[ri, ki] + M.T_SHIFT32), ri, n) / (1.0 - Tl + M.DEN_EPS32)
    return dict(colors=colors, depths=depths, last_trans=Tl, kept=kept, len=pos.sum(1).numpy(), ri=ri, ki=ki)


@pytest.mark.parametrize("c", SMALL, ids=M.case_id)
def test_model_is_the_float64_composition_of_the_oracles_ops(c):
    inp, smp, m = M.build_case(c)
    ref = _composition64(inp, smp)
    assert np.array_equal(ref["kept"], m["kept"]) and np.array_equal(ref["len"], m["len"])
    for name in M.OUTPUTS:
        err = np.abs(ref[name].numpy() - m[name]).max()
        assert err <= 1e-12, (name, err)


@pytest.mark.parametrize("c", [c for c in SMALL if c.name in ("len-C8-S100", "weight-C64-S64", "nat-C16-S100-random")],
                         ids=M.case_id)
def test_closed_forms_are_ragged_cases_and_the_jacobian_is_autograd(c):
    """With the float64 constants of ragged_cases (t_shift 1e-2, 1e-4) the compositing stage, with its
    conditioning numbers, is composite_fwd_ref on the model's own list; and d out / d logit is what
    autograd gives through the float64 composition."""
    inp, smp, _ = M.build_case(c)
    m = M.model(inp, smp, t_shift=rc.T_SHIFT, den_eps=1e-4)
    ri, ki, idx = _list(m)
    lay = rc.Layout(idx, np.ones(c.n_rays), int(m["kept"].sum()))
    case = dict(logit=torch.from_numpy(m["hl"][ri, ki]), dt=torch.from_numpy(smp.dt[ri, ki]),
                rgb=torch.from_numpy(m["rgb"][ri, ki]), t=torch.from_numpy(smp.t[ri, ki]), bg=inp.bg)
    ref = rc.composite_fwd_ref(lay, case)
    some = m["kept"] > 0
    for name in M.OUTPUTS:
        assert np.abs(ref[name] - m[name]).max() <= 1e-12, name
        Ea = M.U * (lay.len.reshape((-1,) + (1,) * (ref[name].ndim - 1)) * ref["msum"][name]
                    + rc.K_COMPOSITE * ref["mop"][name])
        assert np.allclose(Ea[some], m["Ea"][name][some], rtol=1e-9, atol=0), name
    assert np.abs(ref["weights"] - m["w"][ri, ki]).max() <= 1e-12
    # the Jacobian, with the constants the kernels hold
    m = M.model(inp, smp)
    hl = torch.from_numpy(m["hl"][ri, ki]).requires_grad_(True)
    out = _composition64(inp, smp, hl)
    for name, J in (("depths", m["J_depths"][ri, ki]), ("colors", m["J_colors"][ri, ki][:, 1]),
                    ("last_trans", -(m["last_trans"][:, None] * m["sec2"])[ri, ki])):
        y = out[name] if name != "colors" else out[name][:, 1]
        g, = torch.autograd.grad(y.sum(), hl, retain_graph=True)
        assert np.abs(g.numpy() - J).max() <= 1e-9 * max(1.0, np.abs(J).max()), name


def _oracle32(inp, smp, m):
    """the oracle's f32 composition on the model's inputs: its own keep decision (K.seg_scan_fwd), the
    network in torch float32, _composite_oracle"""
    n, S, C = smp.enc.shape
    enc, dt, t = torch.from_numpy(smp.enc), torch.from_numpy(smp.dt), torch.from_numpy(smp.t)
    logit0 = (enc.reshape(-1, C) @ inp.P["w_h"][0] + inp.P["b_h"][0]).reshape(n, S)
    sec = (torch.exp(logit0 - M.DENSITY_SHIFT) * dt * torch.from_numpy(m["occ"])).reshape(-1).contiguous()
    full = torch.from_numpy(np.stack([np.arange(n) * S, np.arange(n) * S + S], 1).astype(np.int32))
    pos = (torch.exp(-K.seg_scan_fwd(sec, full, 0)) > 1e-4).reshape(n, S).long().cumprod(1).bool()
    use = pos & torch.from_numpy(m["occ"])
    length, kept = pos.sum(1).numpy(), use.sum(1).numpy()
    # values: on the model's list (an ambiguous ray may differ by one sample and is not compared)
    ri, ki, idx = _list(m)
    hl, rgb = _network_torch(inp, smp, ri, ki, torch.float32)
    colors, depths, _, last = _composite_oracle(hl, rgb, dt[ri, ki], t[ri, ki], idx, inp.bg)
    return dict(colors=colors, depths=depths, last_trans=last, kept=kept, len=length)


@pytest.mark.parametrize("c", CASES, ids=M.case_id)
def test_f32_oracle_lies_inside_the_bound(c):
    inp, smp, m = M.build_case(c)
    got = _oracle32(inp, smp, m)
    r = M.ratios(got, m)
    print("\n%s (seed %d, %d ambiguous): oracle f32 largest |err| / E  %s" % (
        c.name, inp.seed, int(m["ambiguous"].sum()), "  ".join("%s %.3f" % kv for kv in r.items())))
    fails = M.failures(got, m)
    assert not fails, "%s: %d misses, first: %s" % (c.name, len(fails), fails[0])
    # the model's own values, rounded to f32, pass too
    assert not M.failures({k: m[k].astype(np.float32) if k in M.OUTPUTS else m[k] for k in M.OUTPUTS + ("kept", "len")}, m)


def _mutant(inp, smp, m, mut, n_head=M.WHOLE, loop=M.HEAD_LOOP):
    return M.model(inp, smp, mut=mut, n_head=n_head, loop=loop, at=M.ulp_site(inp, smp, m)[0] if mut == "f16_ulp" else None)


def _worst(mm, m):
    """largest |moved| / E over outputs (what the bar of 2 has to stay under to miss the mutant)"""
    return max(M.ratios(mm, m).values())


@pytest.mark.parametrize("mut", [k for k in M.MUTANTS if k not in M.INFORMATIONAL])
def test_mutant_is_caught_on_every_case_it_applies_to(mut):
    hit, lines = 0, []
    for c in CASES:
        inp, smp, m = M.build_case(c)
        if mut == "prev_sh":
            runs = [(M.WHOLE, loop) for loop in (M.ONE_RAY_LOOP, M.HEAD_LOOP) if c.n_rays > loop]
        elif mut in M.HANDOVER_MUTANTS:
            runs = [(h, 0) for h in M.heads(c.S) if h < c.S]
        else:
            runs = [(M.WHOLE, 0)]
        for n_head, loop in runs:
            if not M.applies(mut, c, m, n_head):
                continue
            mm = _mutant(inp, smp, m, mut, n_head, loop)
            fails = M.failures(mm, m)
            lines.append("  %-24s n_head %-10d %d misses, largest |moved| / E %.3g" % (
                c.name, n_head, len(fails), _worst(mm, m)))
            assert fails, "%s (%s) passes on %s, n_head %d" % (mut, M.MUTANTS[mut], c.name, n_head)
            hit += 1
    print("\n%s: %s\n%s" % (mut, M.MUTANTS[mut], "\n".join(lines)))
    assert hit >= 2 or (mut == "prev_sh" and hit >= 1), (mut, hit)


def test_f16_ulp_shows_in_the_samples_logit_not_in_the_rays_outputs():
    """render_model.INFORMATIONAL.  One f16 ulp of one encoding value, at the kept sample and channel
    where it shows most: the model's head logit of that sample moves by |w_h[0, c]| ulp16 and by nothing
    else, and no other sample's moves.  At C <= 32 that is more than 2 E_logit -- a stage that handed out
    logits would catch it; at C = 64, where E_logit = gamma(65) (|b0| + ..) and |w| is about 1 / 8, it is
    printed.  Through a ray's outputs it stays below 0.5 E there, and at the most opaque kept sample of a
    case (the second sample of a two-sample ray, sec2 of about 19) between 0.66 and 2.86 E (printed): this
    module's GPU test cannot see a single flipped value."""
    seen = 0
    for c in SMALL:
        inp, smp, m = M.build_case(c)
        if not m["kept"].any():
            continue
        (r, k, ch), want = M.ulp_site(inp, smp, m)
        mm = _mutant(inp, smp, m, "f16_ulp")
        moved = np.abs(mm["hl"] - m["hl"])
        v = np.float16(smp.enc[r, k, ch])
        ulp = float(np.nextafter(v, np.float16(np.inf))) - float(v)
        assert abs(moved[r, k] - abs(float(inp.P["w_h"][0, ch])) * ulp) <= 1e-12
        moved[r, k] = 0.0
        assert moved.max() == 0.0
        ratio = abs(float(inp.P["w_h"][0, ch])) * ulp / m["E_hl"][r, k]
        assert abs(ratio - want) <= 1e-9 * want
        # ... and at the most opaque kept sample, where a ray's last_trans is most sensitive to a logit
        sec = np.where(m["ambiguous"][:, None], 0.0, m["sec2"])
        ro, ko = np.unravel_index(int(np.argmax(sec)), sec.shape)
        e16 = smp.enc[ro, ko].astype(np.float16)
        u16 = np.nextafter(e16, np.float16(np.inf)).astype(np.float64) - e16.astype(np.float64)
        co = int(np.argmax(np.abs(inp.P["w_h"][0].double().numpy()) * u16))
        opaque = _worst(M.model(inp, smp, mut="f16_ulp", at=(int(ro), int(ko), co)), m)
        print("%-24s |moved| / E_logit %.3g; on the ray's outputs %.3g E, at its most opaque sample (sec2 %.3g) "
              "%.3g E" % (c.name, ratio, _worst(mm, m), sec[ro, ko], opaque))
        if c.C <= 32:
            assert ratio > M.BAR, (c.name, ratio)
            seen += 1
    assert seen >= 10


# ---- the old bar --------------------------------------------------------------------------------------

def _existing_inputs(S, bias0, occ):
    """The inputs of tests/test_gpu_render_rays.py::test_counts_are_the_marchs_exactly at (16, 2, 2^19):
    _raw_field, _raw_network, _rays and its image ids, 99 rays, with one of its grids"""
    L, F, T = 16, 2, 1 << 19
    fld = _raw_field(L, F, T, 5.0, seed=5 * L + S + F, dev="cpu")
    net = _raw_network(fld, seed=S + L, dev="cpu")
    o, d, noise = _rays(99, S, seed=S + F + 2, dev="cpu", train=True)
    img = torch.randint(0, 5, (99,), generator=torch.Generator().manual_seed(S)).numpy()
    fld["b0"].fill_(bias0)
    net["b_h"][0] = bias0
    c = M.Case("existing-S%d" % S, 32, S, True, 99, "natural", "random", occ)
    bits = None if occ == "none" else M.grids_bool(S)[occ].numpy()
    inp = M.Inputs(c, fld, net, o, d, noise, img, torch.full((99, 3), 0.5), bits, 4.0 / S, 0)
    smp = M.cpu_samples(fld, o, d, noise, S, inp.step)
    return c, inp, smp, M.model(inp, smp)


@pytest.mark.parametrize("S,bias0,occ,missed", [
    (128, 5.0, "random", ("k_ge_S", "chain_T_last", "no_den_eps")),
    (128, 4.0, "none", ("drop_last", "chain_T_last", "no_den_eps")),
    (192, 6.0, "random", ("chain_T_last", "no_den_eps")),
])
def test_old_bar_misses_what_the_bound_catches(S, bias0, occ, missed):
    """On the existing tests' inputs, _close(., ., 1e-4) with exact counts lets `missed` through and the
    bound does not.  Of the other candidates, compositing after the stop and the kept but unoccupied
    sample are caught by the old bar as well on these inputs (through the depths: the weight behind the
    stop, at most 1e-4, sits at the far end of the ray; an unoccupied cell of this fog is as dense as
    its neighbours), and one f16 ulp of one value passes both (render_model.INFORMATIONAL)."""
    c, inp, smp, m = _existing_inputs(S, bias0, occ)
    assert not m["ambiguous"].any()
    for mut in M.MUTANTS:
        if mut in M.HANDOVER_MUTANTS or not M.applies(mut, c, m):
            continue
        mm = _mutant(inp, smp, m, mut)
        old, new = M.old_bar_passes(mm, m), not M.failures(mm, m)
        print("S=%d bias %.0f %-7s %-14s old bar %-7s bound %-7s largest |moved| / E %.3g" % (
            S, bias0, occ, mut, "passes" if old else "catches", "passes" if new else "catches", _worst(mm, m)))
        if mut in missed:
            assert old, (mut, "the existing bar catches it")
            assert not new, (mut, "the bound misses it")
        elif mut == "f16_ulp":
            assert old
        else:
            assert not new, mut


def test_conditions_and_seeds():
    """build_case asserts every case's conditions from the model alone; the seeds and counts, for NOTES"""
    for c in CASES:
        inp, smp, m = M.build_case(c)
        print("%-24s seed %-8d ambiguous %d of %d, kept %d..%d, len %d..%d" % (
            c.name, inp.seed, int(m["ambiguous"].sum()), c.n_rays, m["kept"].min(), m["kept"].max(),
            m["len"].min(), m["len"].max()))
    assert {c.occ for c in CASES} == {"none", "ones", "shell", "random", "empty"}
    assert {c.img for c in CASES} == {"none", "equal", "distinct", "runs3"}
    assert {c.n_rays for c in CASES} >= {1, 7, 8, 9, 95, 96, 97, 99}
    assert {c.C for c in CASES} == {8, 16, 32, 64} and {c.S for c in CASES} == {64, 100, 192}
    assert sorted({c.paired for c in CASES}) == [0, 1]
