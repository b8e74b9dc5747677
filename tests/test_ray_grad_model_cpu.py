"""tests/ray_grad_model.py on the CPU: the closed forms against float64 autograd on the reference's
mask expression, the float32 level sums against the oracle bit for bit, the bound against the float32
oracle composition (not too tight), the two conditions every case is built under, and the changes a
wrong kernel could make that the bound must reject (it has teeth).  Run with -s for the figures."""
import functools

import numpy as np
import pytest
import torch

from oracle import kernels as K
from tests import ray_grad_model as M

CASES = M.cases()
RAY_CASES = [c for c in CASES if c.layer != "level"]


@functools.lru_cache(maxsize=None)
def _built(c):
    return M.build_case(c)


def _worst(got, ref, E):
    return float(M.ratio(got, ref, E).max())


def _contract_autograd(pts, gx, dtype):
    """the reference's ATen mask expression (src/hash_3d_anchored.cpp:79-82) -> x, J^T gx"""
    p = pts.detach().to(dtype).requires_grad_(True)
    norm = p.norm(2, dim=1, keepdim=True)
    mask = norm <= 1.0
    xc = p * mask + ~mask * (1 + 1.0 - 1.0 / norm) * p / norm
    (dp,) = torch.autograd.grad(xc, p, gx.to(dtype))
    return xc.detach(), dp


@pytest.mark.parametrize("c", [c for c in CASES if c.layer in ("points", "dense")], ids=M.case_id)
def test_closed_form_matches_autograd(c):
    """G against a float64 sum over an independent gather of the terms' factors; x and dp against
    float64 autograd through the mask expression; d_d against autograd through d / |d|: within 1e-12
    of each element's scale."""
    inp, m, _ = _built(c)
    fld, keep = inp.fld, ~m["zero"]
    L, F, n = fld["L"], fld["F"], inp.pts.shape[0]
    rows = torch.from_numpy(M.corner_rows(fld, m["x32"]))
    tab = torch.from_numpy(fld["table16"].numpy().view(np.float16).copy())
    G = torch.zeros(n, 3, dtype=torch.float64)
    gk = (inp.g * 128.0).half().float().reshape(n, L, F)
    for l in range(L):
        for d in range(8):
            for k in range(F):
                f = tab[fld["stride"] * l + rows[:, l, d] * F + k].float()
                term = ((f * fld["mul"][l]) * gk[:, l, k]).half().double()
                for axis, bit in enumerate((4, 2, 1)):
                    G[:, axis] += term if d & bit else -term
    G /= 128.0
    assert torch.equal(G, torch.from_numpy(m["G"]))
    gx = torch.from_numpy(m["G"])
    x, dp = _contract_autograd(inp.pts, gx, torch.float64)
    scale = 1e-12 * (1.0 + float(np.abs(m["G"]).max()))
    assert float((x[keep] - torch.from_numpy(m["x"])[keep]).abs().max()) <= 1e-12
    assert float((dp[keep] - torch.from_numpy(m["dp"])[keep]).abs().max()) <= scale
    assert bool(torch.isnan(x[~keep]).all()) and bool(np.isnan(m["dp"][~keep]).all())
    # per ray
    ray = torch.repeat_interleave(torch.arange(inp.bounds.shape[0]), (inp.bounds[:, 1] - inp.bounds[:, 0]).long())
    dpm = torch.from_numpy(m["dp"])
    mm = torch.zeros(inp.bounds.shape[0], 3, dtype=torch.float64).index_add_(0, ray, dpm * inp.t.double()[:, None])
    dv = inp.rays_d.double().requires_grad_(True)
    ok = ~torch.isnan(mm).any(1)
    ((dv / torch.linalg.norm(dv, 2, -1, True))[ok] * mm[ok]).sum().backward()
    ref = dv.grad[ok]
    got = torch.from_numpy(m["d_d"])[ok]
    assert float(((got - ref).abs() / (1e-300 + ref.abs().max(1, keepdim=True)[0])).max()) <= 1e-9


@pytest.mark.parametrize("c", [c for c in CASES if c.layer == "level"], ids=M.case_id)
def test_level_f32_equals_the_oracle(c):
    """with the gradient in one level's channels, oracle.kernels.hash_bwd's point gradient is that
    level's float32 sum, bit for bit"""
    inp, m, _ = _built(c)
    fld = inp.fld
    L, F = fld["L"], fld["F"]
    assert np.array_equal(m["x32"], inp.pts.numpy()), "inside the unit ball the contraction is the identity"
    for l in range(L):
        g = torch.zeros_like(inp.g)
        g[:, l * F:(l + 1) * F] = inp.g[:, l * F:(l + 1) * F]
        _, pg = K.hash_bwd(inp.pts, fld["table16"], fld["primes"], fld["bias"], fld["mul"], g, fld["numel"],
                           L, F, fld["T"], fld["stride"], M.GRAD_SCALE, need_pts_grad=True)
        assert np.array_equal(pg.numpy(), m["level_f32"][:, l]), (M.case_id(c), l)
    assert float(np.abs(m["level_f32"]).max()) > 0
    if c.tag == "subnormal":
        print("\n%s: %.1f %% of the non-zero terms are f16 subnormals" % (M.case_id(c), 100 * m["subnormal"]))
        assert m["subnormal"] > 0.05
    if c.tag == "rows":
        rows = M.corner_rows(fld, m["x32"])
        assert (rows == 0).any() and (rows == fld["T"] - 1).any()
        assert (rows[:, L - 1] == fld["T"] - 1).any(), "the table's last row is not read"


def _oracle_composition(inp, m):
    """tests/test_gpu_pose_grad.py::_oracle_rays_grad in float32 on the model's contracted points"""
    fld = inp.fld
    x = torch.from_numpy(m["x32"])
    _, gx = K.hash_bwd(x, fld["table16"], fld["primes"], fld["bias"], fld["mul"], inp.g, fld["numel"], fld["L"],
                       fld["F"], fld["T"], fld["stride"], M.GRAD_SCALE, need_pts_grad=True)
    _, dp = _contract_autograd(inp.pts, gx, torch.float32)
    n_rays = inp.bounds.shape[0]
    ray = torch.repeat_interleave(torch.arange(n_rays), (inp.bounds[:, 1] - inp.bounds[:, 0]).long())
    d_o = torch.zeros(n_rays, 3).index_add_(0, ray, dp)
    mm = torch.zeros(n_rays, 3).index_add_(0, ray, dp * inp.t[:, None])
    dv = inp.rays_d.clone().requires_grad_(True)
    ((dv / torch.linalg.norm(dv, 2, -1, True)) * torch.nan_to_num(mm)).sum().backward()
    d_d = torch.where(torch.isnan(mm).any(1, keepdim=True), torch.full_like(mm, float("nan")), dv.grad)
    return gx, dp, d_o, d_d


@pytest.mark.parametrize("c", RAY_CASES, ids=M.case_id)
def test_f32_oracle_composition_inside_bound(c):
    """an independent float32 evaluation in another order of operations lies inside 2 E"""
    inp, m, _ = _built(c)
    gx, dp, d_o, d_d = _oracle_composition(inp, m)
    worst = {k: _worst(v, m[k], m["E"][k]) for k, v in (("G", gx), ("dp", dp), ("d_o", d_o), ("d_d", d_d))}
    print("\n%s: float32 oracle |err| / E  %s" % (M.case_id(c), ", ".join("%s %.3f" % kv for kv in worst.items())))
    assert all(v <= M.BAR for v in worst.values()), worst


@pytest.mark.parametrize("c", CASES, ids=M.case_id)
def test_cases_hold_no_ambiguous_sample_and_no_non_finite_term(c):
    inp, m, redrawn = _built(c)
    print("\n%s: %d samples, %.2f %% redrawn, %d ambiguous, terms finite: %s"
          % (M.case_id(c), inp.pts.shape[0], 100 * redrawn, m["ambiguous"], m["finite"]))
    assert m["ambiguous"] == 0
    assert m["finite"]
    assert int(m["zero"].sum()) == (1 if c.layer == "points" else 0)
    for k in ("G", "d_o", "d_d"):
        v = m[k][~np.isnan(m[k]).any(1)]
        assert np.isfinite(v).all() and np.abs(v).max() > 0


def _mutants():
    out = []
    for l in range(32):
        out.append(("level %d dropped" % l, ("no_level", l)))
    for name, l in (("coarsest", 0), ("finest", -1)):
        out.append(("sign of corner 5, axis y, %s level" % name, ("flip", l, 5, 1)))
    out.append(("channel F - 1 ignored", ("no_chan", -1)))
    out.append(("level base T F l", ("base_TF",)))
    out.append(("lane 63 of the second stride lost", "lose_127"))
    out.append(("last sample of a ray lost", "lose_last"))
    out.append(("(a'/n)(p.G) p dropped", "no_pg_term"))
    out.append(("a without 1 / n^2", "a_no_sq"))
    out.append(("t of the next sample", "t_next"))
    out.append(("d_d without n (n.m)", "no_proj"))
    out.append(("1 / |d| omitted", "no_inv_d"))
    # three changes the 5 % bar of tests/test_gpu_pose_grad.py lets through
    out.append(("t scaled by 1.02", "t_102"))
    out.append(("Jacobian evaluated at 1.01 p", "jac_101"))
    out.append(("channel F - 1 of the finest level times 0.98", ("chan_098",)))
    return out


def _applies(mut, fld):
    if isinstance(mut, tuple) and mut[0] == "no_level":
        return mut[1] < fld["L"]
    if mut == ("base_TF",):
        return fld["stride"] != fld["T"] * fld["F"] and fld["L"] > 1
    return True


def test_bound_rejects():
    """each change moves at least one element of at least one case by more than 2 E"""
    caught = {}
    for name, mut in _mutants():
        caught[name] = []
        for c in RAY_CASES:
            inp, m, _ = _built(c)
            fld = inp.fld
            if not _applies(mut, fld):
                continue
            mm = mut
            if isinstance(mut, tuple) and mut[0] == "flip":
                mm = ("flip", mut[1] % fld["L"], mut[2], mut[3])
            if isinstance(mut, tuple) and mut[0] == "no_chan":
                mm = ("no_chan", fld["F"] - 1)
            bad = M.model(inp, mm, base=m)
            moved = max(_worst(bad[k], m[k], m["E"][k]) for k in ("d_o", "d_d"))
            if moved > M.BAR:
                caught[name].append("%s (%.3g)" % (M.case_id(c), moved))
    print("\nchange: cases that catch it (largest |moved| / E)")
    for name, by in caught.items():
        print("  %-42s %s" % (name, ", ".join(by) if by else "NOT CAUGHT"))
    missed = [name for name, by in caught.items() if not by]
    assert not missed, missed
