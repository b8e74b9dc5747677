"""The ray walk on the device against tests/ray_walk_model.py: (a) f2n_sample_rays and f2n_sample_dense
against the float64 model and the f32 restatement, (b) f2n_ray_walk_probe -- make_stride and keep_step
at 64, 16 and 8 lanes to a ray, sample by sample -- against f2n_sample_rays and the restatement, (c) the
real f2n_density_march[_occ] on rays designed to stop at the samples where the 8-, 16- and 64-sample
strides hand over.  Every output is pre-filled with a sentinel and padded; the power of these
assertions is checked on the CPU by tests/test_ray_walk_model_cpu.py."""
import numpy as np
import pytest
import torch

from tests import ragged_cases as rc
from tests import ray_walk_model as M
from tests import util
from tests.ray_grad_model import contract_fwd_model

pytestmark = pytest.mark.gpu

PAD = 70
F32 = np.float32


def _sent(dev, *shape, dtype=torch.float32):
    return torch.full(shape, rc.SENTINEL, dtype=dtype, device=dev)


def _dev(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _untouched(buf, n):
    """rows n.. of a padded buffer still hold the sentinel bit for bit"""
    tail = buf[n:].cpu().numpy()
    return M.bits_equal(tail, np.full(tail.shape, rc.SENTINEL, F32))


def _sample_rays(capi, dev, c, mult):
    n, S = c["n_rays"], c["S"]
    N = n * S
    pts, dirs = _sent(dev, N + PAD, 3), _sent(dev, N + PAD, 3)
    dt, t = _sent(dev, N + PAD), _sent(dev, N + PAD)
    bounds = torch.full((n + 3, 2), -1, dtype=torch.int32, device=dev)
    capi.call("sample_rays", _dev(dev, c["o"]), _dev(dev, c["d"]), _dev(dev, mult), pts, dirs, dt, t,
              bounds, n, S, c["step"])
    for b in (pts, dirs, dt, t):
        assert _untouched(b, N)
    b = bounds.cpu().numpy()
    want = np.full((n + 3, 2), -1, np.int32)
    want[:n, 0] = np.arange(n) * S
    want[:n, 1] = want[:n, 0] + S
    assert np.array_equal(b, want), "bounds"
    return dict(pts=pts[:N].cpu().numpy().reshape(n, S, 3), dirs=dirs[:N].cpu().numpy().reshape(n, S, 3),
                dt=dt[:N].cpu().numpy().reshape(n, S), t=t[:N].cpu().numpy().reshape(n, S))


def _probe(capi, dev, c, mult, W, sec=None):
    n, S = c["n_rays"], c["S"]
    N = n * S
    pts, dt, t, depth = _sent(dev, N + PAD, 3), _sent(dev, N + PAD), _sent(dev, N + PAD), _sent(dev, N + PAD)
    keep = torch.full((N + PAD,), 7, dtype=torch.uint8, device=dev)
    capi.call("ray_walk_probe", _dev(dev, c["o"]), _dev(dev, c["d"]), _dev(dev, mult), _dev(dev, sec), W,
              pts, dt, t, depth, keep, n, S, c["step"], M.THRESH)
    for b in (pts, dt, t, depth):
        assert _untouched(b, N), W
    assert bool((keep[N:] == 7).all()), W
    out = dict(pts=pts[:N].cpu().numpy().reshape(n, S, 3), dt=dt[:N].cpu().numpy().reshape(n, S),
               t=t[:N].cpu().numpy().reshape(n, S))
    if sec is None:     # nothing of the keep decision is written without sec_in
        assert _untouched(depth, 0) and bool((keep == 7).all()), W
    else:
        out["depth"] = depth[:N].cpu().numpy().reshape(n, S)
        out["keep"] = keep[:N].cpu().numpy().reshape(n, S)
        assert set(np.unique(out["keep"])) <= {0, 1}
    return out


def _same_bits(a, b):
    """bit for bit; a NaN for a NaN"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and M.bits_equal(a[~nan], b[~nan])


def _check_samples(got, c, mult, what):
    S = c["S"]
    ref = M.walk_f64(c["o"], c["d"], mult, S, c["step"])
    t32 = M.walk_f32(c["o"], c["d"], mult, S, c["step"])["t"]
    print("%s: worst |err| / E %s" % (what, " ".join("%s %.2f" % kv for kv in M.sample_ratios(got, ref).items())))
    fails = M.sample_failures(got, ref, t32)
    assert fails == [], (what, fails)


# ---- (a) f2n_sample_rays, f2n_sample_dense -----------------------------------------------------------------

@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("S", M.SAMPLE_S)
def test_sample_rays_against_the_model(capi, dev, S, with_noise):
    """bounds exact, t the f32 restatement bit for bit, dirs (every row), pts and dt within BAR E of the
    float64 model element by element, dt_0 == +0; |o| in {0.05, 0.3, 30}, |d| in {1e-3, 1, 1e3}."""
    for n_rays in M.SAMPLE_RAYS:
        c = M.sample_case(n_rays, S, with_noise)
        got = _sample_rays(capi, dev, c, c["noise"])
        _check_samples(got, c, c["noise"], "sample_rays S %d noise %d rays %d" % (S, with_noise, n_rays))


@pytest.mark.parametrize("S", [9, 65, 129])
def test_zero_direction_next_to_healthy_rays(capi, dev, S):
    """A ray with d = 0 in the middle of a workgroup: its dirs, pts and dt (k >= 1) are NaN, its t is
    finite, and every other ray's bits are those of a run without it."""
    n, z = 11, 5
    c, clean = M.sample_case(n, S, True, zero_ray=z), M.sample_case(n, S, True)
    got, base = _sample_rays(capi, dev, c, c["noise"]), _sample_rays(capi, dev, clean, clean["noise"])
    _check_samples(got, c, c["noise"], "zero direction S %d" % S)
    assert np.isnan(got["dirs"][z]).all() and np.isnan(got["pts"][z]).all()
    assert np.isnan(got["dt"][z, 1:]).all() and np.isfinite(got["t"][z]).all()
    others = np.arange(n) != z
    for k in ("pts", "dirs", "dt", "t"):
        assert M.bits_equal(got[k][others], base[k][others]), k
    assert M.bits_equal(got["t"], base["t"])


@pytest.mark.parametrize("S", [17, 100])
def test_sample_dense_affine_with_a_clamped_noise_row(capi, dev, S):
    """noise_affine = 1 and noise_row entries outside [0, n_rays): the clamped row's t in bits (the
    multiplier (u - .5f) + 1.f through the f32 scan), x within contract_fwd_model's bound at
    f2n_sample_rays' point for the same multipliers, dt its dt bit for bit."""
    n = 9
    c = M.sample_case(n, S, True)
    u = (c["noise"] - F32(0.5)).astype(F32)                      # the raw draw in [0, 1)
    rows = np.array([3, -1, n, 0, n + 70, -2 ** 31, 2 ** 31 - 1, 8, 4], dtype=np.int32)
    clamped = np.clip(rows.astype(np.int64), 0, n - 1)
    mult = M.multipliers(u, affine=True)[clamped]
    N = n * S
    x, dt, t = _sent(dev, N + PAD, 3), _sent(dev, N + PAD), _sent(dev, N + PAD)
    bounds = torch.full((n + 3, 2), -1, dtype=torch.int32, device=dev)
    ray_dirs = _sent(dev, n + 3, 3)
    capi.call("sample_dense", _dev(dev, c["o"]), _dev(dev, c["d"]), _dev(dev, u), _dev(dev, rows), 1, x, dt,
              t, bounds, ray_dirs, n, S, c["step"])
    for b in (x, dt, t):
        assert _untouched(b, N)
    assert _untouched(ray_dirs, n) and bool((bounds[n:] == -1).all())
    full = _sample_rays(capi, dev, c, mult)
    got = dict(t=t[:N].cpu().numpy().reshape(n, S), dt=dt[:N].cpu().numpy().reshape(n, S),
               dirs=ray_dirs[:n].cpu().numpy())
    _check_samples(got, c, mult, "sample_dense S %d" % S)
    assert M.bits_equal(got["t"], full["t"]) and M.bits_equal(got["dt"], full["dt"])
    x64, E_x, zero = contract_fwd_model(torch.from_numpy(full["pts"].reshape(-1, 3)))
    assert not zero.any()
    assert M.within(x[:N].cpu().numpy(), x64, E_x).all()


# ---- (b) the probe ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("S", M.SAMPLE_S)
def test_probe_samples_are_sample_rays_samples_at_every_width(capi, dev, S, with_noise):
    """pts, dt and t of f2n_ray_walk_probe at 64, 16 and 8 lanes to a ray equal f2n_sample_rays' bit
    for bit (21 rays: the last wave of every mapping is partly empty; ray 11 has d = 0 and shares a
    wavefront with seven healthy ones at W = 8); depth and keep on random positive optical depths:
    the f32 restatement in bits, the float64 exclusive sum within BAR u D_k depth, the float64 keep
    rule outside the band, at most 2 % of the rays in the band."""
    for n_rays in M.SAMPLE_RAYS:        # the cases of (a)
        c = M.sample_case(n_rays, S, with_noise)
        base = _sample_rays(capi, dev, c, c["noise"])
        for W in M.WIDTHS:
            got = _probe(capi, dev, c, c["noise"], W)
            for k in ("pts", "dt", "t"):
                assert M.bits_equal(got[k], base[k]), (n_rays, W, k)
    c = M.sample_case(21, S, with_noise, zero_ray=11)
    base = _sample_rays(capi, dev, c, c["noise"])
    sec = M.random_sec(21, S)
    for W in M.WIDTHS:
        for s in (None, sec):
            got = _probe(capi, dev, c, c["noise"], W, s)
            for k in ("pts", "dt", "t"):
                assert _same_bits(got[k], base[k]), (W, k)
        fails = M.keep_failures(got["depth"], got["keep"], sec, W)
        assert fails == [], fails
        d64, E = M.depth_model(sec)
        print("probe S %d noise %d W %d: depth worst |err| / E %.2f, rays in the band %d" % (
            S, with_noise, W, M.ratio(got["depth"], d64, E),
            int(M.keep_model(sec, np.zeros_like(d64))["in_band"].sum())))


_stops = {}


def _stop(S):
    if S not in _stops:
        _stops[S] = M.stop_case(S)
    return _stops[S]


@pytest.mark.parametrize("S", M.STOP_S)
def test_probe_on_the_designed_stops(capi, dev, S):
    """The designed optical depths through keep_step at every width: depth in bits and within its
    bound, keep by the float64 rule with NO ray in the band, and the kept prefix is the target."""
    case = _stop(S)
    cond = M.stop_condition(case)
    assert not cond["in_band"].any() and np.array_equal(cond["kept"], case["target"])
    sec = M.stop_sec32(case)
    base = _sample_rays(capi, dev, case, case["noise"])
    for W in M.WIDTHS:
        got = _probe(capi, dev, case, case["noise"], W, sec)
        for k in ("pts", "dt", "t"):
            assert M.bits_equal(got[k], base[k]), (W, k)
        fails = M.keep_failures(got["depth"], got["keep"], sec, W, designed=True)
        assert fails == [], fails
        assert np.array_equal(M.kept_from_keep(got["keep"]), case["target"]), W
    _check_samples(base, case, case["noise"], "designed S %d" % S)


# ---- (c) the real march ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", M.STOP_S)
def test_march_stops_where_the_rays_were_designed_to(capi, dev, S):
    """f2n_density_march on MARCH routes 0, 1, 2 and f2n_density_march_occ with an all-ones grid keep
    exactly target_r samples on every designed ray (w0 = 0: logit == b0, sec_k = expf(b0 - shift)
    dt_k); kept stays -1 behind n_rays; f2n_bounds_from_counts + f2n_sample_compact on those counts
    write f2n_sample_rays' rows and nothing else."""
    case = _stop(S)
    cond = M.stop_condition(case)
    assert not cond["in_band"].any() and np.array_equal(cond["kept"], case["target"])
    R, step = case["n_rays"], case["step"]
    fld = util.make_field(seed=S, **M.STOP_FIELD)
    L, F = fld["L"], fld["F"]
    table16, primes = fld["table16"].to(dev), fld["primes"].to(dev)
    bias, mul = fld["bias"].to(dev), fld["mul"].to(dev)
    w0 = torch.zeros(L * F, device=dev)
    b0 = torch.tensor([M.STOP_B0], device=dev)
    o, d, noise = _dev(dev, case["o"]), _dev(dev, case["d"]), _dev(dev, case["noise"])
    want = case["target"].astype(np.int32)
    behind = np.full(3, -1, np.int32)
    for route in (0, 1, 2):
        kept = torch.full((R + 3,), -1, dtype=torch.int32, device=dev)
        with capi.option("MARCH", route):
            capi.call("density_march", o, d, noise, table16, primes, bias, mul, w0, b0, kept, R, S, step,
                      L, F, fld["T"], fld["stride"], M.THRESH, M.DENSITY_SHIFT)
        k = kept.cpu().numpy()
        assert np.array_equal(k[:R], want), (route, np.flatnonzero(k[:R] != want), k[:R], want)
        assert np.array_equal(k[R:], behind), route
    G = 32
    bits = torch.full((G ** 3 // 32,), -1, dtype=torch.int32, device=dev)
    kept_o = torch.full((R + 3,), -1, dtype=torch.int32, device=dev)
    len_o = torch.full((R + 3,), -1, dtype=torch.int32, device=dev)
    capi.call("density_march_occ", o, d, noise, table16, primes, bias, mul, w0, b0, bits, G, kept_o, len_o,
              R, S, step, L, F, fld["T"], fld["stride"], M.THRESH, M.DENSITY_SHIFT)
    for got in (kept_o, len_o):
        g = got.cpu().numpy()
        assert np.array_equal(g[:R], want) and np.array_equal(g[R:], behind)
    # the compacted rows
    bounds = torch.full((R + 3, 2), -1, dtype=torch.int32, device=dev)
    total = torch.full((1,), -1, dtype=torch.int32, device=dev)
    capi.call("bounds_from_counts", kept, bounds, total, R)
    n = int(want.sum())
    assert int(total.item()) == n and bool((bounds[R:] == -1).all())
    start = np.cumsum(want) - want
    assert np.array_equal(bounds[:R].cpu().numpy(), np.stack([start, start + want], 1))
    full = _sample_rays(capi, dev, case, case["noise"])
    out = [_sent(dev, n + PAD, 3), _sent(dev, n + PAD, 3), _sent(dev, n + PAD), _sent(dev, n + PAD)]
    capi.call("sample_compact", o, d, noise, bounds, *out, R, S, step)
    for name, a in zip(("pts", "dirs", "dt", "t"), out):
        a = a.cpu().numpy()
        exp = np.full_like(a, rc.SENTINEL)
        for r in range(R):
            exp[start[r]:start[r] + want[r]] = full[name][r, :want[r]]
        assert M.bits_equal(a, exp), name
