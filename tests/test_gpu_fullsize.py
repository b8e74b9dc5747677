"""BASELINE.json full sizes (config C2: 65 536 rays x 128 samples = 8.4 M samples per chunk, L = 16,
F = 2, T = 2^19), checked through size-independent properties instead of the oracle (which would need
minutes): partition of unity of the trilinear weights, conservation in the compositing, agreement of
independent kernel implementations of the same operator, permutation equivariance."""
import importlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

L, F, LOG2T, S, R = 16, 2, 19, 128, 65536
T = 1 << LOG2T
C = L * F
N = R * S


@pytest.fixture(scope="module")
def field(capi, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    numel = T * L * F
    table = torch.randn(numel, device=dev, generator=g) * 0.1
    table16 = torch.empty(numel, dtype=torch.int16, device=dev)
    capi.call("table_to_f16", table, table16, numel)
    primes = (torch.randint(1 << 28, 1 << 30, (L, 3), device=dev, generator=g) | 1).to(torch.int32)
    bias = torch.rand(L, 3, device=dev, generator=g) * 1000 + 100
    mul = torch.tensor([2.0 ** (7.0 * l / (L - 1) + 3.0) for l in range(L)], device=dev)
    o = torch.randn(R, 3, device=dev, generator=g) * 0.3
    d = torch.randn(R, 3, device=dev, generator=g)
    noise = torch.rand(R, S, device=dev, generator=g) + 0.5
    return dict(table16=table16, primes=primes, bias=bias, mul=mul, o=o, d=d, noise=noise, g=g)


def _samples(capi, dev, f):
    pts, dirs = torch.empty(N, 3, device=dev), torch.empty(N, 3, device=dev)
    dt, t = torch.empty(N, device=dev), torch.empty(N, device=dev)
    b = torch.empty(R, 2, dtype=torch.int32, device=dev)
    capi.call("sample_rays", f["o"], f["d"], f["noise"], pts, dirs, dt, t, b, R, S, 4.0 / S)
    x = torch.empty_like(pts)
    capi.call("contract_fwd", pts, x, N)
    return pts, dirs, dt, t, b, x


def test_sampler_and_contraction_invariants(capi, dev, field):
    pts, dirs, dt, t, b, x = _samples(capi, dev, field)
    tt = t.reshape(R, S)
    assert (tt[:, 1:] > tt[:, :-1]).all()                    # t strictly increasing along a ray
    assert (dt >= 0).all() and (dt.reshape(R, S)[:, 0] == 0).all()
    assert torch.allclose(dirs.norm(dim=1), torch.ones(N, device=dev), atol=1e-5)
    assert float(x.norm(dim=1).max()) < 2.0                  # contraction maps into the radius-2 ball
    inside = pts.norm(dim=1) <= 1
    assert torch.equal(x[inside], pts[inside])               # identity inside the unit ball
    assert torch.equal(b[:, 1] - b[:, 0], torch.full((R,), S, dtype=torch.int32, device=dev))


def test_hash_fwd_bwd_properties(capi, dev, field):
    f = field
    pts, dirs, dt, t, b, x = _samples(capi, dev, f)
    args = (f["table16"], f["primes"], f["bias"], f["mul"])
    enc_cm = torch.empty(C, N, device=dev)
    capi.call("hash_fwd", x, *args, enc_cm, 1, N, None, N, L, F, T, T)
    # permutation equivariance + layout independence: shuffled points, row-major output
    perm = torch.randperm(N, device=dev)
    enc_rm = torch.empty(N, C, device=dev)
    capi.call("hash_fwd", x[perm].contiguous(), *args, enc_rm, C, 1, None, N, L, F, T, T)
    assert torch.equal(enc_rm, enc_cm.t()[perm])
    # a blend of table values cannot leave their range (weights are a partition of unity)
    tmax = float(f["table16"].view(torch.float16).float().abs().max())
    assert float(enc_cm.abs().max()) <= tmax * (1 + 1e-3)

    # backward: three independent implementations of the same scatter agree
    g = torch.randn(C, N, device=dev, generator=f["g"]) * 1e-3
    numel = T * L * F
    outs = {}
    need = capi.lib().cdll.f2n_hash_bwd_workspace_bytes(N, L, F, T)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    tg = torch.zeros(numel, device=dev)
    capi.call("hash_bwd_binned", x, f["primes"], f["bias"], f["mul"], g, 1, N, tg, N, L, F, T, T,
              128.0, ws, need)
    outs["binned"] = tg
    del ws
    for mode in ("sliced", "atomic"):
        with capi.option("HASH_BWD", {"atomic": 1, "sliced": 2}[mode]):
            tg = torch.zeros(numel, device=dev)
            capi.call("hash_bwd", x, *args, g, 1, N, tg, None, N, L, F, T, T, 128.0)
        outs[mode] = tg
    scale = float(outs["binned"].abs().max())
    for mode in ("sliced", "atomic"):
        assert float((outs[mode] - outs["binned"]).abs().max()) <= 2e-5 * scale, mode
    # the binned path sums exactly in fixed point; only region overflow (coarse levels, applied with
    # float atomics) is order dependent, so two runs agree to rounding of those few entries
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    tg2 = torch.zeros(numel, device=dev)
    capi.call("hash_bwd_binned", x, f["primes"], f["bias"], f["mul"], g, 1, N, tg2, N, L, F, T, T,
              128.0, ws, need)
    assert float((tg2 - outs["binned"]).abs().max()) <= 1e-6 * scale
    assert float((tg2 != outs["binned"]).float().mean()) < 0.05
    # checksum: sum_d w_d = 1, so the whole table gradient sums to the sum of the f16-quantised
    # incoming gradient, up to the f16 rounding of each contribution (relative 2^-11, random sign)
    total_in = (g.float() * 128).to(torch.float16).double().sum() / 128
    total_out = outs["binned"].double().sum()
    budget = float(g.abs().double().sum()) * 2 ** -11 * 0.05   # 5 % of the worst case (all one sign)
    assert abs(float(total_out - total_in)) <= budget + 1e-9


def test_first_pass_kernels_agree_and_composite_conserves(capi, dev, field):
    f = field
    H = importlib.import_module("f2-nerf_amd").load_host()
    H.manual_seed(5)
    ren = H.Renderer(4, n_levels=L, n_channels=F, log2_table=LOG2T, max_samples=S, step=4.0 / S)
    p = ren.named_parameters()
    with torch.no_grad():
        p["scene_field.feat_pool"].normal_(0, 0.1)
        p["scene_field.mlp.bias"][0] = 5.0              # rays terminate part-way
    o, d, noise = f["o"], f["d"], f["noise"]
    bg = torch.rand(R, 3, device=dev, generator=f["g"])
    emb = torch.zeros(R, dtype=torch.int32, device=dev)
    outs = []
    for dense in (0, 1):
        ren.set_dense_first_pass(dense)
        with torch.no_grad():
            c, dep, w, idx = ren.render(o, d, emb, "train", noise, bg)
        outs.append((c, dep, w, idx))
    # the early-terminating march and the encode-once dense pass find the same kept prefix
    assert torch.equal(outs[0][3], outs[1][3])
    # ... and so do the march's older routes (one ray per wavefront, four rays per wavefront)
    ren.set_dense_first_pass(0)
    for route in (1, 2):
        with capi.option("MARCH", route), torch.no_grad():
            _, _, _, idx_r = ren.render(o, d, emb, "train", noise, bg)
        assert torch.equal(idx_r, outs[0][3]), route
    assert torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][0], outs[1][0])
    c, dep, w, idx = outs[0]
    cnt = (idx[:, 1] - idx[:, 0])
    assert int(cnt.min()) >= 1 and int(cnt.max()) <= S and int(cnt.sum()) == w.numel()
    assert int((cnt < S).sum()) > R // 2                 # most rays did terminate
    # conservation: sum_k w_k + T_last = 1 per ray, and colours are a convex blend -> within [-eps, 1+eps]
    wsum = H.flex_sum(w, idx)
    # T_last from the colours with a white / black background pair
    with torch.no_grad():
        c1, _, _, _ = ren.render(o, d, emb, "train", noise, torch.ones(R, 3, device=dev))
        c0, _, _, _ = ren.render(o, d, emb, "train", noise, torch.zeros(R, 3, device=dev))
    t_last = (c1 - c0)[:, 0]
    assert float((wsum + t_last - 1).abs().max()) < 2e-5
    assert float(c0.min()) >= -1e-3 - 1e-6 and float(c1.max()) <= 1 + 1e-3 + 1e-5
    # terminated rays stop exactly where transmittance crosses 1e-4: T_last of a cut ray is tiny
    cut = cnt < S
    assert float(t_last[cut].max()) < 1e-3


# ------------------------------------------------------------------- BASELINE config C5 ----------
# T = 2^22 rows per level, L = 16, F = 8, non-overlapping level stride: a 1 GiB f16 table.

C5 = dict(L=16, F=8, LOG2T=22)


@pytest.fixture(scope="module")
def field_c5(capi, dev):
    L5, F5, T5 = C5["L"], C5["F"], 1 << C5["LOG2T"]
    g = torch.Generator(device=dev).manual_seed(5)
    numel = T5 * L5 * F5
    table = torch.randn(numel, device=dev, generator=g) * 0.1
    table16 = torch.empty(numel, dtype=torch.int16, device=dev)
    capi.call("table_to_f16", table, table16, numel)
    del table
    primes = (torch.randint(1 << 28, 1 << 30, (L5, 3), device=dev, generator=g) | 1).to(torch.int32)
    bias = torch.rand(L5, 3, device=dev, generator=g) * 1000 + 100
    mul = torch.tensor([2.0 ** (7.0 * l / (L5 - 1) + 3.0) for l in range(L5)], device=dev)
    return dict(table16=table16, primes=primes, bias=bias, mul=mul, numel=numel, g=g)


def _ball(n, dev, g):
    dd = torch.randn(n, 3, device=dev, generator=g)
    return (dd / dd.norm(dim=1, keepdim=True) *
            torch.rand(n, 1, device=dev, generator=g) ** (1 / 3) * 2).contiguous()


def test_config_c5_forward_and_backward_against_oracle(capi, dev, field_c5):
    """Config C5 at its own table size against the CPU oracle: hash rows and f16 features bit-exact on
    24 000 points, the two-level binned backward (2048 slices per level) on 70 000 points."""
    from oracle import kernels as K
    f = field_c5
    L5, F5, T5 = C5["L"], C5["F"], 1 << C5["LOG2T"]
    st = T5 * F5
    C5c = L5 * F5
    t16 = f["table16"].cpu()
    primes, bias, mul = f["primes"].cpu(), f["bias"].cpu(), f["mul"].cpu()
    n = 24000
    x = _ball(n, dev, f["g"])
    out = torch.empty(n, C5c, device=dev)
    idx = torch.empty(n, L5, 8, dtype=torch.int32, device=dev)
    capi.call("hash_fwd", x, f["table16"], f["primes"], f["bias"], f["mul"], out, C5c, 1, idx, n, L5,
              F5, T5, st)
    ref_out, ref_idx = K.hash_fwd(x.cpu(), t16, primes, bias, mul, L5, F5, T5, st, want_idx=True)
    assert torch.equal(idx.cpu().to(torch.int64) & 0xffffffff, ref_idx.to(torch.int64) & 0xffffffff)
    assert torch.equal(out.cpu(), ref_out)

    n = 70000
    x = _ball(n, dev, f["g"])
    grad = torch.randn(C5c, n, device=dev, generator=f["g"]) * 1e-3
    need = capi.lib().cdll.f2n_hash_bwd_workspace_bytes(n, L5, F5, T5)
    assert need > 0, "the binned backward must cover config C5 (VERDICT r1 item 3)"
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    tg = torch.zeros(f["numel"], device=dev)
    capi.call("hash_bwd_binned", x, f["primes"], f["bias"], f["mul"], grad, 1, n, tg, n, L5, F5, T5,
              st, 128.0, ws, need)
    ref_tg, _ = K.hash_bwd(x.cpu(), t16, primes, bias, mul, grad.t().contiguous().cpu(), f["numel"],
                           L5, F5, T5, st, 128.0, parallel=True)
    got = tg.cpu()
    scale = ref_tg.abs().max().item()
    # (No element-wise check against K.hash_bwd_exact here: its per-level sums are [L, T*F] int64 --
    # 4 GiB each for S and A at this shape, 2 GiB for N, and the float64 composition of the 2^29
    # table elements needs several times that again, 25 GiB and more of host memory for one test.
    # tests/test_gpu_ops.py makes that check on the same two-level route at T = 2^18 .. 2^21.)
    assert (got - ref_tg).abs().max().item() <= 2e-5 * scale
    assert ((got - ref_tg).norm() / ref_tg.norm()).item() < 1e-5


def test_config_c5_full_batch_properties(capi, dev, field_c5):
    """2^22 points of config C5 (a quarter of its batch; 8.6 GB of encodings for the full 2^24 would
    only repeat this): the binned backward runs in several rounds over the points inside a 20 GiB
    workspace and must (a) agree with the scattered-atomic kernel, (b) conserve the gradient
    (sum_d w_d = 1), (c) be bitwise reproducible: exact fixed-point sums, with the records that find
    a queue or run full (coarse levels: uniformly random points hit only ~36 000 distinct rows of
    level 0, so some slices see several times the mean record count) summed exactly too, through the
    overflow arena -- the counter of f2n_hash_bwd_set_overflow_counter must read 0."""
    f = field_c5
    L5, F5, T5 = C5["L"], C5["F"], 1 << C5["LOG2T"]
    st = T5 * F5
    C5c = L5 * F5
    n = 1 << 22
    x = _ball(n, dev, f["g"])
    g = torch.randn(C5c, n, device=dev, generator=f["g"]) * 1e-3
    need = capi.lib().cdll.f2n_hash_bwd_workspace_bytes(n, L5, F5, T5)
    assert 0 < need <= (64 << 30) + 4096        # the cap include/f2nerf_hip.h documents
    need = min(need, 20 << 30)          # less than one round's worth: at least two rounds
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    overflow = torch.zeros(1, dtype=torch.int64, device=dev)
    assert capi.lib().cdll.f2n_hash_bwd_set_overflow_counter(overflow.data_ptr()) == 0
    outs = []
    try:
        for _ in range(2):
            tg = torch.zeros(f["numel"], device=dev)
            capi.call("hash_bwd_binned", x, f["primes"], f["bias"], f["mul"], g, 1, n, tg, n, L5, F5, T5,
                      st, 128.0, ws, need)
            outs.append(tg)
        torch.cuda.synchronize()
    finally:
        capi.lib().cdll.f2n_hash_bwd_set_overflow_counter(None)
    del ws
    assert int(overflow.item()) == 0                  # nothing was applied with a float atomic
    assert torch.equal(outs[0], outs[1])              # exact sums: independent of summation order
    scale = float(outs[0].abs().max())
    with capi.option("HASH_BWD", 1):
        ta = torch.zeros(f["numel"], device=dev)
        capi.call("hash_bwd", x, f["table16"], f["primes"], f["bias"], f["mul"], g, 1, n, ta, None, n,
                  L5, F5, T5, st, 128.0)
    assert float((ta - outs[0]).abs().max()) <= 2e-5 * scale
    total_in = (g.float() * 128).to(torch.float16).double().sum() / 128
    total_out = outs[0].double().sum()
    budget = float(g.abs().double().sum()) * 2 ** -11 * 0.05
    assert abs(float(total_out - total_in)) <= budget + 1e-9
