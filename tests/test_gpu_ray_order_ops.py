"""The ray-order entry points called directly (tests/test_gpu_ray_order.py reaches them only through
the Renderer, comparing two GPU routes with each other): f2n_ray_keys against a numpy f32
restatement, key for key; f2n_ray_permute, f2n_gather_rows (both code paths), f2n_gather_segments
and f2n_counts_through against plain indexing, bit for bit."""
import numpy as np
import pytest
import torch

from tests import ragged_cases as rc

pytestmark = pytest.mark.gpu


def _sent(dev, *shape, dtype=torch.float32):
    return torch.full(shape, rc.SENTINEL, dtype=dtype, device=dev)


def _same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _key_directions():
    g = np.random.RandomState(4)
    d = [g.randn(10000, 3)]
    eye = np.eye(3)
    d.append(np.concatenate([eye, -eye]))                                   # the six axes
    ties = []
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            for sz in (1.0, -1.0):
                ties.append([sx, sy, sz])                                   # three-way ties
                for small in (0.25, 0.0):                                   # two-way ties, each pair
                    ties += [[sx, sy, small * sz], [sx, small * sy, sz], [small * sx, sy, sz]]
    d.append(np.array(ties) * 0.7)
    edge = []
    for major in range(3):                                                  # u or v exactly +-1
        for su in (1.0, -1.0):
            for v in (0.3, -1.0, 1.0):
                e = np.zeros(3)
                e[major], e[(major + 1) % 3], e[(major + 2) % 3] = 2.0, 2.0 * su, 2.0 * v
                edge.append(e)
    d.append(np.array(edge))
    d.append(g.randn(500, 3) * 1e-41)                                       # denormal components
    d.append(g.randn(500, 3) * 1e-45)                                       # one or two denormal ulps
    big = g.uniform(-1.0, 1.0, (500, 3)) * 3.0e38
    d.append(big)
    d.append(np.array([[3.0e38, -3.0e38, 3.0e38], [3.4e38, 1.0, -2.0], [-3.4028234e38, 0.0, 1.0]]))
    inf, nan = np.inf, np.nan
    d.append(np.array([[0, 0, 0], [0.0, -0.0, 0.0], [inf, 1, 0], [1, -inf, 0], [1, 2, inf],
                       [-inf, inf, inf], [nan, 1, 0], [1, nan, 0], [1, 0, nan], [nan, nan, nan],
                       [nan, inf, 1], [0, 0, 1e-45], [0, 5, 0]]))
    return np.concatenate(d).astype(np.float32)


def test_ray_keys_equal_the_f32_restatement(capi, dev):
    """Face choice with its >= tie order, u and v (one correctly rounded division each), the
    quantisation (a multiply by 1/2, an add, a power-of-two scale), the Hilbert index and the face
    bits: every step is exact or correctly rounded on both sides, so the keys are EQUAL."""
    d = _key_directions()
    n = d.shape[0]
    keys = torch.full((n + 3,), -5, dtype=torch.int32, device=dev)
    capi.call("ray_keys", torch.from_numpy(d).to(dev), keys, n)
    got = keys.cpu().numpy()
    assert np.all(got[n:] == -5)
    want = rc.ray_keys_ref(d)
    bad = np.flatnonzero(got[:n] != want)
    assert bad.size == 0, (bad[:5], d[bad[:5]], got[bad[:5]], want[bad[:5]])
    assert np.all(got[:n] >= 0)
    special = ~np.isfinite(d).all(1) | (np.abs(d).max(1) == 0)
    assert special.sum() >= 11 and np.all(got[:n][special] == 0)
    assert len(set((got[:n] >> 28).tolist())) == 6 and (got[:n] >> 28).max() == 5


@pytest.mark.parametrize("S", [3, 128])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("opt", ["all", "none", "emb", "bg", "noise"])
def test_ray_permute_is_indexing(capi, dev, n, S, opt):
    g = torch.Generator().manual_seed(n + S)
    order = torch.randperm(n, generator=g)
    o, d = torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)
    emb = torch.randint(0, 9, (n,), generator=g, dtype=torch.int32) if opt in ("all", "emb") else None
    bg = torch.rand(n, 3, generator=g) if opt in ("all", "bg") else None
    noise = torch.rand(n, S, generator=g) if opt in ("all", "noise") else None
    to = lambda x: None if x is None else x.to(dev)
    perm = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
    inv = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
    o_p, d_p = _sent(dev, n + 1, 3), _sent(dev, n + 1, 3)
    emb_p = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
    bg_p, noise_p = _sent(dev, n + 1, 3), _sent(dev, n + 1, S)
    capi.call("ray_permute", order.to(dev), n, S, to(o), to(d), to(emb), to(bg), to(noise), perm, o_p,
              d_p, emb_p if emb is not None else None, bg_p if bg is not None else None,
              noise_p if noise is not None else None, inv)
    assert torch.equal(perm[:n].cpu(), order.to(torch.int32)) and int(perm[n]) == -1
    assert torch.equal(inv.cpu()[:n][order], torch.arange(n, dtype=torch.int32)) and int(inv[n]) == -1
    assert _same_bits(o_p[:n], o[order]) and _same_bits(d_p[:n], d[order])
    assert bool((o_p[n] == rc.SENTINEL).all()) and bool((d_p[n] == rc.SENTINEL).all())
    if emb is not None:
        assert torch.equal(emb_p[:n].cpu(), emb[order])
    if bg is not None:
        assert _same_bits(bg_p[:n], bg[order])
    if noise is not None:
        assert _same_bits(noise_p[:n], noise[order])
    # absent inputs leave their outputs alone, and every row past n stays as it was
    assert int(emb_p[n]) == -1 and (emb is not None or bool((emb_p == -1).all()))
    assert bool((bg_p[n] == rc.SENTINEL).all()) and (bg is not None or bool((bg_p == rc.SENTINEL).all()))
    assert bool((noise_p[n] == rc.SENTINEL).all())
    assert noise is not None or bool((noise_p == rc.SENTINEL).all())


@pytest.mark.parametrize("row_floats,offset", [(4, 0), (128, 0), (132, 0), (1, 0), (3, 0), (130, 0),
                                               (4, 1), (128, 1)])
@pytest.mark.parametrize("n", [1, 257])
def test_gather_rows_both_paths(capi, dev, n, row_floats, offset):
    """row_floats % 4 == 0 with 16-byte aligned pointers: the float4 kernel; otherwise, or from a
    source view one float off alignment, the scalar kernel.  dst row i == src row map[i]; the inverse
    map restores the source."""
    g = torch.Generator().manual_seed(n * row_floats + offset)
    store = torch.randn(n * row_floats + offset + 4, generator=g).to(dev)
    src = store[offset:offset + n * row_floats].view(n, row_floats)
    assert src.data_ptr() % 16 == (4 * offset) % 16
    perm = torch.randperm(n, generator=g).to(torch.int32)
    inv = torch.empty_like(perm)
    inv[perm.long()] = torch.arange(n, dtype=torch.int32)
    dst = _sent(dev, n + 1, row_floats)
    capi.call("gather_rows", src, dst, perm.to(dev), n, row_floats)
    assert _same_bits(dst[:n], src.cpu()[perm.long()])
    assert bool((dst[n] == rc.SENTINEL).all())
    back = _sent(dev, n + 1, row_floats)
    capi.call("gather_rows", dst, back, inv.to(dev), n, row_floats)
    assert _same_bits(back[:n], src) and bool((back[n] == rc.SENTINEL).all())


@pytest.mark.parametrize("src_name,dst_name", [("tile", "gaps"), ("unordered", "tile"),
                                               ("gaps", "unordered")])
def test_gather_segments_and_counts_through(capi, dev, src_name, dst_name):
    """Segments of the stride-edge lengths (empty rays, 64 / 65 / 4097 samples) moved between two
    layouts under a random ray permutation: dst segment i = src segment map[i] bit for bit, the
    sentinel kept outside the destination ranges; counts_through then bounds_from_counts reproduces
    the caller-order bounds."""
    src_lay = rc.layout(src_name)
    R = src_lay.n_rays
    g = torch.Generator().manual_seed(R)
    perm = torch.randperm(R, generator=g)
    # destination ray i holds source ray perm[i]: same lengths, laid out in dst_name's manner
    lens = src_lay.len[perm.numpy()]
    rng = np.random.RandomState(R + len(dst_name))
    order = rng.permutation(R) if dst_name == "unordered" else np.arange(R)
    gaps = np.zeros(R, dtype=np.int64) if dst_name == "tile" else rng.choice([0, 1, 5], size=R)
    start = np.zeros(R, dtype=np.int64)
    pos = 0
    for r in order:
        pos += int(gaps[r])
        start[r] = pos
        pos += int(lens[r])
    n_dst = pos + 64
    dst_bounds = torch.from_numpy(np.stack([start, start + lens], 1).astype(np.int32)).contiguous()
    dst_lay = rc.Layout(dst_bounds, np.zeros(R), n_dst)
    src = torch.randn(src_lay.n_total, generator=g)
    dst = _sent(dev, n_dst)
    map32 = perm.to(torch.int32).to(dev)
    capi.call("gather_segments", src.to(dev), src_lay.bounds.to(dev), dst, dst_bounds.to(dev), map32, R)
    want = np.full(n_dst, rc.SENTINEL, np.float32)
    for i in range(R):
        j = int(perm[i])
        want[start[i]:start[i] + lens[i]] = src.numpy()[src_lay.start[j]:src_lay.end[j]]
    got = dst.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert (dst_lay.len == 0).sum() >= 4 and {64, 65, 4097} <= set(lens.tolist())

    counts = torch.full((R + 1,), -1, dtype=torch.int32, device=dev)
    capi.call("counts_through", src_lay.bounds.to(dev), map32, counts, R)
    assert torch.equal(counts[:R].cpu(), torch.from_numpy(lens.astype(np.int32))) and int(counts[R]) == -1
    bounds = torch.full((R, 2), -1, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int32, device=dev)
    capi.call("bounds_from_counts", counts[:R].contiguous(), bounds, total, R)
    cum = np.cumsum(lens)
    assert np.array_equal(bounds.cpu().numpy(), np.stack([cum - lens, cum], 1).astype(np.int32))
    assert int(total.item()) == int(cum[-1])
