"""f2n_depth_splat on the GPU: a few hundred points, two cameras, an 8 x 6 image, once pinhole and
once with k1, k2, p1, p2 set.  The expected map is built in numpy from the pixels f2n_project_points
itself returns for the same points (the two entries share the device function, so the pixel
decisions must agree exactly) and the minimum of |p - t_cam| in float64.

Tolerance of a pixel holding distance d: 5 u d, u = 2^-24, counted from depth_splat.hip's order
d = sqrtf((dx*dx + dy*dy) + dz*dz) with dx = p - t: each difference carries one rounding (relative u,
so 2 u in its square), each square one, each of the two additions one: the radicand is known to 5 u
relative at the most, its root to 2.5 u, and the root's own rounding is allowed 2 u (one ulp).  A minimum
is 1-Lipschitz, so the bound of the elements is the bound of the minimum."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
H, W = 6, 8
LENSES = (None, ((0.05, -0.01, 0.002, -0.003), (-0.04, 0.02, -0.001, 0.004)))


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def _cameras():
    a = np.deg2rad(30.0)
    R1 = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    poses = np.zeros((2, 3, 4))
    poses[0, :, :3] = np.eye(3)
    poses[0, :, 3] = (0.1, -0.2, 0.3)
    poses[1, :, :3] = R1
    poses[1, :, 3] = (1.5, 0.25, -0.5)
    K = np.array([[6.0, 0, 4.0], [0, 6.5, 3.0], [0, 0, 1]])
    return poses.astype(np.float32), np.stack([K, K]).astype(np.float32)


def _back_project(poses, K, cam, row, col, depth):
    """world points that a pinhole camera images at the continuous pixel (row, col), `depth` in front"""
    x = (col - K[cam, 0, 2]) / K[cam, 0, 0]
    y = (row - K[cam, 1, 2]) / K[cam, 1, 1]
    c = np.stack([x * depth, -y * depth, -depth], 1)
    return np.einsum("nij,nj->ni", poses[cam, :, :3].astype(np.float64), c) + poses[cam, :, 3]


def _points(seed=11):
    """-> points [n,3] f32, cam [n] i32 and a tag per point"""
    rng = np.random.RandomState(seed)
    poses, K = _cameras()
    parts, tags = [], []

    def add(tag, cam, row, col, depth, flip=False):
        cam = np.asarray(cam)
        p = _back_project(poses, K, cam, np.asarray(row, float), np.asarray(col, float),
                          np.asarray(depth, float))
        if flip:                      # mirrored through the camera centre: behind it
            p = 2 * poses[cam, :, 3] - p
        parts.append((p, cam))
        tags.extend([tag] * len(cam))

    n = 160
    add("spread", rng.randint(0, 2, n), rng.uniform(0, H, n), rng.uniform(0, W, n), rng.uniform(1, 5, n))
    n = 24
    add("one_pixel", np.full(n, 1), 2.5 + rng.uniform(-.3, .3, n), 3.5 + rng.uniform(-.3, .3, n),
        rng.uniform(1, 5, n))
    n = 30
    add("behind", rng.randint(0, 2, n), rng.uniform(0, H, n), rng.uniform(0, W, n),
        rng.uniform(1, 5, n), flip=True)
    n = 40
    side = rng.randint(0, 4, n)
    row = np.where(side == 0, rng.uniform(-3, -0.01, n), np.where(side == 1, rng.uniform(H + .01, H + 3, n),
                                                                 rng.uniform(0, H, n)))
    col = np.where(side == 2, rng.uniform(-3, -0.01, n), np.where(side == 3, rng.uniform(W + .01, W + 3, n),
                                                                 rng.uniform(0, W, n)))
    add("outside", rng.randint(0, 2, n), row, col, rng.uniform(1, 5, n))
    n = 40                            # on pixel borders, the image's own included
    add("border", rng.randint(0, 2, n), rng.randint(0, H + 1, n).astype(float),
        rng.randint(0, W + 1, n).astype(float), 2.0 ** rng.randint(0, 3, n))
    n = 12
    add("bad_cam", np.zeros(n, dtype=int), rng.uniform(0, H, n), rng.uniform(0, W, n), rng.uniform(1, 5, n))
    pts = np.concatenate([p for p, _ in parts]).astype(np.float32)
    cam = np.concatenate([c for _, c in parts]).astype(np.int32)
    tags = np.array(tags)
    bad = np.flatnonzero(tags == "bad_cam")
    cam[bad] = np.resize(np.array([-1, 2, 3, 1000, -2 ** 31, 2 ** 31 - 1], dtype=np.int64), bad.size)
    order = rng.permutation(len(cam))
    return pts[order], cam[order], tags[order]


def _expected(capi, dev, pts, cam, poses, K, dist):
    """the map from f2n_project_points's own pixels and float64 distances, and its bound"""
    n, n_cams = pts.shape[0], poses.shape[0]
    in_range = (cam >= 0) & (cam < n_cams)
    safe = torch.from_numpy(np.where(in_range, cam, 0).astype(np.int32)).to(dev)
    pix = torch.empty(n, 2, device=dev)
    valid = torch.empty(n, dtype=torch.int32, device=dev)
    capi.call("project_points", torch.from_numpy(pts).to(dev), poses, 12, K, dist, n_cams, safe, pix,
              valid, n)
    pix, valid = pix.cpu().numpy(), valid.cpu().numpy()
    row, col = np.floor(pix[:, 0]), np.floor(pix[:, 1])
    hit = in_range & (valid == 1) & (row >= 0) & (row < H) & (col >= 0) & (col < W)
    t = poses.cpu().numpy().astype(np.float64)[np.where(in_range, cam, 0), :, 3]
    d = np.sqrt(((pts.astype(np.float64) - t) ** 2).sum(1))
    want = np.full((n_cams, H, W), np.inf)
    count = np.zeros((n_cams, H, W), dtype=int)
    for i in np.flatnonzero(hit):
        px = (cam[i], int(row[i]), int(col[i]))
        want[px] = min(want[px], d[i])
        count[px] += 1
    want[np.isinf(want)] = 0.0
    return want, count, hit


@pytest.mark.parametrize("lens", range(len(LENSES)))
def test_splat_against_project_points(host, capi, dev, lens):
    pts, cam, tags = _points()
    poses_np, K_np = _cameras()
    poses, K = torch.from_numpy(poses_np).to(dev), torch.from_numpy(K_np).to(dev)
    dist = None if LENSES[lens] is None else torch.tensor(LENSES[lens], device=dev)
    want, count, hit = _expected(capi, dev, pts, cam, poses, K, dist)
    # the set holds what the test is about
    assert 200 < len(cam) < 400 and count.max() >= 10 and (count > 1).sum() >= 10
    assert hit[tags == "spread"].mean() > 0.8 and not hit[tags == "behind"].any()
    assert not hit[tags == "bad_cam"].any() and hit[tags == "outside"].mean() < 0.2
    assert 0 < hit[tags == "border"].sum() < (tags == "border").sum()
    if LENSES[lens] is None:          # (a lens moves points across the image's edge)
        assert not hit[tags == "outside"].any()
    assert (want > 0).sum() > 40 and (want == 0).sum() > 5

    p_dev, c_dev = torch.from_numpy(pts).to(dev), torch.from_numpy(cam).to(dev)
    runs = []
    for _ in range(2):
        depth = torch.full((2, H, W), float("nan"), device=dev)       # every element is written
        capi.call("depth_splat", p_dev, c_dev, poses, 12, K, dist, 2, H, W, depth, len(cam))
        runs.append(depth)
    assert torch.equal(runs[0], runs[1])                               # (no NaN left: equal bits)
    got = runs[0].cpu().numpy()
    assert np.isfinite(got).all() and (got >= 0).all()
    assert np.array_equal(got > 0, want > 0)                           # the same pixels, exactly
    err, tol = np.abs(got.astype(np.float64) - want), 5 * U * want
    print("  lens %d: %d pixels hit, largest err / (u d) = %.3f" % (
        lens, int((want > 0).sum()), float((err[want > 0] / (U * want[want > 0])).max())))
    assert (err <= tol).all()

    # the host function is that entry; [4,4] poses give the same bits
    assert torch.equal(host.splat_depth(p_dev, c_dev, poses, K, dist, H, W), runs[0])
    poses4 = torch.cat([poses, torch.tensor([0., 0, 0, 1], device=dev).expand(2, 1, 4)], 1)
    assert torch.equal(host.splat_depth(p_dev, c_dev, poses4, K, dist, H, W), runs[0])
    # no points: all zeros
    none = torch.full((2, H, W), float("nan"), device=dev)
    capi.call("depth_splat", p_dev, c_dev, poses, 12, K, dist, 2, H, W, none, 0)
    assert bool((none == 0).all())


def test_gather_depth_is_plain_indexing(host, dev):
    g = torch.Generator().manual_seed(3)
    maps = torch.rand(3, H, W, generator=g).to(dev)
    n = 50
    cam = torch.randint(0, 3, (n,), generator=g, dtype=torch.int32).to(dev)
    ij = torch.stack([torch.randint(0, H, (n,), generator=g), torch.randint(0, W, (n,), generator=g)],
                     1).to(torch.int32).to(dev)
    got = host.gather_depth(maps, cam, ij)
    assert got.shape == (n,) and got.is_contiguous()
    assert torch.equal(got, maps[cam.long(), ij[:, 0].long(), ij[:, 1].long()])
