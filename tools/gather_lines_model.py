#!/usr/bin/env python3
"""CPU model of what one gather instruction of hash_fwd_raytile_kernel asks of the memory system:
the number of distinct 128-byte table lines among its 64 lanes, per level, with the 8 corner loads of
a sample in corner order (F2N_OPT_GATHER_PAIRED = 1: load d fetches corner d of the lane's own cell)
and in vertex-parity order (= 0: load j fetches the vertex whose coordinate parities are j).

  python tools/gather_lines_model.py [--tiles 24] [--seed 0]

The tiles are the benchmark's: views of fox_like_poses (bench.py), 800 x 800 at focal 1111.1,
S = 128 samples in steps of 4/128 with the TRAIN jitter U[0.5, 1.5), contracted; levels
mul_l = 2^(7 l / 15 + 3), biases U[100, 1100), odd 30-bit multipliers, T = 2^19 rows of F = 2 f16
(4 bytes: 32 rows per line).  A tile is 64 rays x 32 samples; its 2048 (ray, sample) pairs are taken
64 at a time in the kernel's depth order (counting sort into 64 bins along the middle ray).  The 64
rays are an 8 x 8 pixel bundle (what the Renderer's bucketing hands the kernel) or a 64-pixel strip
of one image row (rays in the caller's order).  numpy only."""
import argparse
import math

import numpy as np

L, F, LOG2_T, S, TILE_S, RAYS = 16, 2, 19, 128, 32, 64
H = W = 800
FOCAL = 1111.1
ROWS_PER_LINE = 128 // (2 * F)


def fox_like_poses(n, rng):
    """bench.py's arc of cameras (heights from this generator, not torch's)"""
    ang = np.linspace(-100.0, 100.0, n) * math.pi / 180.0
    pos = np.stack([np.cos(ang), np.sin(ang), rng.random(n) * 0.4 - 0.2], 1)
    zc = pos / np.linalg.norm(pos, axis=1, keepdims=True)
    xc = np.cross(np.broadcast_to([0.0, 0.0, 1.0], (n, 3)), zc)
    xc /= np.linalg.norm(xc, axis=1, keepdims=True)
    yc = np.cross(zc, xc)
    center = pos.mean(0)
    radius = np.linalg.norm(pos - center, axis=1).max()
    return np.stack([xc, yc, zc], 2), (pos - center) / radius      # R [n,3,3], t [n,3]


def tile_points(R, t, rows, cols, k0, rng):
    """contracted sample positions [64, 32, 3] of the rays through pixels (rows, cols), samples
    k0 .. k0 + 31 of 128"""
    cam = np.stack([((cols + .5) - W / 2) / FOCAL, -(((rows + .5) - H / 2) / FOCAL), -np.ones(RAYS)], 1)
    d = cam @ R.T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tk = np.cumsum(rng.random((RAYS, S)) + 0.5, 1) * (4.0 / S)
    p = t[None, None, :] + d[:, None, :] * tk[:, k0:k0 + TILE_S, None]
    nrm = np.linalg.norm(p, axis=2, keepdims=True)
    return np.where(nrm <= 1.0, p, (2.0 - 1.0 / nrm) * p / nrm).astype(np.float32)


def depth_order(p):
    """the kernel's counting sort: pair = ray * 32 + sample, 64 bins along the middle ray"""
    mr = RAYS // 2
    a = p[mr, TILE_S - 1] - p[mr, 0]
    inv = 64.0 / max(float(a @ a), 1e-30)
    depth = ((p - p[mr, 0]) @ a) * inv
    bins = np.clip(depth.astype(np.int64), 0, 63).reshape(-1)
    return np.argsort(bins, kind="stable")


def lines_per_instruction(p, order, mul, bias, primes):
    """mean over the tile's 32 x 8 gather instructions of distinct lines, (corner order, parity order)"""
    pts = p.reshape(-1, 3)[order].reshape(-1, 64, 3)                       # [32 instr, 64 lanes, 3]
    c = np.floor(pts * np.float32(mul) + bias.astype(np.float32))
    c = np.maximum(c, 0).astype(np.uint64)
    T = np.uint64(1 << LOG2_T)
    now = paired = 0
    for j in range(8):
        bits = np.array([(j >> 2) & 1, (j >> 1) & 1, j & 1], dtype=np.uint64)
        for scheme in ("now", "paired"):
            # corner order: vertex = cell + bits; parity order: the vertex of the cell with parities = bits
            off = bits if scheme == "now" else (bits ^ (c & np.uint64(1)))
            v = (c + off) * primes
            h = (v[..., 0] ^ v[..., 1] ^ v[..., 2]) & np.uint64(0xffffffff)
            line = (h % T) // np.uint64(ROWS_PER_LINE)
            n = sum(len(np.unique(line[i])) for i in range(line.shape[0]))
            if scheme == "now":
                now += n
            else:
                paired += n
    k = 8.0 * pts.shape[0]
    return now / k, paired / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=24)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    Rs, ts = fox_like_poses(50, rng)
    mul = [2.0 ** (7.0 * l / (L - 1) + 3.0) for l in range(L)]
    bias = rng.random((L, 3)) * 1000.0 + 100.0
    primes = (rng.integers(1 << 28, 1 << 30, (L, 3)) | 1).astype(np.uint64)
    acc = np.zeros((2, L, 2))                                              # [bundle | strip, level, scheme]
    for _ in range(args.tiles):
        v = int(rng.integers(50))
        k0 = int(rng.integers(S // TILE_S)) * TILE_S
        r0, c0 = int(rng.integers(H - 8)), int(rng.integers(W - 64))
        i = np.arange(RAYS)
        shapes = ((r0 + i // 8, c0 + i % 8), (np.full(RAYS, r0), c0 + i))
        for s, (rows, cols) in enumerate(shapes):
            p = tile_points(Rs[v], ts[v], rows.astype(np.float64), cols.astype(np.float64), k0, rng)
            order = depth_order(p)
            for l in range(L):
                acc[s, l] += lines_per_instruction(p, order, mul[l], bias[l], primes[l])
    acc /= args.tiles
    print("distinct 128-byte lines per gather instruction (64 lanes), mean of %d tiles" % args.tiles)
    print("level | 8x8 bundle: corner  parity | 64-pixel strip: corner  parity | ratio bundle  strip")
    for l in range(L):
        print("%5d | %18.1f %7.1f | %22.1f %7.1f | %12.2f %6.2f" %
              (l, acc[0, l, 0], acc[0, l, 1], acc[1, l, 0], acc[1, l, 1],
               acc[0, l, 1] / acc[0, l, 0], acc[1, l, 1] / acc[1, l, 0]))
    tot = acc.sum(1)
    print("  sum | %18.1f %7.1f | %22.1f %7.1f | %12.2f %6.2f" %
          (tot[0, 0], tot[0, 1], tot[1, 0], tot[1, 1], tot[0, 1] / tot[0, 0], tot[1, 1] / tot[1, 0]))


if __name__ == "__main__":
    main()
