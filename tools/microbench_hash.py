#!/usr/bin/env python3
"""Kernel-level micro-benchmark of the hash-grid kernels through the C ABI (ctypes), timed with
torch.cuda events on the current stream (the stream the kernels are launched on).

  python tools/microbench_hash.py [--config c2|c5|c1] [--n N] [--reps R]
  python tools/microbench_hash.py --corner-order [--levels 0,4,8,10,12,14,15] [--reps R]

--corner-order: f2n_hash_fwd_raytile on the contracted points of one chunk of the benchmark's
headline (65 536 rays of an 800 x 800 view in pixel-compact bundles, 128 jittered samples), ONE level
at a time (L = 1 with that level's mul), with the corner loads in corner order (GATHER_PAIRED = 1) and
in vertex-parity order (= 0), the two arms alternating call by call; one JSON line per level, to be
set beside the line counts of tools/gather_lines_model.py.

--level-groups: f2n_hash_fwd_raytile_groups on the same chunk with all 16 levels (the reference's
overlapping stride), under each schedule of --groups and on the one-level-per-workgroup route
(RAYTILE = 32), the arms alternating call by call, nine calls each; one JSON line per arm.
--rays N takes the chunk's first N rays (fewer tiles), --random-rays the reference's own batch of 512
random rays x 1024 samples.

Reports ms and algorithmic GB/s (SURVEY.md 8d bytes) per variant; used to choose layouts/kernels.
"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


ALONE = ",".join(str(l) for l in range(16))
# every level alone | one group | the default | fine levels alone, boundary moved | fine levels in
# pairs, boundaries moved | fine levels in threes | all fine levels together
DEFAULT_GROUPS = ";".join([
    ALONE, "0", "default", "0-5,6-9,10,11,12,13,14,15", "0-9,10,11,12,13,14,15", "0-11,12,13,14,15",
    "0-9,10-11,12-13,14,15", "0-10,11-12,13-14,15", "0-11,12-13,14-15", "0-7,8-9,10-11,12-13,14-15",
    "0-5,6-9,10-11,12-13,14-15", "0-9,10-12,13-15", "0-9,10-15",
])


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ts = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))
    return ts[len(ts) // 2], ts[0]


def alternating(fns, reps, warmup=2):
    """{arm: [ms, ...]}: the arms take turns call by call, each call timed between synchronisations"""
    ms = {k: [] for k in fns}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for it in range(warmup + reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms[k].append(ev[0].elapsed_time(ev[1]))
    return ms


def headline_chunk_points(capi, dev, g, n_rays, S):
    """the contracted points of one chunk of the benchmark's headline: n_rays rays of an 800 x 800 view
    in the Renderer's pixel-compact bundles, S jittered samples"""
    sys.path.insert(0, ROOT)
    from bench import fox_like_poses

    H = importlib.import_module("f2-nerf_amd").load_host()
    intr = torch.tensor([[1111.1, 0, 400.0], [0, 1111.1, 400.0], [0, 0, 1.0]], device=dev)
    o, d = H.get_view_rays(fox_like_poses(50)[7].to(dev), intr, 800, 800)
    lo = 4 * n_rays                                           # the view's fifth chunk: image rows 327-409
    o, d = o[lo:lo + n_rays], d[lo:lo + n_rays]
    order = H.ray_order(d.contiguous())                       # the Renderer's pixel-compact bundles
    o, d = o[order].contiguous(), d[order].contiguous()
    n = n_rays * S
    u = torch.rand(n_rays, S, device=dev, generator=g)        # the raw draw: sample_dense cooks it (TRAIN)
    pts, dt, t = torch.empty(n, 3, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
    bounds = torch.empty(n_rays, 2, device=dev, dtype=torch.int32)
    dirs = torch.empty(n_rays, 3, device=dev)
    capi.call("sample_dense", o, d, u, None, 1, pts, dt, t, bounds, dirs, n_rays, S, 4.0 / S)
    return pts


def parse_groups(text):
    """'0-5,6-9,10,11' -> mask with bits 0, 6, 10, 11; 'default' / a number pass through"""
    if text == "default":
        return None
    if text.startswith("0x"):
        return int(text, 16)
    mask = 0
    for part in text.split(","):
        mask |= 1 << int(part.split("-")[0])
    return mask


def level_groups_arm(args, capi, dev):
    """f2n_hash_fwd_raytile_groups on one headline chunk at L = 16 under each schedule of --groups
    (separated by ';'), and the one-level-per-workgroup route (RAYTILE = 32), alternating call by call"""
    import json

    n_rays, S, F, log2_T, L = 65536, 128, 2, 19, 16
    T = 1 << log2_T
    g = torch.Generator(device=dev).manual_seed(0)
    if args.random_rays:                                      # BASELINE config C4's batch: tiles walk along
        n_rays, S = args.rays or 512, 1024
        o = torch.randn(n_rays, 1, 3, device=dev, generator=g) * 0.3
        d = torch.randn(n_rays, 1, 3, device=dev, generator=g)
        t = (torch.arange(1, S + 1, device=dev).float() * (4.0 / S)).reshape(1, S, 1)
        p = (o + d / d.norm(dim=-1, keepdim=True) * t).reshape(-1, 3)
        nrm = p.norm(dim=1, keepdim=True)
        pts = torch.where(nrm <= 1, p, (2 - 1 / nrm) * p / nrm).contiguous()
    else:
        pts = headline_chunk_points(capi, dev, g, n_rays, S)
        if args.rays:                                         # the chunk's first rays: fewer tiles
            n_rays = args.rays
            pts = pts[:n_rays * S].contiguous()
    n = n_rays * S
    numel = T * (L - 1) + T * F                               # the reference's stride: T elements
    table = torch.randn(numel, device=dev, generator=g) * 0.1
    table16 = torch.empty(numel, dtype=torch.int16, device=dev)
    capi.call("table_to_f16", table, table16, numel)
    primes = (torch.randint(1 << 28, 1 << 30, (L, 3), device=dev, generator=g).to(torch.int32) | 1)
    bias = torch.rand(L, 3, device=dev, generator=g) * 1000 + 100
    mul = torch.tensor([2.0 ** (7.0 * l / (L - 1) + 3.0) for l in range(L)], device=dev)
    out = torch.empty(L * F, n, device=dev)
    default = int(capi.lib().cdll.f2n_hash_raytile_default_groups(L, (n_rays + 63) // 64 * (S // 32)))

    def one_level_route():
        with capi.option("RAYTILE", 32):
            capi.call("hash_fwd_raytile", pts, table16, primes, bias, mul, out, n_rays, S, L, F, T, T)

    def groups_route(mask):
        return lambda: capi.call("hash_fwd_raytile_groups", pts, table16, primes, bias, mul, out, n_rays, S,
                                 L, F, T, T, mask)

    fns = {"one level per workgroup (RAYTILE=32)": one_level_route}
    masks = {}
    for text in args.groups.split(";"):
        mask = parse_groups(text.strip())
        name = "groups " + text.strip()
        masks[name] = default if mask is None else (mask | 1)
        fns[name] = groups_route(masks[name])
    ms = alternating(fns, args.reps)
    for name, v in ms.items():
        print(json.dumps(dict(
            what="hash_fwd_raytile, 16 levels", arm=name, group_starts=hex(masks[name]) if name in masks else None,
            rays=n_rays, samples=S, ms_median=round(sorted(v)[len(v) // 2], 4), ms_min=round(min(v), 4),
            ms_all=[round(x, 4) for x in v])), flush=True)


def corner_order_arm(args, capi, dev):
    import json

    n_rays, S, F, log2_T, Lfull = 65536, 128, 2, 19, 16
    T = 1 << log2_T
    g = torch.Generator(device=dev).manual_seed(0)
    pts = headline_chunk_points(capi, dev, g, n_rays, S)
    n = n_rays * S
    table = torch.randn(T * F, device=dev, generator=g) * 0.1
    table16 = torch.empty(T * F, dtype=torch.int16, device=dev)
    capi.call("table_to_f16", table, table16, T * F)
    out = torch.empty(F, n, device=dev)
    for l in [int(v) for v in args.levels.split(",")]:
        primes = (torch.randint(1 << 28, 1 << 30, (1, 3), device=dev, generator=g).to(torch.int32) | 1)
        bias = torch.rand(1, 3, device=dev, generator=g) * 1000 + 100
        mul = torch.tensor([2.0 ** (7.0 * l / (Lfull - 1) + 3.0)], device=dev)

        def run(order_value):
            def fn():
                capi.set_option("GATHER_PAIRED", order_value)
                capi.call("hash_fwd_raytile", pts, table16, primes, bias, mul, out, n_rays, S, 1, F, T, T * F)
            return fn

        ms = alternating({"corner": run(1), "parity": run(0)}, args.reps)
        capi.set_option("GATHER_PAIRED", 0)
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        print(json.dumps(dict(
            what="hash_fwd_raytile, one level", level=l, mul=round(float(mul[0]), 2), rays=n_rays, samples=S,
            ms_corner=round(med["corner"], 4), ms_parity=round(med["parity"], 4),
            ratio=round(med["parity"] / med["corner"], 3),
            ms_corner_all=[round(v, 4) for v in ms["corner"]], ms_parity_all=[round(v, 4) for v in ms["parity"]],
            ggathers_per_s_corner=round(8 * n / med["corner"] / 1e6, 1),
            ggathers_per_s_parity=round(8 * n / med["parity"] / 1e6, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--reps", type=int, default=None, help="timed calls per arm (5; --level-groups: 9)")
    ap.add_argument("--points", default="rays", choices=["rays", "ball", "view", "view_sm", "view_jit"],
                    help="rays: random rays, samples of a ray consecutive; view: 65536 consecutive pixels of "
                         "an 800-wide pinhole view (focal 1111, camera at distance 1), ray-major as the "
                         "renderer emits them; view_sm: the same points sample-major (lane = adjacent pixel)")
    ap.add_argument("--fwd-only", action="store_true")
    ap.add_argument("--corner-order", action="store_true",
                    help="only the per-level arm of the two corner orders on one headline chunk")
    ap.add_argument("--levels", default="0,4,8,10,12,14,15")
    ap.add_argument("--level-groups", action="store_true",
                    help="only the level schedules of f2n_hash_fwd_raytile_groups on one headline chunk")
    ap.add_argument("--groups", default=DEFAULT_GROUPS,
                    help="schedules separated by ';': the first level of each group, e.g. '0-5,6-9,10,11,12,13,14,15'")
    ap.add_argument("--rays", type=int, default=0,
                    help="--level-groups: only the first RAYS rays of the chunk (64 rays x 32 samples to a tile)")
    ap.add_argument("--random-rays", action="store_true",
                    help="--level-groups: --rays (512) random rays x 1024 samples of 1/256 instead of the chunk")
    args = ap.parse_args()
    capi = importlib.import_module("f2-nerf_amd").capi
    dev = torch.device("cuda:0")
    if args.level_groups:
        args.reps = args.reps or 9
        return level_groups_arm(args, capi, dev)
    args.reps = args.reps or 5
    if args.corner_order:
        return corner_order_arm(args, capi, dev)
    cfg = {"c2": (16, 2, 19, None, 65536 * 128), "c1": (4, 2, 19, None, 65536 * 64),
           "c4": (16, 2, 19, None, 512 * 1024),
           "c5": (16, 8, 22, "disjoint", 1 << 24)}[args.config]
    L, F, log2_T, stride_mode, n = cfg
    if args.n:
        n = args.n
    T = 1 << log2_T
    stride = T if stride_mode is None else T * F
    numel = max(T * L * F, stride * (L - 1) + T * F)
    g = torch.Generator(device=dev).manual_seed(0)
    table = (torch.randn(numel, device=dev, generator=g) * 0.1)
    table16 = torch.empty(numel, dtype=torch.int16, device=dev)
    capi.call("table_to_f16", table, table16, numel)
    primes = torch.randint(1 << 28, 1 << 30, (L, 3), device=dev, generator=g).to(torch.int32) | 1
    bias = torch.rand(L, 3, device=dev, generator=g) * 1000 + 100
    mul = torch.tensor([2.0 ** (7.0 * l / max(L - 1, 1) + 3.0) for l in range(L)], device=dev)
    if args.points == "rays":
        # consecutive samples along rays (what the renderer feeds): 128 per ray, step 1/32
        # (config c4: the reference's 1024 steps of 1/256)
        S = 1024 if args.config == "c4" else 128
        R = n // S
        o = torch.randn(R, 1, 3, device=dev, generator=g) * 0.3
        d = torch.randn(R, 1, 3, device=dev, generator=g)
        d = d / d.norm(dim=-1, keepdim=True)
        t = (torch.arange(1, S + 1, device=dev).float() * (4.0 / S)).reshape(1, S, 1)
        p = (o + d * t).reshape(-1, 3)
        nrm = p.norm(dim=1, keepdim=True)
        pts = torch.where(nrm <= 1, p, (2 - 1 / nrm) * p / nrm).contiguous()
        n = pts.shape[0]
    elif args.points in ("view", "view_sm", "view_jit"):
        S, R, W, f = 128, n // 128, 800, 1111.1
        pix = torch.arange(R, device=dev)
        i, j = (pix // W).float(), (pix % W).float()
        # camera at (1, 0, 0) looking at the origin (-x), pixel (i, j) -> direction
        d = torch.stack([-torch.ones_like(i), (j - 400) / f, -(i - 400) / f], 1)
        d = d / d.norm(dim=1, keepdim=True)
        o = torch.tensor([1.0, 0.0, 0.0], device=dev).expand(R, 3)
        t = ((torch.arange(S, device=dev).float() + 0.5) * (4.0 / S)).reshape(1, S, 1)
        if args.points == "view_jit":                          # TRAIN: every step scaled by U[0.5, 1.5)
            t = ((torch.rand(R, S, device=dev, generator=g) + 0.5).cumsum(1) * (4.0 / S)).reshape(R, S, 1)
        p = (o[:, None] + d[:, None] * t)                      # [R, S, 3]
        if args.points == "view_sm":
            p = p.transpose(0, 1)                              # [S, R, 3]
        p = p.reshape(-1, 3)
        nrm = p.norm(dim=1, keepdim=True)
        pts = torch.where(nrm <= 1, p, (2 - 1 / nrm) * p / nrm).contiguous()
        n = pts.shape[0]
    else:
        dd = torch.randn(n, 3, device=dev, generator=g)
        pts = (dd / dd.norm(dim=1, keepdim=True) * torch.rand(n, 1, device=dev, generator=g) ** (1 / 3) * 2).contiguous()
    C = L * F
    bytes_fwd = 12 + 16 * C + 4 * C
    print("config %s: n=%d L=%d F=%d T=2^%d table %.0f MiB f16, points=%s" %
          (args.config, n, L, F, log2_T, numel * 2 / 2 ** 20, args.points))
    out_rm = torch.empty(n, C, device=dev)
    out_cm = torch.empty(C, n, device=dev)
    for name, out, ldp, ldc in (("fwd row-major [n,C]", out_rm, C, 1), ("fwd chan-major [C,n]", out_cm, 1, n)):
        med, best = timeit(lambda: capi.call("hash_fwd", pts, table16, primes, bias, mul, out, ldp, ldc,
                                             None, n, L, F, T, stride), args.reps)
        print("  %-28s %8.3f ms (best %8.3f)  %7.1f GB/s algorithmic" % (name, med, best, n * bytes_fwd / med / 1e6))
    if args.points in ("rays", "view", "view_jit") and n % 128 == 0:
        S_rt = 1024 if args.config == "c4" else 128
        for walk, name in ((0, "auto"), (1, "across, one sample index"), (3, "across, depth order"), (2, "along a ray")):
            capi.set_option("RAYTILE_WALK", walk)
            med, best = timeit(lambda: capi.call("hash_fwd_raytile", pts, table16, primes, bias, mul, out_cm,
                                                 n // S_rt, S_rt, L, F, T, stride), args.reps)
            print("  %-28s %8.3f ms (best %8.3f)  %7.1f GB/s algorithmic" %
                  ("fwd ray-tile, " + name, med, best, n * bytes_fwd / med / 1e6))
        capi.set_option("RAYTILE_WALK", 0)
    if args.fwd_only:
        return
    grad_rm = torch.randn(n, C, device=dev, generator=g) * 1e-3
    grad_cm = grad_rm.t().contiguous()
    tg = torch.zeros(numel, device=dev)
    for mode in ("atomic", "sliced"):
        capi.set_option("HASH_BWD", {"atomic": 1, "sliced": 2}[mode])
        for name, gr, ldp, ldc in (("row-major", grad_rm, C, 1), ("chan-major", grad_cm, 1, n)):
            try:
                med, best = timeit(lambda: capi.call("hash_bwd", pts, table16, primes, bias, mul, gr, ldp, ldc,
                                                     tg, None, n, L, F, T, stride, 128.0), max(2, args.reps // 2))
                print("  bwd %-7s grads %-10s %8.3f ms (best %8.3f)  %7.1f GB/s algorithmic" %
                      (mode, name, med, best, n * bytes_fwd / med / 1e6))
            except Exception as e:
                print("  bwd %s %s: %s" % (mode, name, e))
    capi.set_option("HASH_BWD", 0)
    need = capi.lib().cdll.f2n_hash_bwd_workspace_bytes(n, L, F, T)
    if need > 0:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        for name, gr, ldp, ldc in (("row-major", grad_rm, C, 1), ("chan-major", grad_cm, 1, n)):
            med, best = timeit(lambda: capi.call("hash_bwd_binned", pts, primes, bias, mul, gr, ldp, ldc, tg,
                                                 n, L, F, T, stride, 128.0, ws, need), max(2, args.reps // 2))
            print("  bwd binned  grads %-10s %8.3f ms (best %8.3f)  %7.1f GB/s algorithmic  (ws %.1f GiB)" %
                  (name, med, best, n * bytes_fwd / med / 1e6, need / 2 ** 30))


if __name__ == "__main__":
    main()
