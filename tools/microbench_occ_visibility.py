#!/usr/bin/env python3
"""What carving the occupancy grid to the training cameras (camera_visibility,
OccupancyGrid.set_allowed) costs and what it buys.

  --part cost     camera_visibility for --cams cameras of --width x --height pixels on a ring around
                  the origin, for every resolution in {128, 256}, pixel stride in {1, 2, 4} and
                  min_views in {1, 2}: milliseconds of the whole call (device events; min_views = 1 is
                  one mark launch and the dilation, min_views = 2 the per-camera loop), the visible
                  fraction, and against pixel stride 1 of the same resolution the cells lost.  A
                  one-time setup cost: the number decides which stride the documents recommend.

  --part effect   The analytic scene of microbench_occupancy.py --part train (24 cameras on a ring),
                  trained from one seed four ways: no grid, the plain grid (attached at its first
                  update), the grid carved at iteration 0 with min_views 1 and with min_views 2.  Per
                  run: occupied fraction, kept samples per ray and iteration time at the iterations of
                  --report (0 .. 256 and the end), PSNR on held-out views of the ring, and PSNR at
                  poses perturbed off the ring with the Localizer's default noise sigmas -- the views
                  whose rays cross the space training never constrained.

Prints one JSON line per measurement (also appended to --out).
"""
import argparse
import importlib
import importlib.util
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location(
    "microbench_occupancy", os.path.join(ROOT, "tools", "microbench_occupancy.py"))
B = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(B)

REPORT = (0, 16, 64, 128, 256)


def part_cost(host, dev, args):
    n, h, w = args.cams, args.height, args.width
    poses = B.ring_poses(n, 0.9, 0.25).to(dev)
    f = 0.8 * w
    K = torch.tensor([[f, 0.0, 0.5 * w], [0.0, f, 0.5 * h], [0.0, 0.0, 1.0]], device=dev)
    intr = K.unsqueeze(0).expand(n, 3, 3).contiguous()
    for G in args.resolutions:
        base = {}
        for stride in args.strides:
            for mv in (1, 2):
                opts = host.VisibilityOptions(resolution=G, pixel_stride=stride, min_views=mv)
                fn = lambda: host.camera_visibility(poses, intr, h, w, opts)
                fn()
                torch.cuda.synchronize()
                ts = sorted(B.timed(fn, args.reps))
                words = fn()
                grid = host.OccupancyGrid(G, str(dev))
                grid.set_allowed(words)
                bits = grid.bits()
                if stride == args.strides[0]:
                    base[mv] = bits
                rec = {"part": "cost", "cams": n, "h": h, "w": w, "resolution": G, "pixel_stride": stride,
                       "min_views": mv, "n_steps": 1536, "step": 1.0 / 256, "dilate": 1,
                       "ms_median": B.med(ts), "ms_min": round(ts[0], 4),
                       "visible_fraction": round(float(bits.float().mean()), 6),
                       "cells_lost_vs_first_stride": int((base[mv] & ~bits).sum()),
                       "cells_gained_vs_first_stride": int((bits & ~base[mv]).sum()),
                       "atomic_issuing_share": "not measured"}
                B.emit(rec, args.out)


def _views(host, hr, poses, Kc, hw):
    with torch.no_grad():
        return torch.stack([hr.render_all_rays(*host.get_view_rays(poses[i], Kc, hw, hw), 16384)[0].clip(0, 1)
                            for i in range(poses.shape[0])])


def _truth(host, poses, Kc, hw):
    return torch.stack([B.analytic_colors(*host.get_view_rays(poses[i], Kc, hw, hw))
                        for i in range(poses.shape[0])])


def train_once(host, dev, args, mode):
    """mode: 'none', 'plain', 'carved1', 'carved2'"""
    hw, n_cams, G = args.image, 24, args.resolution
    poses = B.ring_poses(n_cams, 0.9, 0.25).to(dev)
    held = B.ring_poses(4, 0.9, 0.1, phase=0.13).to(dev)
    Kc = torch.tensor([[0.8 * hw, 0.0, 0.5 * hw], [0.0, 0.8 * hw, 0.5 * hw], [0.0, 0.0, 1.0]], device=dev)
    intr = Kc.unsqueeze(0).expand(n_cams, 3, 3).contiguous()
    images = torch.stack([B.analytic_colors(*host.get_view_rays(poses[i], Kc, hw, hw)).reshape(hw, hw, 3)
                          for i in range(n_cams)]).contiguous()
    # poses off the ring: the Localizer's default noise sigmas around each held-out view
    lp = host.LocalizerParam()
    sigmas = [lp.noise_position_x, lp.noise_position_y, lp.noise_position_z,
              lp.noise_rotation_x, lp.noise_rotation_y, lp.noise_rotation_z]
    gp = torch.Generator(device=dev).manual_seed(21)
    off_ring = torch.cat([host.perturb_poses(held[i], torch.randn(4, 6, device=dev, generator=gp), sigmas)
                          for i in range(held.shape[0])])
    host.manual_seed(11)
    torch.manual_seed(11)
    hr = host.Renderer(n_cams, n_levels=B.L, n_channels=B.F, log2_table=B.LOG2_T, max_samples=B.S, step=B.STEP)
    hr.set_dense_first_pass(-1)
    opt = hr.make_fused_adam(args.lr)
    grid = None if mode == "none" else host.OccupancyGrid(G, str(dev))
    carve_ms = None
    if mode.startswith("carved"):
        t0 = time.perf_counter()
        grid.carve_to_cameras(poses, intr, hw, hw, host.VisibilityOptions(min_views=int(mode[-1])))
        torch.cuda.synchronize()
        carve_ms = round(1e3 * (time.perf_counter() - t0), 3)
        hr.set_occupancy(grid)                       # the carve acts from iteration 0
    gen = torch.Generator(device=dev).manual_seed(5)
    bg_gt = torch.tensor(B.BACKGROUND, device=dev)
    bg = bg_gt.expand(512, 3).contiguous()
    report = set(REPORT) | {args.iters}
    for it in range(args.iters + 1):
        o, d, gt, cam = host.sample_random_rays(poses, intr, hw, hw, 512, images)
        if it in report:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        opt.zero_grad()
        hr.train_step(o, d, cam, gt, 0.0, None, bg, True)
        opt.step()
        if it in report:
            torch.cuda.synchronize()
            B.emit({"part": "effect", "mode": mode, "event": "iteration", "iteration": it,
                    "iteration_ms": round(1e3 * (time.perf_counter() - t0), 3),
                    "kept_per_ray": round(hr.last_n_samples / 512, 2),
                    "occupied_fraction": None if grid is None else round(grid.fraction(), 5)}, args.out)
        if grid is not None and it >= args.first_update and (it - args.first_update) % args.update_every == 0:
            probe = torch.rand(G, G, G, 3, device=dev, generator=gen).clamp_max(1.0 - 2.0 ** -24)
            grid.update(hr.scene_field, args.threshold, args.decay, probe)
            mean = float(grid.density().mean())      # microbench_occupancy.py: a young field
            if mean < args.threshold:
                grid.update(hr.scene_field, mean, 1.0, probe)
            hr.set_occupancy(grid)
    rec = {"part": "effect", "mode": mode, "event": "final", "iterations": args.iters, "resolution": G,
           "carve_ms": carve_ms,
           "occupied_fraction": None if grid is None else round(grid.fraction(), 5),
           "allowed_fraction": None}
    if grid is not None and grid.allowed() is not None:
        probe_grid = host.OccupancyGrid(G, str(dev))
        probe_grid.set_allowed(grid.allowed())
        rec["allowed_fraction"] = round(probe_grid.fraction(), 5)
    for name, views in (("heldout", held), ("off_ring", off_ring)):
        truth = _truth(host, views, Kc, hw)
        hr.set_occupancy(grid)
        rec["psnr_" + name] = round(B.psnr(_views(host, hr, views, Kc, hw), truth), 3)
        hr.set_occupancy(None)
        rec["psnr_%s_gridless_render" % name] = round(B.psnr(_views(host, hr, views, Kc, hw), truth), 3)
    return rec


def part_effect(host, dev, args):
    for mode in args.modes:
        B.emit(train_once(host, dev, args, mode), args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="cost", choices=["cost", "effect"])
    ap.add_argument("--cams", type=int, default=200)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--strides", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--modes", nargs="+", default=["none", "plain", "carved1", "carved2"])
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--image", type=int, default=128)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--first-update", type=int, default=256)
    ap.add_argument("--update-every", type=int, default=16)
    ap.add_argument("--threshold", type=float, default=None)
    ap.add_argument("--decay", type=float, default=None)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pkg = importlib.import_module("f2-nerf_amd")
    host = pkg.load_host()
    if args.threshold is None:
        args.threshold = host.OccupancyGrid.DEFAULT_THRESHOLD
    if args.decay is None:
        args.decay = host.OccupancyGrid.DEFAULT_DECAY
    if args.part == "cost":
        part_cost(host, dev, args)
    else:
        part_effect(host, dev, args)


if __name__ == "__main__":
    main()
