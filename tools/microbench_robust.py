#!/usr/bin/env python3
"""What the robust loss (robust_mask.hip, RobustLoss) costs.

  --part weights  f2n_robust_weights alone (host.robust_weights: the launches plus the four output and
                  workspace allocations) on 16 patches of 16 x 16 (4096 rays, three launches) and on
                  65 536 scattered rays (one launch, one workgroup striding over them), with and
                  without a ray_weight, at the quantile 0.5.  The worst case of the LDS histograms --
                  every residual equal, so every lane of a pass adds to one bin -- is timed beside the
                  random one.
  --part step     A step of 16 patches of 16 x 16 (4096 rays, 1024 samples of 1/256, workload C4's
                  field) on the march route (an occupancy grid attached) and on the dense route:
                  the supervised step with a GIVEN ray_weight -- train_step_supervised, the code of the
                  step before the robust loss existed, which it leaves unchanged -- against
                  train_step_robust forming its own on the same batch, the arms alternating.

Median of --reps windows after --warmup, the arms interleaved.  Prints one JSON line per measurement
(also appended to --out)."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def alternating(fns, reps, warmup, inner=1):
    """{name: sorted ms per call}: the windows interleaved, so drift of the box hits all alike"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / inner)
    return {k: sorted(v) for k, v in ts.items()}


def med(v):
    return round(v[len(v) // 2], 5)


def part_weights(host, dev, args):
    g = torch.Generator(device=dev).manual_seed(1)
    for name, n, P in (("16 patches of 16 x 16", 16 * 256, 16), ("65536 scattered rays", 65536, 0)):
        target = torch.rand(n, 3, device=dev, generator=g)
        colors = target + 0.05 * torch.randn(n, 3, device=dev, generator=g)
        equal = target + 0.25
        m = (torch.rand(n, device=dev, generator=g) > 0.1).float()
        opt = host.RobustLoss(quantile=0.5, patch=P)
        fns = {"random": lambda: host.robust_weights(colors, target, opt),
               "random_weighted": lambda: host.robust_weights(colors, target, opt, m),
               "all_equal": lambda: host.robust_weights(equal, target, opt)}
        stats = fns["random"]()[2].tolist()
        ts = alternating(fns, args.reps, args.warmup, args.inner)
        rec = {"part": "weights", "case": name, "n_rays": n, "patch": P, "quantile": 0.5,
               "launches": 3 if P else 1, "stats": stats}
        for k, v in ts.items():
            rec[k + "_us"] = round(med(v) * 1e3, 2)
            rec[k + "_min_us"] = round(v[0] * 1e3, 2)
        emit(rec, args.out)


def part_step(host, dev, args):
    n, P, S, step = 16, 16, 1024, 1.0 / 256
    n_rays = n * P * P
    host.manual_seed(7)
    torch.manual_seed(7)
    hr = host.Renderer(4, n_levels=16, n_channels=2, log2_table=19, max_samples=S, step=step)
    with torch.no_grad():
        hr.named_parameters()["scene_field.feat_pool"].normal_(0.0, 0.1)
    g = torch.Generator(device=dev).manual_seed(3)
    o = torch.randn(n_rays, 3, device=dev, generator=g) * 0.25
    d = torch.randn(n_rays, 3, device=dev, generator=g)
    gt = torch.rand(n_rays, 3, device=dev, generator=g)
    bg = torch.rand(n_rays, 3, device=dev, generator=g)
    emb = torch.randint(0, 4, (n_rays,), device=dev, generator=g).to(torch.int32)
    noise = torch.rand(n_rays, S, device=dev, generator=g) + 0.5
    grid = host.OccupancyGrid(128, str(dev))
    robust = host.RobustLoss(quantile=0.5, patch=P)
    # the given weights of the supervised arm: those the robust arm forms, so both steps do the same
    # work after the render
    hr.set_dense_first_pass(1)
    given = hr.train_step_robust(o, d, emb, gt, robust, host.PatchLoss(), host.RaySupervision(),
                                 1e-2, noise, bg, False)[6].clone()
    sup = host.RaySupervision(ray_weight=given)

    def arm(use_grid, on):
        def run():
            hr.set_occupancy(grid if use_grid else None)
            hr.set_dense_first_pass(0 if use_grid else 1)
            hr.zero_grad()
            if on:
                hr.train_step_robust(o, d, emb, gt, robust, host.PatchLoss(), host.RaySupervision(),
                                     1e-2, noise, bg)
            else:
                hr.train_step_supervised(o, d, emb, gt, sup, 1e-2, noise, bg)
        return run

    fns = {"march_grid_given": arm(True, False), "march_grid_robust": arm(True, True),
           "dense_given": arm(False, False), "dense_robust": arm(False, True)}
    ts = alternating(fns, args.reps, args.warmup + 1)
    rec = {"part": "step", "patches": n, "side": P, "n_rays": n_rays, "samples_per_ray": S,
           "kept_samples": int(hr.last_n_samples), "quantile": 0.5,
           "inlier_rays": int((given != 0).sum())}
    for k, v in ts.items():
        rec["train_step_ms_" + k] = med(v)
        rec["train_step_min_ms_" + k] = round(v[0], 4)
    for route in ("march_grid", "dense"):
        rec["robust_term_ms_" + route] = round(
            rec["train_step_ms_%s_robust" % route] - rec["train_step_ms_%s_given" % route], 4)
    emit(rec, args.out)
    hr.set_occupancy(None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="weights", choices=["weights", "step"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pkg = importlib.import_module("f2-nerf_amd")
    host = pkg.load_host()
    {"weights": part_weights, "step": part_step}[args.part](host, dev, args)


if __name__ == "__main__":
    main()
