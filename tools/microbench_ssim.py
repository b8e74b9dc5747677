#!/usr/bin/env python3
"""What the fused SSIM kernels (ssim.hip) buy over the same formula spelled in ATen, and what the
D-SSIM term costs a training step.

  --part full     The metric (clip = 1, no map) on 1920 x 1080 pairs, B = 1 and 8: f2n_ssim_fwd against
                  ATen on the same device -- the five maps x, y, x^2, y^2, xy stacked, two grouped
                  conv2d passes (1 x 11, then 11 x 1), the clamps, the index, the mean.  Time and the
                  achieved bytes/s against the 2 * B * h * w * 3 * 4 bytes that must move.
  --part patches  Forward plus backward (CustomOps::Ssim, d_ssim = 1 / B) on 16 patches of 32 x 32 and
                  64 of 16 x 16 against autograd through the ATen spelling, with the number of GPU
                  kernels either one launches (torch.profiler; null where it cannot count).
  --part step     A step of 8 patches of 16 x 16 (2048 rays, 1024 samples of 1/256, workload C4's
                  field) with ssim_weight 0 and 0.2, on the march route (an occupancy grid attached)
                  and on the dense route, the four arms alternating.

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

C1, C2 = 1e-4, 9e-4


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


def taps(dev):
    z = (torch.arange(11, dtype=torch.float64) - 5) / 1.5
    g = torch.exp(-0.5 * z * z)
    return (g / g.sum()).float().to(dev)


def aten_ssim(pred, gt, f, clip):
    """[B,h,w,3] -> [B]: the formula of include/f2nerf_hip.h in ATen"""
    x, y = pred.permute(0, 3, 1, 2), gt.permute(0, 3, 1, 2)
    five = torch.cat([x, y, x * x, y * y, x * y], dim=1)                      # [B,15,h,w]
    t = torch.nn.functional.conv2d(five, f.view(1, 1, 1, 11).expand(15, 1, 1, 11), groups=15)
    t = torch.nn.functional.conv2d(t, f.view(1, 1, 11, 1).expand(15, 1, 11, 1), groups=15)
    mux, muy, exx, eyy, exy = t.split(3, dim=1)
    sxx, syy, sxy = exx - mux * mux, eyy - muy * muy, exy - mux * muy
    if clip:
        sxx, syy = sxx.clamp_min(0), syy.clamp_min(0)
        sxy = torch.sign(sxy) * torch.minimum(torch.sqrt(sxx * syy), sxy.abs())
    S = ((2 * mux * muy + C1) * (2 * sxy + C2)) / ((mux * mux + muy * muy + C1) * (sxx + syy + C2))
    return S.mean(dim=(1, 2, 3))


def count_kernels(fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages()
                   if "memcpy" not in e.key.lower() and "memset" not in e.key.lower())
    except Exception:
        return None


def part_full(host, dev, args):
    h, w = 1080, 1920
    f = taps(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    for B in (1, 8):
        gt = torch.rand(B, h, w, 3, device=dev, generator=g)
        pred = (gt + 0.05 * torch.randn(B, h, w, 3, device=dev, generator=g)).clamp(0, 1)
        with torch.no_grad():
            fns = {"fused": lambda: host.ssim(pred, gt, True, False),
                   "aten": lambda: aten_ssim(pred, gt, f, True)}
            diff = float((fns["fused"]()[0] - fns["aten"]()).abs().max())
            ts = alternating(fns, args.reps, args.warmup, args.inner)
        moved = 2 * B * h * w * 3 * 4
        rec = {"part": "full", "B": B, "h": h, "w": w, "bytes_that_must_move": moved,
               "max_abs_diff_fused_vs_aten": diff}
        for k, v in ts.items():
            rec[k + "_ms"] = med(v)
            rec[k + "_min_ms"] = round(v[0], 5)
            rec[k + "_GBps_of_must_move"] = round(moved / (med(v) * 1e-3) / 1e9, 1)
        rec["speedup"] = round(rec["aten_ms"] / rec["fused_ms"], 2)
        emit(rec, args.out)


def part_patches(host, dev, args):
    f = taps(dev)
    g = torch.Generator(device=dev).manual_seed(2)
    for B, P in ((16, 32), (64, 16)):
        gt = torch.rand(B, P, P, 3, device=dev, generator=g)
        pred = (gt + 0.05 * torch.randn(B, P, P, 3, device=dev, generator=g)).requires_grad_(True)

        def fused():
            pred.grad = None
            (1 - host.ssim_loss(pred, gt)).mean().backward()

        def aten():
            pred.grad = None
            (1 - aten_ssim(pred, gt, f, False)).mean().backward()

        fused()
        ga = pred.grad.clone()
        aten()
        diff = float((pred.grad - ga).abs().max() / ga.abs().max())
        ts = alternating({"fused": fused, "aten": aten}, args.reps, args.warmup, args.inner)
        rec = {"part": "patches", "patches": B, "side": P, "grad_max_rel_diff_fused_vs_aten": diff,
               "fused_kernels": count_kernels(fused), "aten_kernels": count_kernels(aten)}
        for k, v in ts.items():
            rec[k + "_fwd_bwd_us"] = round(med(v) * 1e3, 2)
            rec[k + "_fwd_bwd_min_us"] = round(v[0] * 1e3, 2)
        rec["speedup"] = round(rec["aten_fwd_bwd_us"] / rec["fused_fwd_bwd_us"], 2)
        emit(rec, args.out)


def part_step(host, dev, args):
    n, P, S, step = 8, 16, 1024, 1.0 / 256
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
    sup = host.RaySupervision()

    def arm(use_grid, weight):
        patch = host.PatchLoss(P, weight)

        def run():
            hr.set_occupancy(grid if use_grid else None)
            hr.set_dense_first_pass(0 if use_grid else 1)
            hr.zero_grad()
            hr.train_step_patches(o, d, emb, gt, patch, sup, 1e-2, noise, bg)
        return run

    fns = {"march_grid": arm(True, 0.0), "march_grid_ssim": arm(True, 0.2),
           "dense": arm(False, 0.0), "dense_ssim": arm(False, 0.2)}
    ts = alternating(fns, args.reps, args.warmup + 1)
    rec = {"part": "step", "patches": n, "side": P, "n_rays": n_rays, "samples_per_ray": S,
           "kept_samples": int(hr.last_n_samples), "ssim_weight": 0.2}
    for k, v in ts.items():
        rec["train_step_ms_" + k] = med(v)
        rec["train_step_min_ms_" + k] = round(v[0], 4)
    for route in ("march_grid", "dense"):
        rec["ssim_term_ms_" + route] = round(
            rec["train_step_ms_%s_ssim" % route] - rec["train_step_ms_" + route], 4)
    emit(rec, args.out)
    hr.set_occupancy(None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="full", choices=["full", "patches", "step"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pkg = importlib.import_module("f2-nerf_amd")
    host = pkg.load_host()
    {"full": part_full, "patches": part_patches, "step": part_step}[args.part](host, dev, args)


if __name__ == "__main__":
    main()
