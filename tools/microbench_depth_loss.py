#!/usr/bin/env python3
"""What depth supervision costs, next to the per-ray terms it stands beside.

  --part kernels   f2n_depth_sight_fwd / _bwd and f2n_weight_dist_fwd / _bwd through the C ABI on the
                   SAME bounds, weights, t and dt: 65 536 rays x 128 samples (the bench's training
                   chunk), every ray full, a target inside every ray (every eighth ray: none).  The new
                   kernels read the same three arrays and reduce after the strided loop, without the
                   per-stride scans; the algorithmic bytes per launch are in the record.
  --part splat     f2n_depth_splat: 10^5 points into one 1920 x 1080 camera (points spread over the
                   image, so nearly every one lands); the fill, the splat and the finish in one call.
  --part step      One train_step without a depth target and with one (all three weights set),
                   alternating: one training chunk (65 536 rays, 128 samples) and the C4 batch (512
                   rays, 1024 samples of 1/256).

Median of --reps calls after --warmup (defaults 5 and 2).  Prints one JSON line per measurement (also
appended to --out).
"""
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


def alternating(fns, reps, warmup):
    """{name: sorted ms}: the calls interleaved, so drift of the box hits all of them alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: sorted(v) for k, v in ts.items()}


def med(v):
    return round(v[len(v) // 2], 4)


def targets_along(t_rows, gen):
    """one target per ray somewhere along its samples; every eighth ray has no return"""
    n = t_rows.shape[0]
    frac = 0.1 + 0.8 * torch.rand(n, device=t_rows.device, generator=gen)
    z = t_rows[:, 0] + frac * (t_rows[:, -1] - t_rows[:, 0])
    z[::8] = 0.0
    return z.contiguous()


def part_kernels(capi, dev, args):
    n_rays, S = 65536, 128
    n = n_rays * S
    g = torch.Generator(device=dev).manual_seed(5)
    w = torch.rand(n, device=dev, generator=g) / S
    dt = torch.rand(n, device=dev, generator=g) * (4.0 / S) + 2.0 / S
    t = torch.cumsum(dt.reshape(n_rays, S), 1).reshape(-1).contiguous()
    start = torch.arange(n_rays, device=dev, dtype=torch.int32) * S
    bounds = torch.stack([start, start + S], 1).contiguous()
    z = targets_along(t.reshape(n_rays, S), g)
    eps = 0.05
    d_out1 = torch.randn(n_rays, device=dev, generator=g)
    d_out3 = torch.randn(n_rays, 3, device=dev, generator=g)
    out1, out3 = torch.empty(n_rays, device=dev), torch.empty(n_rays, 3, device=dev)
    dw = torch.empty(n, device=dev)
    fns = {
        "weight_dist_fwd": lambda: capi.call("weight_dist_fwd", w, t, dt, bounds, out1, n_rays),
        "weight_dist_bwd": lambda: capi.call("weight_dist_bwd", w, t, dt, bounds, d_out1, dw, n_rays),
        "depth_sight_fwd": lambda: capi.call("depth_sight_fwd", w, t, dt, bounds, z, eps, out3, n_rays),
        "depth_sight_bwd": lambda: capi.call("depth_sight_bwd", w, t, dt, bounds, z, eps, d_out3, dw,
                                             n_rays),
    }
    ts = alternating(fns, args.reps, args.warmup)
    # bytes if every array is touched once per pass the kernel makes over it (the rays without a
    # return read nothing in the new kernels: 7/8 of the samples)
    live = 7.0 / 8.0
    bytes_once = {"weight_dist_fwd": 12 * n, "weight_dist_bwd": 12 * n * 2 + 4 * n,
                  "depth_sight_fwd": 12 * n * live, "depth_sight_bwd": 12 * n * 2 * live + 4 * n}
    rec = {"part": "kernels", "n_rays": n_rays, "samples_per_ray": S, "rays_without_return": n_rays // 8}
    for k, v in ts.items():
        rec[k + "_ms"] = med(v)
        rec[k + "_min_ms"] = round(v[0], 4)
        rec[k + "_GBs"] = round(bytes_once[k] / (med(v) * 1e-3) / 1e9, 1)
    rec["fwd_over_dist"] = round(rec["depth_sight_fwd_ms"] / rec["weight_dist_fwd_ms"], 2)
    rec["bwd_over_dist"] = round(rec["depth_sight_bwd_ms"] / rec["weight_dist_bwd_ms"], 2)
    emit(rec, args.out)


def part_splat(host, capi, dev, args):
    h, w, n = 1080, 1920, 100000
    g = torch.Generator(device=dev).manual_seed(11)
    K = torch.tensor([[[1000.0, 0, w / 2], [0, 1000.0, h / 2], [0, 0, 1]]], device=dev)
    pose = torch.eye(4, device=dev)[:3].unsqueeze(0).contiguous()
    col = torch.rand(n, device=dev, generator=g) * w
    row = torch.rand(n, device=dev, generator=g) * h
    depth = 1.0 + 9.0 * torch.rand(n, device=dev, generator=g)
    x, y = (col - w / 2) / 1000.0, (row - h / 2) / 1000.0
    pts = torch.stack([x * depth, -y * depth, -depth], 1).contiguous()
    cam = torch.zeros(n, dtype=torch.int32, device=dev)
    lens = torch.tensor([[0.05, -0.01, 0.002, -0.003]], device=dev)
    out = torch.empty(1, h, w, device=dev)
    fns = {
        "pinhole": lambda: capi.call("depth_splat", pts, cam, pose, 12, K, None, 1, h, w, out, n),
        "lens": lambda: capi.call("depth_splat", pts, cam, pose, 12, K, lens, 1, h, w, out, n),
    }
    ts = alternating(fns, args.reps, args.warmup)
    maps = host.splat_depth(pts, cam, pose, K, None, h, w)
    rec = {"part": "splat", "h": h, "w": w, "points": n, "pixels_hit": int((maps > 0).sum())}
    for k, v in ts.items():
        rec["depth_splat_%s_ms" % k] = med(v)
        rec["depth_splat_%s_min_ms" % k] = round(v[0], 4)
    emit(rec, args.out)


def part_step(host, dev, args):
    for name, n_rays, S, step in (("training_chunk", 65536, 128, 4.0 / 128),
                                  ("c4_batch", 512, 1024, 1.0 / 256)):
        host.manual_seed(7)
        torch.manual_seed(7)
        hr = host.Renderer(4, n_levels=16, n_channels=2, log2_table=19, max_samples=S, step=step)
        with torch.no_grad():
            hr.named_parameters()["scene_field.feat_pool"].normal_(0.0, 0.1)
        g = torch.Generator(device=dev).manual_seed(3)
        o = torch.randn(n_rays, 3, device=dev, generator=g) * 0.25
        d = torch.randn(n_rays, 3, device=dev, generator=g)
        gt = torch.rand(n_rays, 3, device=dev, generator=g)
        emb = torch.randint(0, 4, (n_rays,), device=dev, generator=g).to(torch.int32)
        z = 0.5 + 3.0 * torch.rand(n_rays, device=dev, generator=g)
        z[::8] = 0.0
        opts = host.DepthLossOptions(empty=0.1, near=0.1, expected=0.1, eps=0.05)

        def step_with(target):
            def run():
                hr.zero_grad()
                if target is None:
                    hr.train_step(o, d, emb, gt, 1e-2)
                else:
                    hr.train_step(o, d, emb, gt, 1e-2, depth_target=target, depth_loss=opts)
            return run

        ts = alternating({"off": step_with(None), "on": step_with(z)}, args.reps, args.warmup + 1)
        emit({"part": "step", "shape": name, "n_rays": n_rays, "samples_per_ray": S,
              "kept_samples": int(hr.last_n_samples), "var_loss_weight": 1e-2,
              "train_step_ms_no_target": med(ts["off"]), "train_step_ms_depth_terms": med(ts["on"]),
              "train_step_min_ms_no_target": round(ts["off"][0], 4),
              "train_step_min_ms_depth_terms": round(ts["on"][0], 4)}, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="kernels", choices=["kernels", "splat", "step"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pkg = importlib.import_module("f2-nerf_amd")
    if args.part == "kernels":
        part_kernels(pkg.capi, dev, args)
    elif args.part == "splat":
        part_splat(pkg.load_host(), pkg.capi, dev, args)
    else:
        part_step(pkg.load_host(), dev, args)


if __name__ == "__main__":
    main()
