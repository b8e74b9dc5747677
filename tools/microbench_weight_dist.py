#!/usr/bin/env python3
"""What the distortion loss costs, next to the regulariser it stands beside.

  --part kernels   f2n_weight_dist_fwd / _bwd and f2n_weight_var_fwd / _bwd through the C ABI on the
                   SAME bounds and weights: 65 536 rays x 128 samples (a headline chunk) and 512 rays x
                   1024 samples (the C4 batch), every ray full.  The new kernels read three arrays
                   (weights, t, dt) to weight_var's one and scan twice per stride; the algorithmic
                   bytes per launch are in the record.
  --part step      One train_step with dist_loss_weight = 0 and = 0.01, alternating: the C4 batch
                   (512 rays, 1024 samples of 1/256) and one headline chunk (65 536 rays, 128 samples).

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


def part_kernels(capi, dev, args):
    for n_rays, S in ((65536, 128), (512, 1024)):
        n = n_rays * S
        g = torch.Generator(device=dev).manual_seed(5)
        w = torch.rand(n, device=dev, generator=g) / S
        dt = torch.rand(n, device=dev, generator=g) * (4.0 / S) + 2.0 / S
        t = torch.cumsum(dt.reshape(n_rays, S), 1).reshape(-1).contiguous()
        start = torch.arange(n_rays, device=dev, dtype=torch.int32) * S
        bounds = torch.stack([start, start + S], 1).contiguous()
        d_out = torch.randn(n_rays, device=dev, generator=g)
        out = torch.empty(n_rays, device=dev)
        dw = torch.empty(n, device=dev)
        fns = {
            "weight_var_fwd": lambda: capi.call("weight_var_fwd", w, bounds, out, n_rays),
            "weight_var_bwd": lambda: capi.call("weight_var_bwd", w, bounds, d_out, dw, n_rays),
            "weight_dist_fwd": lambda: capi.call("weight_dist_fwd", w, t, dt, bounds, out, n_rays),
            "weight_dist_bwd": lambda: capi.call("weight_dist_bwd", w, t, dt, bounds, d_out, dw, n_rays),
        }
        ts = alternating(fns, args.reps, args.warmup)
        # bytes if every array is touched once per pass the kernel makes over it
        bytes_once = {"weight_var_fwd": 4 * n * 2, "weight_var_bwd": 4 * n * 3 + 4 * n,
                      "weight_dist_fwd": 12 * n, "weight_dist_bwd": 12 * n * 2 + 4 * n}
        rec = {"part": "kernels", "n_rays": n_rays, "samples_per_ray": S}
        for k, v in ts.items():
            rec[k + "_ms"] = med(v)
            rec[k + "_min_ms"] = round(v[0], 4)
            rec[k + "_GBs"] = round(bytes_once[k] / (med(v) * 1e-3) / 1e9, 1)
        rec["fwd_over_var"] = round(rec["weight_dist_fwd_ms"] / rec["weight_var_fwd_ms"], 2)
        rec["bwd_over_var"] = round(rec["weight_dist_bwd_ms"] / rec["weight_var_bwd_ms"], 2)
        emit(rec, args.out)


def part_step(host, dev, args):
    for name, n_rays, S, step in (("c4_batch", 512, 1024, 1.0 / 256), ("headline_chunk", 65536, 128, 4.0 / 128)):
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

        def step_with(lam):
            def run():
                hr.zero_grad()
                hr.train_step(o, d, emb, gt, 1e-2, dist_loss_weight=lam)
            return run

        ts = alternating({"off": step_with(0.0), "on": step_with(0.01)}, args.reps, args.warmup + 1)
        emit({"part": "step", "shape": name, "n_rays": n_rays, "samples_per_ray": S,
              "kept_samples": int(hr.last_n_samples), "var_loss_weight": 1e-2,
              "train_step_ms_weight_0": med(ts["off"]), "train_step_ms_weight_0.01": med(ts["on"]),
              "train_step_min_ms_weight_0": round(ts["off"][0], 4),
              "train_step_min_ms_weight_0.01": round(ts["on"][0], 4)}, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="kernels", choices=["kernels", "step"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pkg = importlib.import_module("f2-nerf_amd")
    if args.part == "kernels":
        part_kernels(pkg.capi, dev, args)
    else:
        part_step(pkg.load_host(), dev, args)


if __name__ == "__main__":
    main()
