#!/usr/bin/env python3
"""Pose optimisation at the localiser's chunk (reference Localizer::optimize_pose_by_differential,
src/localizer.cpp:142-167): one 256x256 view = 65536 rays of S = 1024 samples at step 1/256, VALIDATE,
L = 16, F = 2, T = 2^19.  Times get_view_rays(pose) + render + MSE + backward to the pose, four ways:

  op     rays that require grad go op by op (RendererOptions::fused_ray_grad off, the default)
  fused  they take the fused path (Renderer.set_fused_ray_grad(True))
  x  field requiring grad (loss.backward(), the table / MLP / embedding gradients are formed too)
  x  field frozen (requires_grad_(False) on every parameter: only the pose gradient)

and for two densities: "trained" (a trained-like table, most rays terminate) and "dense" (a density
so low that no ray terminates: every one of the 67 M samples is kept).

  python tools/microbench_pose_grad.py [--density trained|dense|both] [--routes op,fused]
                                       [--fields grad,frozen] [--reps 3]

Prints one JSON line per configuration: median and minimum ms per iteration, kept samples.
"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = W = 256
S, STEP, L, F, LOG2_T = 1024, 1.0 / 256, 16, 2, 19


def make_renderer(host, density, dev):
    torch.manual_seed(7)
    hr = host.Renderer(1, n_levels=L, n_channels=F, log2_table=LOG2_T, max_samples=S, step=STEP)
    p = hr.named_parameters()
    g = torch.Generator(device=dev).manual_seed(7)
    with torch.no_grad():
        fp = p["scene_field.feat_pool"]
        fp.copy_(torch.randn(fp.shape, device=dev, generator=g) * 0.1)  # trained-like table
        # density logit bias: 5 lets most rays terminate within their 1024 samples, -10 none
        p["scene_field.mlp.bias"][0] = 5.0 if density == "trained" else -10.0
    return hr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--density", default="both", choices=["trained", "dense", "both"])
    ap.add_argument("--routes", default="op,fused")
    ap.add_argument("--fields", default="grad,frozen")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    host = importlib.import_module("f2-nerf_amd").load_host()
    pose0 = torch.tensor([[1.0, 0.0, 0.0, 0.05], [0.0, 1.0, 0.0, -0.03], [0.0, 0.0, 1.0, 0.02]],
                         device=dev)
    K = torch.tensor([[0.9 * W, 0.0, 0.5 * W], [0.0, 0.9 * H, 0.5 * H], [0.0, 0.0, 1.0]], device=dev)
    target = torch.rand(H * W, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    densities = ["trained", "dense"] if args.density == "both" else [args.density]
    for density in densities:
        hr = make_renderer(host, density, dev)
        hr.set_dense_first_pass(-1)
        params = hr.named_parameters()
        for field in args.fields.split(","):
            for k, v in params.items():
                if k != "scene_field.prim_pool":
                    v.requires_grad_(field == "grad")
            for route in args.routes.split(","):
                hr.set_fused_ray_grad(route == "fused")

                def step():
                    hr.zero_grad()
                    pose = pose0.clone().requires_grad_(True)
                    o, d = host.get_view_rays(pose, K, H, W)
                    colors, depths, weights, idx = hr.render(o, d, None, "validate")
                    loss = torch.nn.functional.mse_loss(colors, target)
                    loss.backward()
                    return pose.grad

                for _ in range(args.warmup):
                    step()
                torch.cuda.synchronize()
                ts = []
                for _ in range(args.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    gp = step()
                    e1.record()
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1))
                ts.sort()
                print(json.dumps({
                    "density": density, "route": route, "field": field, "rays": H * W,
                    "samples_per_ray": S, "kept_samples": int(hr.last_n_samples),
                    "ms_median": round(ts[len(ts) // 2], 3), "ms_min": round(ts[0], 3),
                    "pose_grad_norm": float(gp.norm()),
                }), flush=True)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
