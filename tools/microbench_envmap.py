#!/usr/bin/env python3
"""What a learned background (EnvMap, Renderer.set_background) costs.

  --part kernels  f2n_envmap_fwd, f2n_envmap_bwd and f2n_envmap_grad_apply on 65 536 rays and R = 128,
                  each timed on its own, at sky fractions 0.2 and 1.0 (the share of the rays whose d_bg
                  is not zero: an opaque ray issues no atomic).  A kernel takes microseconds, so one
                  timed window is --inner back-to-back launches between two device events.
  --part step     The supervised step of tools/microbench_supervision.py (workload C4's batch: 512 rays,
                  1024 samples of 1/256; ray weights, alpha targets, opacity weight 0.1) four ways, the
                  arms alternating: on the march route (an occupancy grid attached) without and with
                  the map, and on the dense route without and with it -- where a bg that carries a
                  gradient gives up the lean and the bucketed form.  Without the map the step gets a
                  bg_color and composites its target; with it bg_color is left to the map and
                  composite_target is off.
                  Then, on that step's real d_bg, the largest relative difference between the
                  fixed-point texture gradient and float64 sums of the same contributions: what the
                  shift of 48 bits costs.

Median of --reps windows after --warmup.  Prints one JSON line per measurement (also appended to
--out)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
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


def part_kernels(host, capi, dev, args):
    n, R = 65536, 128
    g = torch.Generator(device=dev).manual_seed(11)
    dirs = torch.randn(n, 3, device=dev, generator=g)
    tex = torch.randn(6, R, R, 3, device=dev, generator=g)
    bg = host.envmap_query(dirs, tex)
    acc = torch.zeros(18 * R * R, dtype=torch.int64, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    d_tex = torch.empty_like(tex)
    out = torch.empty_like(bg)
    full = torch.randn(n, 3, device=dev, generator=g) * 1e-3
    for frac in (0.2, 1.0):
        sky = (torch.rand(n, device=dev, generator=g) < frac).float().unsqueeze(1)
        d_bg = (full * sky).contiguous()
        fns = {
            "fwd": lambda: capi.call("envmap_fwd", dirs, tex, R, out, n),
            "bwd": lambda: capi.call("envmap_bwd", dirs, bg, d_bg, R, acc, flags, n),
            "apply": lambda: capi.call("envmap_grad_apply", acc, R, d_tex, 0),
        }
        ts = alternating(fns, args.reps, args.warmup, args.inner)
        atomics = int((d_bg != 0).sum()) * 4
        emit({"part": "kernels", "n_rays": n, "R": R, "sky_fraction": frac,
              "sky_measured": round(float(sky.mean()), 4), "atomics_per_bwd_at_most": atomics,
              "inner": args.inner, "fwd_us": round(med(ts["fwd"]) * 1e3, 2),
              "bwd_us": round(med(ts["bwd"]) * 1e3, 2), "apply_us": round(med(ts["apply"]) * 1e3, 2),
              "fwd_min_us": round(ts["fwd"][0] * 1e3, 2), "bwd_min_us": round(ts["bwd"][0] * 1e3, 2),
              "apply_min_us": round(ts["apply"][0] * 1e3, 2), "flags": int(flags)}, args.out)


def part_step(host, capi, dev, args):
    n_rays, S, step, R = 512, 1024, 1.0 / 256, 128
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
    m = (torch.rand(n_rays, device=dev, generator=g) > 0.1).float()
    alpha = torch.rand(n_rays, device=dev, generator=g).round()
    noise = torch.rand(n_rays, S, device=dev, generator=g) + 0.5
    sup = host.RaySupervision(ray_weight=m, alpha=alpha, opacity_weight=0.1)
    sup_map = host.RaySupervision(ray_weight=m, alpha=alpha, opacity_weight=0.1, composite_target=False)
    env = host.EnvMap(R)
    with torch.no_grad():
        env.texture.normal_(0.0, 1.0)
    grid = host.OccupancyGrid(128, str(dev))

    def arm(use_grid, use_map):
        def run():
            hr.set_occupancy(grid if use_grid else None)
            hr.set_dense_first_pass(0 if use_grid else 1)
            hr.set_background(env if use_map else None)
            hr.zero_grad()
            env.zero_grad()
            hr.train_step_supervised(o, d, emb, gt, sup_map if use_map else sup, 1e-2, noise,
                                     None if use_map else bg)
        return run

    fns = {"march_grid": arm(True, False), "march_grid_map": arm(True, True),
           "dense": arm(False, False), "dense_map": arm(False, True)}
    ts = alternating(fns, args.reps, args.warmup + 1)
    rec = {"part": "step", "shape": "c4_batch", "n_rays": n_rays, "samples_per_ray": S, "R": R,
           "kept_samples": int(hr.last_n_samples), "sky_rays": int(((alpha == 0) & (m != 0)).sum())}
    for k, v in ts.items():
        rec["train_step_ms_" + k] = med(v)
        rec["train_step_min_ms_" + k] = round(v[0], 4)
    emit(rec, args.out)

    # the cost of the fixed point on this step's real d_bg
    from tests import envmap_model as em

    hr.set_occupancy(grid)
    hr.set_dense_first_pass(0)
    hr.set_background(None)
    leaf = env.query(d).detach().requires_grad_(True)
    hr.zero_grad()
    hr.train_step_supervised(o, d, emb, gt, sup_map, 1e-2, noise, leaf)
    hr.set_background(env)
    env.zero_grad()
    hr.zero_grad()
    hr.train_step_supervised(o, d, emb, gt, sup_map, 1e-2, noise, None)
    torch.cuda.synchronize()
    fixed = env.texture.grad.double().cpu().numpy().reshape(-1)
    f64 = em.backward_float64(d.cpu().numpy(), leaf.detach().cpu().numpy(), leaf.grad.cpu().numpy(), R)
    live = f64 != 0
    rel = np.abs(fixed[live] - f64[live]) / np.abs(f64[live])
    # ... and against float64 sums of the kernel's own float32 gl (three float32 roundings before the
    # products): what is left is the 2^-48 quantum per contribution and the one rounding to float32
    b32, g32 = leaf.detach().cpu().numpy(), leaf.grad.cpu().numpy()
    gl32 = (g32 * (b32 * (np.float32(1) - b32)).astype(np.float32)).astype(np.float32)
    geo = em.geometry(d.cpu().numpy(), R)
    same = np.zeros_like(f64)
    elem = geo["idx"][:, :, None] * 3 + np.arange(3)[None, None, :]
    np.add.at(same, elem.reshape(-1),
              (gl32.astype(np.float64)[:, None, :] * geo["w"].astype(np.float64)[:, :, None]).reshape(-1))
    mag = np.zeros_like(f64)
    np.add.at(mag, elem.reshape(-1),
              np.abs(gl32.astype(np.float64)[:, None, :] * geo["w"].astype(np.float64)[:, :, None]).reshape(-1))
    rel_same = np.abs(fixed[live] - same[live]) / np.abs(same[live])
    emit({"part": "fixed_point", "R": R, "n_rays": n_rays, "shift": em.SHIFT,
          "max_rel_diff_vs_float64_of_the_same_f32_gl": float(rel_same.max()),
          "max_diff_vs_float64_over_sum_of_abs": float((np.abs(fixed[live] - f64[live]) / mag[live]).max()),
          "largest_cancellation_sum_of_abs_over_abs_sum": float((mag[live] / np.abs(f64[live])).max()),
          "d_bg_abs_max": float(leaf.grad.abs().max()),
          "d_bg_abs_min_nonzero": float(leaf.grad[leaf.grad != 0].abs().min()),
          "texels_touched": int(live.sum()) // 1, "max_rel_diff_vs_float64": float(rel.max()),
          "float32_ulp": 2.0 ** -24, "flags": env.flags()}, args.out)
    hr.set_background(None)
    hr.set_occupancy(None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="kernels", choices=["kernels", "step"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pkg = importlib.import_module("f2-nerf_amd")
    host = pkg.load_host()
    {"kernels": part_kernels, "step": part_step}[args.part](host, pkg.capi, dev, args)


if __name__ == "__main__":
    main()
