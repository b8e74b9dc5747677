#!/usr/bin/env python3
"""What refining the calibration costs: the per-camera gradient kernel beside its pose twin, and a
training step with and without the IntrinsicsRefiner.

  --part kernels   f2n_cam_intr_grad beside f2n_cam_pose_grad on the same camera-sorted batch (the
                   same n, E, ij, d_rays_d, cam_start), 24 cameras with (k1, k2, p1, p2) of a mild
                   barrel lens, at n = 512, 65 536 and 1 048 576 rays.  Median of --reps after
                   --warmup, the two alternating.

  --part step      One training step (draw the batch, train_step with backward) at the C4 batch (512
                   rays x 1024 samples of 1/256) and at one headline chunk (65 536 rays x 128 samples),
                   24 cameras on a ring that one physical camera took.  Two arms, alternating:
                     pose   rays from PoseRefiner.sample_random_rays: the step as it was before the
                            calibration could be refined (the yardstick);
                     both   rays from IntrinsicsRefiner.sample_random_rays(pose_refiner.poses(), ...):
                            adds f2n_intr_compose, f2n_cam_intr_grad and f2n_intr_compose_bwd.

Prints one JSON line per measurement (also appended to --out).
"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import microbench_occupancy as scene  # noqa: E402  (the camera ring, the timers)
from microbench_pose_refine import N_CAMS, intrinsics  # noqa: E402

LENS = (-0.1, 0.02, 1e-3, -2e-3)


def part_kernels(host, dev, args):
    capi = importlib.import_module("f2-nerf_amd.capi")
    hw = args.image
    _, intr = intrinsics(hw, dev)
    poses = scene.ring_poses(N_CAMS, 0.9, 0.25).to(dev).contiguous()
    dist = torch.tensor(LENS, device=dev).expand(N_CAMS, 4).contiguous()
    cdll = capi.lib().cdll
    for n in (512, 65536, 1 << 20):
        g = torch.Generator(device=dev).manual_seed(n)
        cam = torch.randint(0, N_CAMS, (n,), device=dev, generator=g, dtype=torch.int32).sort().values
        ij = torch.randint(0, hw, (n, 2), device=dev, generator=g, dtype=torch.int32)
        d_o = torch.randn(n, 3, device=dev, generator=g)
        d_d = torch.randn(n, 3, device=dev, generator=g)
        cam_start = torch.searchsorted(cam, torch.arange(N_CAMS + 1, device=dev, dtype=torch.int32),
                                       out_int32=True)
        d_poses = torch.empty(N_CAMS, 12, device=dev)
        d_intr = torch.empty(N_CAMS, 8, device=dev)
        ws_p = torch.empty(cdll.f2n_cam_pose_grad_workspace_floats(n, N_CAMS), device=dev)
        ws_i = torch.empty(cdll.f2n_cam_intr_grad_workspace_floats(n, N_CAMS), device=dev)

        def pose():
            capi.call("cam_pose_grad", intr, dist, ij, d_o, d_d, cam_start, None, d_poses, 12, ws_p, n,
                      N_CAMS)

        def calib():
            capi.call("cam_intr_grad", poses, 12, intr, dist, ij, d_d, cam_start, None, d_intr, ws_i, n,
                      N_CAMS)

        ts = scene.alternating({"cam_pose_grad": pose, "cam_intr_grad": calib}, args.reps, args.warmup)
        rec = {"part": "kernels", "n_rays": n, "n_cameras": N_CAMS, "distorted": True}
        for k, v in ts.items():
            rec[k + "_ms"] = scene.med(v)
            rec[k + "_min_ms"] = round(v[0], 4)
        scene.emit(rec, args.out)


def part_step(host, dev, args):
    hw = args.image
    _, intr = intrinsics(hw, dev)
    poses = scene.ring_poses(N_CAMS, 0.9, 0.25).to(dev)
    dist = torch.tensor(LENS, device=dev).expand(N_CAMS, 4).contiguous()
    for name, n_rays, S, step in (("c4_batch", 512, 1024, 1.0 / 256),
                                  ("headline_chunk", 65536, 128, 4.0 / 128)):
        if name not in args.shapes.split(","):
            continue
        host.manual_seed(7)
        torch.manual_seed(7)
        hr = host.Renderer(N_CAMS, n_levels=16, n_channels=2, log2_table=19, max_samples=S, step=step)
        with torch.no_grad():
            hr.named_parameters()["scene_field.feat_pool"].normal_(0.0, 0.1)
        hr.set_fused_ray_grad(True)
        poser = host.PoseRefiner(poses)
        fixed = torch.zeros(N_CAMS, dtype=torch.int32, device=dev)
        fixed[0] = 1
        poser.set_fixed(fixed)
        calib = host.IntrinsicsRefiner(intr, dist)
        with torch.no_grad():  # corrections that are not zero: the compose kernels do their work
            poser.delta.normal_(0.0, 1e-3)
            calib.gamma.normal_(0.0, 1e-3)
        gt = torch.rand(n_rays, 3, device=dev)
        kept = {}

        def pose_only():
            o, d, _, cam = poser.sample_random_rays(intr, hw, hw, n_rays, dist=dist)
            hr.zero_grad()
            poser.zero_grad()
            hr.train_step(o, d, cam, gt, 1e-2)
            kept["pose"] = int(hr.last_n_samples)

        def both():
            o, d, _, cam = calib.sample_random_rays(poser.poses(), hw, hw, n_rays)
            hr.zero_grad()
            poser.zero_grad()
            calib.zero_grad()
            hr.train_step(o, d, cam, gt, 1e-2)
            kept["both"] = int(hr.last_n_samples)

        arms = {"pose": pose_only, "both": both}
        ts = scene.alternating({k: arms[k] for k in args.arms.split(",")}, args.reps, args.warmup)
        rec = {"part": "step", "shape": name, "n_rays": n_rays, "samples_per_ray": S,
               "n_cameras": N_CAMS, "kept_samples": kept}
        for k, v in ts.items():
            rec["step_ms_" + k] = scene.med(v)
            rec["step_min_ms_" + k] = round(v[0], 4)
            rec["step_max_ms_" + k] = round(v[-1], 4)
        if len(ts) == 2:
            rec["calibration_over_pose_ms"] = round(rec["step_ms_both"] - rec["step_ms_pose"], 4)
        scene.emit(rec, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="kernels", choices=["kernels", "step"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--arms", default="pose,both")
    ap.add_argument("--shapes", default="c4_batch,headline_chunk")
    ap.add_argument("--image", type=int, default=128)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    host = importlib.import_module("f2-nerf_amd").load_host()
    (part_kernels if args.part == "kernels" else part_step)(host, dev, args)


if __name__ == "__main__":
    main()
