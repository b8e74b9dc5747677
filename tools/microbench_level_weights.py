#!/usr/bin/env python3
"""What level weights cost and save: a training step and a one-pass render at L = 16 with
4, 8, 12 and 16 active levels, skip_masked_levels on and off, against the renderer without weights.

  --part step     One training step (draw the batch, train_step with backward) at the C4 batch (512
                  rays x 1024 samples of 1/256) and at one headline chunk (65 536 rays x 128 samples),
                  24 cameras on a ring, the field of microbench_pose_refine.py --part step.  Arms,
                  alternating in one process:
                    none         no weights set: the step as it is without this feature;
                    a<k>_skip    set_coarse_to_fine(k): k levels at weight 1, the rest at 0, walked
                                 levels = k (Hash3DAnchoredOptions::skip_masked_levels, the default);
                    a<k>_walk    the same weights with every level walked: the fold alone.
                  Median of --reps after --warmup, with min..max.

  --part render   Renderer.render_rays (one launch, f2n_render_rays_lod) of --rays rays x 128 samples
                  on the same field, a validation render; the same arms.

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

N_CAMS, L, F = 24, 16, 2
SHAPES = (("c4_batch", 512, 1024, 1.0 / 256), ("headline_chunk", 65536, 128, 4.0 / 128))


def renderer(host, S, step):
    host.manual_seed(7)
    torch.manual_seed(7)
    hr = host.Renderer(N_CAMS, n_levels=L, n_channels=F, log2_table=19, max_samples=S, step=step)
    with torch.no_grad():
        hr.named_parameters()["scene_field.feat_pool"].normal_(0.0, 0.1)
    return hr


def arms_of(hr, levels, body):
    """{arm: fn}: `body` under each setting of the weights"""
    def arm(k, skip):
        def fn():
            if k is None:
                hr.clear_level_weights()
            else:
                hr.set_skip_masked_levels(skip)
                hr.set_coarse_to_fine(float(k))
            body()
        return fn
    arms = {"none": arm(None, True)}
    for k in levels:
        arms["a%d_skip" % k] = arm(k, True)
        arms["a%d_walk" % k] = arm(k, False)
    return arms


def record(rec, ts, out):
    for k, v in ts.items():
        rec["ms_" + k] = scene.med(v)
        rec["min_max_ms_" + k] = [round(v[0], 4), round(v[-1], 4)]
    scene.emit(rec, out)


def part_step(host, dev, args):
    hw = args.image
    Kc = torch.tensor([[0.8 * hw, 0.0, 0.5 * hw], [0.0, 0.8 * hw, 0.5 * hw], [0.0, 0.0, 1.0]], device=dev)
    intr = Kc.unsqueeze(0).expand(N_CAMS, 3, 3).contiguous()
    poses = scene.ring_poses(N_CAMS, 0.9, 0.25).to(dev)
    for name, n_rays, S, step in SHAPES:
        if name not in args.shapes.split(","):
            continue
        hr = renderer(host, S, step)
        gt = torch.rand(n_rays, 3, device=dev)

        def body():
            o, d, _, cam = host.sample_random_rays(poses, intr, hw, hw, n_rays)
            hr.zero_grad()
            hr.train_step(o, d, cam, gt, 1e-2)

        ts = scene.alternating(arms_of(hr, args.levels, body), args.reps, args.warmup)
        record({"part": "step", "shape": name, "n_rays": n_rays, "samples_per_ray": S, "L": L, "F": F,
                "reps": args.reps}, ts, args.out)


def part_render(host, dev, args):
    S, step = 128, 4.0 / 128
    hr = renderer(host, S, step)
    with torch.no_grad():
        hr.named_parameters()["scene_field.mlp.bias"][0] = 4.0
    o, d = scene.inward_rays(args.rays, dev, 3)[:2]
    kept = {}

    def body():
        with torch.no_grad():
            kept["n"] = hr.render_rays(o, d, None, "validate")[3]

    ts = scene.alternating(arms_of(hr, args.levels, body), args.reps, args.warmup)
    record({"part": "render", "n_rays": args.rays, "samples_per_ray": S, "L": L, "F": F, "reps": args.reps,
            "kept_per_ray_last_arm": round(float(kept["n"].float().mean()), 2)}, ts, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="step", choices=["step", "render"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--levels", type=lambda s: [int(v) for v in s.split(",")], default=[4, 8, 12, 16])
    ap.add_argument("--shapes", default="c4_batch,headline_chunk")
    ap.add_argument("--image", type=int, default=128)
    ap.add_argument("--rays", type=int, default=65536)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    host = importlib.import_module("f2-nerf_amd").load_host()
    if args.part == "step":
        part_step(host, dev, args)
    else:
        part_render(host, dev, args)


if __name__ == "__main__":
    main()
