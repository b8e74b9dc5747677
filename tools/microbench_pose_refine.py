#!/usr/bin/env python3
"""What refining the training poses costs per step, and whether it finds poses that are known.

  --part step      One training step (draw the batch, train_step with backward) at the C4 batch (512
                   rays x 1024 samples of 1/256) and at one headline chunk (65 536 rays x 128 samples),
                   24 cameras on a ring.  Three arms, alternating:
                     plain    rays from sample_random_rays (no gradient to the poses);
                     leaf     the same rays as leaves that require grad, fused_ray_grad on: what the
                              route for rays with a gradient and f2n_hash_rays_grad cost on their own;
                     refiner  rays from PoseRefiner.sample_random_rays: adds f2n_pose_compose, the sort
                              of the camera draw, f2n_cam_pose_grad and f2n_pose_compose_bwd.
                   Median of --reps after --warmup (defaults 5 and 2).  --arms / --shapes pick a
                   subset (one arm and one shape per rocprofv3 --kernel-trace --stats run gives that
                   arm's kernel times).  --exact-grad switches the field's exact_point_grad on for
                   the whole part (the leaf and refiner arms then run f2n_hash_rays_grad_exact).

  --part kernels   f2n_hash_rays_grad (quirk Q5) against f2n_hash_rays_grad_exact on the same kept
                   samples, at the same two shapes: the samples a validation render of the step part's
                   field keeps for a batch drawn from the camera ring, a random d(enc) in the
                   channel-major storage the shade backward leaves.  The two kernels alternate in one
                   process, --inner launches (default 20) per timed window, --reps windows each
                   (at least five pairs), device events around each window.

  --part recover   The analytic sphere scene and the ring of 24 cameras of microbench_occupancy.py
                   --part train.  The training poses are the true ones displaced by a known noise
                   (--rot-noise radians about a random axis, --pos-noise in each coordinate); camera 0
                   is exact and fixed (the gauge).  One run with a PoseRefiner (Adam, --pose-lr) and
                   one without from the same seed.  Every --report-every iterations: the mean rotation
                   error (angle of R_est R_true^T) and the mean translation error over the displaced
                   cameras, and the PSNR of four held-out views rendered from their true poses.
                   --exact-grad: the refiner run receives the encoding's true derivative.  Its
                   magnitude is a third to a quarter of Q5's: --pose-lr is NOT rescaled.
                   --c2f START:END:BASE: coarse-to-fine level weights on the refiner run
                   (host.CoarseToFine: alpha = BASE before iteration START, n_levels from END on,
                   Renderer.set_coarse_to_fine every iteration; the held-out views are rendered with
                   the weights of the moment).  --pose-lr-decay G: the pose optimiser's rate falls
                   to G * --pose-lr over the run, exponentially (done here, in the tool: the refiner
                   has no schedule of its own).

Prints one JSON line per measurement (also appended to --out).
"""
import argparse
import importlib
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import microbench_occupancy as scene  # noqa: E402  (the sphere scene, the camera ring, the timers)

N_CAMS = 24
SHAPES = (("c4_batch", 512, 1024, 1.0 / 256), ("headline_chunk", 65536, 128, 4.0 / 128))


def intrinsics(hw, dev):
    Kc = torch.tensor([[0.8 * hw, 0.0, 0.5 * hw], [0.0, 0.8 * hw, 0.5 * hw], [0.0, 0.0, 1.0]], device=dev)
    return Kc, Kc.unsqueeze(0).expand(N_CAMS, 3, 3).contiguous()


def part_step(host, dev, args):
    hw = args.image
    Kc, intr = intrinsics(hw, dev)
    poses = scene.ring_poses(N_CAMS, 0.9, 0.25).to(dev)
    for name, n_rays, S, step in SHAPES:
        if name not in args.shapes.split(","):
            continue
        host.manual_seed(7)
        torch.manual_seed(7)
        hr = host.Renderer(N_CAMS, n_levels=16, n_channels=2, log2_table=19, max_samples=S, step=step)
        with torch.no_grad():
            hr.named_parameters()["scene_field.feat_pool"].normal_(0.0, 0.1)
        hr.set_fused_ray_grad(True)
        hr.set_exact_ray_grad(args.exact_grad)
        refiner = host.PoseRefiner(poses)
        fixed = torch.zeros(N_CAMS, dtype=torch.int32, device=dev)
        fixed[0] = 1
        refiner.set_fixed(fixed)
        with torch.no_grad():  # corrections that are not zero: the compose kernel does its work
            refiner.delta.normal_(0.0, 1e-3)
        gt = torch.rand(n_rays, 3, device=dev)
        kept = {}

        def plain():
            o, d, _, cam = host.sample_random_rays(poses, intr, hw, hw, n_rays)
            hr.zero_grad()
            hr.train_step(o, d, cam, gt, 1e-2)
            kept["plain"] = int(hr.last_n_samples)

        def leaf():
            o, d, _, cam = host.sample_random_rays(poses, intr, hw, hw, n_rays)
            hr.zero_grad()
            hr.train_step(o.requires_grad_(True), d.requires_grad_(True), cam, gt, 1e-2)
            kept["leaf"] = int(hr.last_n_samples)

        def refined():
            o, d, _, cam = refiner.sample_random_rays(intr, hw, hw, n_rays)
            hr.zero_grad()
            refiner.zero_grad()
            hr.train_step(o, d, cam, gt, 1e-2)
            kept["refiner"] = int(hr.last_n_samples)

        arms = {"plain": plain, "leaf": leaf, "refiner": refined}
        ts = scene.alternating({k: arms[k] for k in args.arms.split(",")}, args.reps, args.warmup)
        rec = {"part": "step", "shape": name, "n_rays": n_rays, "samples_per_ray": S,
               "n_cameras": N_CAMS, "kept_samples": kept, "exact_grad": args.exact_grad}
        for k, v in ts.items():
            rec["step_ms_" + k] = scene.med(v)
            rec["step_min_ms_" + k] = round(v[0], 4)
            rec["step_max_ms_" + k] = round(v[-1], 4)
        if len(ts) == 3:
            rec["route_and_hash_rays_grad_ms"] = round(rec["step_ms_leaf"] - rec["step_ms_plain"], 4)
            rec["refiner_over_leaf_ms"] = round(rec["step_ms_refiner"] - rec["step_ms_leaf"], 4)
        scene.emit(rec, args.out)


def part_kernels(host, capi, dev, args):
    hw = args.image
    Kc, intr = intrinsics(hw, dev)
    poses = scene.ring_poses(N_CAMS, 0.9, 0.25).to(dev)
    L, F = 16, 2
    for name, n_rays, S, step in SHAPES:
        if name not in args.shapes.split(","):
            continue
        host.manual_seed(7)
        torch.manual_seed(7)
        hr = host.Renderer(N_CAMS, n_levels=L, n_channels=F, log2_table=19, max_samples=S, step=step)
        with torch.no_grad():
            hr.named_parameters()["scene_field.feat_pool"].normal_(0.0, 0.1)
        o, d, _, cam = host.sample_random_rays(poses, intr, hw, hw, n_rays)
        with torch.no_grad():
            bounds = hr.render(o, d, None, "validate")[3].contiguous()
            pts_all, _, _, t_all, b_all = hr.pts_sampler.get_samples(o, d, "validate", None)
        length = (bounds[:, 1] - bounds[:, 0]).long()
        k = torch.arange(S, device=dev)[None]
        keep = k < length[:, None]
        src = (b_all[:, :1].long() + k)[keep]                   # a ray keeps a prefix of its samples
        pts, t = pts_all[src].contiguous(), t_all[src].contiguous()
        n = int(pts.shape[0])
        assert n == int(bounds[-1, 1]) and n > 0
        f = hr.scene_field
        fa = (f.table_f16(), f.prim_pool, f.bias_pool.detach(), f.level_mul)
        shape = (L, F, f.local_size, f.level_stride)
        g = torch.Generator(device=dev).manual_seed(5)
        g_enc = torch.randn(L * F, n, device=dev, generator=g) * 5e-3
        outs = {a: (torch.empty(n_rays, 3, device=dev), torch.empty(n_rays, 3, device=dev))
                for a in ("q5", "exact")}

        def q5():
            for _ in range(args.inner):
                capi.call("hash_rays_grad", pts, t, bounds, d, *fa, g_enc, 1, n, *outs["q5"], n_rays, *shape,
                          128.0)

        def exact():
            for _ in range(args.inner):
                capi.call("hash_rays_grad_exact", pts, t, bounds, d, *fa, g_enc, 1, n, *outs["exact"], n_rays,
                          *shape)

        ts = scene.alternating({"hash_rays_grad": q5, "hash_rays_grad_exact": exact}, max(args.reps, 5),
                               args.warmup)
        rec = {"part": "kernels", "shape": name, "n_rays": n_rays, "samples_per_ray": S, "kept_samples": n,
               "L": L, "F": F, "log2_T": 19, "pairs": max(args.reps, 5), "launches_per_window": args.inner}
        for key, v in ts.items():
            per = [x / args.inner for x in v]
            rec[key + "_ms"] = scene.med(per)
            rec[key + "_min_max_ms"] = [round(per[0], 4), round(per[-1], 4)]
        rec["exact_over_q5"] = round(rec["hash_rays_grad_exact_ms"] / rec["hash_rays_grad_ms"], 3)
        rec["norm_ratio_q5_over_exact_d_o"] = round(float(outs["q5"][0].norm() / outs["exact"][0].norm()), 3)
        scene.emit(rec, args.out)


def displaced(poses, rot_noise, pos_noise, seed):
    """Left-multiplied rotations by rot_noise about random axes and shifts of pos_noise * N(0, 1);
    camera 0 stays exact."""
    g = torch.Generator().manual_seed(seed)
    E = poses.shape[0]
    axis = torch.randn(E, 3, generator=g, dtype=torch.float64)
    w = axis / axis.norm(dim=1, keepdim=True) * rot_noise
    w[0] = 0.0
    z = torch.zeros(E, dtype=torch.float64)
    hat = torch.stack([torch.stack([z, -w[:, 2], w[:, 1]], 1), torch.stack([w[:, 2], z, -w[:, 0]], 1),
                       torch.stack([-w[:, 1], w[:, 0], z], 1)], 1)
    R = torch.linalg.matrix_exp(hat) @ poses[:, :, :3].to(torch.float64)
    shift = torch.randn(E, 3, generator=g, dtype=torch.float64) * pos_noise
    shift[0] = 0.0
    t = poses[:, :, 3].to(torch.float64) + shift
    return torch.cat([R, t.unsqueeze(2)], 2).to(torch.float32).contiguous()


def pose_errors(est, true):
    """(mean rotation angle in degrees, mean translation distance) over cameras 1.."""
    rel = est[1:, :, :3].to(torch.float64) @ true[1:, :, :3].to(torch.float64).transpose(1, 2)
    cos = ((rel.diagonal(dim1=1, dim2=2).sum(1) - 1.0) / 2.0).clamp(-1.0, 1.0)
    rot = torch.rad2deg(torch.acos(cos)).mean()
    pos = (est[1:, :, 3] - true[1:, :, 3]).norm(dim=1).mean()
    return float(rot), float(pos)


def recover_once(host, dev, args, refine):
    hw = args.image
    Kc, intr = intrinsics(hw, dev)
    true = scene.ring_poses(N_CAMS, 0.9, 0.25)
    held = scene.ring_poses(4, 0.9, 0.1, phase=0.13).to(dev)
    noisy = displaced(true, args.rot_noise, args.pos_noise, 17).to(dev)
    true = true.to(dev)
    images = torch.stack([scene.analytic_colors(*host.get_view_rays(true[i], Kc, hw, hw)).reshape(hw, hw, 3)
                          for i in range(N_CAMS)]).contiguous()
    truth = torch.stack([scene.analytic_colors(*host.get_view_rays(held[i], Kc, hw, hw))
                         for i in range(held.shape[0])])
    host.manual_seed(11)
    torch.manual_seed(11)
    hr = host.Renderer(N_CAMS, n_levels=scene.L, n_channels=scene.F, log2_table=scene.LOG2_T,
                       max_samples=scene.S, step=scene.STEP)
    hr.set_dense_first_pass(-1)
    hr.set_fused_ray_grad(True)
    hr.set_exact_ray_grad(args.exact_grad and refine)
    opt = hr.make_fused_adam(args.lr)
    refiner = pose_opt = None
    if refine:
        refiner = host.PoseRefiner(noisy)
        fixed = torch.zeros(N_CAMS, dtype=torch.int32, device=dev)
        fixed[0] = 1
        refiner.set_fixed(fixed)
        pose_opt = refiner.make_adam(args.pose_lr)
    bg = torch.tensor(scene.BACKGROUND, device=dev).expand(512, 3).contiguous()
    c2f = None
    if args.c2f and refine:
        start, end, base = (float(v) for v in args.c2f.split(":"))
        c2f = host.CoarseToFine(start=start, end=end, base=base)
        hr.set_coarse_to_fine(c2f.alpha_at(0.0, scene.L))

    def report(it):
        est = refiner.poses().detach() if refine else noisy
        rot, pos = pose_errors(est, true)
        with torch.no_grad():
            views = torch.stack([
                hr.render_all_rays(*host.get_view_rays(held[i], Kc, hw, hw), 16384)[0].clip(0, 1)
                for i in range(held.shape[0])])
        scene.emit({"part": "recover", "refiner": refine, "iteration": it,
                    "rot_err_deg": round(rot, 4), "pos_err": round(pos, 5),
                    "psnr_heldout": round(scene.psnr(views, truth), 3),
                    "rot_noise_deg": round(math.degrees(args.rot_noise), 3),
                    "pos_noise": args.pos_noise, "pose_lr": args.pose_lr if refine else None,
                    "exact_grad": bool(args.exact_grad and refine),
                    "c2f": args.c2f if c2f is not None else None,
                    "alpha": round(c2f.alpha_at(float(it), scene.L), 4) if c2f is not None else None,
                    "active_levels": int(hr.active_levels()),
                    "pose_lr_decay": args.pose_lr_decay if refine else None},
                   args.out)

    report(0)
    for it in range(1, args.iters + 1):
        if c2f is not None:
            hr.set_coarse_to_fine(c2f.alpha_at(float(it), scene.L))
        if refine and args.pose_lr_decay != 1.0:
            pose_opt.set_lr(args.pose_lr * args.pose_lr_decay ** (it / args.iters))
        if refine:
            o, d, gt, cam = refiner.sample_random_rays(intr, hw, hw, 512, images=images)
            pose_opt.zero_grad()
        else:
            o, d, gt, cam = host.sample_random_rays(noisy, intr, hw, hw, 512, images)
        opt.zero_grad()
        hr.train_step(o, d, cam, gt, 0.0, None, bg, True)
        opt.step()
        if refine:
            pose_opt.step()
        if it % args.report_every == 0 or it == args.iters:
            report(it)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="step", choices=["step", "kernels", "recover"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--arms", default="plain,leaf,refiner",
                    help="--part step: a subset, e.g. one arm for a kernel trace of its own")
    ap.add_argument("--shapes", default="c4_batch,headline_chunk")
    ap.add_argument("--image", type=int, default=128)
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--report-every", type=int, default=500)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--pose-lr", type=float, default=1e-3)
    ap.add_argument("--rot-noise", type=float, default=0.03, help="radians")
    ap.add_argument("--pos-noise", type=float, default=0.02)
    ap.add_argument("--exact-grad", action="store_true",
                    help="Hash3DAnchoredOptions::exact_point_grad on: the encoding's true derivative")
    ap.add_argument("--c2f", default="", metavar="START:END:BASE",
                    help="--part recover: coarse-to-fine level weights on the refiner run")
    ap.add_argument("--pose-lr-decay", type=float, default=1.0,
                    help="--part recover: the pose rate ends at this fraction of --pose-lr")
    ap.add_argument("--inner", type=int, default=20, help="--part kernels: launches per timed window")
    ap.add_argument("--no-baseline", action="store_true",
                    help="--part recover: skip the run without a refiner")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pkg = importlib.import_module("f2-nerf_amd")
    host = pkg.load_host()
    if args.part == "step":
        part_step(host, dev, args)
    elif args.part == "kernels":
        part_kernels(host, pkg.capi, dev, args)
    else:
        for refine in (True,) if args.no_baseline else (True, False):
            recover_once(host, dev, args, refine)


if __name__ == "__main__":
    main()
