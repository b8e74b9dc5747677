#!/usr/bin/env python3
"""One localisation step at the shape the reference's ROS node runs (Localizer::
optimize_pose_by_random_search + calc_average_pose, src/localizer.cpp:64-128,176-316): P = 100 and 50
particles, K = 256 pixels, VALIDATE, S = 1024 samples at step 1/256, L = 16, F = 2, T = 2^19, a
trained-like field in the terminating regime (as tools/microbench_pose_grad.py, density "trained").

  arm A  this library's Localizer: f2n_perturb_poses, one f2n_gen_rays launch, the fused render,
         f2n_pose_scores, f2n_average_pose
  arm B  the reference's arrangement on this library's public operators: per particle three host
         rotations copied up and three mm; a get_rays_from_pose per pose and two cats; the same
         render; clip, index and the squared-error reduction as ATen launches on the image's device
         (the GPU, as in the ROS node), the P losses copied to the host for pow and normalisation;
         per particle a rotation copied down and the quaternion mean on the host

Both arms are driven from Python, so arm B's loops pay interpreter time the reference's C++ loops do
not; its launches and blocking copies are the reference's.  The render is common to both.

Each phase is timed with the host clock around a final synchronise (the point is the host share),
median of --reps after --warmup; "step_ms" is the whole step timed the same way without the
synchronises between phases.  Arm A's step_ms times the public methods
(optimize_pose_by_random_search + calc_average_pose); its phase_ms times this tool's re-assembly of
the same launches from the bound pieces, since the class offers no place to synchronise inside.  One JSON line per arm and P; --out appends them to a file.

  python tools/microbench_localizer.py [--particles 100,50] [--reps 5] [--warmup 2] [--out FILE]
"""
import argparse
import importlib
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = W = 256
K_PIX = 256
S, STEP, L, F, LOG2_T = 1024, 1.0 / 256, 16, 2, 19
PHASES = ("pose_generation", "ray_generation", "render", "scoring", "average")


def make_renderer(host, dev):
    torch.manual_seed(7)
    hr = host.Renderer(1, n_levels=L, n_channels=F, log2_table=LOG2_T, max_samples=S, step=STEP)
    p = hr.named_parameters()
    g = torch.Generator(device=dev).manual_seed(7)
    with torch.no_grad():
        fp = p["scene_field.feat_pool"]
        fp.copy_(torch.randn(fp.shape, device=dev, generator=g) * 0.1)  # trained-like table
        p["scene_field.mlp.bias"][0] = 5.0  # most rays terminate within their 1024 samples
    return hr


class Clock:
    """Host wall clock per phase, each closed by a synchronise."""

    def __init__(self, sync):
        self.sync, self.ms, self.t = sync, {}, None

    def start(self):
        torch.cuda.synchronize()
        self.t = time.perf_counter()

    def lap(self, name):
        if self.sync:
            torch.cuda.synchronize()
            now = time.perf_counter()
            self.ms[name] = self.ms.get(name, 0.0) + (now - self.t) * 1e3
            self.t = now


def arm_a(host, loc, pose, image, P, clock):
    with torch.no_grad():
        if not clock.sync:  # the public step
            particles = loc.optimize_pose_by_random_search(pose, image, P, 1.0)
            return host.Localizer.calc_average_pose(particles)
        noise = torch.randn(P, 6, device=pose.device)
        poses = host.perturb_poses(pose, noise, loc.noise_sigmas(1.0))
        clock.lap("pose_generation")
        pix = torch.randperm(H * W, device=pose.device)[:K_PIX]
        ij = torch.stack([pix // W, pix % W], 1).to(torch.int32)
        o, d = loc.pose_rays(poses, ij)
        clock.lap("ray_generation")
        colors, _ = loc.renderer.render_all_rays(o, d, 1 << 16)
        clock.lap("render")
        loss, weights = host.pose_scores(colors, image, ij)
        weights_host = weights.cpu()  # the one read of the particle form
        clock.lap("scoring")
        avg = host.average_pose(poses, weights_host.to(pose.device))
        clock.lap("average")
        return avg


def _host_rotation(axis, theta):
    c, s = math.cos(theta), math.sin(theta)
    m = {0: [[1, 0, 0], [0, c, s], [0, -s, c]], 1: [[c, 0, -s], [0, 1, 0], [s, 0, c]],
         2: [[c, s, 0], [-s, c, 0], [0, 0, 1]]}[axis]
    return torch.tensor(m, dtype=torch.float32)


def _quat(m):
    t = m[0][0] + m[1][1] + m[2][2]
    if t > 0:
        t = math.sqrt(t + 1.0)
        r = 0.5 / t
        return [0.5 * t, (m[2][1] - m[1][2]) * r, (m[0][2] - m[2][0]) * r, (m[1][0] - m[0][1]) * r]
    i = 0
    if m[1][1] > m[0][0]:
        i = 1
    if m[2][2] > m[i][i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
    q = [0.0] * 4
    q[1 + i] = 0.5 * t
    r = 0.5 / t
    q[0] = (m[k][j] - m[j][k]) * r
    q[1 + j] = (m[j][i] + m[i][j]) * r
    q[1 + k] = (m[k][i] + m[i][k]) * r
    return q


def arm_b(host, hr, intrinsic, sigmas, pose, image, P, clock):
    dev = pose.device
    with torch.no_grad():
        poses = []
        for i in range(P):
            cur = pose.clone()
            if i > 0:
                n = torch.randn(6).tolist()
                for a in range(3):
                    cur[a][3] += sigmas[a] * n[a]
                rot = [_host_rotation(a, sigmas[3 + a] * n[3 + a] * math.pi / 180.0).to(dev)
                       for a in range(3)]
                cur[:3, :3] = rot[2].mm(rot[1].mm(rot[0].mm(cur[:3, :3])))
            poses.append(cur)
        clock.lap("pose_generation")
        pix = torch.randperm(H * W)[:K_PIX]  # the host shuffle
        i_idx, j_idx = (pix // W).to(dev), (pix % W).to(dev)
        ij = torch.stack([i_idx, j_idx], -1).to(torch.float32)
        rays = [host.get_rays_from_pose(p[None], intrinsic[None], ij) for p in poses]
        o, d = torch.cat([r[0] for r in rays]), torch.cat([r[1] for r in rays])
        clock.lap("ray_generation")
        colors, _ = hr.render_all_rays(o, d, 1 << 16)
        clock.lap("render")
        pred = colors.view(P, K_PIX, 3).clip(0.0, 1.0).to(image.device)
        gt = image[i_idx.to(image.device), j_idx.to(image.device)]
        diff = pred - gt
        score = (diff * diff).mean(-1).sum(-1).cpu()
        score = K_PIX / (score + 1e-6)
        score = torch.pow(score, 5)
        score /= score.sum()
        weights = score.tolist()
        clock.lap("scoring")
        pos = torch.zeros(3, 1, device=dev)
        quats = []
        for p, wgt in zip(poses, weights):
            pos += p[:3, 3:4] * wgt
            quats.append(_quat(p[:3, :3].to(torch.float64).cpu().tolist()))
        acc = [0.0] * 4
        for q in quats:
            sgn = -1.0 if sum(a * b for a, b in zip(q, quats[0])) < 0 else 1.0
            acc = [a + sgn * b for a, b in zip(acc, q)]
        norm = math.sqrt(sum(a * a for a in acc))
        w_, x, y, z = (a / norm for a in acc)
        rot = torch.tensor([
            [1 - 2 * (y * y + z * z), 2 * (x * y - w_ * z), 2 * (x * z + w_ * y)],
            [2 * (x * y + w_ * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w_ * x)],
            [2 * (x * z - w_ * y), 2 * (y * z + w_ * x), 1 - 2 * (x * x + y * y)]],
            dtype=torch.float64).to(torch.float32).to(dev)
        avg = torch.zeros_like(pose)
        avg[:3, 3:4] = pos
        avg[:3, :3] = rot
        clock.lap("average")
        return avg


def measure(fn, reps, warmup):
    """-> (median ms per phase, median whole-step ms)"""
    for _ in range(warmup):
        for sync in (True, False):
            c = Clock(sync)
            c.start()
            fn(c)
    phase_runs, steps = [], []
    for _ in range(reps):
        c = Clock(True)
        c.start()
        fn(c)
        phase_runs.append(c.ms)
        c = Clock(False)
        c.start()
        fn(c)
        torch.cuda.synchronize()
        steps.append((time.perf_counter() - c.t) * 1e3)
    med = lambda v: sorted(v)[len(v) // 2]
    return {k: round(med([r[k] for r in phase_runs]), 3) for k in PHASES}, round(med(steps), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", default="100,50")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    host = importlib.import_module("f2-nerf_amd").load_host()
    hr = make_renderer(host, dev)
    pose = torch.tensor([[1.0, 0.0, 0.0, 0.05], [0.0, 1.0, 0.0, -0.03], [0.0, 0.0, 1.0, 0.02]],
                        device=dev)
    Kc = torch.tensor([[0.9 * W, 0.0, 0.5 * W], [0.0, 0.9 * H, 0.5 * H], [0.0, 0.0, 1.0]], device=dev)
    loc = host.Localizer(host.LocalizerParam(), hr, Kc, H, W, torch.zeros(3, device=dev), 1.0)
    with torch.no_grad():
        image = loc.render_image(pose).contiguous()  # what the camera would see from the true pose
    sigmas = loc.noise_sigmas(1.0)
    lines = []
    for P in (int(v) for v in args.particles.split(",")):
        arms = {
            "A": lambda c, P=P: arm_a(host, loc, pose, image, P, c),
            "B": lambda c, P=P: arm_b(host, hr, Kc, sigmas, pose, image, P, c),
        }
        for arm, fn in arms.items():
            phases, step = measure(fn, args.reps, args.warmup)
            non_render = round(sum(v for k, v in phases.items() if k != "render"), 3)
            lines.append(json.dumps({
                "arm": arm, "particles": P, "pixels": K_PIX, "samples_per_ray": S,
                "kept_samples": int(hr.last_n_samples), "phase_ms": phases,
                "non_render_ms": non_render, "step_ms": step, "reps": args.reps}))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
