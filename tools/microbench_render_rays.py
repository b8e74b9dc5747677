#!/usr/bin/env python3
"""A/B of the one-kernel inference render (RendererOptions::one_pass, f2n_render_rays) against the
default routes of the same build, on three shapes:

  a  the localiser step of tools/microbench_localizer.py: P = 100 particles x K = 256 pixels = 25 600
     rays, VALIDATE, S = 1024 at step 1/256, L = 16, F = 2, T = 2^19, trained-like field (head bias 5):
     the render alone (render_all_rays on the particles' rays) and the whole public step
  b  an 800 x 800 VALIDATE view (bench.py's first camera, focal 1111.1) at S = 128 in 65 536-ray
     chunks, thin medium (head bias 0: nothing terminates) -- the README's inference workload
  c  the same view in the terminating regime (head bias 8: about 3.5 kept samples per ray)

Each call alternates with its counterpart (off, on, off, on, ...); median of --reps after --warmup;
host wall clock around a synchronise.  This process never opens the GPU: every shape runs in a child
process under its own time limit, and a child that fails ends the run.  --profile adds one
`rocprofv3 --kernel-trace --stats` run of shape a in a fresh child.  One JSON line per shape and arm;
--out appends them to a file.

--head 0,64,-1 adds arms for RendererOptions::one_pass_head (0: the one-launch kernel again, 64: the
first 64 samples eight rays to a wavefront and the survivors one wavefront each, -1: whole rays eight to
a wavefront); all arms -- off, on, and these -- alternate call by call, and the lines are appended to
profiles/render_rays_head_ab.jsonl unless --out names another file.

--corner-order doubles every arm: once with the density chain's corner loads in vertex-parity order
(F2N_OPT_GATHER_PAIRED = 0, the default) and once in corner order (= 1, arms named "...+corner").

  python tools/microbench_render_rays.py [--shapes a,b,c] [--reps 5] [--warmup 2] [--out FILE]
                                         [--head 0,64,-1] [--corner-order] [--profile DIR]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHILD_TIMEOUT_S = 240


def _median(v):
    return sorted(v)[len(v) // 2]


HEADS = []   # --head: further arms "head=<n>" after "off" and "on"
CORNER = []  # --corner-order: every arm again as "<arm>+corner" with F2N_OPT_GATHER_PAIRED = 1


def _arms():
    arms = ["off", "on"] + ["head=%d" % h for h in HEADS]
    return arms + [a + "+corner" for a in arms] if CORNER else arms


def _ab(torch, hr, fn, reps, warmup):
    """{arm: [ms, ...]} with the arms alternating call by call"""
    capi = importlib.import_module("f2-nerf_amd").capi
    ms = {arm: [] for arm in _arms()}
    for it in range(warmup + reps):
        for arm_order in _arms():
            arm = arm_order.replace("+corner", "")
            capi.set_option("GATHER_PAIRED", int(arm_order.endswith("+corner")))
            hr.set_one_pass(arm != "off")
            hr.set_one_pass_head(int(arm[5:]) if arm.startswith("head=") else 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= warmup:
                ms[arm_order].append((time.perf_counter() - t0) * 1e3)
    capi.set_option("GATHER_PAIRED", 0)
    hr.set_one_pass(False)
    hr.set_one_pass_head(0)
    return ms


def _lines(shape, what, n_rays, S, ms, extra):
    out = []
    for arm in _arms():
        med = _median(ms[arm])
        out.append(json.dumps(dict(
            shape=shape, what=what, one_pass=arm, rays=n_rays, samples_per_ray=S,
            ms=round(med, 3), ms_all=[round(v, 3) for v in ms[arm]],
            mrays_per_s=round(n_rays / med / 1e3, 2), **extra)))
    return out


def run_shape(shape, reps, warmup):
    import torch

    host = importlib.import_module("f2-nerf_amd").load_host()
    dev = torch.device("cuda:0")
    lines = []
    with torch.no_grad():
        if shape == "a":
            mb = importlib.import_module("tools.microbench_localizer")
            P = 100
            hr = mb.make_renderer(host, dev)
            pose = torch.tensor([[1.0, 0.0, 0.0, 0.05], [0.0, 1.0, 0.0, -0.03], [0.0, 0.0, 1.0, 0.02]],
                                device=dev)
            Kc = torch.tensor([[0.9 * mb.W, 0.0, 0.5 * mb.W], [0.0, 0.9 * mb.H, 0.5 * mb.H],
                               [0.0, 0.0, 1.0]], device=dev)
            loc = host.Localizer(host.LocalizerParam(), hr, Kc, mb.H, mb.W, torch.zeros(3, device=dev), 1.0)
            image = loc.render_image(pose).contiguous()
            poses = host.perturb_poses(pose, torch.randn(P, 6, device=dev), loc.noise_sigmas(1.0))
            pix = torch.randperm(mb.H * mb.W, device=dev)[:mb.K_PIX]
            ij = torch.stack([pix // mb.W, pix % mb.W], 1).to(torch.int32)
            o, d = loc.pose_rays(poses, ij)
            n = o.shape[0]
            _, _, _, kept = hr.render_rays(o, d, None, "validate")
            extra = dict(kept_samples=int(kept.sum()))
            ms = _ab(torch, hr, lambda: hr.render_all_rays(o, d, 1 << 16), reps, warmup)
            lines += _lines("a", "render_all_rays of the particles' rays", n, mb.S, ms, extra)

            def step():
                particles = loc.optimize_pose_by_random_search(pose, image, P, 1.0)
                host.Localizer.calc_average_pose(particles)
            ms = _ab(torch, hr, step, reps, warmup)
            lines += _lines("a", "optimize_pose_by_random_search + calc_average_pose", n, mb.S, ms, extra)
        else:
            bench = importlib.import_module("bench")
            h = w = 800
            S = 128
            torch.manual_seed(7)
            hr = host.Renderer(1, n_levels=16, n_channels=2, log2_table=19, max_samples=S, step=4.0 / S)
            p = hr.named_parameters()
            g = torch.Generator(device=dev).manual_seed(7)
            fp = p["scene_field.feat_pool"]
            fp.copy_(torch.randn(fp.shape, device=dev, generator=g) * 0.1)   # trained-like table
            p["scene_field.mlp.bias"][0] = 0.0 if shape == "b" else 8.0
            pose = bench.fox_like_poses(50)[0].to(dev)
            Kc = torch.tensor([[1111.1, 0.0, w / 2], [0.0, 1111.1, h / 2], [0.0, 0.0, 1.0]], device=dev)
            o, d = host.get_view_rays(pose, Kc, h, w)
            kept = torch.cat([hr.render_rays(o[lo:lo + 65536], d[lo:lo + 65536], None, "validate")[3]
                              for lo in range(0, h * w, 65536)])
            extra = dict(kept_samples=int(kept.sum()), kept_per_ray=round(float(kept.float().mean()), 2))
            ms = _ab(torch, hr, lambda: hr.render_image(pose, Kc, h, w, 65536), reps, warmup)
            lines += _lines(shape, "render_image 800x800, 65536-ray chunks", h * w, S, ms, extra)
    for ln in lines:
        print(ln, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--shape", default="", help="(child) run this one shape in this process")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--head", default="", metavar="N,N,..",
                    help="further arms: one_pass with one_pass_head = N (0, -1 or a multiple of 64)")
    ap.add_argument("--corner-order", action="store_true",
                    help="every arm also with F2N_OPT_GATHER_PAIRED = 1 (the density chain in corner order)")
    ap.add_argument("--profile", default="", metavar="DIR",
                    help="also one rocprofv3 --kernel-trace --stats run of shape a into DIR")
    args = ap.parse_args()
    HEADS[:] = [int(v) for v in args.head.split(",") if v]
    CORNER[:] = [True] if args.corner_order else []
    if args.shape:
        run_shape(args.shape, args.reps, args.warmup)
        return 0
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--warmup", str(args.warmup)]
    if CORNER:
        me += ["--corner-order"]
    if HEADS:
        me += ["--head=" + args.head]
        if not args.out:
            args.out = os.path.join(ROOT, "profiles", "render_rays_head_ab.jsonl")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for shape in args.shapes.split(","):
        res = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), *me, "--shape", shape],
                             cwd=ROOT, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode != 0:  # a fault, an abort or a time limit: nothing more is started
            print("shape %s ended with status %d: stopping" % (shape, res.returncode), file=sys.stderr)
            return res.returncode
        if args.out:
            with open(args.out, "a") as f:
                f.write("".join(ln + "\n" for ln in res.stdout.splitlines() if ln.startswith("{")))
    if args.profile:
        os.makedirs(args.profile, exist_ok=True)
        res = subprocess.run(
            ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), "rocprofv3", "--kernel-trace", "--stats",
             "--output-format", "csv", "-d", args.profile, "--", sys.executable,
             os.path.abspath(__file__), "--shape", "a", "--reps", "3", "--warmup", "1"], cwd=ROOT)
        return res.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
