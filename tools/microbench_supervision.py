#!/usr/bin/env python3
"""What masked training costs: the mask pack, the masked pixel draw and the supervised step.

  --part pack   f2n_mask_pack (PixelMask.from_mask) on 200 images of 1920 x 1080 (415 M pixels, 52 MB
                of bits), half of the pixels valid.
  --part draw   f2n_draw_pixels_masked at valid fractions 1.0, 0.9, 0.5 and 0.1 (random pixels of a
                64-image 540 x 960 set) for 4096 and 65 536 rays, A = 32, against the three
                torch.randint calls of sample_random_rays for the same batch; the fraction of rays
                whose attempts all missed is in the record.
  --part step   One train_step of the reference's batch (workload C4: 512 rays, 1024 samples of 1/256)
                without supervision and with it (ray weights with a tenth of the rays masked, alpha
                targets, opacity weight 0.1), the arms alternating.

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


def part_pack(host, dev, args):
    E, h, w = 200, 1080, 1920
    g = torch.Generator(device=dev).manual_seed(5)
    mask = torch.randint(0, 2, (E, h, w), device=dev, generator=g, dtype=torch.uint8)
    keep = {}

    def run():
        keep["pm"] = host.PixelMask.from_mask(mask)

    ts = alternating({"pack": run}, args.reps, args.warmup)
    n = E * h * w
    emit({"part": "pack", "E": E, "h": h, "w": w, "pixels": n, "bits_MB": round(n / 8 / 1e6, 1),
          "valid": int(keep["pm"].count), "mask_pack_ms": med(ts["pack"]),
          "mask_pack_min_ms": round(ts["pack"][0], 4),
          "mask_pack_GBs": round((n + n / 8) / (med(ts["pack"]) * 1e-3) / 1e9, 1)}, args.out)


def part_draw(host, dev, args):
    E, h, w = 64, 540, 960
    g = torch.Generator(device=dev).manual_seed(7)
    u = torch.rand(E, h, w, device=dev, generator=g)
    iopt = dict(dtype=torch.int32, device=dev)
    for n in (4096, 65536):

        def randints():
            torch.randint(E, (n,), **iopt)
            torch.randint(0, h, (n,), **iopt)
            torch.randint(0, w, (n,), **iopt)

        for frac in (1.0, 0.9, 0.5, 0.1):
            pm = host.PixelMask.from_mask((u < frac).to(torch.uint8))
            seed = [0]

            def draw():
                seed[0] += 1
                return host.draw_pixels_masked(pm, n, seed[0], 32)

            ts = alternating({"draw": draw, "randint": randints}, args.reps, args.warmup)
            tries = host.draw_pixels_masked(pm, n, 12345, 32)[2]
            emit({"part": "draw", "n_rays": n, "valid_fraction": frac, "attempts": 32,
                  "valid_measured": round(int(pm.count) / (E * h * w), 4),
                  "missed_fraction": round(float((tries == 0).float().mean()), 5),
                  "mean_tries": round(float(tries[tries > 0].float().mean()), 3),
                  "draw_ms": med(ts["draw"]), "draw_min_ms": round(ts["draw"][0], 4),
                  "three_randint_ms": med(ts["randint"]),
                  "three_randint_min_ms": round(ts["randint"][0], 4)}, args.out)


def part_step(host, dev, args):
    n_rays, S, step = 512, 1024, 1.0 / 256
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
    sup = host.RaySupervision(ray_weight=m, alpha=alpha, opacity_weight=0.1)
    weights_only = host.RaySupervision(ray_weight=m)

    def off():
        hr.zero_grad()
        hr.train_step(o, d, emb, gt, 1e-2, None, bg)

    def on(s):
        def run():
            hr.zero_grad()
            hr.train_step_supervised(o, d, emb, gt, s, 1e-2, None, bg)
        return run

    ts = alternating({"off": off, "weights": on(weights_only), "on": on(sup)}, args.reps,
                     args.warmup + 1)
    emit({"part": "step", "shape": "c4_batch", "n_rays": n_rays, "samples_per_ray": S,
          "kept_samples": int(hr.last_n_samples), "var_loss_weight": 1e-2, "masked_rays": int((m == 0).sum()),
          "train_step_ms_no_supervision": med(ts["off"]),
          "train_step_ms_ray_weights": med(ts["weights"]),
          "train_step_ms_weights_alpha_opacity": med(ts["on"]),
          "train_step_min_ms_no_supervision": round(ts["off"][0], 4),
          "train_step_min_ms_ray_weights": round(ts["weights"][0], 4),
          "train_step_min_ms_weights_alpha_opacity": round(ts["on"][0], 4)}, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="draw", choices=["pack", "draw", "step"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    host = importlib.import_module("f2-nerf_amd").load_host()
    {"pack": part_pack, "draw": part_draw, "step": part_step}[args.part](host, dev, args)


if __name__ == "__main__":
    main()
