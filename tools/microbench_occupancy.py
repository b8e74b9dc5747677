#!/usr/bin/env python3
"""What an occupancy grid (OccupancyGrid, Renderer.set_occupancy) buys, measured two ways.

  --part mechanism   The fog-like "trained" table of the other microbenches (randn * 0.1, density bias
                     5: rays terminate after ~320 samples, but there is no empty space in it) with
                     HAND-SET grids: a ball around the origin occupying about 50 %, 10 % and 2 % of the
                     unit ball's cells, and all ones (the price of attaching a grid before its first
                     update).  Per grid: kept samples per ray, f2n_density_march against
                     f2n_density_march_occ, the whole VALIDATE render at the localiser's shape (65 536
                     rays x 1024 samples of 1/256, cameras outside the ball looking in) and one
                     train_step at the C4 shape (512 x 1024), each against the same call without a
                     grid, alternating.

  --part train       The whole feature on a field this tool trains itself: an analytic scene (a few
                     shaded spheres in front of a constant background, ground truth by ray-sphere
                     intersection on the device), random rays from a ring of cameras, train_step +
                     FusedAdam at the C4 shape, OccupancyGrid.update every --update-every iterations
                     with the default threshold and decay (jittered probes), the grid attached from
                     the first update on.  One run with the grid and one without from the same seed.
                     Reports the occupied fraction over time, kept samples per ray and iteration time
                     with and without the grid at the end, PSNR on held-out views for both runs, and
                     the PSNR of the grid render against the gridless render of the final field.

Prints one JSON line per measurement (also appended to --out).
"""
import argparse
import importlib
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, STEP, L, F, LOG2_T = 1024, 1.0 / 256, 16, 2, 19


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def timed(fn, reps):
    """ms of each of `reps` calls (device events around the call)."""
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def alternating(fns, reps, warmup=2):
    """{name: sorted ms}: the calls interleaved, so drift of the box hits all of them alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k] += timed(fn, 1)
    return {k: sorted(v) for k, v in ts.items()}


def med(v):
    return round(v[len(v) // 2], 4)


def fog_renderer(host, dev, n_images=1):
    torch.manual_seed(7)
    hr = host.Renderer(n_images, n_levels=L, n_channels=F, log2_table=LOG2_T, max_samples=S, step=STEP)
    p = hr.named_parameters()
    g = torch.Generator(device=dev).manual_seed(7)
    with torch.no_grad():
        fp = p["scene_field.feat_pool"]
        fp.copy_(torch.randn(fp.shape, device=dev, generator=g) * 0.1)
        p["scene_field.mlp.bias"][0] = 5.0
    return hr


def ball_bits(G, radius, dev):
    c = (torch.arange(G, dtype=torch.float32, device=dev) + 0.5) * (4.0 / G) - 2.0
    cz, cy, cx = torch.meshgrid(c, c, c, indexing="ij")
    return (cx * cx + cy * cy + cz * cz) < radius * radius


def inward_rays(n, dev, seed, cam_radius=1.5, spread=0.5):
    """Cameras on a sphere outside the unit ball, looking at points scattered around the origin."""
    g = torch.Generator(device=dev).manual_seed(seed)
    o = torch.randn(n, 3, device=dev, generator=g)
    o = o / o.norm(dim=1, keepdim=True) * cam_radius
    target = (torch.rand(n, 3, device=dev, generator=g) * 2 - 1) * spread
    return o.contiguous(), (target - o).contiguous()


def part_mechanism(host, capi, dev, args):
    hr = fog_renderer(host, dev, n_images=4)
    hr.set_dense_first_pass(-1)
    fld = hr.scene_field
    p = hr.named_parameters()
    w0 = p["scene_field.mlp.weight"].detach()[0].contiguous()
    b0 = p["scene_field.mlp.bias"].detach()[0:1].contiguous()
    table16 = fld.table_f16()
    G = args.resolution
    n_view, n_train = 65536, 512
    o, d = inward_rays(n_view, dev, 1)
    to, td = inward_rays(n_train, dev, 2)
    g = torch.Generator(device=dev).manual_seed(3)
    noise = torch.rand(n_train, S, device=dev, generator=g) + 0.5
    bg = torch.rand(n_train, 3, device=dev, generator=g)
    gt = torch.rand(n_train, 3, device=dev, generator=g)
    emb = torch.randint(0, 4, (n_train,), device=dev, generator=g).to(torch.int32)
    unit_cells = float(ball_bits(G, 1.0, dev).sum())

    kept = torch.empty(n_view, dtype=torch.int32, device=dev)
    length = torch.empty(n_view, dtype=torch.int32, device=dev)
    common = (fld.prim_pool, fld.bias_pool, fld.level_mul, w0, b0)
    tail = (n_view, S, STEP, L, F, fld.local_size, fld.level_stride, 1e-4, 3.0)

    def march():
        capi.call("density_march", o, d, None, table16, *common, kept, *tail)

    def march_one_ray():  # the one-ray-per-wavefront form the _occ kernel starts from
        with capi.option("MARCH", 1):
            capi.call("density_march", o, d, None, table16, *common, kept, *tail)

    def render(grid):
        def run():
            hr.set_occupancy(grid)
            with torch.no_grad():
                hr.render(o, d, None, "validate")
        return run

    def train(grid):
        def run():
            hr.set_occupancy(grid)
            hr.zero_grad()
            hr.train_step(to, td, emb, gt, 1e-2, noise, bg, True)
        return run

    grids = [("ones", None)] + [("ball_%g" % f, f ** (1.0 / 3.0)) for f in (0.5, 0.1, 0.02)]
    for name, radius in grids:
        grid = host.OccupancyGrid(G, str(dev))
        if radius is not None:
            grid.set_bits(ball_bits(G, radius, dev))
        words = grid.words

        def march_occ():
            capi.call("density_march_occ", o, d, None, table16, *common, words, G, kept, length, *tail)

        t = alternating({"march8": march, "march1": march_one_ray, "march_occ": march_occ}, args.reps)
        march()
        kept_plain = float(kept.sum()) / n_view
        march_occ()
        rec = {"part": "mechanism", "grid": name, "resolution": G,
               "occupied_of_unit_ball": round(float(grid.bits().sum()) / unit_cells, 4),
               "kept_per_ray_no_grid": round(kept_plain, 2),
               "kept_per_ray_grid": round(float(kept.sum()) / n_view, 2),
               "len_per_ray_grid": round(float(length.sum()) / n_view, 2),
               "march8_ms": med(t["march8"]), "march1_ms": med(t["march1"]),
               "march_occ_ms": med(t["march_occ"])}
        t = alternating({"off": render(None), "on": render(grid)}, args.reps)
        rec.update(render_ms_no_grid=med(t["off"]), render_ms_grid=med(t["on"]),
                   render_min_no_grid=round(t["off"][0], 4), render_min_grid=round(t["on"][0], 4))
        t = alternating({"off": train(None), "on": train(grid)}, args.reps)
        hr.set_occupancy(None)
        train(None)()
        n_off = int(hr.last_n_samples)
        train(grid)()
        n_on = int(hr.last_n_samples)
        hr.set_occupancy(None)
        rec.update(train_step_ms_no_grid=med(t["off"]), train_step_ms_grid=med(t["on"]),
                   train_kept_per_ray_no_grid=round(n_off / n_train, 2),
                   train_kept_per_ray_grid=round(n_on / n_train, 2))
        emit(rec, args.out)


# ---- the self-trained field ----------------------------------------------------------------------

SPHERES = (  # centre, radius, colour
    ((0.00, 0.00, 0.00), 0.22, (0.9, 0.2, 0.2)),
    ((0.35, 0.10, -0.10), 0.14, (0.2, 0.8, 0.3)),
    ((-0.30, -0.05, 0.20), 0.16, (0.2, 0.3, 0.9)),
    ((0.05, 0.32, 0.25), 0.10, (0.9, 0.8, 0.2)),
)
BACKGROUND = (0.55, 0.6, 0.7)
LIGHT = (0.4, 0.7, 0.6)


def analytic_colors(o, d):
    """Nearest ray-sphere hit, Lambert-shaded; the constant background elsewhere.  o, d [n,3]."""
    dn = d / d.norm(dim=1, keepdim=True)
    best_t = torch.full((o.shape[0],), float("inf"), device=o.device)
    color = torch.tensor(BACKGROUND, device=o.device).expand(o.shape[0], 3).clone()
    light = torch.tensor(LIGHT, device=o.device)
    light = light / light.norm()
    for centre, radius, rgb in SPHERES:
        c = torch.tensor(centre, device=o.device)
        oc = o - c
        b = (oc * dn).sum(1)
        disc = b * b - ((oc * oc).sum(1) - radius * radius)
        t = -b - disc.clamp_min(0).sqrt()
        hit = (disc > 0) & (t > 0) & (t < best_t)
        n = (oc + dn * t.unsqueeze(1)) / radius
        shade = 0.35 + 0.65 * (n * light).sum(1).clamp_min(0)
        color = torch.where(hit.unsqueeze(1), torch.tensor(rgb, device=o.device) * shade.unsqueeze(1), color)
        best_t = torch.where(hit, t, best_t)
    return color


def look_at(position, target=(0.0, 0.0, 0.0)):
    p = torch.tensor(position)
    f = torch.tensor(target) - p
    f = f / f.norm()
    s = torch.linalg.cross(f, torch.tensor((0.0, 0.0, 1.0)))
    s = s / s.norm()
    u = torch.linalg.cross(s, f)
    return torch.cat([torch.stack([s, u, -f], 1), p.unsqueeze(1)], 1)  # [3,4]: the camera looks down -z


def ring_poses(n, radius, height, phase=0.0):
    return torch.stack([look_at((radius * math.cos(a), radius * math.sin(a), height))
                        for a in [phase + 2 * math.pi * i / n for i in range(n)]])


def psnr(a, b):
    mse = float((a - b).square().mean())
    return 10.0 * math.log10(1.0 / max(mse, 1e-12))


def train_once(host, dev, args, use_grid, out_records):
    hw = args.image
    n_cams = 24
    poses = ring_poses(n_cams, 0.9, 0.25).to(dev)
    held = ring_poses(4, 0.9, 0.1, phase=0.13).to(dev)
    Kc = torch.tensor([[0.8 * hw, 0.0, 0.5 * hw], [0.0, 0.8 * hw, 0.5 * hw], [0.0, 0.0, 1.0]], device=dev)
    intr = Kc.unsqueeze(0).expand(n_cams, 3, 3).contiguous()
    images = []
    for i in range(n_cams):
        o, d = host.get_view_rays(poses[i], Kc, hw, hw)
        images.append(analytic_colors(o, d).reshape(hw, hw, 3))
    images = torch.stack(images).contiguous()
    host.manual_seed(11)
    torch.manual_seed(11)
    hr = host.Renderer(n_cams, n_levels=L, n_channels=F, log2_table=LOG2_T, max_samples=S, step=STEP)
    hr.set_dense_first_pass(-1)
    opt = hr.make_fused_adam(args.lr)
    grid = host.OccupancyGrid(args.resolution, str(dev)) if use_grid else None
    G = args.resolution
    gen = torch.Generator(device=dev).manual_seed(5)
    bg_gt = torch.tensor(BACKGROUND, device=dev)
    for it in range(1, args.iters + 1):
        o, d, gt, cam = host.sample_random_rays(poses, intr, hw, hw, 512, images)
        opt.zero_grad()
        # the scene's background is a constant: it is the render's background colour too
        hr.train_step(o, d, cam, gt, 0.0, None, bg_gt.expand(512, 3).contiguous(), True)
        opt.step()
        if use_grid and it >= args.first_update and (it - args.first_update) % args.update_every == 0:
            probe = torch.rand(G, G, G, 3, device=dev, generator=gen).clamp_max(1.0 - 2.0 ** -24)
            grid.update(hr.scene_field, args.threshold, args.decay, probe)
            # a young field sits below any fixed threshold everywhere, and a sample that is skipped
            # gets no gradient: until the grid's mean density passes the threshold, the mean is the
            # threshold (instant-ngp's rule).  Same probe, decay 1: the densities stay as they are.
            mean = float(grid.density().mean())
            if mean < args.threshold:
                grid.update(hr.scene_field, mean, 1.0, probe)
            hr.set_occupancy(grid)
            if ((it - args.first_update) // args.update_every) % args.report_every == 0:
                out_records.append({"part": "train", "event": "update", "iteration": it,
                                    "occupied_fraction": round(grid.fraction(), 5),
                                    "kept_per_ray": round(hr.last_n_samples / 512, 2)})
    # ---- the end state
    o, d, gt, cam = host.sample_random_rays(poses, intr, hw, hw, 512, images)
    bg = bg_gt.expand(512, 3).contiguous()

    def step(g):
        def run():
            hr.set_occupancy(g)
            hr.zero_grad()
            hr.train_step(o, d, cam, gt, 0.0, None, bg, True)
        return run

    final_grid = grid
    if final_grid is None:  # the gridless run: build a grid from its final field for the end figures
        final_grid = host.OccupancyGrid(G, str(dev))
        for _ in range(8):
            probe = torch.rand(G, G, G, 3, device=dev, generator=gen).clamp_max(1.0 - 2.0 ** -24)
            final_grid.update(hr.scene_field, args.threshold, args.decay, probe)
    t = alternating({"off": step(None), "on": step(final_grid)}, args.reps)
    step(None)()
    kept_off = hr.last_n_samples / 512
    step(final_grid)()
    kept_on = hr.last_n_samples / 512
    views = {}
    for name, g in (("off", None), ("on", final_grid)):
        hr.set_occupancy(g)
        with torch.no_grad():
            views[name] = torch.stack([
                hr.render_all_rays(*host.get_view_rays(held[i], Kc, hw, hw), 16384)[0].clip(0, 1)
                for i in range(held.shape[0])])
    truth = torch.stack([analytic_colors(*host.get_view_rays(held[i], Kc, hw, hw)) for i in range(held.shape[0])])
    hr.set_occupancy(None)
    return {"part": "train", "event": "final", "trained_with_grid": use_grid, "iterations": args.iters,
            "threshold": args.threshold, "decay": args.decay, "resolution": G,
            "occupied_fraction": round(final_grid.fraction(), 5),
            "kept_per_ray_no_grid": round(kept_off, 2), "kept_per_ray_grid": round(kept_on, 2),
            "train_step_ms_no_grid": med(t["off"]), "train_step_ms_grid": med(t["on"]),
            "psnr_heldout_no_grid_render": round(psnr(views["off"], truth), 3),
            "psnr_heldout_grid_render": round(psnr(views["on"], truth), 3),
            "psnr_grid_vs_gridless_render": round(psnr(views["on"], views["off"]), 3)}


def part_train(host, dev, args):
    for use_grid in (True, False):
        records = []
        final = train_once(host, dev, args, use_grid, records)
        for r in records:
            emit(r, args.out)
        emit(final, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="mechanism", choices=["mechanism", "train"])
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--image", type=int, default=128)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--first-update", type=int, default=256)
    ap.add_argument("--update-every", type=int, default=16)
    ap.add_argument("--report-every", type=int, default=16)
    ap.add_argument("--threshold", type=float, default=None)
    ap.add_argument("--decay", type=float, default=None)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pkg = importlib.import_module("f2-nerf_amd")
    host = pkg.load_host()
    if args.threshold is None:
        args.threshold = host.OccupancyGrid.DEFAULT_THRESHOLD
    if args.decay is None:
        args.decay = host.OccupancyGrid.DEFAULT_DECAY
    if args.part == "mechanism":
        part_mechanism(host, pkg.capi, dev, args)
    else:
        part_train(host, dev, args)


if __name__ == "__main__":
    main()
