#!/usr/bin/env python3
"""What a mesh of the density costs: the logits of a 256^3 lattice over [-2, 2]^3 on the bench's
synthetic field (L = 16, F = 2, T = 2^19), and marching tetrahedra on them.

  --part lattice   (a) f2n_density_lattice: a wavefront is a 4 x 4 x 4 brick of vertices
                   (b) the same arithmetic with a wavefront as 64 consecutive x
                       (tools/probes/density_lattice_rows.hip, built here on first use)
                   (c) what the library could do before: the points from ATen, f2n_contract_fwd,
                       f2n_hash_fwd (channel-major [C, n]) and the chain as an ATen product.  (c) is not
                       the same number bit for bit: one matrix product instead of the fmaf chain, and
                       positions from addcmul, which is no fmaf.
                   Checked before they are timed: (a) == (b) as bits; (c) on the kernels' positions with
                   its encoding summed in float64 within 1e-4.
  --part mesh      f2n_mesh_count, the two int64 scans with the host read of their totals, and
                   f2n_mesh_emit on (a)'s logits, at the level that puts about 1 % of the cells on the
                   surface (found by bisection over the level, reported), and marching_tets as a whole.

Method: median of --reps (5) after 2 warm-ups, the arms alternating call by call, device events around
each call.  Prints one JSON line per measurement (also appended to --out).
"""
import argparse
import ctypes
import importlib
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import microbench_occupancy as scene  # noqa: E402  (the timers)
from microbench_normals import L, F, LOG2_T, fog_renderer  # noqa: E402  (the bench's synthetic field)

N, LO, HI = 256, -2.0, 2.0
PROBE_SRC = os.path.join(ROOT, "tools", "probes", "density_lattice_rows.hip")
PROBE_LIB = os.path.join(ROOT, "tools", "probes", "libdensity_lattice_rows.so")


def rows_probe():
    """the row-mapped kernel as a ctypes function with f2n_density_lattice's signature"""
    build = importlib.import_module("f2-nerf_amd._build")
    if not os.path.exists(PROBE_LIB) or os.path.getmtime(PROBE_LIB) < os.path.getmtime(PROBE_SRC):
        subprocess.run([build.HIPCC, *build.HIP_FLAGS, "-shared", "-I", build.INCLUDE_DIR, "-I", build.KERNEL_DIR,
                        "-o", PROBE_LIB, PROBE_SRC], check=True)
    fn = ctypes.CDLL(PROBE_LIB).f2n_density_lattice_rows
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_float] * 6 + [ctypes.c_int] * 5 + [ctypes.c_uint32, ctypes.c_int64,
                                                                                      ctypes.c_void_p]
    return fn


def field_args(hr):
    f = hr.scene_field
    w0, b0 = f.density_head()
    return (f.table_f16(), f.prim_pool, f.bias_pool.detach(), f.level_mul), w0, b0, (L, F, f.local_size, f.level_stride)


def part_lattice(host, capi, dev, args):
    hr = fog_renderer(host, dev, 128, 4.0 / 128)
    fa, w0, b0, shape = field_args(hr)
    n = N ** 3
    step = (HI - LO) / (N - 1)
    box = (LO, LO, LO, step, step, step, N, N, N)
    out_a, out_b = torch.empty(N, N, N, device=dev), torch.empty(N, N, N, device=dev)
    rows = rows_probe()

    def brick():
        capi.call("density_lattice", *fa, w0, b0, out_a, *box, *shape)

    def row():
        st = rows(*[t.data_ptr() for t in (*fa, w0, b0, out_b)], *box, *shape, capi.current_stream())
        assert st == 0, st

    axis = torch.arange(N, device=dev, dtype=torch.float32)
    enc = torch.empty(L * F, n, device=dev)
    out_c = [None]

    def op_by_op(c=None):
        if c is None:
            c = torch.addcmul(torch.tensor(LO, device=dev), axis, torch.tensor(step, device=dev))
        z, y, x = torch.meshgrid(c, c, c, indexing="ij")
        pts = torch.stack([x, y, z], -1).reshape(n, 3)
        xc = torch.empty_like(pts)
        capi.call("contract_fwd", pts, xc, n)
        capi.call("hash_fwd", xc, *fa, enc, 1, n, None, n, *shape)
        out_c[0] = torch.addmv(b0.expand(n), enc.t(), w0)

    # Checked before timing: (a) == (b) as bits; (c) on the kernels' own positions (the fmaf, formed in
    # float64 here) with its encoding summed in float64 agrees to rounding.  As timed, (c) takes its
    # positions from addcmul, which is no fmaf: 158 of the 256 coordinates differ by an ulp, and the
    # encoding of a few points in 10^4 moves by up to 0.2 with them -- reported, not asserted.
    step32 = torch.tensor(step, device=dev).double()
    brick(), row(), op_by_op((axis.double() * step32 + LO).float())
    torch.cuda.synchronize()
    assert torch.equal(out_a.view(torch.int32), out_b.view(torch.int32)), "the two mappings disagree"
    exact = (enc.t()[: 1 << 22].double() @ w0.double() + b0.double()).float()
    diff64 = float((exact - out_a.flatten()[: 1 << 22]).abs().nan_to_num(0.0).max())
    assert diff64 < 1e-4, diff64
    op_by_op()
    diff = float((out_c[0].reshape(N, N, N) - out_a).abs().nan_to_num(0.0).max())
    ts = scene.alternating({"brick": brick, "rows": row, "op_by_op": op_by_op}, args.reps)
    rec = {"part": "lattice", "lattice": [N, N, N], "box": [LO, HI], "L": L, "F": F, "log2_T": LOG2_T,
           "reps": args.reps, "op_by_op_max_abs_diff": diff,
           "op_by_op_on_fmaf_positions_f64_sum_max_abs_diff": diff64}
    for k, v in ts.items():
        rec[k + "_ms"] = scene.med(v)
        rec[k + "_min_max_ms"] = [round(v[0], 4), round(v[-1], 4)]
    rec["gvertices_per_s_brick"] = round(n / scene.med(ts["brick"]) * 1e-6, 3)
    rec["rows_over_brick"] = round(scene.med(ts["rows"]) / scene.med(ts["brick"]), 3)
    rec["op_by_op_over_brick"] = round(scene.med(ts["op_by_op"]) / scene.med(ts["brick"]), 3)
    scene.emit(rec, args.out)


def part_mesh(host, capi, dev, args):
    hr = fog_renderer(host, dev, 128, 4.0 / 128)
    step = (HI - LO) / (N - 1)
    lo3, step3 = (LO,) * 3, (step,) * 3
    logit = host.density_lattice(hr.scene_field, lo3, step3, (N, N, N))
    n = N ** 3
    mask, vc, tc = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(3))

    def count(level):
        capi.call("mesh_count", logit, mask, vc, tc, N, N, N, level)

    def share(level):
        count(level)
        return float((tc > 0).sum()) / (N - 1) ** 3

    lo_q, hi_q = 0.5, 1.0            # quantiles of the logits: the surface shrinks as the level rises
    flat = logit.flatten()[:: 64].float().nan_to_num(0.0).sort().values
    for _ in range(24):
        q = 0.5 * (lo_q + hi_q)
        level = float(flat[min(int(q * flat.numel()), flat.numel() - 1)])
        if share(level) > 0.01:
            lo_q = q
        else:
            hi_q = q
    on_surface = share(level)
    state = {}

    def scans():
        vi, ti = torch.cumsum(vc, 0, dtype=torch.int64), torch.cumsum(tc, 0, dtype=torch.int64)
        totals = torch.stack([vi[-1], ti[-1]]).cpu()
        state.update(voff=vi - vc, toff=ti - tc, V=int(totals[0]), T=int(totals[1]))

    def emit():
        capi.call("mesh_emit", logit, mask, state["voff"], state["toff"], state["vertices"], state["triangles"],
                  state["V"], state["T"], *lo3, *step3, level, N, N, N)

    count(level), scans()
    state["vertices"] = torch.empty(state["V"], 3, device=dev)
    state["triangles"] = torch.empty(state["T"], 3, dtype=torch.int32, device=dev)
    emit()
    whole = host.marching_tets(logit, level, lo3, step3)
    assert torch.equal(whole[0], state["vertices"]) and torch.equal(whole[1], state["triangles"])
    ts = scene.alternating({"count": lambda: count(level), "scans_and_read": scans, "emit": emit,
                            "marching_tets": lambda: host.marching_tets(logit, level, lo3, step3)}, args.reps)
    rec = {"part": "mesh", "lattice": [N, N, N], "level": round(level, 4), "cells_on_surface": round(on_surface, 5),
           "vertices": state["V"], "triangles": state["T"], "reps": args.reps}
    for k, v in ts.items():
        rec[k + "_ms"] = scene.med(v)
        rec[k + "_min_max_ms"] = [round(v[0], 4), round(v[-1], 4)]
    scene.emit(rec, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="lattice", choices=["lattice", "mesh"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_microbench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pkg = importlib.import_module("f2-nerf_amd")
    host = pkg.load_host()
    if args.part == "lattice":
        part_lattice(host, pkg.capi, dev, args)
    else:
        part_mesh(host, pkg.capi, dev, args)


if __name__ == "__main__":
    main()
