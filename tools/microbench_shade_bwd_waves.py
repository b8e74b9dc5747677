"""shade_bwd alone at several sizes per launch, one-wave (SHADE_BWD_WAVES=1) against two-wave (=2) form,
C = 32, one image id: where the size threshold F2N_SHADE_BWD_TWO_WAVES_MIN_SAMPLES comes from

  --ray-const   instead: the ray-uniform entries that form the per-ray constant per stride
                (f2n_shade_fwd_raydirs / f2n_shade_bwd_raydirs) against the ones that load it
                (f2n_shade_ray_const once, then f2n_shade_fwd_rays_const / f2n_shade_bwd_rays_const) on
                one headline chunk's shape, 65 536 rays x 128 samples, C = 32, one image id; the arms
                alternate call by call, device events around each call, medians of --reps"""
import argparse, importlib, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
capi = importlib.import_module("f2-nerf_amd").capi
dev = torch.device("cuda:0")
C, E = 32, 50
def t(fn, reps=20):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps
def params():
    return [torch.randn(16, C, device=dev) * .3, torch.randn(16, device=dev) * .1, torch.randn(64, 32, device=dev) * .3,
            torch.randn(64, device=dev) * .1, torch.randn(3, 64, device=dev) * .3, torch.randn(3, device=dev) * .1]
def ray_const(n_rays, S, reps):
    n = n_rays * S
    g = torch.Generator(device=dev).manual_seed(0)
    enc = torch.randn(C, n, device=dev, generator=g) * 0.1
    rd = torch.randn(n_rays, 3, device=dev, generator=g); rd /= rd.norm(dim=1, keepdim=True)
    img = torch.full((n_rays,), 7, device=dev, dtype=torch.int32)
    P, emb = params(), torch.randn(E, 16, device=dev) * .1
    dl, dr = torch.randn(n, device=dev), torch.randn(n, 3, device=dev)
    out = {k: (torch.empty(n, device=dev), torch.empty(n, 3, device=dev), torch.empty(C, n, device=dev)) for k in "ab"}
    G = [torch.zeros_like(p) for p in P] + [torch.zeros_like(emb)]
    rc = torch.empty(n_rays, 80, device=dev)
    arms = {
        "fwd_forming": lambda: capi.call("shade_fwd_raydirs", enc, C, rd, img, *P, emb, *out["a"][:2], n_rays, S),
        "fwd_loading": lambda: capi.call("shade_fwd_rays_const", enc, C, rc, img, *P, emb, *out["b"][:2], n_rays, S),
        "ray_const": lambda: capi.call("shade_ray_const", rd, P[2], P[3], rc, n_rays),
        "bwd_forming": lambda: capi.call("shade_bwd_raydirs", enc, C, rd, img, *P, emb, dl, dr, out["a"][2], *G, n_rays, S),
        "bwd_loading": lambda: capi.call("shade_bwd_rays_const", enc, C, rd, rc, img, *P, emb, dl, dr, out["b"][2], *G, n_rays, S),
    }
    arms["ray_const"]()
    for fn in arms.values(): fn()
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(out["a"], out["b"]))
    ms = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    med = {k: round(sorted(v)[len(v) // 2], 4) for k, v in ms.items()}
    print(json.dumps({"bench": "shade_ray_const", "n_rays": n_rays, "S": S, "C": C, "reps": reps,
                      "outputs_equal": same, "median_ms": med}), flush=True)
ap = argparse.ArgumentParser()
ap.add_argument("--ray-const", action="store_true")
ap.add_argument("--reps", type=int, default=50)
args = ap.parse_args()
if args.ray_const:
    ray_const(65536, 128, args.reps)
    sys.exit(0)
for n in (1 << 17, 229376, 1 << 19, 1 << 20, 3 << 19, 1 << 21, 1 << 22, 65536 * 128):
    g = torch.Generator(device=dev).manual_seed(0)
    enc = torch.randn(C, n, device=dev, generator=g) * 0.1
    dirs = torch.randn(n, 3, device=dev, generator=g); dirs /= dirs.norm(dim=1, keepdim=True)
    img = torch.full((n,), 7, device=dev, dtype=torch.int32)
    P = params()
    emb = torch.randn(E, 16, device=dev) * .1
    dl, dr = torch.randn(n, device=dev), torch.randn(n, 3, device=dev)
    denc = torch.empty(C, n, device=dev)
    G = [torch.zeros_like(p) for p in P] + [torch.zeros_like(emb)]
    res = []
    for w in (1, 2, 1, 2):
        capi.set_option("SHADE_BWD_WAVES", w)
        res.append(t(lambda: capi.call("shade_bwd", enc, C, dirs, img, *P, emb, dl, dr, denc, *G, None, n)))
    capi.set_option("SHADE_BWD_WAVES", 0)
    print("n=%9d one-wave %.4f %.4f ms  two-wave %.4f %.4f ms" % (n, res[0], res[2], res[1], res[3]), flush=True)
