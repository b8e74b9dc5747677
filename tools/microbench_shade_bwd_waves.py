"""shade_bwd alone at several sizes per launch, one-wave (SHADE_BWD_WAVES=1) against two-wave (=2) form,
C = 32, one image id: where the size threshold F2N_SHADE_BWD_TWO_WAVES_MIN_SAMPLES comes from"""
import importlib, os, sys
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
for n in (1 << 17, 229376, 1 << 19, 1 << 20, 3 << 19, 1 << 21, 1 << 22, 65536 * 128):
    g = torch.Generator(device=dev).manual_seed(0)
    enc = torch.randn(C, n, device=dev, generator=g) * 0.1
    dirs = torch.randn(n, 3, device=dev, generator=g); dirs /= dirs.norm(dim=1, keepdim=True)
    img = torch.full((n,), 7, device=dev, dtype=torch.int32)
    P = [torch.randn(16, C, device=dev) * .3, torch.randn(16, device=dev) * .1, torch.randn(64, 32, device=dev) * .3,
         torch.randn(64, device=dev) * .1, torch.randn(3, 64, device=dev) * .3, torch.randn(3, device=dev) * .1]
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
