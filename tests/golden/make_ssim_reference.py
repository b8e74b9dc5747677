"""Records tests/golden/ssim/ssim_reference.npz: seeded image pairs and what the reference's own rgb_ssim
(scripts/eval.py:29-75 of the reference tree) returns for them, as mean and as map.

The function is taken out of the reference's file at run time with `ast` -- eval.py as a whole needs
lpips and cv2 -- and none of its text is kept here.  Run once, where the reference tree and scipy
are present:

    python -m tests.golden.make_ssim_reference            (F2N_REFERENCE names the tree)
"""
import ast
import os

import numpy as np

REF = os.environ.get("F2N_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ssim", "ssim_reference.npz")
SEED = 20221


def reference_rgb_ssim():
    import scipy.signal

    path = os.path.join(REF, "scripts", "eval.py")
    tree = ast.parse(open(path).read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "rgb_ssim"]
    assert len(fn) == 1
    space = {"np": np, "scipy": scipy}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), space)
    return space["rgb_ssim"]


def pairs():
    """name -> (pred, gt) float32 [h, w, 3]; the stackable cases share 26 x 43"""
    g = np.random.default_rng(SEED)
    out = {}
    for h, w in ((11, 11), (11, 12), (12, 11), (16, 16), (26, 43), (33, 70)):
        out["noise_%dx%d" % (h, w)] = (g.random((h, w, 3)), g.random((h, w, 3)))
    h, w = 26, 43
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ramp = np.stack([i / (h - 1.0), j / (w - 1.0), (i + j) / (h + w - 2.0)], axis=-1)
    out["ramp_noise"] = (ramp + 0.05 * g.standard_normal((h, w, 3)), ramp)
    out["black_self"] = (np.zeros((h, w, 3)), np.zeros((h, w, 3)))
    out["flat07_self"] = (np.full((h, w, 3), 0.7), np.full((h, w, 3), 0.7))
    out["flat02_flat08"] = (np.full((h, w, 3), 0.2), np.full((h, w, 3), 0.8))
    out["flat_noise"] = (np.full((h, w, 3), 0.5), g.random((h, w, 3)))
    out["ramp_negative"] = (ramp - 0.5, 0.5 - ramp)
    a = g.random((h, w, 3))
    b = np.clip(a + 0.03 * g.standard_normal((h, w, 3)), 0.0, 1.0)
    out["quantised"] = (np.round(a * 255.0) / 255.0, np.round(b * 255.0) / 255.0)
    return {k: (p.astype(np.float32), q.astype(np.float32)) for k, (p, q) in out.items()}


def main():
    rgb_ssim = reference_rgb_ssim()
    arrays = {}
    for name, (pred, gt) in pairs().items():
        p64, g64 = pred.astype(np.float64), gt.astype(np.float64)
        arrays[name + ".pred"] = pred
        arrays[name + ".gt"] = gt
        arrays[name + ".ssim"] = np.float64(rgb_ssim(p64, g64, 1.0))
        arrays[name + ".map"] = np.asarray(rgb_ssim(p64, g64, 1.0, return_map=True), dtype=np.float64)
        print("%-16s %s  ssim %.6f" % (name, pred.shape[:2], arrays[name + ".ssim"]))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
