"""marching_tets (f2n_mesh_count, f2n_mesh_emit) against tests/mesh_model.py -- the same triangles, the
same number of vertices, positions within BAR E of the float64 ones and equal where E = 0 -- and
extract_mesh against the pieces it is made of, bit for bit.  The fields are those of
tests/test_mesh_model_cpu.py, whose checks hold the model itself."""
import math

import numpy as np
import pytest
import torch

from tests import mesh_model as M
from tests import test_mesh_model_cpu as C
from tests.ray_grad_model import ratio
from tests.test_mesh_ply_cpu import read_ply

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def _fields():
    out = {"random_8x7x6": (C._random((6, 7, 8), 1), 0.0, C.LO, C.STEP),
           "random_9x9x9": (C._random((9, 9, 9), 2), 0.0, C.LO, C.STEP),
           "random_5x6x7": (C._random((7, 6, 5), 6), 0.25, C.LO, C.STEP),
           "ties": (C._ties((4, 5, 6), 4), 0.0, C.LO, C.STEP),
           "ties_above": (-C._ties((4, 5, 6), 4), 0.0, C.LO, C.STEP),
           "constant": (np.full((4, 5, 6), 1.5, dtype=np.float32), 1.5, C.LO, C.STEP),
           "2x2x2": (C._random((2, 2, 2), 8), 0.0, C.LO, C.STEP)}
    sphere, lo, step = C._sphere()
    out["sphere"] = (sphere, 0.0, lo, step)
    for tag, n, c in (("x", (1.0, 0.0, 0.0), 0.03), ("-z", (0.0, 0.0, -1.0), 0.011), ("oblique", (0.3, -0.5, 0.81), 0.07)):
        values, lo, step = C._plane(n, c)
        out["plane_" + tag] = (values, 0.0, lo, step)
    base = C._random((5, 6, 7), 5)
    for tag, bad in (("nan", np.nan), ("-inf", -np.inf), ("+inf", np.inf)):
        values = base.copy()
        values[2, 3, 3] = bad
        values[0, 0, 0] = bad          # a lattice corner as well
        out["random_" + tag] = (values, 0.0, C.LO, C.STEP)
    return out


FIELDS = _fields()


@pytest.mark.parametrize("name", list(FIELDS))
def test_marching_tets_is_the_model(pkg, dev, name):
    H = pkg.load_host()
    values, level, lo, step = FIELDS[name]
    m = M.marching_tets(values, level, lo, step)
    v_dev = torch.from_numpy(values).to(dev)
    vertices, triangles = H.marching_tets(v_dev, level, lo, step)
    assert vertices.dtype == torch.float32 and triangles.dtype == torch.int32
    assert tuple(vertices.shape) == m["vertices"].shape and tuple(triangles.shape) == m["triangles"].shape
    assert np.array_equal(triangles.cpu().numpy(), m["triangles"])
    r = ratio(vertices, m["vertices"], m["E"])
    worst = float(r.max()) if r.size else 0.0
    print("\n%s: %d vertices, %d triangles, largest |err| / E %.3f" % (
        name, vertices.shape[0], triangles.shape[0], worst))
    assert worst <= M.BAR
    again = H.marching_tets(v_dev, level, lo, step)
    assert torch.equal(vertices, again[0]) and torch.equal(triangles, again[1])
    if name == "constant":
        assert vertices.shape[0] == 0 and triangles.shape[0] == 0


def test_emit_skips_what_the_totals_do_not_hold(pkg, capi, dev):
    """totals smaller than the counts: the stores beyond them are skipped, nothing past the arrays"""
    values, level, lo, step = FIELDS["random_5x6x7"]
    nz, ny, nx = values.shape
    n = values.size
    v = torch.from_numpy(values).to(dev)
    mask, vc, tc = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(3))
    capi.call("mesh_count", v, mask, vc, tc, nx, ny, nz, level)
    m = M.marching_tets(values, level, lo, step)
    assert np.array_equal(mask.cpu().numpy(), m["mask"])
    V, T = int(vc.sum()), int(tc.sum())
    assert (V, T) == (m["vertices"].shape[0], m["triangles"].shape[0])
    voff = torch.cumsum(vc, 0, dtype=torch.int64) - vc
    toff = torch.cumsum(tc, 0, dtype=torch.int64) - tc
    vertices = torch.full((V, 3), SENTINEL, device=dev)
    triangles = torch.full((T, 3), -7, dtype=torch.int32, device=dev)
    capi.call("mesh_emit", v, mask, voff, toff, vertices, triangles, V // 2, T // 3, *lo, *step, level, nx, ny, nz)
    torch.cuda.synchronize()
    assert bool((vertices[V // 2:] == SENTINEL).all()) and bool((triangles[T // 3:] == -7).all())
    assert not bool((vertices[:V // 2] == SENTINEL).any()) and np.array_equal(
        triangles[:T // 3].cpu().numpy(), m["triangles"][:T // 3])
    # offsets that point nowhere: skipped as well
    capi.call("mesh_emit", v, mask, voff - (1 << 40), toff + (1 << 40), vertices, triangles, V, T, *lo, *step, level,
              nx, ny, nz)
    torch.cuda.synchronize()
    assert bool((vertices[V // 2:] == SENTINEL).all()) and bool((triangles[T // 3:] == -7).all())


def _renderer(H, dev, L, F, log2_T):
    H.manual_seed(5)
    r = H.Renderer(1, n_levels=L, n_channels=F, log2_table=log2_T, max_samples=32, step=4.0 / 32)
    p = r.named_parameters()
    g = torch.Generator().manual_seed(L + F)
    with torch.no_grad():
        fp = p["scene_field.feat_pool"]
        fp.copy_((torch.randn(fp.shape, generator=g) * 0.1).to(dev))
        p["scene_field.mlp.bias"][0] = 4.0
    return r


@pytest.mark.parametrize("L,F,log2_T", [(16, 2, 19), (8, 4, 12)], ids=["ref", "f4"])
def test_extract_mesh_is_its_pieces(pkg, dev, tmp_path, L, F, log2_T):
    H = pkg.load_host()
    r = _renderer(H, dev, L, F, log2_T)
    fld = r.scene_field
    g = torch.Generator().manual_seed(2)
    o = (torch.randn(64, 3, generator=g) * 0.2).to(dev)
    d = torch.randn(64, 3, generator=g).to(dev)
    before = r.render_rays(o, d, None, "validate")

    dims, lo, hi = (12, 10, 9), (-1.2, -1.0, -0.9), (1.3, 1.1, 1.0)
    step = tuple(float((np.float32(h) - np.float32(l)) / np.float32(n - 1)) for l, h, n in zip(lo, hi, dims))
    logit = H.density_lattice(fld, lo, step, dims)
    sigma = float(torch.exp(logit - H.DENSITY_SHIFT).flatten().median())          # a float32 value
    level = float(np.float32(math.log(sigma)) + np.float32(H.DENSITY_SHIFT))
    vertices, triangles, normals = H.extract_mesh(r, lo, hi, dims, sigma, True)
    assert vertices.shape[0] > 0 and triangles.shape[0] > 0
    pv, pt = H.marching_tets(logit, level, lo, step)
    assert torch.equal(vertices, pv) and torch.equal(triangles, pt)
    assert int(triangles.min()) >= 0 and int(triangles.max()) == vertices.shape[0] - 1
    plain = H.extract_mesh(r, lo, hi, dims, sigma)
    assert plain[2] is None and torch.equal(plain[0], vertices) and torch.equal(plain[1], triangles)

    grad = fld.density_grad(vertices)
    length = (grad * grad).sum(1, keepdim=True).sqrt()
    want = torch.where(length > 0, -grad / length, torch.zeros_like(grad))
    assert torch.equal(normals, want)
    assert bool(((normals.norm(dim=1) - 1).abs() < 1e-5).all())

    path = str(tmp_path / "scene.ply")
    H.save_ply(path, vertices, triangles, normals)
    rows, tri, _ = read_ply(path)
    assert np.array_equal(rows.view(np.int32), torch.cat([vertices, normals], 1).cpu().numpy().view(np.int32))
    assert np.array_equal(tri, triangles.cpu().numpy())

    after = r.render_rays(o, d, None, "validate")
    for a, b in zip(before, after):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)
    with pytest.raises(RuntimeError, match="positive"):
        H.extract_mesh(r, lo, hi, dims, 0.0)
