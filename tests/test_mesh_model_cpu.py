"""tests/mesh_model.py held to properties it is not built from: a consistent, closed, outward-wound
surface on random data, a sphere and planes; every mutant of the model fails one of them.  The
tetrahedra, the inside rule and the lattice geometry are restated here independently."""
import itertools
from fractions import Fraction

import numpy as np
import pytest

from tests import mesh_model as M

PERMS = list(itertools.permutations(range(3)))      # lexicographic: xyz xzy yxz yzx zxy zyx


def _random(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _ties(shape, seed):
    """values in {-1, 0}: at level 0 nothing is inside"""
    return -(np.random.default_rng(seed).random(shape) < 0.7).astype(np.float32)


def _directed(tri):
    return np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]).astype(np.int64)


def _faces_of(m, shape):
    """[V, 6] bool: the mesh vertex's lattice edge lies in boundary face (axis, side)"""
    nz, ny, nx = shape
    dims = (nx, ny, nz)
    o = m["owner"]
    coord = [o % nx, o // nx % ny, o // (nx * ny)]
    out = np.zeros((o.shape[0], 6), dtype=bool)
    for a in range(3):
        still = (m["d"] >> a & 1) == 0
        out[:, 2 * a] = still & (coord[a] == 0)
        out[:, 2 * a + 1] = still & (coord[a] == dims[a] - 1)
    return out


def edge_consistency(m, shape):
    """-> (every directed edge once, unpaired edges not inside one boundary face)"""
    V = max(m["vertices"].shape[0], 1)
    e = _directed(m["triangles"])
    key = e[:, 0] * V + e[:, 1]
    once = np.unique(key).shape[0] == key.shape[0]
    lone = ~np.isin(e[:, 1] * V + e[:, 0], key)
    faces = _faces_of(m, shape)
    excused = (faces[e[:, 0]] & faces[e[:, 1]]).any(1)
    return once, int((lone & ~excused).sum())


def _positions(shape, lo, step):
    nz, ny, nx = shape
    return [M.axis_positions(n, l, h).astype(np.float64) for n, l, h in zip((nx, ny, nz), lo, step)]


def winding_violations(values, level, m, lo, step):
    """triangles whose normal does not point from its tetrahedron's inside corners (value > level,
    decided here) to its outside ones, triangles in a tetrahedron that is not mixed, and the difference
    between the number of triangles and what the mixed tetrahedra ask for"""
    nz, ny, nx = values.shape
    pos = _positions(values.shape, lo, step)
    with np.errstate(invalid="ignore"):
        inside = values > np.float32(level)
    want = 0
    for z, y, x in itertools.product(range(nz - 1), range(ny - 1), range(nx - 1)):
        for a, b, _ in PERMS:
            path = [(0, 0, 0), tuple(int(i == a) for i in range(3)), tuple(int(i in (a, b)) for i in range(3)),
                    (1, 1, 1)]
            k = sum(bool(inside[z + c[2], y + c[1], x + c[0]]) for c in path)
            want += (0, 1, 2, 1, 0)[k]
    bad = 0
    v = m["vertices"]
    for tri, cell, k in zip(m["triangles"], m["tri_cell"], m["tri_tet"]):
        x, y, z = int(cell % nx), int(cell // nx % ny), int(cell // (nx * ny))
        a, b, _ = PERMS[int(k)]
        path = [(0, 0, 0), tuple(int(i == a) for i in range(3)), tuple(int(i in (a, b)) for i in range(3)), (1, 1, 1)]
        pts = np.array([[pos[0][x + c[0]], pos[1][y + c[1]], pos[2][z + c[2]]] for c in path])
        ins = np.array([bool(inside[z + c[2], y + c[1], x + c[0]]) for c in path])
        if ins.all() or not ins.any():
            bad += 1
            continue
        n = np.cross(v[tri[1]] - v[tri[0]], v[tri[2]] - v[tri[0]])
        if not n @ (pts[~ins].mean(0) - pts[ins].mean(0)) > 0:
            bad += 1
    return bad, m["triangles"].shape[0] - want


LO, STEP = (-1.0, -0.5, 0.25), (0.25, 0.125, 0.5)


@pytest.mark.parametrize("shape,seed", [((6, 7, 8), 1), ((9, 9, 9), 2)], ids=["8x7x6", "9x9x9"])
def test_random_field_is_consistent(shape, seed):
    """1: every directed edge once, its reverse present unless both ends lie in one boundary face, seven
    edge directions in use"""
    values = _random(shape, seed)
    m = M.marching_tets(values, 0.0, LO, STEP)
    print("\n%s: %d vertices, %d triangles" % (shape, m["vertices"].shape[0], m["triangles"].shape[0]))
    once, lone = edge_consistency(m, shape)
    assert once and lone == 0
    assert set(m["d"].tolist()) == set(range(1, 8))
    assert m["triangles"].min() >= 0 and m["triangles"].max() == m["vertices"].shape[0] - 1
    assert np.unique(m["triangles"]).shape[0] == m["vertices"].shape[0]      # no vertex without a triangle
    # the stated orders
    assert (np.diff(m["owner"] * 8 + m["d"]) > 0).all()
    assert (np.diff(m["tri_cell"] * 6 + m["tri_tet"]) >= 0).all()


def _sphere():
    n, lo, step = 21, (-1.0,) * 3, (0.1,) * 3
    p = _positions((n, n, n), lo, step)
    r = np.sqrt(p[2][:, None, None] ** 2 + p[1][None, :, None] ** 2 + p[0][None, None, :] ** 2)
    return (0.7 - r).astype(np.float32), lo, step


def sphere_violations(m, shape, step):
    v, tri = m["vertices"], m["triangles"]
    once, lone = edge_consistency(m, shape)
    lone_any = int((~np.isin(_directed(tri)[:, ::-1] @ [v.shape[0], 1], _directed(tri) @ [v.shape[0], 1])).sum())
    euler = v.shape[0] - 3 * tri.shape[0] // 2 + tri.shape[0]
    vol = np.einsum("ij,ij->i", v[tri[:, 0]], np.cross(v[tri[:, 1]], v[tri[:, 2]])).sum() / 6.0
    off = np.abs(np.linalg.norm(v, axis=1) - 0.7).max()
    return dict(once=once, lone=lone + lone_any, euler=euler, volume=vol, off=off)


def test_sphere_is_closed_and_outward():
    """2: closed, V - E + F = 2, positive volume, every vertex within sqrt(3) step of the sphere"""
    values, lo, step = _sphere()
    m = M.marching_tets(values, 0.0, lo, step)
    r = sphere_violations(m, values.shape, step)
    print("\nsphere: %d vertices, %d triangles, volume %.4f (4/3 pi r^3 = %.4f)" % (
        m["vertices"].shape[0], m["triangles"].shape[0], r["volume"], 4.0 / 3.0 * np.pi * 0.7 ** 3))
    assert r["once"] and r["lone"] == 0 and r["euler"] == 2
    assert 0.9 * 4.0 / 3.0 * np.pi * 0.7 ** 3 < r["volume"] < 4.0 / 3.0 * np.pi * 0.7 ** 3
    assert r["off"] <= np.sqrt(3.0) * 0.1


def _plane(normal, c, shape=(9, 10, 11), lo=(-0.5, -0.4, -0.3), step=(0.1, 0.09, 0.08)):
    p = _positions(shape, lo, step)
    s = normal[0] * p[0][None, None, :] + normal[1] * p[1][None, :, None] + normal[2] * p[2][:, None, None] - c
    return s.astype(np.float32), lo, step


def plane_violations(m, values, normal, c, lo, step):
    """-> (vertices off the plane by more than the bound, share of area not facing -n, total area)"""
    nz, ny, nx = values.shape
    v, tri = m["vertices"], m["triangles"]
    far = m["owner"] + (m["d"] & 1) + (m["d"] >> 1 & 1) * nx + (m["d"] >> 2 & 1) * nx * ny
    sa, sb = values.ravel()[m["owner"]].astype(np.float64), values.ravel()[far].astype(np.float64)
    # the interpolant of values rounded once to float32 crosses zero where the plane's own function is
    # at most u (|s_a| + |s_b|); the vertex itself is within E of that point
    tol = M.U * (np.abs(sa) + np.abs(sb)) + M.BAR * (m["E"] * np.abs(normal)).sum(1) + 1e-13
    off = int((np.abs(v @ normal - c) > tol).sum())
    n = np.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]])
    area = np.linalg.norm(n, axis=1)
    unit = -np.asarray(normal) / np.linalg.norm(normal)
    sliver = area < 1e-5 * min(step) ** 2
    facing = (n[~sliver] @ unit) >= (1.0 - 1e-6) * area[~sliver]
    wrong = (area[~sliver][~facing].sum() + area[sliver].sum()) / area.sum()
    return off, wrong, area.sum() / 2.0


@pytest.mark.parametrize("normal,c", [((1.0, 0.0, 0.0), 0.03), ((0.0, 0.0, -1.0), 0.011), ((0.3, -0.5, 0.81), 0.07)],
                         ids=["x", "-z", "oblique"])
def test_planes(normal, c):
    """3: vertices on the plane, normals along -n, and the axis-aligned area"""
    values, lo, step = _plane(normal, c)
    m = M.marching_tets(values, 0.0, lo, step)
    assert m["triangles"].shape[0] > 0
    off, wrong, area = plane_violations(m, values, np.asarray(normal), c, lo, step)
    assert off == 0 and wrong < 1e-9
    nz, ny, nx = values.shape
    ext = [(n - 1) * h for n, h in zip((nx, ny, nz), step)]
    if normal[0] == 1.0:
        assert abs(area - ext[1] * ext[2]) < 1e-6 * area
    if normal[2] == -1.0:
        assert abs(area - ext[0] * ext[1]) < 1e-6 * area
    once, lone = edge_consistency(m, values.shape)
    assert once and lone == 0


def test_winding():
    """4: normals point from the inside corners to the outside ones; nothing where nothing is inside"""
    values = _random((5, 6, 7), 3)
    m = M.marching_tets(values, 0.0, LO, STEP)
    assert winding_violations(values, 0.0, m, LO, STEP) == (0, 0)
    ties = _ties((4, 5, 6), 4)
    assert winding_violations(ties, 0.0, M.marching_tets(ties, 0.0, LO, STEP), LO, STEP) == (0, 0)


@pytest.mark.parametrize("mut", M.MUTANTS)
def test_mutants_fail(mut):
    """5: each mutant breaks one of the checks above"""
    failed = []
    values = _random((6, 7, 8), 1)
    m = M.marching_tets(values, 0.0, LO, STEP, mut=mut)
    once, lone = edge_consistency(m, values.shape)
    if not once or lone:
        failed.append("edges")
    sphere, lo, step = _sphere()
    r = sphere_violations(M.marching_tets(sphere, 0.0, lo, step, mut=mut), sphere.shape, step)
    if not r["once"] or r["lone"] or r["euler"] != 2:
        failed.append("sphere")
    small = _random((5, 6, 7), 3)
    if winding_violations(small, 0.0, M.marching_tets(small, 0.0, LO, STEP, mut=mut), LO, STEP) != (0, 0):
        failed.append("winding")
    ties = _ties((4, 5, 6), 4)
    if winding_violations(ties, 0.0, M.marching_tets(ties, 0.0, LO, STEP, mut=mut), LO, STEP) != (0, 0):
        failed.append("winding at ties")
    print("\n%s fails: %s" % (mut, ", ".join(failed)))
    assert failed


def test_non_finite_values():
    """6: a NaN vertex is outside, its edges carry their vertex at t = 0.5, nothing else changes; +inf is
    inside, -inf outside"""
    base = _random((5, 6, 7), 5)
    at = (2, 3, 3)
    for bad, stand_in in ((np.nan, -1e30), (-np.inf, -1e30), (np.inf, 1e30)):
        values, plain = base.copy(), base.copy()
        values[at], plain[at] = bad, stand_in
        m, p = M.marching_tets(values, 0.0, LO, STEP), M.marching_tets(plain, 0.0, LO, STEP)
        assert np.array_equal(m["triangles"], p["triangles"]) and np.array_equal(m["mask"], p["mask"])
        nz, ny, nx = values.shape
        here = (at[0] * ny + at[1]) * nx + at[2]
        far = m["owner"] + (m["d"] & 1) + (m["d"] >> 1 & 1) * nx + (m["d"] >> 2 & 1) * nx * ny
        touched = (m["owner"] == here) | (far == here)
        assert touched.any()
        assert np.array_equal(m["vertices"][~touched], p["vertices"][~touched])
        assert np.isfinite(m["vertices"]).all() and np.isfinite(m["E"]).all()
        if bad != bad:
            assert m["snapped"][touched].all() and not m["snapped"][~touched].any()
            assert (m["t32"][touched] == 0.5).all()
            pos = _positions(values.shape, LO, STEP)
            o, f = m["owner"][touched], far[touched]
            for a, n_a in enumerate((1, nx, nx * ny)):
                dim = (nx, ny, nz)[a]
                mid = 0.5 * (pos[a][o // n_a % dim] + pos[a][f // n_a % dim])
                assert (np.abs(m["vertices"][touched][:, a] - mid) <= M.BAR * m["E"][touched][:, a]).all()


def test_constant_field_is_empty():
    """7"""
    for value, level in ((1.5, 1.5), (1.5, 0.0), (-2.0, 0.0)):
        m = M.marching_tets(np.full((4, 5, 6), value, dtype=np.float32), level, LO, STEP)
        assert m["vertices"].shape == (0, 3) and m["triangles"].shape == (0, 3) and not m["mask"].any()


def test_case_words_hold_the_table():
    """the packing mesh.hip carries, unpacked again"""
    for code, w in enumerate(M.case_words()):
        tris = M.case_triangles(code)
        assert w >> 18 == len(tris) == (0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0)[code]
        for j, tri in enumerate(tris):
            assert tuple(w >> (9 * j + 3 * c) & 7 for c in range(3)) == tri


def test_fmaf32_is_correctly_rounded():
    rng = np.random.default_rng(7)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32) * np.float32(1e-3)
    c = rng.standard_normal(4000).astype(np.float32)
    # sums that land on a float32 tie once the product's low bits are dropped
    a[:4] = np.float32(1.0 + 2.0 ** -23)
    b[:4] = np.float32(2.0 ** -24) * np.array([1, -1, 1, -1], dtype=np.float32) * a[:4]
    c[:4] = np.array([1.0, 1.0, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -23], dtype=np.float32)
    got = M.fmaf32(a, b, c)
    for i in range(a.shape[0]):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo_, hi_ = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        err = abs(exact - Fraction(float(got[i])))
        for other in (lo_, hi_):
            e2 = abs(exact - Fraction(float(other)))
            assert err < e2 or (err == e2 and not (int(got[i].view(np.int32)) & 1)), i
