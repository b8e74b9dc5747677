"""Marching tetrahedra on a scalar lattice, restated in NumPy: what f2n_mesh_count / f2n_mesh_emit
(mesh.hip) must produce, in the order they must produce it, with positions in float64 and a
per-element rounding bound.  No tests in here: tests/test_mesh_model_cpu.py checks the restatement by
properties it does not take from it, tests/test_gpu_mesh.py holds the kernels to it.  Also fmaf32, a
correctly rounded float32 fused multiply-add, for the lattice positions here and the logit chain of
tests/test_gpu_density_lattice.py.

Lattice.  values [nz, ny, nx] float32, x fastest; vertex (x, y, z) has lattice index (z ny + y) nx + x and
position p = fmaf((float)i, step, lo) per axis.  A vertex is inside iff value > level; NaN is outside.

Edges.  Direction d = dx + 2 dy + 4 dz in 1..7.  Vertex a owns the edges a -> a + d whose far end lies in
the lattice.  An owned edge whose ends differ in `inside` carries one mesh vertex (bit d - 1 of the
owner's mask): t = (level - s_a) / (s_b - s_a) in float32, t = 0.5 if !(t >= 0 && t <= 1),
p = fmaf(t, p_b - p_a, p_a) per axis.  Mesh vertices are ordered by (owner lattice index, d).

Tetrahedra (Kuhn).  Cell v = the vertex at its low corner, cells in lattice-index order.  Tetrahedron k
of a cell runs v, v + c1, v + c2, v + 7 with corners written as direction bits:
    k   axes order   c1  c2   orientation det[c1 - 0, c2 - 0, 7 - 0]
    0   x y z        1   3    +
    1   x z y        1   5    -
    2   y x z        2   3    -
    3   y z x        2   6    +
    4   z x y        4   5    +
    5   z y x        4   6    -
Local corners 0..3 in that order, local edges 0..5 = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); edge (i, j) is
owned by corner i and has d = c_j - c_i.

Triangles, for a positively oriented tetrahedron; a negative one swaps the 2nd and 3rd vertex of each.
    one inside corner p    q < r < s the others, r and s swapped if (p, q, r, s) is an odd permutation:
                           (pq, pr, ps)
    one outside corner p   the same q, r, s: (pq, ps, pr)
    two inside P < Q       R < S the others, swapped if (P, Q, R, S) is odd: the quad PR PS QS QR, split
                           along PR - QS: (PR, PS, QS) then (PR, QS, QR)
so (b - a) x (c - a) points from the inside corners to the outside ones and the first vertex of a
triangle is the one named first above.  Triangles are ordered by (cell, tetrahedron, triangle).

Bound.  u = 2^-24, the helpers of tests/ray_grad_model.py (one rounding u |result| per float32 operation,
errors propagated through the absolute-value form): level - s_a, s_b - s_a, their quotient, p_b - p_a
and the fmaf -- one subtraction, one division, one subtraction, one fmaf on the path of the longest
term.  Where the edge does not move along an axis p_b - p_a is 0 and fmaf(t, 0, p_a) = p_a: E = 0 there.
Where an end (or the float32 s_b - s_a) is not finite t is 0.5 or a signed zero exactly and only the
last two operations round.  Bar: |got - f64| <= BAR E, BAR = 2, equal where E = 0.  Nothing here was
measured on a kernel.

Mutants (`mut`): 'flip' tetrahedron 3 wound the other way, 'repeat' tetrahedron 5 takes the axes order
of tetrahedron 4, 'split' the quad cut as PR PS QR QS, 'ge' inside iff value >= level.
"""
import itertools

import numpy as np

from tests.ray_grad_model import BAR, U, _div, _fma, _sub, _v  # noqa: F401

TET_C1 = (1, 1, 2, 2, 4, 4)
TET_C2 = (3, 5, 3, 6, 5, 6)
TET_SIGN = (1, -1, -1, 1, 1, -1)
LOCAL_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
MUTANTS = ("flip", "repeat", "split", "ge")
_POP = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def fmaf32(a, b, c):
    """fmaf(a, b, c) of float32 values, correctly rounded.  The product of two float32 is exact in
    float64; the sum is rounded to odd there (TwoSum gives the side the exact value lies on), and a
    53-bit round-to-odd value rounds to 24 bits as the exact one does."""
    a, b, c = (np.atleast_1d(np.asarray(v, dtype=np.float32)).astype(np.float64) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        move = (err != 0) & even & np.isfinite(s) & np.isfinite(err)
        s = np.where(move, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def axis_positions(n, lo, step):
    """float32 [n]: fmaf((float)i, step, lo)"""
    return fmaf32(np.arange(n, dtype=np.float32), np.float32(step), np.float32(lo))


def _parity(perm):
    return sum(1 for i, j in itertools.combinations(range(4), 2) if perm[i] > perm[j]) & 1


def case_triangles(code, split="PRQS"):
    """triangles of a positively oriented tetrahedron whose local corner i is inside iff bit i of code:
    a list of triples of local edge ids"""
    edge = {e: i for i, e in enumerate(LOCAL_EDGES)}

    def E(i, j):
        return edge[(min(i, j), max(i, j))]

    ins = [i for i in range(4) if code >> i & 1]
    out = [i for i in range(4) if not code >> i & 1]
    if len(ins) in (1, 3):
        p = ins[0] if len(ins) == 1 else out[0]
        q, r, s = [i for i in range(4) if i != p]
        if _parity((p, q, r, s)):
            r, s = s, r
        return [(E(p, q), E(p, r), E(p, s))] if len(ins) == 1 else [(E(p, q), E(p, s), E(p, r))]
    if len(ins) == 2:
        (P, Q), (R, S) = ins, out
        if _parity((P, Q, R, S)):
            R, S = S, R
        pr, ps, qs, qr = E(P, R), E(P, S), E(Q, S), E(Q, R)
        if split == "PRQS":
            return [(pr, ps, qs), (pr, qs, qr)]
        return [(pr, ps, qr), (pr, qr, qs)]      # the crossed quad PR PS QR QS
    return []


def case_words():
    """the 16 cases as mesh.hip packs them: 3 bits per local edge, triangle 0 in bits 0-8, triangle 1 in
    bits 9-17, the number of triangles in bits 18-19"""
    words = []
    for code in range(16):
        w = 0
        tris = case_triangles(code)
        for j, tri in enumerate(tris):
            for c, e in enumerate(tri):
                w |= e << (9 * j + 3 * c)
        words.append(w | len(tris) << 18)
    return words


def _offsets(d):
    return d & 1, d >> 1 & 1, d >> 2 & 1


def marching_tets(values, level, lo, step, mut=None):
    """values [nz, ny, nx] float32, lo / step 3 floats (x, y, z) -> dict:
    vertices [V, 3] float64, E [V, 3], triangles [T, 3] int32, owner [V], d [V], t32 [V], snapped [V]
    (t replaced by 0.5), tri_cell [T], tri_tet [T], mask [N] uint8."""
    s = np.ascontiguousarray(values, dtype=np.float32)
    nz, ny, nx = s.shape
    N = nx * ny * nz
    level = np.float32(level)
    with np.errstate(invalid="ignore"):
        inside = (s >= level) if mut == "ge" else (s > level)
    lin = np.arange(N, dtype=np.int64).reshape(nz, ny, nx)

    # ---- mesh vertices ------------------------------------------------------------------------------------
    cross = np.zeros((N, 7), dtype=bool)
    for d in range(1, 8):
        dx, dy, dz = _offsets(d)
        a = inside[:nz - dz, :ny - dy, :nx - dx]
        b = inside[dz:, dy:, dx:]
        cross[lin[:nz - dz, :ny - dy, :nx - dx].ravel(), d - 1] = (a != b).ravel()
    mask = (cross * (1 << np.arange(7))).sum(1).astype(np.uint8)
    voff = np.cumsum(_POP[mask]) - _POP[mask]
    owner, dm1 = np.nonzero(cross)                 # row-major: by owner, then by d
    d_of = dm1 + 1
    V = owner.shape[0]
    pos = [axis_positions(n, l, h) for n, l, h in zip((nx, ny, nz), lo, step)]
    oc = [owner % nx, owner // nx % ny, owner // (nx * ny)]
    far = owner + (d_of & 1) + (d_of >> 1 & 1) * nx + (d_of >> 2 & 1) * nx * ny
    sa, sb = s.ravel()[owner], s.ravel()[far]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        den32 = sb - sa
        t32 = (level - sa) / den32
        snapped = ~((t32 >= 0) & (t32 <= 1))
        t32 = np.where(snapped, np.float32(0.5), t32)
        exact_t = snapped | ~np.isfinite(sa) | ~np.isfinite(sb) | ~np.isfinite(den32)
        fin_a, fin_b = np.where(exact_t, 0.0, sa), np.where(exact_t, 1.0, sb)
        t = _div(_sub(_v(np.full(V, float(level))), _v(fin_a)), _sub(_v(fin_b), _v(fin_a)))
        t = (np.where(exact_t, t32.astype(np.float64), t[0]), np.where(exact_t, 0.0, t[1]))
    vertices, E = np.zeros((V, 3)), np.zeros((V, 3))
    for a in range(3):
        moves = (d_of >> a & 1) == 1
        pa = pos[a][oc[a]].astype(np.float64)
        pb = pos[a][oc[a] + moves].astype(np.float64)
        v, e = _fma(t, _sub(_v(pb), _v(pa)), _v(pa))
        vertices[:, a] = np.where(moves, v, pa)
        E[:, a] = np.where(moves, e, 0.0)

    # ---- triangles ----------------------------------------------------------------------------------------
    c1, c2, sign = list(TET_C1), list(TET_C2), list(TET_SIGN)
    if mut == "flip":
        sign[3] = -sign[3]
    if mut == "repeat":
        c1[5], c2[5], sign[5] = c1[4], c2[4], sign[4]
    table = [case_triangles(code, "PRQR" if mut == "split" else "PRQS") for code in range(16)]
    cells = lin[:nz - 1, :ny - 1, :nx - 1].ravel()
    flat_in = inside.ravel()
    stride = lambda c: (c & 1) + (c >> 1 & 1) * nx + (c >> 2 & 1) * nx * ny  # noqa: E731
    rows = []
    for k in range(6):
        corners = (0, c1[k], c2[k], 7)
        code = sum(flat_in[cells + stride(c)].astype(np.int64) << i for i, c in enumerate(corners))
        for cs in range(1, 15):
            sel = cells[code == cs]
            if not sel.size:
                continue
            for j, tri in enumerate(table[cs]):
                if sign[k] < 0:
                    tri = (tri[0], tri[2], tri[1])
                idx = []
                for e in tri:
                    i0, i1 = LOCAL_EDGES[e]
                    own = sel + stride(corners[i0])
                    dd = corners[i1] - corners[i0]
                    idx.append(voff[own] + _POP[mask[own] & ((1 << (dd - 1)) - 1)])
                rows.append(np.stack([sel, np.full_like(sel, k), np.full_like(sel, j), *idx], 1))
    if rows:
        rows = np.concatenate(rows)
        rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    else:
        rows = np.zeros((0, 6), dtype=np.int64)
    return dict(vertices=vertices, E=E, triangles=rows[:, 3:].astype(np.int32), owner=owner, d=d_of,
                t32=t32, snapped=snapped, tri_cell=rows[:, 0], tri_tet=rows[:, 1], mask=mask,
                tets=(tuple(c1), tuple(c2), tuple(sign)))
