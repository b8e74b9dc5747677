"""Numpy model, in exact integers and float64, of error-guided ray sampling (error_map.hip:
f2n_mask_cell_counts, f2n_error_map_accum, f2n_error_map_apply, f2n_error_cdf,
f2n_draw_pixels_guided).  No tests in here: tests/test_error_map_model_cpu.py checks the model on the
CPU, tests/test_gpu_error_map.py holds the HIP kernels to it with array_equal.  Written from the
definitions in include/f2nerf_hip.h, not from the kernels.  Philox and the masked draw are those of
tests/supervision_model.py.

GEOMETRY.  Pixel (e, i, j) lies in cell c = (e*gh + (i*gh)//h)*gw + (j*gw)//w; cell row a covers pixel
rows ceil(a*h/gh) .. ceil((a+1)*h/gh) - 1, columns alike.

ACCUMULATE.  e = (d0^2 + d1^2) + d2^2 in float64 with d = C - (a*gt + (1 - a)*bg), q = rint(min(e, 4) *
2^20) (half to even); a ray with weight 0, a non-finite e or (cam, i, j) outside the set leaves no trace.

APPLY.  value = f32(decay*value + (1 - decay) * (sum / (2^20 * cnt))) where cnt > 0; accumulators zeroed.

CDF.  mass = quant(value) * counts, quant(v) = clamp(rint(v * 2^16), 1, 2^24), non-finite -> 1; cdf =
inclusive prefix sum in uint64.

DRAW.  T = rint(u * 2^32); block (x0..x3) = Philox(r, 0, 0, 0).  x3 < T or total == 0: the masked draw.
Else t = ((x0 << 32 | x1) * total) >> 64, cell = first c with cdf[c] > t, attempts with counter
(r, a, 1, 0) inside the cell.  weight = f32(1 / (((1 - u) * q) * N / total + u)), 0 where tries == 0.
"""
import numpy as np

from tests import supervision_model as sm

F32 = np.float32
Q_ERR = 2.0 ** 20
Q_VAL = 2.0 ** 16
Q_CAP = 1 << 24
SCAN_TILE = 2048                       # cells per scan workgroup of error_map.hip (256 lanes x 8)


class Grid:
    def __init__(self, E, h, w, gh, gw):
        assert 1 <= gh <= h and 1 <= gw <= w
        self.E, self.h, self.w, self.gh, self.gw = E, h, w, gh, gw
        self.n_cells = E * gh * gw

    def first(self, a, h, gh):
        """first pixel row of cell row a (a may be an array; a == gh gives h)"""
        return (np.asarray(a, dtype=np.int64) * h + gh - 1) // gh

    def cell_of(self, e, i, j):
        e, i, j = (np.asarray(x, dtype=np.int64) for x in (e, i, j))
        return (e * self.gh + (i * self.gh) // self.h) * self.gw + (j * self.gw) // self.w

    def cell_box(self, c):
        """-> e, i0, rows, j0, cols of cell(s) c"""
        c = np.asarray(c, dtype=np.int64)
        b, a, e = c % self.gw, (c // self.gw) % self.gh, c // (self.gw * self.gh)
        i0, j0 = self.first(a, self.h, self.gh), self.first(b, self.w, self.gw)
        return (e, i0, self.first(a + 1, self.h, self.gh) - i0, j0,
                self.first(b + 1, self.w, self.gw) - j0)

    def pixel_cells(self):
        """int64 [E, h, w]: the cell of every pixel"""
        e, i, j = np.meshgrid(np.arange(self.E), np.arange(self.h), np.arange(self.w), indexing="ij")
        return self.cell_of(e, i, j)


def cell_counts(grid, mask=None):
    """valid pixels per cell, int32 [n_cells]; mask uint8 / bool [E, h, w] or None (closed form)"""
    if mask is None:
        _, _, rows, _, cols = grid.cell_box(np.arange(grid.n_cells))
        return (rows * cols).astype(np.int32)
    valid = np.asarray(mask).reshape(-1) != 0
    cells = grid.pixel_cells().reshape(-1)
    return np.bincount(cells[valid], minlength=grid.n_cells).astype(np.int32)


def ray_errors(colors, gt, alpha=None, bg=None):
    """float64 [n]: e_r in the kernel's order"""
    C, g = np.asarray(colors, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    if alpha is not None:
        a = np.asarray(alpha, dtype=np.float64)[:, None]
        om = 1.0 - a
        g = a * g + om * np.asarray(bg, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = C - g
        d2 = d * d
        return (d2[:, 0] + d2[:, 1]) + d2[:, 2]


def accumulate(grid, acc_sum, acc_cnt, colors, gt, cam, ij, ray_weight=None, alpha=None, bg=None):
    """adds into acc_sum (uint64 [n_cells]) and acc_cnt (uint32 [n_cells]) in place"""
    err = ray_errors(colors, gt, alpha, bg)
    cam, ij = np.asarray(cam, dtype=np.int64), np.asarray(ij, dtype=np.int64)
    keep = np.isfinite(err)
    if ray_weight is not None:
        keep &= np.asarray(ray_weight) != 0
    keep &= (cam >= 0) & (cam < grid.E) & (ij[:, 0] >= 0) & (ij[:, 0] < grid.h)
    keep &= (ij[:, 1] >= 0) & (ij[:, 1] < grid.w)
    q = np.rint(np.minimum(err[keep], 4.0) * Q_ERR).astype(np.uint64)
    cells = grid.cell_of(cam[keep], ij[keep, 0], ij[keep, 1])
    np.add.at(acc_sum, cells, q)
    np.add.at(acc_cnt, cells, np.uint32(1))


def apply(value, acc_sum, acc_cnt, decay):
    """value float32 [n_cells] updated in place; the accumulators are zeroed"""
    hit = acc_cnt > 0
    d = np.float64(F32(decay))
    mean = acc_sum[hit].astype(np.float64) / (Q_ERR * acc_cnt[hit].astype(np.float64))
    value[hit] = (d * value[hit].astype(np.float64) + (1.0 - d) * mean).astype(F32)
    acc_sum[:] = 0
    acc_cnt[:] = 0


def quant(value):
    """uint64 [n]: clamp(rint(value * 2^16), 1, 2^24), non-finite -> 1"""
    v = np.asarray(value, dtype=F32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.where(np.isfinite(v), v * Q_VAL, 1.0)
    x = np.clip(x, 1.0, float(Q_CAP))
    return np.rint(x).astype(np.uint64)


def cdf(value, counts):
    mass = quant(value) * np.maximum(np.asarray(counts, dtype=np.int64), 0).astype(np.uint64)
    return np.cumsum(mass, dtype=np.uint64)


def threshold(u):
    """T of a float32 uniform_fraction"""
    return int(np.rint(np.float64(F32(u)) * 2.0 ** 32))


def weight_f64(u, q, n_valid, total):
    """the importance weight in float64, in the kernel's order"""
    uu = threshold(u) / 2.0 ** 32
    return 1.0 / ((((1.0 - uu) * np.asarray(q, dtype=np.float64)) * np.float64(n_valid)) /
                  np.float64(np.uint64(total)) + uu)


def draw(grid, mask, value, cdf_, n, seed, attempts, u):
    """-> cam [n] i32, ij [n, 2] i32, tries [n] i32, weight [n] f64 (0 where tries == 0), guided [n]
    bool (the branch each ray took).  mask uint8 / bool [E, h, w] or None."""
    E, h, w = grid.E, grid.h, grid.w
    valid = np.ones(E * h * w, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    n_valid = int(valid.sum())
    total = int(cdf_[-1])
    T = threshold(u)
    seed_lo, seed_hi = seed & sm.MASK32, (seed >> 32) & sm.MASK32
    r = np.arange(n, dtype=np.uint64)
    x0, x1, _, x3 = sm.philox4x32_10(r, 0, 0, 0, seed_lo, seed_hi)
    uniform = (x3 < np.uint64(T)) if total else np.ones(n, dtype=bool)
    # the uniform branch is the masked draw itself
    cam, ij, tries = (a.astype(np.int64) for a in sm.draw(valid.reshape(E, h, w), n, seed, attempts))
    g = np.flatnonzero(~uniform)
    if g.size:
        z = (x0[g].astype(object) << 32) | x1[g].astype(object)            # Python integers
        t = np.array([(int(v) * total) >> 64 for v in z], dtype=np.uint64)
        cell = np.searchsorted(cdf_, t, side="right")                      # first c with cdf[c] > t
        e, i0, rows, j0, cols = grid.cell_box(cell)
        cam[g], tries[g] = e, 0
        open_ = np.ones(g.size, dtype=bool)
        for a in range(attempts):
            if not open_.any():
                break
            y0, y1, _, _ = sm.philox4x32_10(r[g], a, 1, 0, seed_lo, seed_hi)
            i = i0 + (y0 * rows.astype(np.uint64) >> np.uint64(32)).astype(np.int64)
            j = j0 + (y1 * cols.astype(np.uint64) >> np.uint64(32)).astype(np.int64)
            go = g[open_]
            ij[go, 0], ij[go, 1] = i[open_], j[open_]
            hit = open_ & valid[(e * h + i) * w + j]
            tries[g[hit]] = a + 1
            open_ &= ~hit
    weight = np.zeros(n)
    kept = tries > 0
    if total:
        q = quant(value)[grid.cell_of(cam[kept], ij[kept, 0], ij[kept, 1])]
        weight[kept] = weight_f64(u, q, n_valid, total)
    else:
        weight[kept] = 1.0
    return cam.astype(np.int32), ij.astype(np.int32), tries.astype(np.int32), weight, ~uniform


def pixel_pdf(grid, mask, value, u):
    """float64 [E*h*w]: the probability that one draw with unlimited attempts lands on each pixel"""
    E, h, w = grid.E, grid.h, grid.w
    valid = np.ones(E * h * w, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    counts = cell_counts(grid, mask)
    total = float(cdf(value, counts)[-1])
    uu = threshold(u) / 2.0 ** 32
    q = quant(value)[grid.pixel_cells().reshape(-1)].astype(np.float64)
    return np.where(valid, (1.0 - uu) * q / total + uu / valid.sum(), 0.0)


def ulp_f32(x):
    """spacing of float32 at |x|"""
    return np.spacing(np.abs(np.asarray(x, dtype=F32))).astype(np.float64)
