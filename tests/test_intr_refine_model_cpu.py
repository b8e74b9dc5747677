"""The formulas and bounds of tests/intr_refine_model.py, on the CPU: the float64 per-ray terms against
central differences of the float64 camera model (the arbiter of the formulas), TERM_TOL re-measured on
the float32 restatement, three mutants that must leave the bounds, the correction's backward against
differences of its forward, and the calibration recovered from rays alone.

Measured here: the largest |analytic - central difference| over the six sets, the four corners and the
centre pixel is 0.024 of its bound (test_terms_agree_with_central_differences prints it per set); the
float32 restatement's largest error / mag is 3.95e-7; the recovery's loss falls 1.8e4-fold with
|gamma0 - gamma0*| = 3.4e-3 and |gamma1 - gamma1*| = 3.2e-3."""
import numpy as np
import pytest

from tests import intr_refine_model as im
from tests import lens_model as lm
from tests import pose_refine_model as pm

# Central differences with steps of 2^-6 pixel (fx, fy, cx, cy) and 2^-14 (coefficients), moves that
# float32 holds exactly or nearly so (the move actually made is what divides).  The truncation is
# h^2 f''' / 6.  At the corners of the strongest sets r2 reaches 2, and each derivative in k2 brings a
# factor r2^2 / det of about ten, so f''' can be 1e3 times the term: with h = 6.1e-5 that is 6e-7 of
# it, and less for every other parameter (h / fx = 3.9e-4 for the four in pixels).  The float64
# Newton solution (30 steps) is converged to 1e-16, which the division by h raises to 2e-12.  1e-4 of
# mag stands a hundred times above the truncation and a hundred times below what a wrong formula
# moves (the mutants below).  (With steps of 2^-4 and 2^-10 the k2 column of set 0 reads 1.4e-4: the
# truncation, which these steps divide by 256.)  Beside it stands the rounding of the two losses that
# are subtracted, 16 float64 ulps of sum |d_d| |R v| over the step: at the centre pixel the k2 term is
# 1e-10 (r2^2 = 1e-9) and a difference cannot resolve it to 1e-4 of itself.
FD_RTOL = 1e-4
FD_ULPS = 16
FD_STEP = (2.0 ** -6,) * 4 + (2.0 ** -14,) * 4

CORNERS = np.array([[0, 0], [0, lm.W - 1], [lm.H - 1, 0], [lm.H - 1, lm.W - 1],
                    [int(round(lm.CY - 0.5)), int(round(lm.CX - 0.5))]], dtype=np.int32)


def _calibration(K32, k32, q, step):
    """(K, k) float32 with parameter q moved by `step`, and the move as float32 made it."""
    K, k = K32.copy(), k32.copy()
    cell = ((K, (0, 0)), (K, (1, 1)), (K, (0, 2)), (K, (1, 2)), (k, 0), (k, 1), (k, 2), (k, 3))[q]
    arr, at = cell
    before = float(arr[at])
    arr[at] = np.float32(before + step)
    return K, k, float(arr[at]) - before


def _fd_case(which):
    rng = np.random.default_rng(41 + which)
    n = CORNERS.shape[0]
    return dict(ij=CORNERS, K=lm.intrinsic(), k=np.asarray(im.SETS6[which], dtype=np.float32),
                R=lm.rotations(n, 43 + which), d_d=rng.standard_normal((n, 3)).astype(np.float32))


def _ray_loss(c, K, k):
    v = lm.camera_dirs(k, c["ij"], K, np.float64, steps=30)
    world = np.einsum("nab,nb->na", c["R"].astype(np.float64), v)
    return (world * c["d_d"].astype(np.float64)).sum(1)


def _fd_floor(c):
    v = lm.camera_dirs(c["k"], c["ij"], c["K"], np.float64, steps=30)
    world = np.einsum("nab,nb->na", c["R"].astype(np.float64), v)
    size = (np.abs(world) * np.abs(c["d_d"].astype(np.float64))).sum(1)
    return FD_ULPS * 2.0 ** -52 * size[:, None] / np.asarray(FD_STEP)[None, :]


def _fd_terms(c):
    fd = np.zeros((c["ij"].shape[0], 8))
    for q in range(8):
        Kp, kp, up = _calibration(c["K"], c["k"], q, FD_STEP[q])
        Km, km, dn = _calibration(c["K"], c["k"], q, -FD_STEP[q])
        fd[:, q] = (_ray_loss(c, Kp, kp) - _ray_loss(c, Km, km)) / (up - dn)
    return fd


def _analytic(c, **mutant):
    v = lm.camera_dirs(c["k"], c["ij"], c["K"], np.float64, steps=30)
    return im.ray_terms(c["ij"], c["K"], c["k"], v[:, 0], -v[:, 1], c["R"], c["d_d"], np.float64, **mutant)


@pytest.mark.parametrize("which", range(6))
def test_terms_agree_with_central_differences(which):
    c = _fd_case(which)
    fd = _fd_terms(c)
    t, mag = _analytic(c)
    assert (mag > 0).all() and np.abs(t).max() > 1e-3
    bound = FD_RTOL * mag + _fd_floor(c)
    ratio = np.abs(t - fd) / bound
    print("set %d: largest |analytic - difference| / bound per parameter" % which,
          dict(zip(im.NAMES, ["%.1e" % r for r in ratio.max(0)])))
    assert (ratio <= 1.0).all(), ratio.max(0)
    assert (_fd_floor(c) < 1e-3 * FD_RTOL * mag)[:4].all()  # at the corners the floor is idle


def _f32_error(which):
    c = im.term_case(which)
    x, y = im.forward_xy32(c["k"], c["ij"], c["K"])
    t64, m64 = im.ray_terms(c["ij"], c["K"], c["k"], x, y, c["R"], c["d_d"], np.float64)
    t32, _ = im.ray_terms(c["ij"], c["K"], c["k"], x, y, c["R"], c["d_d"], np.float32)
    assert (m64 > 0).all()
    return np.abs(t32.astype(np.float64) - t64) / m64


def test_term_tol_covers_f32_restatement():
    worst = max(float(_f32_error(w).max()) for w in range(6))
    print("largest |f32 restatement - f64| / mag: %.3e" % worst)
    assert lm.pow2_ceil(4.0 * worst) == im.TERM_TOL
    assert worst <= im.TERM_TOL / 4


@pytest.mark.parametrize("which", range(6))
def test_wrong_formulas_leave_the_bounds(which):
    """Float64 terms of a wrong formula against the float64 terms, at the bound the kernel is held to
    (TERM_TOL mag) and at the bound of the differences (FD_RTOL mag): the identity for the Jacobian of
    a distorted camera, and the sign of gy."""
    c = im.term_case(which)
    x, y = im.forward_xy32(c["k"], c["ij"], c["K"])
    args = (c["ij"], c["K"], c["k"], x, y, c["R"], c["d_d"], np.float64)
    t, mag = im.ray_terms(*args)
    for name, mutant in (("J = I", dict(jac_identity=True)), ("gy flipped", dict(flip_gy=True))):
        bad, _ = im.ray_terms(*args, **mutant)
        off = np.abs(bad - t)
        if name == "J = I" and not c["k"].any():
            assert (off == 0).all()  # a pinhole camera's Jacobian IS the identity
            continue
        # on most of the image, in every parameter that the mutation reaches: gy enters the terms of
        # fx and cx only through b, the off-diagonal of J
        cols = [1, 3, 4, 5, 6, 7] if name == "gy flipped" else list(range(8))
        assert ((off > im.TERM_TOL * mag).mean(0) > 0.9)[cols].all(), (name, which)
        assert ((off > FD_RTOL * mag).mean(0) > 0.5)[cols].all(), (name, which)
    # and the differences see them too
    f = _fd_case(which)
    fd = _fd_terms(f)
    _, fmag = _analytic(f)
    for name, mutant in (("J = I", dict(jac_identity=True)), ("gy flipped", dict(flip_gy=True))):
        if name == "J = I" and not f["k"].any():
            continue
        bad, _ = _analytic(f, **mutant)
        assert (np.abs(bad - fd) > FD_RTOL * fmag + _fd_floor(f)).any(), (name, which)


# ---- the correction --------------------------------------------------------------------------------

def _compose_case(E, G, seed=3):
    rng = np.random.default_rng(seed)
    K = np.tile(lm.intrinsic()[None], (E, 1, 1)) * (1.0 + 0.1 * rng.random((E, 1, 1))).astype(np.float32)
    K[:, 2, 2] = 1.0
    dist = np.asarray([lm.SETS[e % len(lm.SETS)] for e in range(E)], dtype=np.float32)
    gamma = (rng.standard_normal((G, 8)) * 0.05).astype(np.float32)
    group = rng.integers(0, G, E).astype(np.int32)
    return K.astype(np.float32), dist, gamma, group


def test_centre_moves_in_units_of_the_base_focal_length():
    K, dist, gamma, group = _compose_case(65, 3)
    good, _ = im.compose64(K, dist, gamma, group)
    bad, _ = im.compose64(K, dist, gamma, group, cx_by_new_fx=True)
    # the bound the kernel is held to: one float32 ulp
    assert (np.abs(bad - good)[:, 0, 2] > pm.ulp32(good[:, 0, 2])).all()
    assert (np.abs(bad - good)[:, 1, 2] > pm.ulp32(good[:, 1, 2])).all()
    assert (good[:, 0, 2] - K[:, 0, 2] == gamma.astype(np.float64)[group, 2] * K[:, 0, 0]).all()
    # zero gamma and negative groups: the base rows
    same, same_d = im.compose64(K, dist, np.zeros_like(gamma), group)
    assert (same == K).all() and (same_d == dist).all()
    fixed, fixed_d = im.compose64(K, dist, gamma, -1 - group)
    assert (fixed == K).all() and (fixed_d == dist).all()


def test_compose_backward_agrees_with_differences_of_the_forward():
    E, G = 13, 3
    K, dist, gamma, group = _compose_case(E, G)
    group[5] = -1
    rng = np.random.default_rng(8)
    d_K = rng.standard_normal((E, 3, 3))
    d_dist = rng.standard_normal((E, 4))
    learn = np.array([1, 1, 0, 1, 1, 0, 1, 1])
    got, mag, cnt = im.compose_bwd64(K, gamma, group, learn, d_K, d_dist)
    assert cnt.sum() == E - 1 and (got[:, [2, 5]] == 0).all()
    free, _, _ = im.compose_bwd64(K, gamma, group, None, d_K, d_dist)
    mask = np.zeros((3, 3))
    mask[0, 0] = mask[1, 1] = mask[0, 2] = mask[1, 2] = 1.0

    def loss(c):
        Kn, Dn = im.compose64(K, dist, c, group)
        return (Kn * d_K * mask).sum() + (Dn * d_dist).sum()

    h = 1e-6
    for g in range(G):
        for q in range(8):
            c = gamma.astype(np.float64)
            up, dn = c.copy(), c.copy()
            up[g, q] += h
            dn[g, q] -= h
            fd = (loss(up) - loss(dn)) / (2 * h)
            assert abs(fd - free[g, q]) <= 1e-7 * max(1.0, abs(free[g, q])), (g, q, fd, free[g, q])
    assert (np.abs(got) <= mag).all()


# ---- recovery --------------------------------------------------------------------------------------

def test_calibration_is_recovered_from_rays_alone():
    """Adam (lr 1e-3, betas 0.9 / 0.99) for 300 steps from gamma = 0 on 512 seeded pixels a step.  The
    loss is compared on the whole image.  Focal length and k1 trade off, so gamma is not asked to
    arrive, only gamma0 and gamma1 to within 0.01 and the loss to fall a thousandfold."""
    every = np.stack(np.meshgrid(np.arange(im.REC_H), np.arange(im.REC_W), indexing="ij"), -1)
    every = every.reshape(-1, 2).astype(np.int32)
    target_all = im.recovery_dirs64(im.REC_GAMMA, every)[0]
    gamma = np.zeros(8)
    first, _ = im.recovery_loss_and_grad(gamma, every, target_all)
    m, v = np.zeros(8), np.zeros(8)
    b1, b2, eps = 0.9, 0.99, 1e-15
    for step in range(im.REC_STEPS):
        ij = im.recovery_pixels(step)
        target = im.recovery_dirs64(im.REC_GAMMA, ij)[0]
        _, g = im.recovery_loss_and_grad(gamma, ij, target)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        gamma = gamma - im.REC_LR * (m / (1 - b1 ** (step + 1))) / (
            np.sqrt(v / (1 - b2 ** (step + 1))) + eps)
    last, _ = im.recovery_loss_and_grad(gamma, every, target_all)
    print("loss %.3e -> %.3e (%.3g-fold), gamma - gamma* =" % (first, last, first / last),
          np.array2string(gamma - im.REC_GAMMA, precision=4))
    assert first / last >= 1e3
    assert abs(gamma[0] - im.REC_GAMMA[0]) < 0.01 and abs(gamma[1] - im.REC_GAMMA[1]) < 0.01
