"""The learned background's kernels against tests/envmap_model.py: the forward within the model's
counted bound, the backward's integer sums and the applied gradient bit for bit, the flags, and
EnvMap.query's autograd node.  R in {2, 5, 64} (at R = 2 every lookup clamps or sits between the
only two texels), n in {1, 63, 257} rays (one lane each in 256-lane workgroups: a partial workgroup,
and more than one).  Directions are the special set of the model (axes, corners, edge midpoints,
-0.0, scales 1e-20 and 1e20, a NaN beside a larger component), the degenerate rays, and random ones.
Every output buffer is written through the C ABI into the middle of a larger one that carries guard
sentinels."""
import importlib

import numpy as np
import pytest
import torch

from tests import envmap_model as em

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 8
SENTINEL = -7777.0
RS = (2, 5, 64)
NS = (1, 63, 257)


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def _dirs(n, seed):
    """n directions: the special and the degenerate ones first (as many as fit), then random"""
    pool = np.concatenate([em.special_dirs(), em.degenerate_dirs()])
    if n < len(pool):
        pick = np.random.RandomState(seed).choice(len(pool), n, replace=False)
        return pool[np.sort(pick)]
    return np.concatenate([pool, em.random_dirs(n - len(pool), seed)])


def _tex(R, seed):
    return (np.random.RandomState(100 + seed).randn(6, R, R, 3) * 2.0).astype(F32)


def _guarded(n, dev, dtype=torch.float32, fill=SENTINEL):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, fill=SENTINEL):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


def _forward(capi, dev, dirs, tex, R):
    n = len(dirs)
    d = torch.from_numpy(np.ascontiguousarray(dirs)).to(dev)
    t = torch.from_numpy(tex).to(dev)
    buf, bg = _guarded(3 * n, dev)
    capi.call("envmap_fwd", d, t, R, bg, n)
    torch.cuda.synchronize()
    assert _guards_intact(buf, 3 * n)
    return d, bg.clone().reshape(n, 3)


def _d_bg(n, seed):
    """|d_bg| <= 1e3, with exact zeros: whole rays (the opaque ones) and single channels"""
    rng = np.random.RandomState(200 + seed)
    g = (rng.randn(n, 3) * 300.0).clip(-1e3, 1e3)
    g[rng.rand(n) < 0.4] = 0.0
    g[rng.rand(n, 3) < 0.1] = 0.0
    g[0, 1] = 0.0
    if n > 2:
        g[1] = (1e3, -1e3, 1e-30)
    return g.astype(F32)


def _backward(capi, dev, d, bg, g, R, acc_view=None, flags_view=None):
    n = d.shape[0]
    n_acc = em.texels(R) * 3
    bufs = None
    if acc_view is None:
        acc_buf, acc_view = _guarded(n_acc, dev, torch.int64, 0)
        acc_buf[:GUARD] = acc_buf[GUARD + n_acc:] = -7777
        flag_buf, flags_view = _guarded(1, dev, torch.int32, 0)
        flag_buf[:GUARD] = flag_buf[GUARD + 1:] = -7777
        bufs = (acc_buf, flag_buf)
    capi.call("envmap_bwd", d, bg.contiguous(), torch.from_numpy(g).to(dev), R, acc_view, flags_view, n)
    torch.cuda.synchronize()
    if bufs:
        assert _guards_intact(bufs[0], n_acc, -7777) and _guards_intact(bufs[1], 1, -7777)
    return acc_view, flags_view, bufs


WORST = {}


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("R", RS)
def test_forward_within_the_bound(capi, dev, R, n):
    dirs, tex = _dirs(n, R + n), _tex(R, n)
    _, bg = _forward(capi, dev, dirs, tex, R)
    want, tol = em.forward(dirs, tex, R)
    err = np.abs(bg.cpu().numpy().astype(np.float64) - want)
    ratio = float((err / np.maximum(tol, 1e-300))[tol > 0].max()) if (tol > 0).any() else 0.0
    WORST[(R, n)] = ratio
    print("  R = %d, n = %d: worst error / bound = %.3f (over all cases so far %.3f)" % (
        R, n, ratio, max(WORST.values())))
    assert (err <= tol).all()
    dead = ~em.geometry(dirs, R)["live"]
    assert (bg.cpu().numpy()[dead] == 0.5).all()
    # a texture of zeros: the render's own inference default, exactly
    _, half = _forward(capi, dev, dirs, np.zeros_like(tex), R)
    assert bool((half == 0.5).all())


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("R", RS)
def test_backward_and_apply_bit_for_bit(capi, dev, R, n):
    dirs, tex = _dirs(n, 3 * R + n), _tex(R, n + 1)
    d, bg = _forward(capi, dev, dirs, tex, R)
    g = _d_bg(n, R + n)
    assert (np.abs(g) <= 1e3).all() and (g == 0).any()
    want, want_flags = em.backward(dirs, bg.cpu().numpy(), g, R)
    assert want_flags == 0                                    # at this size the cap cannot apply
    want64 = torch.from_numpy(em.acc_int64(want))
    acc, flags, _ = _backward(capi, dev, d, bg, g, R)
    assert torch.equal(acc.cpu(), want64) and int(flags) == 0
    if n > 2:
        assert bool(want64.ne(0).any())
    again, _, _ = _backward(capi, dev, d, bg, g, R)           # two runs: the same bits
    assert torch.equal(again, acc)
    # apply: the gradient's bits, acc left at zero, accumulate honoured
    n_el = em.texels(R) * 3
    buf, d_tex = _guarded(n_el, dev)
    capi.call("envmap_grad_apply", acc, R, d_tex, 0)
    torch.cuda.synchronize()
    want_g = em.apply(want)
    assert _guards_intact(buf, n_el)
    assert torch.equal(d_tex.cpu(), torch.from_numpy(want_g))
    assert not bool(acc.any())
    prev = torch.from_numpy(np.random.RandomState(R).randn(n_el).astype(F32))
    d_tex.copy_(prev)
    capi.call("envmap_grad_apply", again, R, d_tex, 1)
    torch.cuda.synchronize()
    assert torch.equal(d_tex.cpu(), torch.from_numpy(em.apply(want, prev.numpy())))
    assert not bool(again.any()) and _guards_intact(buf, n_el)


def test_257_rays_in_one_texel(capi, dev):
    """every ray inside one texel's cell of face +z (R = 5): four elements per channel take 257
    contributions each, from two workgroups"""
    R, n = 5, 257
    rng = np.random.RandomState(5)
    # u = (s/2 + 1/2) 5 - 1/2 in (2, 3)  <=>  s in (0, 0.4): the corners are texels 2 and 3 both ways
    st = 0.02 + 0.36 * rng.rand(n, 2)
    dirs = (np.concatenate([st, np.ones((n, 1))], 1) * np.exp(rng.randn(n, 1))).astype(F32)
    geo = em.geometry(dirs, R)
    assert len({tuple(r) for r in geo["idx"].tolist()}) == 1 and (geo["w"] > 0).all()
    tex = _tex(R, 8)
    d, bg = _forward(capi, dev, dirs, tex, R)
    g = (rng.randn(n, 3) * 300.0).clip(-1e3, 1e3).astype(F32)
    g[::9] = 0.0
    want, want_flags = em.backward(dirs, bg.cpu().numpy(), g, R)
    acc, flags, _ = _backward(capi, dev, d, bg, g, R)
    assert want_flags == 0 and int(flags) == 0
    assert torch.equal(acc.cpu(), torch.from_numpy(em.acc_int64(want)))
    assert int(acc.ne(0).sum()) == 12
    again, _, _ = _backward(capi, dev, d, bg, g, R)
    assert torch.equal(again, acc)


@pytest.mark.parametrize("bad,want_flags", [((np.inf,), 1), ((np.nan,), 1), ((1e30,), 2),
                                            ((-np.inf, 1e30), 3), ((), 0)])
def test_flags_not_faults(capi, dev, bad, want_flags):
    """d_bg of inf, NaN and 1e30: a flag each, nothing added for the first two, the cap for the third,
    and the finite rays summed exactly.  The rays with the bad values look up the inside of a face
    with four distinct texels, so that no element takes two capped contributions."""
    R, n = 5, 63
    dirs = _dirs(n, 11).copy()
    dirs[:4] = [(0.1, 0.2, 1.0), (-1.0, 0.3, -0.1), (0.3, 2.0, 0.5), (0.2, -0.3, -1.5)]
    tex = _tex(R, 4)
    d, bg = _forward(capi, dev, dirs, tex, R)
    g = _d_bg(n, 6)
    for k, v in enumerate(bad):
        g[k, k % 3] = v
    want, model_flags = em.backward(dirs, bg.cpu().numpy(), g, R)
    assert model_flags == want_flags
    acc, flags, _ = _backward(capi, dev, d, bg, g, R)
    assert int(flags) == want_flags
    assert torch.equal(acc.cpu(), torch.from_numpy(em.acc_int64(want)))
    # the flags are or-ed into: a clean batch afterwards leaves them
    acc.zero_()
    clean = _d_bg(n, 7)
    _backward(capi, dev, d, bg, clean, R, acc, flags)
    assert int(flags) == want_flags
    assert torch.equal(acc.cpu(), torch.from_numpy(em.acc_int64(em.backward(dirs, bg.cpu().numpy(), clean, R)[0])))


def test_no_rays_launches_nothing(capi, dev):
    R = 5
    acc = torch.zeros(em.texels(R) * 3, dtype=torch.int64, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    some = torch.zeros(3, device=dev)
    capi.call("envmap_fwd", some, torch.zeros(6, R, R, 3, device=dev), R, some, 0)
    capi.call("envmap_bwd", some, some, some, R, acc, flags, 0)
    torch.cuda.synchronize()
    assert not bool(acc.any()) and int(flags) == 0


@pytest.mark.parametrize("R", [5, 64])
def test_query_autograd(host, dev, R):
    """EnvMap.query: the forward is f2n_envmap_fwd, an upstream factor of 4 reaches the texture
    gradient exactly, acc is zero afterwards, an all-zero upstream gradient gives an all-zero one, and
    save / load round-trips the texture alone"""
    n = 257
    env = host.EnvMap(R)
    assert env.resolution == R and env.texture.shape == (6, R, R, 3) and not bool(env.texture.any())
    dirs = _dirs(n, R)
    d = torch.from_numpy(dirs).to(dev)
    assert bool((env.query(d) == 0.5).all())
    tex = _tex(R, 2)
    with torch.no_grad():
        env.texture.copy_(torch.from_numpy(tex))
    G = torch.from_numpy(_d_bg(n, 3)).to(dev)
    bg = env.query(d)
    assert bg.requires_grad and torch.equal(bg.detach(), host.envmap_query(d, env.texture))
    (bg * G * 4.0).sum().backward()
    torch.cuda.synchronize()
    want, flags = em.backward(dirs, bg.detach().cpu().numpy(), (G * 4.0).cpu().numpy(), R)
    assert flags == 0 and env.flags() == 0
    assert torch.equal(env.texture.grad.cpu().reshape(-1), torch.from_numpy(em.apply(want)))
    assert bool(env.texture.grad.ne(0).any()) and not bool(env.acc.any())
    # the free functions are the node's two halves
    acc = torch.zeros_like(env.acc)
    fl = torch.zeros(1, dtype=torch.int32, device=dev)
    host.envmap_bwd(d, bg.detach(), G * 4.0, R, acc, fl)
    d_tex = torch.empty_like(env.texture)
    host.envmap_grad_apply(acc, R, d_tex)
    assert torch.equal(d_tex, env.texture.grad) and not bool(acc.any())
    env.zero_grad()
    (env.query(d) * 0.0).sum().backward()
    assert not bool(env.texture.grad.any()) and not bool(env.acc.any())
    # a non-finite upstream gradient is a flag, read once
    (env.query(d) * float("inf")).sum().backward()
    assert env.flags() == 1 and env.flags() == 0


def test_save_and_load(host, dev, tmp_path):
    env = host.EnvMap(5)
    with torch.no_grad():
        env.texture.copy_(torch.from_numpy(_tex(5, 12)))
    path = str(tmp_path / "env.pt")
    env.save(path)
    other = host.EnvMap(5)
    other.load(path)
    assert torch.equal(other.texture, env.texture) and other.texture.requires_grad
    assert env.make_adam(1e-2).n_groups() == 1
