"""f2n_density_lattice against the entries it must agree with bit for bit: positions by the stated
fmaf in float32 (tests/mesh_model.py::fmaf32, correctly rounded), f2n_contract_fwd and f2n_hash_fwd on
the same device, and the chain logit = fmaf(enc_c, w0[c], logit) from b0 evaluated exactly and rounded
once per step.  Lattices with partial bricks on every side, a box that holds both branches of the
contraction and one with a vertex exactly at the origin (NaN, quirk Q6, for itself only)."""
import numpy as np
import pytest
import torch

from oracle import kernels as K
from oracle.ref_render import _is_prime
from tests import mesh_model as M

pytestmark = pytest.mark.gpu

FIELDS = {                      # name: (L, F, T, disjoint level windows)
    "ref": (16, 2, 1 << 19, False),
    "f4": (8, 4, 1 << 12, True),
    "np2_f1": (16, 1, 5000, False),
    "f8": (8, 8, 1 << 12, True),
}
LATTICES = [(5, 6, 7), (2, 2, 2), (17, 4, 33), (9, 9, 9)]          # (nx, ny, nz)
BOXES = {"wide": None, "origin": (-1.0, 0.25)}                     # wide: [-3, 3]^3
SENTINEL = -12345.0
OK, INVALID, UNSUPPORTED = 0, -1, -3
_cache = {}


def field(name, dev):
    if name not in _cache:
        L, F, T, disjoint = FIELDS[name]
        g = torch.Generator().manual_seed(100 + list(FIELDS).index(name))
        stride = T * F if disjoint else T
        numel = max(T * L * F, stride * (L - 1) + T * F)
        primes = []
        while len(primes) < 3 * L:
            v = int(torch.randint(1 << 28, 1 << 30, (1,), generator=g))
            if _is_prime(v):
                primes.append(v)
        _cache[name] = dict(
            L=L, F=F, T=T, stride=stride, table16=K.cast_f16(torch.randn(numel, generator=g) * 0.1).to(dev),
            primes=torch.tensor(primes, dtype=torch.int32).reshape(L, 3).to(dev),
            bias=(torch.rand(L, 3, generator=g) * 1000.0 + 100.0).to(dev), mul=K.level_mul(L).to(dev),
            w0=(torch.randn(L * F, generator=g) * 0.5).to(dev), b0=torch.randn(1, generator=g).to(dev))
    return _cache[name]


def box(kind, dims):
    if BOXES[kind] is None:
        return (np.float32(-3.0),) * 3, tuple(np.float32(6.0) / np.float32(n - 1) for n in dims)
    lo, step = BOXES[kind]
    return (np.float32(lo),) * 3, (np.float32(step),) * 3


def lattice(capi, dev, f, dims, lo, step, out=None):
    nx, ny, nz = dims
    if out is None:
        out = torch.full((nz, ny, nx), SENTINEL, device=dev)
    capi.call("density_lattice", f["table16"], f["primes"], f["bias"], f["mul"], f["w0"], f["b0"], out,
              *[float(v) for v in lo], *[float(v) for v in step], nx, ny, nz, f["L"], f["F"], f["T"], f["stride"])
    return out


def expected(capi, dev, f, dims, lo, step):
    """-> float32 [nz, ny, nx] and the raw positions [n, 3]"""
    nx, ny, nz = dims
    px, py, pz = (M.axis_positions(n, l, h) for n, l, h in zip(dims, lo, step))
    pts = np.stack([np.broadcast_to(px[None, None, :], (nz, ny, nx)), np.broadcast_to(py[None, :, None], (nz, ny, nx)),
                    np.broadcast_to(pz[:, None, None], (nz, ny, nx))], -1).reshape(-1, 3)
    n, C = pts.shape[0], f["L"] * f["F"]
    p = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
    x, enc = torch.empty_like(p), torch.empty(n, C, device=dev)
    capi.call("contract_fwd", p, x, n)
    capi.call("hash_fwd", x, f["table16"], f["primes"], f["bias"], f["mul"], enc, C, 1, None, n, f["L"], f["F"],
              f["T"], f["stride"])
    enc, w0 = enc.cpu().numpy(), f["w0"].cpu().numpy()
    logit = np.full(n, f["b0"].cpu().numpy()[0], dtype=np.float32)
    for c in range(C):
        logit = M.fmaf32(enc[:, c], w0[c], logit)
    return logit.reshape(nz, ny, nx), pts


@pytest.mark.parametrize("kind", list(BOXES))
@pytest.mark.parametrize("dims", LATTICES, ids=lambda d: "%dx%dx%d" % d)
@pytest.mark.parametrize("name", list(FIELDS))
def test_lattice_logits_bit_for_bit(capi, dev, name, dims, kind):
    f = field(name, dev)
    lo, step = box(kind, dims)
    got = lattice(capi, dev, f, dims, lo, step)
    assert not bool((got == SENTINEL).any())                        # every element written, partial bricks too
    assert torch.equal(got.view(torch.int32), lattice(capi, dev, f, dims, lo, step).view(torch.int32))
    want, pts = expected(capi, dev, f, dims, lo, step)
    got = got.cpu().numpy()
    origin = (pts == 0).all(1).reshape(want.shape)
    if kind == "origin":
        assert int(origin.sum()) == (1 if min(dims) >= 5 else 0)    # vertex (4, 4, 4)
    assert np.isnan(got[origin]).all() and np.isnan(want[origin]).all()
    assert np.isfinite(got[~origin]).all()
    assert np.array_equal(got[~origin].view(np.int32), want[~origin].view(np.int32))
    if kind == "wide" and min(dims) > 2:
        r = np.linalg.norm(pts.astype(np.float64), axis=1)
        assert (r <= 1).any() and (r > 1).any()                     # both branches of the contraction


def test_host_surface_is_the_entry(pkg, capi, dev):
    """density_lattice(Hash3DAnchored) = the entry on the field's own tensors, head and f16 shadow"""
    H = pkg.load_host()
    H.manual_seed(3)
    fld = H.Hash3DAnchored(n_levels=8, n_channels=4, log2_table=12)
    with torch.no_grad():
        fld.feat_pool.copy_(torch.randn(fld.feat_pool.shape, generator=torch.Generator().manual_seed(1)).to(dev) * 0.1)
    w0, b0 = fld.density_head()
    f = dict(L=8, F=4, T=fld.local_size, stride=fld.level_stride, table16=fld.table_f16(), primes=fld.prim_pool,
             bias=fld.bias_pool.detach(), mul=fld.level_mul, w0=w0, b0=b0)
    dims, lo, step = (6, 5, 9), (-2.0, -1.5, -1.0), (0.7, 0.6, 0.3)
    got = H.density_lattice(fld, lo, step, dims)
    assert got.shape == (9, 5, 6) and got.dtype == torch.float32
    assert torch.equal(got, lattice(capi, dev, f, dims, lo, step))
    for bad in ((1, 5, 9), (6, 5, 1)):
        with pytest.raises(RuntimeError, match="at least 2"):
            H.density_lattice(fld, lo, step, bad)
    with pytest.raises(RuntimeError, match="positive"):
        H.density_lattice(fld, lo, (0.7, 0.0, 0.3), dims)


def test_invalid_arguments_launch_nothing(capi, dev):
    f = field("f4", dev)
    c = capi.lib().cdll
    out = torch.full((7, 6, 5), SENTINEL, device=dev)
    stream = capi.current_stream()

    def call(dims=(5, 6, 7), step=(0.1, 0.1, 0.1), L=None, null=None):
        a = [f[k].data_ptr() for k in ("table16", "primes", "bias", "mul", "w0", "b0")] + [out.data_ptr()]
        if null is not None:
            a[null] = None
        return c.f2n_density_lattice(*a, -1.0, -1.0, -1.0, *step, *dims, f["L"] if L is None else L, f["F"], f["T"],
                                     f["stride"], stream)

    assert call(dims=(1, 6, 7)) == INVALID and call(dims=(5, 6, 1)) == INVALID
    assert call(step=(0.1, 0.0, 0.1)) == INVALID and call(step=(-0.1, 0.1, 0.1)) == INVALID
    assert call(L=33) == UNSUPPORTED
    for k in range(7):
        assert call(null=k) == INVALID, k
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call() == OK
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())
