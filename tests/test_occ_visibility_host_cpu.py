"""The host side of the camera carve that needs no kernel: the options' defaults and the
OccupancyGrid's allowed mask through set_bits() on a CPU grid (the AND is one ATen op)."""
import importlib

import pytest
import torch

from tests.util import _pack


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


def test_visibility_options_defaults(host):
    o = host.VisibilityOptions()
    assert (o.resolution, o.pixel_stride, o.n_steps, o.min_views, o.dilate) == (128, 1, -1, 1, 1)
    assert o.step == 1.0 / 256
    o = host.VisibilityOptions(resolution=64, pixel_stride=4, n_steps=96, step=0.5, min_views=2, dilate=0)
    assert (o.resolution, o.pixel_stride, o.n_steps, o.step, o.min_views, o.dilate) == (64, 4, 96, 0.5, 2, 0)
    o.dilate = 2
    assert o.dilate == 2


def test_allowed_mask_on_a_cpu_grid(host):
    G = 32
    g = torch.Generator().manual_seed(3)
    grid = host.OccupancyGrid(G, "cpu")
    assert grid.allowed() is None
    allowed_b = torch.rand(G, G, G, generator=g) < 0.5
    allowed = _pack(allowed_b.reshape(-1))
    grid.set_allowed(allowed)
    assert torch.equal(grid.allowed(), allowed) and grid.allowed().data_ptr() != allowed.data_ptr()
    assert torch.equal(grid.words, allowed)                    # a fresh grid is all ones: at once
    assert torch.equal(grid.bits(), allowed_b)
    assert abs(grid.fraction() - float(allowed_b.float().mean())) < 1e-6
    rnd = torch.rand(G, G, G, generator=g) < 0.5
    grid.set_bits(rnd)
    assert torch.equal(grid.bits(), rnd & allowed_b)
    assert torch.equal(grid.words, _pack(rnd.reshape(-1)) & allowed)
    allowed.zero_()                                            # the grid holds a copy
    assert torch.equal(grid.bits(), rnd & allowed_b)
    grid.clear_allowed()
    assert grid.allowed() is None
    assert torch.equal(grid.bits(), rnd & allowed_b)           # clearing alone changes no bit
    grid.set_bits(rnd)
    assert torch.equal(grid.bits(), rnd)
    for bad in (_pack(allowed_b.reshape(-1))[:-1], _pack(allowed_b.reshape(-1)).float()):
        with pytest.raises(RuntimeError, match="set_allowed"):
            grid.set_allowed(bad)


def test_the_carve_has_no_cpu_fallback(host):
    with pytest.raises(RuntimeError, match="GPU"):
        host.camera_visibility(torch.zeros(3, 3, 4), torch.zeros(3, 3, 3), 12, 20)
    with pytest.raises(RuntimeError, match="GPU"):
        host.camera_view_counts(torch.zeros(3, 3, 4), torch.zeros(3, 3, 3), 12, 20)
