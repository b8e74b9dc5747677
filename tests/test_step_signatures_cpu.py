"""The Python signatures of the Renderer's training entries, as pybind11 renders them in the first line
of __doc__: argument names, order and defaults, which bench.py and every tool rely on.  The literals
were copied from a build made before the C++ side moved to one LossTerms / LossOutputs signature.

A default that is an object prints as <... object at 0xADDRESS>; the address differs from process to
process, so it -- and nothing else -- is cut from both sides before they are compared."""
import importlib
import re

import pytest

SIGNATURES = {
    "train_step":
        "train_step(self: _f2nerf_host.Renderer, rays_o: torch.Tensor, rays_d: torch.Tensor, "
        "emb_idx: torch.Tensor, gt_colors: torch.Tensor, var_loss_weight: typing.SupportsFloat = 0.0, "
        "noise: torch.Tensor | None = None, bg_color: torch.Tensor | None = None, "
        "backward: bool = True, dist_loss_weight: typing.SupportsFloat = 0.0, "
        "depth_target: torch.Tensor | None = None, "
        "depth_loss: _f2nerf_host.DepthLossOptions = <_f2nerf_host.DepthLossOptions object at 0x>) "
        "-> tuple",
    "train_step_supervised":
        "train_step_supervised(self: _f2nerf_host.Renderer, rays_o: torch.Tensor, "
        "rays_d: torch.Tensor, emb_idx: torch.Tensor, gt_colors: torch.Tensor, "
        "sup: _f2nerf_host.RaySupervision, var_loss_weight: typing.SupportsFloat = 0.0, "
        "noise: torch.Tensor | None = None, bg_color: torch.Tensor | None = None, "
        "backward: bool = True, dist_loss_weight: typing.SupportsFloat = 0.0, "
        "depth_target: torch.Tensor | None = None, "
        "depth_loss: _f2nerf_host.DepthLossOptions = <_f2nerf_host.DepthLossOptions object at 0x>) "
        "-> tuple",
    "train_step_patches":
        "train_step_patches(self: _f2nerf_host.Renderer, rays_o: torch.Tensor, rays_d: torch.Tensor, "
        "emb_idx: torch.Tensor, gt_colors: torch.Tensor, patch: _f2nerf_host.PatchLoss, "
        "sup: _f2nerf_host.RaySupervision = <_f2nerf_host.RaySupervision object at 0x>, "
        "var_loss_weight: typing.SupportsFloat = 0.0, noise: torch.Tensor | None = None, "
        "bg_color: torch.Tensor | None = None, backward: bool = True, "
        "dist_loss_weight: typing.SupportsFloat = 0.0, depth_target: torch.Tensor | None = None, "
        "depth_loss: _f2nerf_host.DepthLossOptions = <_f2nerf_host.DepthLossOptions object at 0x>) "
        "-> tuple",
    "train_step_robust":
        "train_step_robust(self: _f2nerf_host.Renderer, rays_o: torch.Tensor, rays_d: torch.Tensor, "
        "emb_idx: torch.Tensor, gt_colors: torch.Tensor, robust: _f2nerf_host.RobustLoss, "
        "patch: _f2nerf_host.PatchLoss = <_f2nerf_host.PatchLoss object at 0x>, "
        "sup: _f2nerf_host.RaySupervision = <_f2nerf_host.RaySupervision object at 0x>, "
        "var_loss_weight: typing.SupportsFloat = 0.0, noise: torch.Tensor | None = None, "
        "bg_color: torch.Tensor | None = None, backward: bool = True, "
        "dist_loss_weight: typing.SupportsFloat = 0.0, depth_target: torch.Tensor | None = None, "
        "depth_loss: _f2nerf_host.DepthLossOptions = <_f2nerf_host.DepthLossOptions object at 0x>) "
        "-> tuple",
    "render_for_loss":
        "render_for_loss(self: _f2nerf_host.Renderer, rays_o: torch.Tensor, rays_d: torch.Tensor, "
        "emb_idx: torch.Tensor | None = None, mode: str = 'train', noise: torch.Tensor | None = None, "
        "bg_color: torch.Tensor | None = None, want_dist: bool = False, "
        "depth_target: torch.Tensor | None = None, depth_eps: typing.SupportsFloat = 0.0) -> tuple",
    "render_for_loss_result":
        "render_for_loss_result(self: _f2nerf_host.Renderer, rays_o: torch.Tensor, "
        "rays_d: torch.Tensor, emb_idx: torch.Tensor | None = None, mode: str = 'train', "
        "noise: torch.Tensor | None = None, bg_color: torch.Tensor | None = None, "
        "want_dist: bool = False, depth_target: torch.Tensor | None = None, "
        "depth_eps: typing.SupportsFloat = 0.0, want_opacity: bool = False) "
        "-> _f2nerf_host.RenderResult",
}


@pytest.fixture(scope="module")
def host():
    return importlib.import_module("f2-nerf_amd").load_host()


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signature(host, name):
    line = getattr(host.Renderer, name).__doc__.split("\n")[0]
    assert re.sub(r" at 0x[0-9a-fA-F]+>", " at 0x>", line) == SIGNATURES[name]
