// ssim.hpp -- structural similarity on the device: the metric the reference computes on the host
// (rgb_ssim, scripts/eval.py:29-75), its differentiable form for a D-SSIM loss on patches, the
// per-view scores of an evaluation, and the patch draw that gives a training batch image structure.
// The reference trains on scattered pixels only (src/dataset.cpp:150-171) and has no such loss.
#pragma once

#include <torch/torch.h>

#include <cstdint>

#include "pixel_mask.hpp"

namespace f2n
{

struct SsimOut
{
  torch::Tensor ssim;  // [B]
  torch::Tensor map;   // [B, h-10, w-10, 3], undefined unless asked for
};

// f2n_ssim_fwd: pred, gt [B,h,w,3] or [h,w,3] (B = 1) f32 on the GPU, h, w >= 11.  clip: the
// reference's three clamps (the metric); without them the expression the gradient belongs to.
// Not differentiated -- CustomOps::Ssim (ragged_ops.hpp) is.
SsimOut ssim(
  const torch::Tensor & pred, const torch::Tensor & gt, bool clip = true, bool want_map = false);

// The scores of B rendered views against their images, device tensors [B], no host read:
//   mse   mean over pixels and channels of (pred - gt)^2
//   psnr  -10 log10(mse)
//   ssim  the clipped form on both inputs clamped to [0, 1], as scripts/eval.py sees 8-bit images
//   score h w / (sum over pixels of the channel mean of (pred - gt)^2 + 1e-6): the quantity of
//         src/main_functions/test.cpp:38-40
struct ImageScores
{
  torch::Tensor mse, psnr, ssim, score;
};
ImageScores image_scores(const torch::Tensor & pred, const torch::Tensor & gt);

struct PatchDraw
{
  torch::Tensor cam;           // [n P^2] i32
  torch::Tensor ij;            // [n P^2, 2] i32 (row, col)
  torch::Tensor tries;         // [n] i32: attempts used, 0 = every attempt missed
  torch::Tensor patch_weight;  // [n] f32: 1, or 0 where tries is 0
};

// f2n_draw_patches: n_patches patches of P x P pixels from E images of h x w, patch-major and
// row-major inside a patch (pixel (u, v) of patch b is ray b P^2 + u P + v).  With a mask a patch is
// kept only if all its pixels are valid.  A pure function of its arguments: Philox4x32-10 keyed by
// the seed.  device: where the outputs live when there is no mask to take it from.
PatchDraw draw_patches(
  int64_t E, int64_t h, int64_t w, int64_t n_patches, int64_t P, uint64_t seed,
  const PixelMask & mask = {}, int attempts = 32,
  const torch::Device & device = torch::Device(torch::kCUDA));

struct PatchBatch
{
  MaskedBatch batch;           // ray_weight: the patch's weight on each of its rays
  torch::Tensor patch_weight;  // [n_patches]
};

// sample_masked_rays (pixel_mask.hpp) with the patch draw: the same f2n_gen_rays / f2n_gen_rays_dist
// launch get_rays_from_cameras makes for the same (cam, ij) -- the same bits -- and gt / alpha
// gathered the same way.  mask may be empty (no bits).  Not differentiated.
PatchBatch sample_patch_rays(
  const torch::Tensor & poses, const torch::Tensor & intrinsics, int64_t h, int64_t w,
  int64_t n_patches, int64_t P, uint64_t seed, const torch::Tensor & images = {},
  const PixelMask & mask = {}, const torch::Tensor & dist = {}, int attempts = 32);

}  // namespace f2n
