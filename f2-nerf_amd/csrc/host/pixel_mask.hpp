// pixel_mask.hpp -- per-pixel validity masks of an image set and the training batch that respects
// them.  The reference has no mask: Dataset::sample_random_rays (src/dataset.cpp:150-171) draws over
// the whole image.  Masks arrive as tensors (reading them from disk is the caller's business).
#pragma once

#include <torch/torch.h>

#include <cstdint>

#include "rays.hpp"

namespace f2n
{

// The mask of E images of h x w pixels as bits on the device (f2n_mask_pack): global pixel
// g = (e*h + i)*w + j is bit (g & 31) of word (g >> 5).  52 MB for 200 images of 1920x1080, where a
// list of the valid pixels' indices would be gigabytes.
struct PixelMask
{
  torch::Tensor bits;   // [ceil(E*h*w / 32)] int32 holding the uint32 words
  torch::Tensor count;  // [1] int64 on the device: the number of valid pixels (never read here)
  int64_t E = 0, h = 0, w = 0;

  // mask: [E, h, w] (or [h, w] for one image) uint8 or bool on the GPU, non-zero = valid
  static PixelMask from_mask(const torch::Tensor & mask);
};

// f2n_draw_pixels_masked: n pixels of the set, each on a valid pixel unless all `attempts` draws
// missed.  Returns {cam [n] i32, ij [n,2] i32 (row, col), tries [n] i32 (0 = every attempt missed)}.
// The draw is a pure function of (mask, n, seed, attempts): Philox4x32-10 keyed by the seed.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> draw_pixels_masked(
  const PixelMask & mask, int64_t n, uint64_t seed, int attempts = 32);

struct MaskedBatch
{
  Rays rays;
  torch::Tensor gt;          // [n,3], undefined without images
  torch::Tensor alpha;       // [n], undefined unless images has four channels
  torch::Tensor cam;         // [n] i32
  torch::Tensor ray_weight;  // [n] f32: 1 where the draw found a valid pixel, else 0
  torch::Tensor ij;          // [n,2] i32 (row, col)
  torch::Tensor tries;       // [n] i32
};

// sample_random_rays (rays.hpp) restricted to the valid pixels of `mask`: the draw above, then the
// f2n_gen_rays / f2n_gen_rays_dist launch get_rays_from_cameras makes for the same (cam, ij) -- the
// same bits.  images: optional [E,h,w,3] or [E,h,w,4] f32 on the GPU; with four channels alpha is the
// fourth.  A ray whose attempts all missed keeps its last (invalid) pixel and gets ray_weight 0.
// Nothing is read back to the host.  Not differentiated.
MaskedBatch sample_masked_rays(
  const torch::Tensor & poses, const torch::Tensor & intrinsics, const PixelMask & mask,
  int64_t batch_size, uint64_t seed, const torch::Tensor & images = {},
  const torch::Tensor & dist = {}, int attempts = 32);

}  // namespace f2n
