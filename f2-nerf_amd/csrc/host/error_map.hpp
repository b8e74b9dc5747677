// error_map.hpp -- error-guided ray sampling: a per-image grid of running colour errors and the
// training batch drawn from it (error_map.hip; the per-image error map of instant-ngp).  The
// reference has none of it: Dataset::sample_random_rays (src/dataset.cpp:150-171) draws uniformly
// over pixels, and sample_masked_rays (pixel_mask.hpp) uniformly over valid pixels.
#pragma once

#include <torch/torch.h>

#include <cstdint>

#include "pixel_mask.hpp"

namespace f2n
{

struct ErrorMapOptions
{
  // Cells per image.  32 x 32: a cell of a 1920 x 1080 image is 60 x 34 pixels, small enough to
  // separate a facade's edge from its flat middle, and 200 such images make a 1.6 MB CDF that stays
  // in L2.
  int gh = 32, gw = 32;
  // Weight of the old value when update() folds a round of errors in.  0.95: with an update every
  // few steps a cell forgets an error in about 20 of them, slower than the render improves.
  float decay = 0.95f;
  // Share of the rays drawn uniformly over valid pixels.  0.1 bounds every importance weight by
  // 1 / 0.1 = 10, so no single ray dominates the loss, and keeps every pixel reachable.
  float uniform_fraction = 0.1f;
  // Attempts per ray, in the uniform branch over the set and in the guided branch inside the cell:
  // 32, the masked draw's default, for the same reason (pixel_mask.hip).
  int attempts = 32;
  // Every cell starts at 1, the colour error of an untrained render: equal values make the first
  // draws uniform over valid pixels, and the first update pulls the hit cells down from it.
  float init_value = 1.f;
};

// What draw() returns: sample_masked_rays' (cam, ij, tries) and the importance weight
// uniform pdf / pdf used (0 where every attempt missed).
struct GuidedDraw
{
  torch::Tensor cam, ij, tries, ray_weight;
};

// The map of E images of h x w pixels.  It owns value [n_cells] f32, counts [n_cells] i32 (valid
// pixels per cell), cdf [n_cells] u64 (held as int64), the accumulators and the scan scratch.  No
// call reads the device, so every call can be captured in a hipGraph.
class ErrorMap
{
public:
  ErrorMap(
    int64_t E, int64_t h, int64_t w, const ErrorMapOptions & options, const torch::Device & device);
  // ... with a mask: counts and the draw follow its valid pixels (the mask's E, h, w)
  ErrorMap(const PixelMask & mask, const ErrorMapOptions & options);

  // f2n_error_map_accum: the errors of one rendered batch.  colors, gt [n,3]; cam [n] i32, ij [n,2]
  // i32 as the draw returned them; ray_weight, alpha [n] and bg [n,3] optional (alpha needs bg).
  // The raw error is recorded: ray_weight only says which rays to skip (m_r == 0).
  void accumulate(
    const torch::Tensor & colors, const torch::Tensor & gt, const torch::Tensor & cam,
    const torch::Tensor & ij, const torch::Tensor & ray_weight = {}, const torch::Tensor & alpha = {},
    const torch::Tensor & bg = {});

  // f2n_error_map_apply, then f2n_error_cdf
  void update();

  // f2n_draw_pixels_guided: a pure function of (the map's state, n, seed)
  GuidedDraw draw(int64_t n, uint64_t seed) const;

  ErrorMapOptions options;
  int64_t E = 0, h = 0, w = 0, n_cells = 0;
  torch::Tensor value, counts, cdf, acc_sum, acc_cnt;
  torch::Tensor bits;     // the mask's words; undefined without a mask
  torch::Tensor n_valid;  // [1] int64 on the device: the mask's count, or E*h*w

private:
  void init(const torch::Device & device);
  torch::Tensor scan_partial_;
};

// sample_masked_rays with the guided draw: the same f2n_gen_rays / f2n_gen_rays_dist launch for the
// drawn (cam, ij) -- the same bits -- and ray_weight is the importance weight.  images as there.
MaskedBatch sample_guided_rays(
  const torch::Tensor & poses, const torch::Tensor & intrinsics, const ErrorMap & map,
  int64_t batch_size, uint64_t seed, const torch::Tensor & images = {},
  const torch::Tensor & dist = {});

}  // namespace f2n
