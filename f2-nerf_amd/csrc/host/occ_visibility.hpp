// occ_visibility.hpp -- the cells of the occupancy bitfield that the training cameras can sample
// (f2n_occ_mark_rays / f2n_occ_dilate / f2n_occ_count_add / f2n_occ_count_bits).  No reference
// counterpart: the reference fork has no occupancy grid (occupancy_grid.hpp).
//
// Where no training ray samples, nothing supervises the density; OccupancyGrid::update keeps or drops
// such cells by chance, and a render from a pose off the training trajectory (the Localizer's
// particles) crosses them.  camera_visibility is the set OccupancyGrid::set_allowed takes.
//
// Definition (include/f2nerf_hip.h, "occupancy bitfield"): camera c marks the cells that the VALIDATE
// samples k < n_steps of its walked pixels contract into;
//   seen_c = dilate^d(marks of c),  count = min(255, sum_c seen_c),  visible = count >= min_views.
//
// Why dilate = 1 and n_steps = ceil(1.5 max_samples): a TRAIN sample lies at t = step * sum(noise),
// noise in [0.5, 1.5), so t <= 1.5 S step and t is within step / 2 of a VALIDATE sample of the same
// ray; the contraction is 1-Lipschitz, so while step / 2 <= 4 / G (one cell) the contracted TRAIN
// sample lies in the 27-neighbourhood of a marked cell.  With pixel_stride = 1 every sample a training
// draw can produce is therefore visible at min_views = 1.  The functions refuse dilate >= 1 with
// step / 2 > 4 / G.  pixel_stride = s > 1 is the caller's trade: neighbouring walked rays are t s / f
// apart at distance t (f the focal length in pixels), which has to stay below a cell as well; that is
// not enforced.
#pragma once

#include "pixel_mask.hpp"
#include "points_sampler.hpp"

namespace f2n
{

struct VisibilityOptions
{
  int64_t resolution = 128;   // G: a power of two in 32..256
  int pixel_stride = 1;       // rows and columns min(a s, n - 1): the border is always walked
  int n_steps = -1;           // VALIDATE samples per ray; < 0: ceil(1.5 PtsSamplerOptions().max_samples)
  float step = 1.0f / 256;    // the sampler's step (PtsSamplerOptions::step)
  int min_views = 1;          // cameras that have to see a cell (1..255)
  int dilate = 1;             // d in {0, 1, 2}
};

// poses [n,3,4] or [n,4,4]: the NORMALISED poses the field trains in (SceneNormalisation::poses);
// intrinsics [n,3,3]; dist [n,4] or undefined (pinhole); mask: E == n, the same h and w, or null.
// -> uint8 [G,G,G], indexed [cz][cy][cx].  Per camera a memset, a mark, d dilations and a count_add on
// the current stream; nothing is read back.
torch::Tensor camera_view_counts(
  const torch::Tensor & poses, const torch::Tensor & intrinsics, int64_t h, int64_t w,
  const VisibilityOptions & opts = {}, const torch::Tensor & dist = {},
  const PixelMask * mask = nullptr);

// -> int32 [G^3 / 32] holding the uint32 words of `count >= min_views`.  min_views == 1 is the
// dilation of the union: one mark launch over all cameras instead of the loop.
torch::Tensor camera_visibility(
  const torch::Tensor & poses, const torch::Tensor & intrinsics, int64_t h, int64_t w,
  const VisibilityOptions & opts = {}, const torch::Tensor & dist = {},
  const PixelMask * mask = nullptr);

}  // namespace f2n
