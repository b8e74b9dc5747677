// occupancy_grid.hpp -- OccupancyGrid: a bitfield over contracted space that lets the early-stop march
// skip empty space (f2n_occ_update / f2n_occ_lookup / f2n_density_march_occ / f2n_sample_compact_occ).
//
// Upstream F2-NeRF skips empty space with an occupancy grid; the reference fork stripped it and kept
// only its trace (reference src/main_functions/train_manager.cpp:102), so there is no reference class
// to mirror.  The grid is NOT a registered parameter or buffer of anything: renderer.pt keeps the
// reference's layout, and a grid is rebuilt from the field with a few update() passes after loading.
//
// Semantics (include/f2nerf_hip.h, "occupancy bitfield"): G^3 bits over [-2, 2)^3; a render with a
// grid is the render without one with the density of every sample in an unoccupied cell set to
// exactly zero, and those samples dropped.  A fresh grid is all ones: nothing is skipped until the
// first update().
//
// The allowed mask (set_allowed / carve_to_cameras): a set of cells, usually the ones the training
// cameras can sample (occ_visibility.hpp), outside which no bit is ever on.  While it is set,
// words_ &= allowed_ at once, after every update() and after every set_bits(): one in-place ATen op, no
// host read.  density() is untouched, so clear_allowed() and an update() restore the plain grid.  Like
// the grid itself the mask is not a parameter or buffer: it is rebuilt from the cameras after loading.
#pragma once

#include "hash_3d_anchored.hpp"
#include "occ_visibility.hpp"

class OccupancyGrid
{
  using Tensor = torch::Tensor;

public:
  // Defaults of update().  The threshold is a DENSITY (sigma = exp(logit - 3)), not an optical depth:
  // a sample whose density equals it carries at most threshold * 1.5 * step of optical depth under
  // TRAIN jitter (1.0 at the reference's step of 1/256: 0.006 per sample).  The probe is one point per
  // cell and no bound on the cell's density, which is why a cell once seen dense decays slowly
  // (density = max(density * decay, sigma)) and why callers may jitter the probe.
  static constexpr float kDefaultThreshold = 1.0f;
  static constexpr float kDefaultDecay = 0.95f;

  explicit OccupancyGrid(int64_t resolution = 128, torch::Device device = f2n::default_device());

  // One pass over all cells with the field's current table and density head.  probe: [G,G,G,3] (or
  // [G^3,3]) offsets in [0,1) inside each cell, indexed [cz][cy][cx] -> (ux, uy, uz); undefined = the
  // cell centres.  The caller schedules it (every N training iterations; a handful of passes after
  // loading a checkpoint).
  void update(
    Hash3DAnchored & field, float threshold = kDefaultThreshold, float decay = kDefaultDecay,
    const Tensor & probe = Tensor());

  void set_bits(const Tensor & occupied);  // bool [G,G,G], indexed [cz][cy][cx]
  Tensor bits() const;                     // bool [G,G,G]: the effective bits (inside the allowed mask)
  Tensor density() const { return density_.view({G_, G_, G_}); }
  Tensor occupied(const Tensor & points) const;  // raw points [n,3] -> bool [n]
  double fraction() const;                       // occupied cells / all cells (a host read)

  // words: int32 [G^3/32] as camera_visibility returns them (copied).  Without a mask update() and
  // set_bits() make exactly the launches they make without this feature.
  void set_allowed(const Tensor & words);
  void clear_allowed() { allowed_ = Tensor(); }
  const Tensor & allowed() const { return allowed_; }  // undefined = no mask
  // set_allowed(camera_visibility(...)) at the grid's own resolution (opts.resolution is ignored)
  void carve_to_cameras(
    const Tensor & poses, const Tensor & intrinsics, int64_t h, int64_t w,
    f2n::VisibilityOptions opts = {}, const Tensor & dist = {},
    const f2n::PixelMask * mask = nullptr);

  int64_t resolution() const { return G_; }
  const Tensor & words() const { return words_; }  // int32 [G^3/32]: the bitfield as the kernels read it
  const uint32_t * words_ptr() const
  {
    return reinterpret_cast<const uint32_t *>(words_.data_ptr<int32_t>());
  }

private:
  int64_t G_;
  Tensor words_;    // int32 [G^3 / 32]
  Tensor density_;  // float [G^3]
  Tensor allowed_;  // int32 [G^3 / 32], undefined = no mask
};
