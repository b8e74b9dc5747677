// pose_refiner.hpp -- PoseRefiner: per-image SE(3) corrections of the training poses, refined while
// the field trains.
//
// The reference has no camera optimiser: its only pose optimisation is Adam on the twelve raw entries
// of one [3,4] matrix (src/localizer.cpp:142-167), which leaves SO(3) after the first step, and its
// training batch (Dataset::sample_random_rays, src/dataset.cpp:150-171) treats the poses as data.
// Here every image e has a 6-vector delta_e = (omega, tau) and the pose the rays are made from is
//   R' = Exp(omega) R,  t' = t + tau        (f2n_pose_compose; left multiplication, NeRF frame).
// The rays of a batch reach delta through f2n_cam_pose_grad (one sum per camera, no atomics) and
// f2n_pose_compose_bwd.  With all deltas zero the poses, the rays and a training step are bit for bit
// those without the refiner.
//
// Like OccupancyGrid it is not part of Renderer: renderer.pt keeps the reference's layout, and the
// refiner is saved and loaded on its own (torch::save / torch::load of the module).
//
//   renderer.options_.fused_ray_grad = true;
//   auto [rays, gt, cam] = refiner.sample_random_rays(intrinsics, h, w, n, images);
//   f2n::train_step(renderer, rays.origins, rays.dirs, cam, gt, terms);   // a f2n::LossTerms
//   field_adam.step();  pose_adam.step();   // pose_adam over refiner.optim_param_groups(lr)
#pragma once

#include <torch/torch.h>

#include <tuple>
#include <vector>

#include "rays.hpp"

// out [E,3,4] = f2n_pose_compose(base [E,3|4,4], delta [E,6], fixed [E] i32 or undefined),
// differentiable in delta (f2n_pose_compose_bwd); base and fixed are constants.
torch::Tensor pose_compose(
  const torch::Tensor & base, const torch::Tensor & delta, const torch::Tensor & fixed = {});
// d_delta [E,6] of d_out [E,3,4]: the backward entry on its own
torch::Tensor pose_compose_bwd(
  const torch::Tensor & base, const torch::Tensor & delta, const torch::Tensor & fixed,
  const torch::Tensor & d_out);

class PoseRefiner : public torch::nn::Module
{
  using Tensor = torch::Tensor;

public:
  // base_poses [E,3,4] or [E,4,4] (rows 0..2 are kept), on the device the refiner lives on
  explicit PoseRefiner(const Tensor & base_poses);

  int64_t n_cameras() const { return base_.size(0); }
  // the refined poses [E,3,4], differentiable in delta
  Tensor poses() const;
  // mask [E] (bool or integer): cameras whose correction stays zero -- at least one, or the scene as a
  // whole is free to drift (the gauge)
  void set_fixed(const Tensor & mask);

  // The training batch of sample_random_rays (rays.hpp) with rays that carry a gradient to delta.
  // Cameras are drawn on the device and SORTED before the pixels are drawn, so the per-camera sums of
  // the backward need no permutation of anything; the batch is otherwise the same distribution.
  // cam_idx [n] i32 and ij [n,2] i32, when given, replace the draws (a reproducible batch); a given
  // cam_idx need not be sorted.  images: optional [E,h,w,3].  dist: [E,4].
  // Returns {rays, gt_colors [n,3] (undefined without images), cam_indices [n] i32}.
  std::tuple<Rays, Tensor, Tensor> sample_random_rays(
    const Tensor & intrinsics, int h, int w, int64_t batch_size, const Tensor & images = {},
    const Tensor & dist = {}, const Tensor & cam_idx = {}, const Tensor & ij = {});

  // Adam over delta with the reference's betas and eps (0.9, 0.99, 1e-15), no weight decay: a decay
  // would pull the corrections to zero, i.e. back to the poses that are known to be inexact
  std::vector<torch::optim::OptimizerParamGroup> optim_param_groups(float lr);

  // [E,2] on the device: rotation angle |omega| (radians) and translation norm |tau|
  Tensor correction_norms() const;

  Tensor delta_;  // parameter "delta" [E,6], zeros
  Tensor base_;   // buffer "base" [E,3,4]
  Tensor fixed_;  // buffer "fixed" [E] i32
};
