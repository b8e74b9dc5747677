// intrinsics_refiner.hpp -- IntrinsicsRefiner: a shared correction of fx, fy, cx, cy, k1, k2, p1, p2
// per physical camera, refined while the field trains; the other half of the camera optimiser that
// PoseRefiner (pose_refiner.hpp) begins.
//
// The reference reads the calibration per image from cams_meta.tsv (src/dataset.cpp:59-63) and takes
// it as exact.  With a focal length a percent off, a pose optimiser absorbs the error as a wrong
// translation along the optical axis.  Here image e belongs to the physical camera g = group[e], and
// each camera has eight dimensionless numbers c = gamma[g]:
//   fx' = fx exp(c0)   fy' = fy exp(c1)   cx' = cx + c2 fx   cy' = cy + c3 fy      (base fx, fy)
//   k1' = k1 + c4      k2' = k2 + c5      p1' = p1 + c6      p2' = p2 + c7         (f2n_intr_compose)
// The rays of a batch reach gamma through f2n_cam_intr_grad (one sum per image, no atomics) and
// f2n_intr_compose_bwd (one sum per camera).  With gamma zero the calibration, the rays and a training
// step are bit for bit those without the refiner.
//
// Like PoseRefiner it is not part of Renderer: renderer.pt keeps the reference's layout, and the
// refiner is saved and loaded on its own (torch::save / torch::load of the module).
//
//   renderer.options_.fused_ray_grad = true;
//   auto [rays, gt, cam] = calib.sample_random_rays(pose_refiner.poses(), h, w, n, images);
//   f2n::train_step(renderer, rays.origins, rays.dirs, cam, gt, terms);   // a f2n::LossTerms
//   field_adam.step();  pose_adam.step();  calib_adam.step();
#pragma once

#include <torch/torch.h>

#include <array>
#include <tuple>
#include <vector>

#include "rays.hpp"

// {K' [E,3,3], dist' [E,4]} = f2n_intr_compose(base_K [E,3,3], base_dist [E,4] or undefined = zeros,
// gamma [G,8], group [E] i32), differentiable in gamma alone (f2n_intr_compose_bwd, with the columns
// that learn [8] i32 marks 0 left without a gradient; undefined = all learned).  group must lie below
// G: checked here with one host read (IntrinsicsRefiner checks once, when it is built).
std::tuple<torch::Tensor, torch::Tensor> intr_compose(
  const torch::Tensor & base_K, const torch::Tensor & base_dist, const torch::Tensor & gamma,
  const torch::Tensor & group, const torch::Tensor & learn = {});
// d_gamma [G,8] of d_K [E,3,3] and d_dist [E,4] (either may be undefined = zeros): the backward entry
// on its own
torch::Tensor intr_compose_bwd(
  const torch::Tensor & base_K, const torch::Tensor & base_dist, const torch::Tensor & gamma,
  const torch::Tensor & group, const torch::Tensor & learn, const torch::Tensor & d_K,
  const torch::Tensor & d_dist);

class IntrinsicsRefiner : public torch::nn::Module
{
  using Tensor = torch::Tensor;

public:
  // base_intrinsics [E,3,3]; base_dist [E,4] or undefined (pinhole cameras: zeros); group [E] integer,
  // the physical camera of each image, or undefined: one camera took them all
  explicit IntrinsicsRefiner(
    const Tensor & base_intrinsics, const Tensor & base_dist = {}, const Tensor & group = {});

  int64_t n_images() const { return base_K_.size(0); }
  int64_t n_groups() const { return gamma_.size(0); }
  // the effective calibration, differentiable in gamma: [E,3,3] and [E,4]
  Tensor intrinsics() const { return std::get<0>(calibration()); }
  Tensor dist() const { return std::get<1>(calibration()); }
  // both from one f2n_intr_compose launch
  std::tuple<Tensor, Tensor> calibration() const;

  // which of (fx, fy, cx, cy, k1, k2, p1, p2) are learned; the others keep a zero gradient, so Adam
  // leaves them where they are
  void set_learned(const std::array<bool, 8> & mask);
  // mask [E] (bool or integer): images whose calibration stays the base one
  void set_fixed(const Tensor & mask);

  // PoseRefiner::sample_random_rays with rays that carry a gradient to gamma (and to `poses`, when
  // they require one: pass pose_refiner.poses() to train both).  Cameras are drawn on the device and
  // sorted before the pixels are drawn; cam_idx [n] i32 and ij [n,2] i32, when given, replace the
  // draws.  poses [E,3|4,4].  images: optional [E,h,w,3].
  // Returns {rays, gt_colors [n,3] (undefined without images), cam_indices [n] i32}.
  std::tuple<Rays, Tensor, Tensor> sample_random_rays(
    const Tensor & poses, int h, int w, int64_t batch_size, const Tensor & images = {},
    const Tensor & cam_idx = {}, const Tensor & ij = {});

  // Adam over gamma with the reference's betas and eps (0.9, 0.99, 1e-15), no weight decay: a decay
  // would pull the calibration back to the one that is known to be inexact
  std::vector<torch::optim::OptimizerParamGroup> optim_param_groups(float lr);

  // [E,8] on the device: effective minus base (fx, fy, cx, cy, k1, k2, p1, p2)
  Tensor corrections() const;

  Tensor gamma_;      // parameter "gamma" [G,8], zeros
  Tensor base_K_;     // buffer "base_K" [E,3,3]
  Tensor base_dist_;  // buffer "base_dist" [E,4]
  Tensor group_;      // buffer "group" [E] i32: g, or -1 - g for a fixed image of camera g
  Tensor learn_;      // buffer "learn" [8] i32
};
