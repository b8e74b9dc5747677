// robust_loss.hpp -- the weights of a trimmed colour loss: the rays of a batch whose colour residual
// the static field cannot explain (moving cars, pedestrians, wipers, the ego vehicle's shadow) are
// dropped from the loss without anybody supplying a mask.  The recipe is RobustNeRF's (Sabour et al.,
// CVPR 2023, section 3.2): keep the residuals below a quantile, then smooth that inlier mask over
// image patches.  The reference has no such loss (src/main_functions/train_manager.cpp:78-96).
#pragma once

#include <torch/torch.h>

namespace f2n
{

// quantile >= 1: off.  The defaults of the other fields are the paper's: half of the 3 x 3 window,
// 0.6 of a block of 8 x 8 inside patches of 16 x 16.  The schedule of the quantile, if any, stays with
// the caller.
struct RobustLoss
{
  float quantile = 1.f;     // the share of the considered rays kept by the residual alone
  float box_thresh = .5f;   // step 5: the share of inliers in the 3 x 3 window that restores a pixel
  float nbhd_thresh = .6f;  // step 6: the share of restored pixels that restores a whole block
  int patch = 0;            // P: the rays are n_patches * P^2, patch-major; 0: scattered rays
  int nbhd = 8;             // the side of a block; clamped to P
  bool active() const { return !(quantile >= 1.f); }
};

struct RobustWeights
{
  torch::Tensor weight;  // [n] f32: m_r where the ray is an inlier, else +0
  torch::Tensor omega;   // [n] u8: the 0/1 label itself
  torch::Tensor stats;   // [4] f32: {T, N_c, sum of the pixel labels, sum of the final labels}
};

// f2n_robust_weights (include/f2nerf_hip.h has the rule): colors, target [n, 3] f32 on the GPU,
// ray_weight [n] or undefined (= 1).  One launch for scattered rays, three for patches; no host read,
// so a captured step stays capturable.  A quantile >= 1 is taken as 1 here: every considered ray with
// a finite residual is an inlier.  Not differentiated.
RobustWeights robust_weights(
  const torch::Tensor & colors, const torch::Tensor & target, const torch::Tensor & ray_weight,
  const RobustLoss & opt);

}  // namespace f2n
