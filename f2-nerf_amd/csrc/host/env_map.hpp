// env_map.hpp -- f2n::EnvMap: a learned background, a cube map of colour logits looked up by ray
// direction (f2n_envmap_fwd / f2n_envmap_bwd / f2n_envmap_grad_apply; include/f2nerf_hip.h has the
// layout and envmap.hip the evaluation order).
//
// The reference has no such model: its render blends a constant behind the field
// (src/renderer.cpp:103-110: rand in TRAIN, 0.5 otherwise), so the sky of every rendered outdoor view
// is flat grey.  With a map attached (Renderer::set_background) every render that is not handed a
// bg_color blends query(rays_d) instead, and the colour loss trains the texture through
// d colours / d bg = the transmittance left behind the field.  A texture of zeros is 0.5f exactly:
// an attached, untrained map renders what the renderer renders without one in inference.
//
// Like PoseRefiner and OccupancyGrid it is not part of Renderer: renderer.pt keeps the reference's
// layout, and the map is saved and loaded on its own (torch::save / torch::load of the module).
//
// The gradient goes to the texture only.  Directions get none: pose optimisation through the sky
// is out of scope.
//
//   auto env = std::make_shared<f2n::EnvMap>(128, device);
//   renderer.set_background(env);
//   f2n::LossTerms terms;  terms.sup.alpha = alpha;  terms.sup.opacity_weight = 1e-2f;
//   terms.sup.composite_target = false;           // the colour target is the image, sky included
//   f2n::train_step(renderer, o, d, cam, gt, terms, noise);   // bg_color left undefined
//   field_adam.step();  sky_adam.step();          // sky_adam over env->optim_param_groups(lr)
#pragma once

#include <torch/torch.h>

#include <vector>

namespace f2n
{

// bg [n,3] = f2n_envmap_fwd(dirs [n,3], texture [6,R,R,3]); nothing is recorded by autograd
torch::Tensor envmap_query(const torch::Tensor & dirs, const torch::Tensor & texture);
// f2n_envmap_bwd on its own: adds the fixed-point contributions of d_bg [n,3] to acc (int64
// [6*R*R*3]) and ors into flags (int32 [1]); bg is envmap_query's output for the same dirs
void envmap_bwd(
  const torch::Tensor & dirs, const torch::Tensor & bg, const torch::Tensor & d_bg, int64_t R,
  torch::Tensor acc, torch::Tensor flags);
// f2n_envmap_grad_apply on its own: d_tex [6,R,R,3] (+)= acc * 2^-48, acc = 0
void envmap_grad_apply(torch::Tensor acc, int64_t R, torch::Tensor d_tex, bool accumulate);

class EnvMap : public torch::nn::Module
{
  using Tensor = torch::Tensor;

public:
  // resolution R of a face, 2 .. 4096
  explicit EnvMap(int64_t resolution, const torch::Device & device);

  int64_t resolution() const { return texture_.size(1); }

  // bg [n,3] of dirs [n,3] (any length), differentiable in the texture: one autograd node, the
  // forward one launch, the backward f2n_envmap_bwd + f2n_envmap_grad_apply.  dirs get no gradient.
  Tensor query(const Tensor & dirs);

  // Adam over the texture with the reference's betas and eps (0.9, 0.99, 1e-15), no weight decay:
  // a decay would pull the logits to zero, i.e. the sky back to the grey it is there to replace
  std::vector<torch::optim::OptimizerParamGroup> optim_param_groups(float lr);

  // what the backwards since the last call reported: bit 0 a gradient that was not finite was
  // dropped, bit 1 a contribution was capped.  The one host read of the class; resets the flags.
  int flags();

  Tensor texture_;  // parameter "texture" [6,R,R,3], zeros
  // not registered (they stay out of the file): the fixed-point sums, zero between backwards, and
  // the flags word
  Tensor acc_;    // int64 [6*R*R*3]
  Tensor flags_;  // int32 [1]
};

}  // namespace f2n
