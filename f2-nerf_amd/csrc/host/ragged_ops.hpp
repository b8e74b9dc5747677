// ragged_ops.hpp -- the reference's free-function operator surface over ragged per-ray runs:
//   FlexOps::Sum / FlexOps::AccumulateSum          (reference src/CustomOps/FlexOps.hpp:14-20)
//   CustomOps::WeightVar                           (src/CustomOps/CustomOps.hpp:23-28)
//   CustomOps::WeightDist                          (no counterpart: the distortion loss beside it)
//   CustomOps::DepthSight                          (no counterpart: the line-of-sight depth losses)
//   CustomOps::Ssim                                (no counterpart: SSIM with a gradient, ssim.cpp)
//   CustomOps::ScatterAdd / CustomOps::ScatterIdx  (src/CustomOps/Scatter.hpp:16-21)
//   torch::autograd::TruncExp                      (src/CustomOps/CustomOps.hpp:13-19)
// Same names, argument meaning and autograd behaviour; the kernels behind them are the wave-per-ray
// HIP kernels of libf2nerf_hip.so.  Also declares the fused compositing Function the Renderer uses.
#pragma once

#include "common.hpp"

namespace torch::autograd
{

class TruncExp : public Function<TruncExp>
{
public:
  static variable_list forward(AutogradContext * ctx, Tensor input);
  static variable_list backward(AutogradContext * ctx, variable_list grad_output);
};

}  // namespace torch::autograd

namespace FlexOps
{
torch::Tensor Sum(torch::Tensor val, torch::Tensor idx_start_end);
torch::Tensor AccumulateSum(torch::Tensor val, torch::Tensor idx_start_end, bool include_this);
}  // namespace FlexOps

namespace CustomOps
{
torch::Tensor WeightVar(torch::Tensor weights, torch::Tensor idx_start_end);
// Not in the reference (it has WeightVar alone, src/CustomOps/CustomOps.cu:13-67, used at
// src/main_functions/train_manager.cpp:80-93): the interval distortion loss of mip-NeRF 360 per ray,
//   D_r = sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 dt_i,  m = t - dt / 2  ->  [n_rays]
// over the kept samples' real positions (t: interval end as the sampler gives it, dt: width; m must
// not decrease along a ray).  The gradient goes to `weights` only: t and dt are sample positions,
// which are data on every training route, and receive none.
torch::Tensor WeightDist(
  torch::Tensor weights, torch::Tensor t, torch::Tensor dt, torch::Tensor idx_start_end);
// Not in the reference either (it reads no range data; same site, src/main_functions/train_manager.cpp:80-93):
// the three line-of-sight terms of depth supervision per ray (f2n_depth_sight_fwd / _bwd),
//   (E_r, N_r, X_r) = (sum_front w^2, (1 - sum_band w)^2, (sum w m - z_r)^2)  ->  [n_rays, 3]
// with m = t - dt / 2, front: m < z - eps, band: z - eps <= m <= z + eps; z [n_rays] is the ray's
// target distance in the units of t, a ray whose z is not finite and > 0 gives zeros and no gradient.
// The gradient goes to `weights` only: t, dt and z receive none.
torch::Tensor DepthSight(
  torch::Tensor weights, torch::Tensor t, torch::Tensor dt, torch::Tensor idx_start_end,
  torch::Tensor z, double eps);
// Not in the reference, whose rgb_ssim (scripts/eval.py:29-75) is a host-side metric: the structural
// similarity of image pairs in its unclamped, differentiable form (f2n_ssim_fwd with clip = 0 /
// f2n_ssim_bwd; defined in ssim.cpp).  pred, gt [B,h,w,3] (or [h,w,3]: B = 1), h, w >= 11  ->  [B].
// The gradient goes to `pred` only.
torch::Tensor Ssim(torch::Tensor pred, torch::Tensor gt);
torch::Tensor ScatterAdd(torch::Tensor emb, torch::Tensor idx, torch::Tensor to_add);
torch::Tensor ScatterIdx(int n_all_pts, torch::Tensor idx_start_end, torch::Tensor emb_idx);
}  // namespace CustomOps

namespace f2n
{

struct CompositeOut
{
  Tensor colors;   // [n_rays, 3]
  Tensor depths;   // [n_rays]
  Tensor weights;  // [n]
};

// Fused statement of reference src/renderer.cpp:93,107-118 (density activation, alpha, exclusive
// optical-depth scan, weights, colour/depth sums, background blend), differentiable in `field_out`
// (column 0 = density logit; gradient returned dense, zero in the other columns) and `rgb`.
// `bounds_tile_samples`: the caller guarantees that the rays' [start, end) ranges tile [0, n) (the
// Renderer's own bounds do): per-sample outputs are then written whole and need no zero fill.
CompositeOut composite(
  const Tensor & field_out, const Tensor & rgb, const Tensor & dt, const Tensor & t,
  const Tensor & idx_start_end, const Tensor & bg_color, bool bounds_tile_samples = false);


struct ShadeOut
{
  Tensor logit;  // [n]    density logit = row 0 of the field head
  Tensor rgb;    // [n, 3]
};

// The per-sample network between hash encode and compositing as one kernel per direction
// (f2n_shade_fwd / f2n_shade_bwd): field head Linear(C->16), shading-feature assembly with the
// per-image appearance embedding, SH(dirs), colour MLP 32-64-3 and the scaled sigmoid
// (reference src/hash_3d_anchored.cpp:86, src/renderer.cpp:93-106, src/sh_shader.cpp:22-29).
// `enc` is the [n, C] hash encoding (channel-major storage is consumed in place); `sample_img`
// [n] int32 or undefined (no embedding).  Differentiable in enc and all seven parameter tensors.
ShadeOut shade(
  const Tensor & enc, const Tensor & dirs, const Tensor & sample_img, const Tensor & w_h,
  const Tensor & b_h, const Tensor & w1, const Tensor & b1, const Tensor & w2, const Tensor & b2,
  const Tensor & app_emb);

// The same network on the sampler's dense grid: `enc` [n_rays * S, C] in ray-major order, S % 64
// == 0, `dirs` the per-sample [n, 3] array holding the ray's direction in every sample of the ray,
// `ray_img` [n_rays] int32 or undefined.  What is the same along a ray (SH(dirs), the embedding
// row, the SH half of the hidden layer) is done once per 64 samples (f2n_shade_fwd_rays /
// f2n_shade_bwd_rays).  logit equals shade()'s bit for bit, rgb and the gradients to rounding.
// dirs_per_ray: `dirs` is [n_rays, 3], one direction per ray (f2n_shade_fwd_raydirs /
// f2n_shade_bwd_raydirs): the same kernels and, for the same directions, the same bits.  Such
// directions that carry no gradient take the per-ray constant: the forward allocates [n_rays, 80],
// runs f2n_shade_ray_const once inside its own timed operator and calls f2n_shade_fwd_rays_const,
// the backward calls f2n_shade_bwd_rays_const on the saved buffer -- the same bits again, 16 matrix
// products per stride fewer in each kernel.
ShadeOut shade_rays(
  const Tensor & enc, const Tensor & dirs, const Tensor & ray_img, int64_t S, const Tensor & w_h,
  const Tensor & b_h, const Tensor & w1, const Tensor & b1, const Tensor & w2, const Tensor & b2,
  const Tensor & app_emb, bool dirs_per_ray = false);

// F2N_OPT_DENSE_LEAN = 0: the autograd nodes between the per-ray results and the network
// (CompositeFn, WeightVarFn, WeightDistFn, DepthSightFn, the Renderer's RayUnpermuteFn) take an undefined gradient
// as undefined -- no zero tensor of n samples is made, gathered and read for it.
bool lean_grads();

// n samples form a dense [n_rays, S] grid that shade_rays serves, and no option asks for the
// per-sample kernels (F2N_OPT_SHADE_RAYS = 1, or the vector kernels of F2N_OPT_SHADE_FWD / _BWD)
bool shade_rays_applies(int64_t n, int64_t n_rays, int64_t S);

// The loss of the training iteration (reference src/main_functions/train_manager.cpp:78-96) as one
// autograd node over f2n_loss_fwd: returns [4] = {loss, color_loss, var_loss, sum of squared colour
// error}; differentiable in colors [n_rays, 3] and var [n_rays] through element 0 (the others carry no
// gradient).  loss = mean sqrt((colors-gt)^2 + 1e-4) + var_loss_weight * mean sqrt(var + 1e-2).
Tensor train_loss(
  const Tensor & colors, const Tensor & gt_colors, const Tensor & var, float var_loss_weight);

// The same loss with per-ray weights and alpha targets, as one autograd node over f2n_loss_sup_fwd
// (it stands beside the reference's src/main_functions/train_manager.cpp:78-96, which has no mask):
// returns [6] = {loss, colour, var, opacity term, weighted sum of squared colour error, sum of the ray
// weights}; differentiable in colors [n_rays, 3], var [n_rays] and opacity [n_rays] through element 0.
// opacity, ray_weight [n_rays], alpha [n_rays] and bg_color [n_rays, 3] may each be undefined:
// no weight means 1, no alpha means the plain ground truth and no opacity term; alpha needs bg_color
// (the background the render blended in) and, with opacity_weight != 0, the rendered opacity.
// gt_colors, ray_weight, alpha and bg_color get no gradient.  Both means divide by the sum of the
// weights (1 when that is not positive), formed on the device: no host read.
Tensor train_loss_sup(
  const Tensor & colors, const Tensor & gt_colors, const Tensor & var, const Tensor & opacity,
  const Tensor & ray_weight, const Tensor & alpha, const Tensor & bg_color, float var_loss_weight,
  float opacity_weight);

// C = L*F values the fused kernel is built for
inline bool shade_supported(int64_t C) { return C == 8 || C == 16 || C == 32 || C == 64; }

}  // namespace f2n
