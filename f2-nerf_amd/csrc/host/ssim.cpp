// ssim.cpp -- see ssim.hpp; CustomOps::Ssim (ragged_ops.hpp) is defined here, beside its kernels' host.
#include "ssim.hpp"

#include "common.hpp"
#include "ragged_ops.hpp"

using Tensor = torch::Tensor;

namespace
{

struct ImagePair
{
  Tensor pred, gt;  // [B,h,w,3] f32, contiguous, on the GPU
  int64_t B, h, w;
};

ImagePair image_pair(const Tensor & pred_in, const Tensor & gt_in, const char * what)
{
  Tensor pred = f2n::dev_f32(pred_in, "pred"), gt = f2n::dev_f32(gt_in, "gt");
  if (pred.dim() == 3) pred = pred.unsqueeze(0);
  if (gt.dim() == 3) gt = gt.unsqueeze(0);
  TORCH_CHECK(
    pred.dim() == 4 && pred.size(3) == 3 && pred.sizes() == gt.sizes(), what,
    ": pred and gt must both be [B,h,w,3] or [h,w,3]");
  TORCH_CHECK(
    pred.size(0) <= 65535 && pred.size(1) >= 11 && pred.size(2) >= 11 &&
      pred.size(1) <= INT32_MAX && pred.size(2) <= INT32_MAX,
    what, ": at most 65535 images, of 11 x 11 pixels or more");
  return {pred, gt, pred.size(0), pred.size(1), pred.size(2)};
}

// f2n_ssim_fwd on a checked pair -> ssim [B]; map / gmaps are filled where asked for
Tensor ssim_forward(const ImagePair & p, bool clip, Tensor * map, Tensor * gmaps)
{
  const auto fopt = p.pred.options();
  Tensor out = torch::empty({p.B}, fopt);
  if (map) *map = torch::empty({p.B, p.h - 10, p.w - 10, 3}, fopt);
  if (gmaps) *gmaps = torch::empty({p.B, p.h - 10, p.w - 10, 9}, fopt);
  if (p.B == 0) return out;
  Tensor partial = torch::empty(
    {f2n_ssim_workspace_doubles((int)p.B, (int)p.h, (int)p.w)}, fopt.dtype(torch::kFloat64));
  f2n::check(
    f2n_ssim_fwd(
      p.pred.data_ptr<float>(), p.gt.data_ptr<float>(), (int)p.B, (int)p.h, (int)p.w, clip ? 1 : 0,
      out.data_ptr<float>(), map ? map->data_ptr<float>() : nullptr,
      gmaps ? gmaps->data_ptr<float>() : nullptr, partial.data_ptr<double>(),
      f2n::current_stream(p.pred)),
    "f2n_ssim_fwd");
  return out;
}

// ssim [B] of the unclamped form, differentiable in pred.  The forward leaves the three partial maps
// per channel (gmaps) for the backward, which filters them and recomputes nothing.
class SsimFn : public torch::autograd::Function<SsimFn>
{
public:
  static Tensor forward(torch::autograd::AutogradContext * ctx, Tensor pred, Tensor gt)
  {
    const ImagePair p = image_pair(pred, gt.detach(), "CustomOps::Ssim");
    Tensor gmaps;
    Tensor out = ssim_forward(p, false, nullptr, &gmaps);
    ctx->save_for_backward({p.pred, p.gt, gmaps});
    ctx->saved_data["squeeze"] = pred.dim() == 3;
    ctx->set_materialize_grads(false);
    return out;
  }

  static torch::autograd::variable_list backward(
    torch::autograd::AutogradContext * ctx, torch::autograd::variable_list grad)
  {
    if (!grad[0].defined()) return {Tensor(), Tensor()};
    auto sv = ctx->get_saved_variables();
    const Tensor &pred = sv[0], &gt = sv[1], &gmaps = sv[2];
    Tensor d_ssim = f2n::dev_f32(grad[0], "CustomOps::Ssim grad");
    TORCH_CHECK(d_ssim.numel() == pred.size(0), "CustomOps::Ssim grad must be [B]");
    Tensor d_pred = torch::empty_like(pred);
    if (pred.size(0) > 0)
      f2n::check(
        f2n_ssim_bwd(
          pred.data_ptr<float>(), gt.data_ptr<float>(), gmaps.data_ptr<float>(),
          d_ssim.data_ptr<float>(), (int)pred.size(0), (int)pred.size(1), (int)pred.size(2),
          d_pred.data_ptr<float>(), f2n::current_stream(pred)),
        "f2n_ssim_bwd");
    if (ctx->saved_data["squeeze"].toBool()) d_pred = d_pred.squeeze(0);
    return {d_pred, Tensor()};
  }
};

}  // namespace

Tensor CustomOps::Ssim(Tensor pred, Tensor gt) { return SsimFn::apply(pred, gt); }

namespace f2n
{

SsimOut ssim(const Tensor & pred, const Tensor & gt, bool clip, bool want_map)
{
  torch::NoGradGuard no_grad;
  const ImagePair p = image_pair(pred.detach(), gt.detach(), "f2n::ssim");
  SsimOut out;
  out.ssim = ssim_forward(p, clip, want_map ? &out.map : nullptr, nullptr);
  return out;
}

ImageScores image_scores(const Tensor & pred, const Tensor & gt)
{
  torch::NoGradGuard no_grad;
  const ImagePair p = image_pair(pred.detach(), gt.detach(), "f2n::image_scores");
  const Tensor diff = p.pred - p.gt;
  const Tensor per_pixel = (diff * diff).mean(-1);  // [B,h,w]
  ImageScores s;
  s.mse = per_pixel.mean({1, 2});
  s.psnr = -10.f * torch::log10(s.mse);
  s.score = (double)(p.h * p.w) / (per_pixel.sum({1, 2}) + 1e-6f);
  const ImagePair clamped{p.pred.clamp(0.f, 1.f), p.gt.clamp(0.f, 1.f), p.B, p.h, p.w};
  s.ssim = ssim_forward(clamped, true, nullptr, nullptr);
  return s;
}

PatchDraw draw_patches(
  int64_t E, int64_t h, int64_t w, int64_t n_patches, int64_t P, uint64_t seed,
  const PixelMask & mask, int attempts, const torch::Device & device)
{
  const bool masked = mask.bits.defined();
  TORCH_CHECK(
    !masked || (mask.bits.is_cuda() && mask.E == E && mask.h == h && mask.w == w),
    "draw_patches: the mask and E, h, w disagree");
  TORCH_CHECK(
    E >= 1 && E <= INT32_MAX && h <= INT32_MAX && w <= INT32_MAX && n_patches >= 0 && P >= 11 &&
      P <= std::min(h, w) && n_patches * P * P <= INT32_MAX,
    "draw_patches: patches of 11 .. min(h, w) pixels a side, and fewer than 2^31 rays");
  const auto iopt = int_on(masked ? mask.bits.device() : device);
  PatchDraw d;
  d.cam = torch::empty({n_patches * P * P}, iopt);
  d.ij = torch::empty({n_patches * P * P, 2}, iopt);
  d.tries = torch::empty({n_patches}, iopt);
  d.patch_weight = torch::empty({n_patches}, iopt.dtype(torch::kFloat32));
  if (n_patches == 0) return d;
  check(
    f2n_draw_patches(
      masked ? (const uint32_t *)mask.bits.data_ptr<int32_t>() : nullptr, (int)E, (int)h, (int)w,
      (int)n_patches, (int)P, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), attempts,
      d.cam.data_ptr<int32_t>(), d.ij.data_ptr<int32_t>(), d.tries.data_ptr<int32_t>(),
      d.patch_weight.data_ptr<float>(), current_stream(d.cam)),
    "f2n_draw_patches");
  return d;
}

PatchBatch sample_patch_rays(
  const Tensor & poses, const Tensor & intrinsics, int64_t h, int64_t w, int64_t n_patches,
  int64_t P, uint64_t seed, const Tensor & images, const PixelMask & mask, const Tensor & dist,
  int attempts)
{
  torch::NoGradGuard no_grad;
  const int64_t E = poses.size(0);
  PatchDraw d = draw_patches(E, h, w, n_patches, P, seed, mask, attempts, poses.device());
  PatchBatch out;
  MaskedBatch & b = out.batch;
  b.cam = d.cam;
  b.ij = d.ij;
  b.tries = d.tries;
  out.patch_weight = d.patch_weight;
  b.rays = get_rays_from_cameras(poses.detach(), intrinsics, b.cam, b.ij, dist);
  // (expand + reshape: repeat_interleave would read its output size back)
  b.ray_weight = d.patch_weight.unsqueeze(1).expand({n_patches, P * P}).reshape({-1});
  if (images.defined()) {
    TORCH_CHECK(
      images.dim() == 4 && images.size(0) == E && images.size(1) == h && images.size(2) == w &&
        (images.size(3) == 3 || images.size(3) == 4),
      "images must be [E,h,w,3] or [E,h,w,4] with the poses' E and the given h, w");
    const int64_t C = images.size(3);
    Tensor ij64 = b.ij.to(torch::kLong);
    Tensor flat = (b.cam.to(torch::kLong) * h + ij64.select(1, 0)) * w + ij64.select(1, 1);
    Tensor px = images.contiguous().view({-1, C}).index({flat}).to(poses.device());
    b.gt = px.narrow(1, 0, 3).contiguous();
    if (C == 4) b.alpha = px.select(1, 3).contiguous();
  }
  return out;
}

}  // namespace f2n
