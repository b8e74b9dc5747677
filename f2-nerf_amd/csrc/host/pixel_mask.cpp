// pixel_mask.cpp -- PixelMask, the masked pixel draw and the masked training batch (pixel_mask.hpp).
#include "pixel_mask.hpp"

#include "common.hpp"

namespace f2n
{

PixelMask PixelMask::from_mask(const Tensor & mask_in)
{
  TORCH_CHECK(mask_in.defined(), "mask is undefined");
  TORCH_CHECK(
    mask_in.is_cuda(),
    "mask must live on the GPU: the F2-NeRF hot path has no CPU implementation in this library");
  TORCH_CHECK(
    mask_in.scalar_type() == torch::kUInt8 || mask_in.scalar_type() == torch::kBool,
    "mask must be uint8 or bool");
  Tensor mask = mask_in.dim() == 2 ? mask_in.unsqueeze(0) : mask_in;
  TORCH_CHECK(mask.dim() == 3, "mask must be [E,h,w] or [h,w]");
  mask = mask.contiguous();
  TORCH_CHECK(
    mask.size(0) <= INT32_MAX && mask.size(1) <= INT32_MAX && mask.size(2) <= INT32_MAX,
    "mask too large");
  PixelMask pm;
  pm.E = mask.size(0);
  pm.h = mask.size(1);
  pm.w = mask.size(2);
  const int64_t n_words = f2n_mask_words((int)pm.E, (int)pm.h, (int)pm.w);
  TORCH_CHECK(n_words > 0, "mask must hold between 1 and 2^36 - 1 pixels");
  pm.bits = torch::empty({n_words}, int_on(mask.device()));
  pm.count = torch::empty({1}, torch::TensorOptions().dtype(torch::kInt64).device(mask.device()));
  Tensor partial = torch::empty(
    {f2n_mask_pack_workspace_words((int)pm.E, (int)pm.h, (int)pm.w)}, int_on(mask.device()));
  check(
    f2n_mask_pack(
      (const uint8_t *)mask.data_ptr(), (int)pm.E, (int)pm.h, (int)pm.w,
      (uint32_t *)pm.bits.data_ptr<int32_t>(), pm.count.data_ptr<int64_t>(),
      (uint32_t *)partial.data_ptr<int32_t>(), current_stream(mask)),
    "f2n_mask_pack");
  return pm;
}

std::tuple<Tensor, Tensor, Tensor> draw_pixels_masked(
  const PixelMask & mask, int64_t n, uint64_t seed, int attempts)
{
  TORCH_CHECK(mask.bits.defined() && mask.bits.is_cuda(), "the PixelMask is empty");
  TORCH_CHECK(n >= 0 && n <= INT32_MAX, "batch size out of range");
  const auto iopt = int_on(mask.bits.device());
  Tensor cam = torch::empty({n}, iopt), ij = torch::empty({n, 2}, iopt), tries = torch::empty({n}, iopt);
  check(
    f2n_draw_pixels_masked(
      (const uint32_t *)mask.bits.data_ptr<int32_t>(), (int)mask.E, (int)mask.h, (int)mask.w,
      (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), attempts, cam.data_ptr<int32_t>(),
      ij.data_ptr<int32_t>(), tries.data_ptr<int32_t>(), (int)n, current_stream(mask.bits)),
    "f2n_draw_pixels_masked");
  return {cam, ij, tries};
}

MaskedBatch sample_masked_rays(
  const Tensor & poses, const Tensor & intrinsics, const PixelMask & mask, int64_t batch_size,
  uint64_t seed, const Tensor & images, const Tensor & dist, int attempts)
{
  torch::NoGradGuard no_grad;
  TORCH_CHECK(poses.size(0) == mask.E, "the mask and the poses disagree on the number of images");
  MaskedBatch b;
  std::tie(b.cam, b.ij, b.tries) = draw_pixels_masked(mask, batch_size, seed, attempts);
  b.rays = get_rays_from_cameras(poses.detach(), intrinsics, b.cam, b.ij, dist);
  b.ray_weight = (b.tries > 0).to(torch::kFloat32);
  if (images.defined()) {
    TORCH_CHECK(
      images.dim() == 4 && images.size(0) == mask.E && images.size(1) == mask.h &&
        images.size(2) == mask.w && (images.size(3) == 3 || images.size(3) == 4),
      "images must be [E,h,w,3] or [E,h,w,4] with the mask's E, h, w");
    const int64_t C = images.size(3);
    Tensor ij64 = b.ij.to(torch::kLong);
    Tensor flat = (b.cam.to(torch::kLong) * mask.h + ij64.select(1, 0)) * mask.w + ij64.select(1, 1);
    Tensor px = images.contiguous().view({-1, C}).index({flat}).to(poses.device());
    b.gt = px.narrow(1, 0, 3).contiguous();
    if (C == 4) b.alpha = px.select(1, 3).contiguous();
  }
  return b;
}

}  // namespace f2n
