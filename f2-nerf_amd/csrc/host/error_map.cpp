// error_map.cpp -- ErrorMap and the guided training batch (error_map.hpp).
#include "error_map.hpp"

#include "common.hpp"

namespace f2n
{

namespace
{
torch::TensorOptions i64_on(const torch::Device & d)
{
  return torch::TensorOptions().dtype(torch::kInt64).device(d);
}
}  // namespace

ErrorMap::ErrorMap(
  int64_t E_, int64_t h_, int64_t w_, const ErrorMapOptions & opt, const torch::Device & device)
: options(opt), E(E_), h(h_), w(w_)
{
  init(device);
}

ErrorMap::ErrorMap(const PixelMask & mask, const ErrorMapOptions & opt)
: options(opt), E(mask.E), h(mask.h), w(mask.w), bits(mask.bits), n_valid(mask.count)
{
  TORCH_CHECK(mask.bits.defined() && mask.bits.is_cuda(), "the PixelMask is empty");
  init(mask.bits.device());
}

void ErrorMap::init(const torch::Device & device)
{
  TORCH_CHECK(
    device.is_cuda(),
    "the error map must live on the GPU: the F2-NeRF hot path has no CPU implementation in this "
    "library");
  TORCH_CHECK(E > 0 && h > 0 && w > 0 && E <= INT32_MAX && h <= INT32_MAX && w <= INT32_MAX, "sizes");
  TORCH_CHECK(
    options.gh >= 1 && options.gw >= 1 && options.gh <= h && options.gw <= w,
    "the grid must have between 1 and h x w cells per image");
  const int64_t cells = E * options.gh * options.gw;
  TORCH_CHECK(cells < ((int64_t)1 << 24), "the error map holds fewer than 2^24 cells");
  n_cells = cells;
  const int64_t n_partial = f2n_error_cdf_workspace_words((int)n_cells);
  TORCH_CHECK(n_partial > 0, "f2n_error_cdf_workspace_words");
  value = torch::full({n_cells}, options.init_value, float_on(device));
  counts = torch::empty({n_cells}, int_on(device));
  cdf = torch::empty({n_cells}, i64_on(device));
  acc_sum = torch::zeros({n_cells}, i64_on(device));
  acc_cnt = torch::zeros({n_cells}, int_on(device));
  scan_partial_ = torch::empty({n_partial}, i64_on(device));
  if (!n_valid.defined()) n_valid = torch::full({1}, E * h * w, i64_on(device));
  check(
    f2n_mask_cell_counts(
      bits.defined() ? (const uint32_t *)bits.data_ptr<int32_t>() : nullptr, (int)E, (int)h, (int)w,
      options.gh, options.gw, counts.data_ptr<int32_t>(), current_stream(value)),
    "f2n_mask_cell_counts");
  check(
    f2n_error_cdf(
      value.data_ptr<float>(), counts.data_ptr<int32_t>(), (int)n_cells,
      (uint64_t *)cdf.data_ptr<int64_t>(), (uint64_t *)scan_partial_.data_ptr<int64_t>(),
      current_stream(value)),
    "f2n_error_cdf");
}

void ErrorMap::accumulate(
  const Tensor & colors_in, const Tensor & gt_in, const Tensor & cam_in, const Tensor & ij_in,
  const Tensor & ray_weight, const Tensor & alpha, const Tensor & bg)
{
  torch::NoGradGuard no_grad;
  const Tensor colors = dev_f32(colors_in.detach(), "colors"), gt = dev_f32(gt_in, "gt");
  const Tensor cam = dev_i32(cam_in, "cam"), ij = dev_i32(ij_in, "ij");
  const int64_t n = cam.numel();
  TORCH_CHECK(n <= INT32_MAX, "batch size out of range");
  TORCH_CHECK(
    colors.numel() == 3 * n && gt.numel() == 3 * n && ij.numel() == 2 * n,
    "accumulate: colors, gt [n,3] and ij [n,2] must match cam [n]");
  Tensor m, a, b;
  if (ray_weight.defined()) {
    m = dev_f32(ray_weight, "ray_weight");
    TORCH_CHECK(m.numel() == n, "ray_weight must be [n]");
  }
  if (alpha.defined()) {
    TORCH_CHECK(bg.defined(), "accumulate: an alpha target needs the bg the render blended in");
    a = dev_f32(alpha, "alpha");
    b = dev_f32(bg.detach(), "bg");
    TORCH_CHECK(a.numel() == n && b.numel() == 3 * n, "alpha must be [n] and bg [n,3]");
  }
  check(
    f2n_error_map_accum(
      fptr(colors), fptr(gt), fptr(a), fptr(b), fptr(m), iptr(cam), iptr(ij), (int)n, (int)E, (int)h,
      (int)w, options.gh, options.gw, (uint64_t *)acc_sum.data_ptr<int64_t>(),
      (uint32_t *)acc_cnt.data_ptr<int32_t>(), current_stream(value)),
    "f2n_error_map_accum");
}

void ErrorMap::update()
{
  check(
    f2n_error_map_apply(
      value.data_ptr<float>(), (uint64_t *)acc_sum.data_ptr<int64_t>(),
      (uint32_t *)acc_cnt.data_ptr<int32_t>(), (int)n_cells, options.decay, current_stream(value)),
    "f2n_error_map_apply");
  check(
    f2n_error_cdf(
      value.data_ptr<float>(), counts.data_ptr<int32_t>(), (int)n_cells,
      (uint64_t *)cdf.data_ptr<int64_t>(), (uint64_t *)scan_partial_.data_ptr<int64_t>(),
      current_stream(value)),
    "f2n_error_cdf");
}

GuidedDraw ErrorMap::draw(int64_t n, uint64_t seed) const
{
  TORCH_CHECK(n >= 0 && n <= INT32_MAX, "batch size out of range");
  const auto iopt = int_on(value.device());
  GuidedDraw d;
  d.cam = torch::empty({n}, iopt);
  d.ij = torch::empty({n, 2}, iopt);
  d.tries = torch::empty({n}, iopt);
  d.ray_weight = torch::empty({n}, float_on(value.device()));
  check(
    f2n_draw_pixels_guided(
      bits.defined() ? (const uint32_t *)bits.data_ptr<int32_t>() : nullptr,
      counts.data_ptr<int32_t>(), value.data_ptr<float>(), (const uint64_t *)cdf.data_ptr<int64_t>(),
      n_valid.data_ptr<int64_t>(), (int)E, (int)h, (int)w, options.gh, options.gw,
      (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), options.attempts,
      options.uniform_fraction, d.cam.data_ptr<int32_t>(), d.ij.data_ptr<int32_t>(),
      d.tries.data_ptr<int32_t>(), d.ray_weight.data_ptr<float>(), (int)n, current_stream(value)),
    "f2n_draw_pixels_guided");
  return d;
}

MaskedBatch sample_guided_rays(
  const Tensor & poses, const Tensor & intrinsics, const ErrorMap & map, int64_t batch_size,
  uint64_t seed, const Tensor & images, const Tensor & dist)
{
  torch::NoGradGuard no_grad;
  TORCH_CHECK(poses.size(0) == map.E, "the error map and the poses disagree on the number of images");
  MaskedBatch b;
  GuidedDraw d = map.draw(batch_size, seed);
  b.cam = d.cam;
  b.ij = d.ij;
  b.tries = d.tries;
  b.ray_weight = d.ray_weight;
  b.rays = get_rays_from_cameras(poses.detach(), intrinsics, b.cam, b.ij, dist);
  if (images.defined()) {
    TORCH_CHECK(
      images.dim() == 4 && images.size(0) == map.E && images.size(1) == map.h &&
        images.size(2) == map.w && (images.size(3) == 3 || images.size(3) == 4),
      "images must be [E,h,w,3] or [E,h,w,4] with the map's E, h, w");
    const int64_t C = images.size(3);
    Tensor ij64 = b.ij.to(torch::kLong);
    Tensor flat = (b.cam.to(torch::kLong) * map.h + ij64.select(1, 0)) * map.w + ij64.select(1, 1);
    Tensor px = images.contiguous().view({-1, C}).index({flat}).to(poses.device());
    b.gt = px.narrow(1, 0, 3).contiguous();
    if (C == 4) b.alpha = px.select(1, 3).contiguous();
  }
  return b;
}

}  // namespace f2n
