// occ_visibility.cpp -- see occ_visibility.hpp.
#include "occ_visibility.hpp"

#include <cmath>

#include "common.hpp"

using Tensor = torch::Tensor;

namespace
{

// the checked inputs of one carve, as the entries take them
struct Carve
{
  Tensor poses, K, dist;
  const f2n::PixelMask * mask;
  int pose_ld, n_cams, h, w, stride, n_steps, dilate, G;
  float step;
  void * stream;

  const uint32_t * mask_bits() const
  {
    return mask ? reinterpret_cast<const uint32_t *>(mask->bits.data_ptr<int32_t>()) : nullptr;
  }
};

uint32_t * words_of(Tensor & t) { return reinterpret_cast<uint32_t *>(t.data_ptr<int32_t>()); }

Carve checked(
  const Tensor & poses, const Tensor & intrinsics, int64_t h, int64_t w,
  const f2n::VisibilityOptions & o, const Tensor & dist, const f2n::PixelMask * mask)
{
  TORCH_CHECK(
    poses.dim() == 3 && poses.size(2) == 4 && (poses.size(1) == 3 || poses.size(1) == 4),
    "camera_visibility: poses must be [n,3,4] or [n,4,4]");
  Carve c;
  c.poses = f2n::dev_f32(poses.detach(), "poses");
  const int64_t n = poses.size(0);
  TORCH_CHECK(n < (int64_t(1) << 31), "camera_visibility: too many cameras");
  c.pose_ld = (int)(poses.size(1) * 4);
  c.n_cams = (int)n;
  TORCH_CHECK(intrinsics.numel() == n * 9, "camera_visibility: intrinsics must be [n,3,3]");
  c.K = f2n::dev_f32(intrinsics.detach(), "intrinsics");
  TORCH_CHECK(c.K.device() == c.poses.device(), "intrinsics must be on the poses' device");
  if (dist.defined()) {
    TORCH_CHECK(
      dist.numel() == n * 4 && dist.size(-1) == 4,
      "dist must hold (k1, k2, p1, p2) for each of the ", n, " cameras");
    c.dist = f2n::dev_f32(dist.detach(), "dist");
    TORCH_CHECK(c.dist.device() == c.poses.device(), "dist must be on the poses' device");
  }
  TORCH_CHECK(
    h >= 1 && w >= 1 && h < (int64_t(1) << 31) && w < (int64_t(1) << 31),
    "camera_visibility: h and w must be positive");
  c.h = (int)h;
  c.w = (int)w;
  c.mask = mask;
  if (mask) {
    TORCH_CHECK(
      mask->E == n && mask->h == h && mask->w == w,
      "camera_visibility: the mask must cover the same ", n, " images of ", h, " x ", w, " pixels");
    TORCH_CHECK(mask->bits.device() == c.poses.device(), "the mask must be on the poses' device");
  }
  const int64_t G = o.resolution;
  TORCH_CHECK(
    G >= 32 && G <= 256 && (G & (G - 1)) == 0,
    "camera_visibility: resolution must be a power of two in 32..256, got ", G);
  c.G = (int)G;
  TORCH_CHECK(o.pixel_stride >= 1, "camera_visibility: pixel_stride must be at least 1");
  c.stride = o.pixel_stride;
  c.n_steps =
    o.n_steps < 0 ? (int)std::ceil(1.5 * (double)PtsSamplerOptions().max_samples) : o.n_steps;
  TORCH_CHECK(
    c.n_steps >= 1 && c.n_steps <= 65536, "camera_visibility: n_steps must be in 1..65536");
  TORCH_CHECK(
    o.step > 0.f && std::isfinite(o.step), "camera_visibility: step must be positive and finite");
  c.step = o.step;
  TORCH_CHECK(
    o.min_views >= 1 && o.min_views <= 255, "camera_visibility: min_views must be in 1..255");
  TORCH_CHECK(
    o.dilate >= 0 && o.dilate <= 2, "camera_visibility: dilate must be 0, 1 or 2, got ", o.dilate);
  c.dilate = o.dilate;
  // the soundness argument of occ_visibility.hpp: a TRAIN sample is within step / 2 of a marked one
  TORCH_CHECK(
    c.dilate == 0 || 0.5 * (double)c.step <= 4.0 / (double)G,
    "camera_visibility: with dilate >= 1 half a step (", 0.5 * (double)c.step,
    ") must not exceed a cell (", 4.0 / (double)G, ")");
  c.stream = f2n::current_stream(c.poses);
  return c;
}

// bits |= marks of cameras [first, first + n)
void mark(const Carve & c, int first, int n, Tensor & bits)
{
  f2n::check(
    f2n_occ_mark_rays(
      c.poses.data_ptr<float>(), c.pose_ld, c.K.data_ptr<float>(), f2n::fptr(c.dist), first, n, c.h,
      c.w, c.stride, c.mask_bits(), c.n_steps, c.step, words_of(bits), c.G, c.stream),
    "f2n_occ_mark_rays");
}

// dilate^d of a: the result is a or b, whichever the last pass wrote
Tensor & dilated(const Carve & c, Tensor & a, Tensor & b)
{
  Tensor * src = &a;
  Tensor * dst = &b;
  for (int d = 0; d < c.dilate; d++) {
    f2n::check(f2n_occ_dilate(words_of(*src), words_of(*dst), c.G, c.stream), "f2n_occ_dilate");
    std::swap(src, dst);
  }
  return *src;
}

Tensor view_counts(const Carve & c)
{
  const int64_t cells = (int64_t)c.G * c.G * c.G;
  const torch::Device dev = c.poses.device();
  Tensor count = torch::zeros({cells}, torch::TensorOptions().dtype(torch::kUInt8).device(dev));
  Tensor a = torch::empty({cells / 32}, f2n::int_on(dev)), b = torch::empty_like(a);
  for (int cam = 0; cam < c.n_cams; cam++) {
    a.zero_();
    mark(c, cam, 1, a);
    Tensor & seen = dilated(c, a, b);
    f2n::check(
      f2n_occ_count_add(words_of(seen), count.data_ptr<uint8_t>(), c.G, c.stream),
      "f2n_occ_count_add");
  }
  return count;
}

}  // namespace

namespace f2n
{

Tensor camera_view_counts(
  const Tensor & poses, const Tensor & intrinsics, int64_t h, int64_t w,
  const VisibilityOptions & opts, const Tensor & dist, const PixelMask * mask)
{
  torch::NoGradGuard no_grad;
  const Carve c = checked(poses, intrinsics, h, w, opts, dist, mask);
  return view_counts(c).view({c.G, c.G, c.G});
}

Tensor camera_visibility(
  const Tensor & poses, const Tensor & intrinsics, int64_t h, int64_t w,
  const VisibilityOptions & opts, const Tensor & dist, const PixelMask * mask)
{
  torch::NoGradGuard no_grad;
  const Carve c = checked(poses, intrinsics, h, w, opts, dist, mask);
  const int64_t cells = (int64_t)c.G * c.G * c.G;
  if (opts.min_views == 1) {  // dilate^d of the union: every camera in one launch
    Tensor a = torch::zeros({cells / 32}, int_on(c.poses.device())), b = torch::empty_like(a);
    mark(c, 0, c.n_cams, a);
    return dilated(c, a, b);
  }
  Tensor count = view_counts(c);
  Tensor bits = torch::empty({cells / 32}, int_on(c.poses.device()));
  check(
    f2n_occ_count_bits(count.data_ptr<uint8_t>(), opts.min_views, words_of(bits), c.G, c.stream),
    "f2n_occ_count_bits");
  return bits;
}

}  // namespace f2n
