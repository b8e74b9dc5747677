// occupancy_grid.cpp -- see occupancy_grid.hpp.
#include "occupancy_grid.hpp"

using Tensor = torch::Tensor;

OccupancyGrid::OccupancyGrid(int64_t resolution, torch::Device device) : G_(resolution)
{
  TORCH_CHECK(
    G_ >= 32 && G_ <= 256 && (G_ & (G_ - 1)) == 0,
    "OccupancyGrid: resolution must be a power of two in 32..256, got ", G_);
  const int64_t cells = G_ * G_ * G_;
  words_ = torch::full({cells / 32}, -1, f2n::int_on(device));  // all ones: nothing skipped
  density_ = torch::zeros({cells}, f2n::float_on(device));
}

void OccupancyGrid::update(Hash3DAnchored & field, float threshold, float decay, const Tensor & probe)
{
  torch::NoGradGuard no_grad;
  TORCH_CHECK(words_.is_cuda(), "OccupancyGrid::update: the grid must live on the GPU");
  const int64_t cells = G_ * G_ * G_;
  Tensor u;
  if (probe.defined()) {
    TORCH_CHECK(probe.numel() == cells * 3, "OccupancyGrid::update: probe must be [G,G,G,3]");
    u = f2n::dev_f32(probe.detach(), "probe");
  }
  Tensor table16 = field.table_f16();
  const f2n::FieldArgs g = field.kernel_args(table16);
  auto head = field.density_head();
  f2n::check(
    f2n_occ_update(
      g.table, g.primes, g.bias, g.mul, head.first.data_ptr<float>(), head.second.data_ptr<float>(),
      f2n::fptr(u), density_.data_ptr<float>(),
      reinterpret_cast<uint32_t *>(words_.data_ptr<int32_t>()), (int)G_, g.L_walk, g.F, g.T,
      g.level_stride, 3.f, threshold, decay, f2n::current_stream(words_)),
    "f2n_occ_update");
  if (allowed_.defined()) words_.bitwise_and_(allowed_);
}

void OccupancyGrid::set_bits(const Tensor & occupied)
{
  const int64_t cells = G_ * G_ * G_;
  TORCH_CHECK(
    occupied.scalar_type() == torch::kBool && occupied.numel() == cells,
    "OccupancyGrid::set_bits: bool [G,G,G]");
  // bit j of word w = cell 32 w + j; the sum is < 2^32 and wraps into the int32 word
  Tensor shifts = torch::arange(32, torch::TensorOptions().dtype(torch::kInt64).device(words_.device()));
  Tensor packed =
    torch::bitwise_left_shift(
      occupied.to(words_.device()).reshape({cells / 32, 32}).to(torch::kInt64), shifts)
      .sum(1);
  packed = torch::where(packed >= (int64_t(1) << 31), packed - (int64_t(1) << 32), packed);
  words_.copy_(packed.to(torch::kInt32));
  if (allowed_.defined()) words_.bitwise_and_(allowed_);
}

void OccupancyGrid::set_allowed(const Tensor & words)
{
  torch::NoGradGuard no_grad;
  TORCH_CHECK(
    words.defined() && words.scalar_type() == torch::kInt32 && words.numel() == words_.numel(),
    "OccupancyGrid::set_allowed: int32 [G^3 / 32] words");
  allowed_ = words.detach().to(words_.device()).reshape({words_.numel()}).clone();
  words_.bitwise_and_(allowed_);
}

void OccupancyGrid::carve_to_cameras(
  const Tensor & poses, const Tensor & intrinsics, int64_t h, int64_t w,
  f2n::VisibilityOptions opts, const Tensor & dist, const f2n::PixelMask * mask)
{
  opts.resolution = G_;
  set_allowed(f2n::camera_visibility(poses, intrinsics, h, w, opts, dist, mask));
}

Tensor OccupancyGrid::bits() const
{
  Tensor shifts = torch::arange(32, torch::TensorOptions().dtype(torch::kInt64).device(words_.device()));
  Tensor w = words_.to(torch::kInt64).unsqueeze(1);
  return torch::bitwise_and(torch::bitwise_right_shift(w, shifts), 1).ne(0).reshape({G_, G_, G_});
}

Tensor OccupancyGrid::occupied(const Tensor & points) const
{
  TORCH_CHECK(words_.is_cuda(), "OccupancyGrid::occupied: the grid must live on the GPU");
  TORCH_CHECK(points.dim() == 2 && points.size(1) == 3, "OccupancyGrid::occupied: points must be [n, 3]");
  const Tensor pts = f2n::dev_f32(points.detach(), "points");
  const int64_t n = pts.size(0);
  Tensor out = torch::empty({n}, torch::TensorOptions().dtype(torch::kUInt8).device(pts.device()));
  f2n::check(
    f2n_occ_lookup(
      pts.data_ptr<float>(), n, words_ptr(), (int)G_, out.data_ptr<uint8_t>(),
      f2n::current_stream(pts)),
    "f2n_occ_lookup");
  return out.to(torch::kBool);
}

double OccupancyGrid::fraction() const { return bits().to(torch::kFloat32).mean().item<double>(); }
