// depth_targets.cpp -- see depth_targets.hpp.
#include "depth_targets.hpp"

namespace f2n
{

Tensor splat_depth(
  const Tensor & points, const Tensor & cam_idx, const Tensor & poses_in, const Tensor & intrinsics,
  const Tensor & dist, int h, int w)
{
  Tensor pts = dev_f32(points, "points");
  TORCH_CHECK(pts.dim() == 2 && pts.size(1) == 3, "points must be [N,3]");
  const int64_t n = pts.size(0);
  Tensor cam = dev_i32(cam_idx, "cam_idx");
  TORCH_CHECK(cam.dim() == 1 && cam.size(0) == n, "cam_idx must be [N]");
  TORCH_CHECK(
    poses_in.dim() == 3 && poses_in.size(2) == 4 && (poses_in.size(1) == 3 || poses_in.size(1) == 4),
    "poses must be [E,3,4] or [E,4,4]");
  Tensor poses = dev_f32(poses_in.detach(), "poses");
  const int pose_ld = (int)(poses.size(1) * 4);
  const int64_t E = poses.size(0);
  Tensor K = dev_f32(intrinsics, "intrinsics");
  TORCH_CHECK(
    K.dim() == 3 && K.size(0) == E && K.size(1) == 3 && K.size(2) == 3,
    "intrinsics must be [E,3,3] with the poses' E");
  Tensor D;
  if (dist.defined()) {
    TORCH_CHECK(
      dist.numel() == E * 4 && dist.size(-1) == 4,
      "dist must hold (k1, k2, p1, p2) for each of the ", E, " cameras");
    D = dev_f32(dist.detach(), "dist").view({E, 4});
  }
  TORCH_CHECK(
    poses.device() == pts.device() && K.device() == pts.device() && cam.device() == pts.device() &&
      (!D.defined() || D.device() == pts.device()),
    "points, cam_idx, poses, intrinsics and dist must be on the same device");
  TORCH_CHECK(E >= 1 && h >= 1 && w >= 1, "splat_depth: at least one camera and a positive image size");
  TORCH_CHECK(E * (int64_t)h * w < ((int64_t)1 << 31), "splat_depth: E * h * w must stay below 2^31");
  Tensor depth = torch::empty({E, h, w}, pts.options());
  check(
    f2n_depth_splat(
      fptr(pts), iptr(cam), poses.data_ptr<float>(), pose_ld, K.data_ptr<float>(), fptr(D), E, h, w,
      depth.data_ptr<float>(), n, current_stream(pts)),
    "f2n_depth_splat");
  return depth;
}

Tensor gather_depth(const Tensor & depth_maps, const Tensor & cam_idx, const Tensor & ij)
{
  TORCH_CHECK(depth_maps.dim() == 3, "depth_maps must be [E,h,w]");
  TORCH_CHECK(ij.dim() == 2 && ij.size(1) == 2, "ij must be [n,2]");
  TORCH_CHECK(cam_idx.dim() == 1 && cam_idx.size(0) == ij.size(0), "cam_idx must be [n]");
  const int64_t h = depth_maps.size(1), w = depth_maps.size(2);
  const Tensor i = ij.select(1, 0).to(torch::kLong), j = ij.select(1, 1).to(torch::kLong);
  const Tensor cam = cam_idx.to(torch::kLong);
  // a camera, row or column outside the maps is "no return" (0), never another pixel's value: the
  // index is clamped into range for the read and the result selected, on the device, without a host read
  const int64_t E = depth_maps.size(0);
  const Tensor inside = (cam >= 0)
                          .logical_and(cam < E)
                          .logical_and(i >= 0)
                          .logical_and(i < h)
                          .logical_and(j >= 0)
                          .logical_and(j < w);
  const Tensor flat = (cam.clamp(0, E - 1) * h + i.clamp(0, h - 1)) * w + j.clamp(0, w - 1);
  const auto dev = depth_maps.device();
  const Tensor z = depth_maps.reshape({-1}).index({flat.to(dev)});
  return torch::where(inside.to(dev), z, torch::zeros_like(z)).contiguous();
}

}  // namespace f2n
