// rays.cpp -- see rays.hpp.  The reference's get_rays_from_pose is an ATen chain ending in a batched
// 3x3 GEMM with one problem per ray (src/rays.cpp:7-28; 8.4 ms for the 640 000 rays of an 800x800
// view through rocBLAS); here it is one launch of f2n_gen_rays.
#include "rays.hpp"

#include "common.hpp"

using Tensor = torch::Tensor;

namespace
{

// poses as [B, 3|4, 4] contiguous f32 on the GPU -> (pointer, floats per pose)
std::pair<Tensor, int> pose_blocks(const Tensor & pose)
{
  TORCH_CHECK(
    pose.dim() == 3 && pose.size(2) == 4 && (pose.size(1) == 3 || pose.size(1) == 4),
    "pose must be [B,3,4] or [B,4,4]");
  return {f2n::dev_f32(pose, "pose"), (int)(pose.size(1) * 4)};
}

// dist as [n_cams,4] contiguous f32 on the poses' device; undefined stays undefined (pinhole)
Tensor dist_rows(const Tensor & dist, int64_t n_cams, const Tensor & poses)
{
  if (!dist.defined()) return dist;
  TORCH_CHECK(
    dist.numel() == n_cams * 4 && dist.size(-1) == 4,
    "dist must hold (k1, k2, p1, p2) for each of the ", n_cams, " cameras");
  Tensor d = f2n::dev_f32(dist.detach(), "dist").view({n_cams, 4});
  TORCH_CHECK(d.device() == poses.device(), "dist must be on the poses' device");
  return d;
}

Rays launch_gen_rays(
  const Tensor & pose, const Tensor & intrinsic, const Tensor & cam_idx, const Tensor & ij,
  int64_t first_pixel, int width, int64_t n, const Tensor & dist = {})
{
  auto [poses, pose_ld] = pose_blocks(pose);
  Tensor K = f2n::dev_f32(intrinsic, "intrinsic");
  TORCH_CHECK(
    K.dim() == 3 && K.size(1) == 3 && K.size(2) == 3 && K.size(0) == poses.size(0),
    "intrinsic must be [B,3,3] with the poses' B");
  Rays rays{torch::empty({n, 3}, poses.options()), torch::empty({n, 3}, poses.options())};
  if (dist.defined()) {
    Tensor D = dist_rows(dist, poses.size(0), poses);
    f2n::check(
      f2n_gen_rays_dist(
        poses.data_ptr<float>(), pose_ld, K.data_ptr<float>(), D.data_ptr<float>(), poses.size(0),
        f2n::iptr(cam_idx), f2n::iptr(ij), first_pixel, width, rays.origins.data_ptr<float>(),
        rays.dirs.data_ptr<float>(), n, f2n::current_stream(poses)),
      "f2n_gen_rays_dist");
    return rays;
  }
  f2n::check(
    f2n_gen_rays(
      poses.data_ptr<float>(), pose_ld, K.data_ptr<float>(), poses.size(0), f2n::iptr(cam_idx),
      f2n::iptr(ij), first_pixel, width, rays.origins.data_ptr<float>(),
      rays.dirs.data_ptr<float>(), n, f2n::current_stream(poses)),
    "f2n_gen_rays");
  return rays;
}

// launch_gen_rays with a backward to the pose (the intrinsics are constants, as in the reference's
// pose optimisation, src/localizer.cpp:142-167).  ij empty = pixel first_pixel + r of a `width`-wide
// image, dist empty = pinhole (undefined tensors cannot pass through apply()).  No cam_idx: every ray
// uses pose 0, or ray r pose r.
class GenRaysFn : public torch::autograd::Function<GenRaysFn>
{
public:
  static torch::autograd::variable_list forward(
    torch::autograd::AutogradContext * ctx, Tensor pose, Tensor intrinsic, Tensor ij, Tensor dist,
    int64_t first_pixel, int64_t width, int64_t n)
  {
    if (ij.numel() == 0) ij = Tensor();
    if (dist.numel() == 0) dist = Tensor();
    dist = dist_rows(dist, pose.size(0), pose);
    Rays rays = launch_gen_rays(pose, intrinsic, Tensor(), ij, first_pixel, (int)width, n, dist);
    ctx->save_for_backward({f2n::dev_f32(intrinsic, "intrinsic"), ij, dist});
    ctx->saved_data["first_pixel"] = first_pixel;
    ctx->saved_data["width"] = width;
    ctx->saved_data["pose_shape"] = pose.sizes().vec();
    return {rays.origins, rays.dirs};
  }

  static torch::autograd::variable_list backward(
    torch::autograd::AutogradContext * ctx, torch::autograd::variable_list grad)
  {
    auto saved = ctx->get_saved_variables();
    const Tensor & K = saved[0];
    const Tensor & ij = saved[1];
    const Tensor & dist = saved[2];
    const auto shape = ctx->saved_data["pose_shape"].toIntVector();
    const int64_t n_cams = shape[0];
    const int pose_ld = (int)(shape[1] * 4);
    const auto opt = K.options();
    const Tensor & ref = grad[0].defined() ? grad[0] : grad[1];
    const int64_t n = ref.defined() ? ref.size(0) : 0;
    Tensor d_o = grad[0].defined() ? f2n::dev_f32(grad[0], "grad rays_o") : torch::zeros({n, 3}, opt);
    Tensor d_d = grad[1].defined() ? f2n::dev_f32(grad[1], "grad rays_d") : torch::zeros({n, 3}, opt);
    Tensor ws = torch::empty({f2n_gen_rays_bwd_workspace_floats(n)}, opt);
    if (dist.defined()) {
      // (no rays: the entry writes nothing)
      Tensor d_pose = n > 0 ? torch::empty(shape, opt) : torch::zeros(shape, opt);
      f2n::check(
        f2n_gen_rays_dist_bwd(
          K.data_ptr<float>(), dist.data_ptr<float>(), n_cams, f2n::iptr(ij),
          ctx->saved_data["first_pixel"].toInt(), (int)ctx->saved_data["width"].toInt(),
          d_o.data_ptr<float>(), d_d.data_ptr<float>(), d_pose.data_ptr<float>(), pose_ld,
          ws.data_ptr<float>(), n, f2n::current_stream(K)),
        "f2n_gen_rays_dist_bwd");
      return {d_pose, Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
    }
    Tensor d_pose = torch::empty(shape, opt);
    f2n::check(
      f2n_gen_rays_bwd(
        K.data_ptr<float>(), n_cams, f2n::iptr(ij), ctx->saved_data["first_pixel"].toInt(),
        (int)ctx->saved_data["width"].toInt(), d_o.data_ptr<float>(), d_d.data_ptr<float>(),
        d_pose.data_ptr<float>(), pose_ld, ws.data_ptr<float>(), n, f2n::current_stream(K)),
      "f2n_gen_rays_bwd");
    return {d_pose, Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

// rays of one view (ij undefined) or of the given pixels, through GenRaysFn when the pose wants a
// gradient
Rays gen_rays(
  const Tensor & pose, const Tensor & intrinsic, const Tensor & ij, int64_t first_pixel, int width,
  int64_t n, const Tensor & dist)
{
  if (!(torch::GradMode::is_enabled() && pose.requires_grad()))
    return launch_gen_rays(pose, intrinsic, Tensor(), ij, first_pixel, width, n, dist);
  const Tensor pixels = ij.defined() ? ij : torch::empty({0}, f2n::int_on(pose.device()));
  const Tensor lens = dist.defined() ? dist.detach() : torch::empty({0}, f2n::float_on(pose.device()));
  auto out =
    GenRaysFn::apply(pose, intrinsic.detach(), pixels, lens, first_pixel, (int64_t)width, n);
  return {out[0], out[1]};
}

// The camera-sorted ray list that the per-camera sums walk, made with ATen ops on the device:
// cam_start (the E + 1 segment bounds) and `order`, empty when cam_idx is already sorted.
struct CamOrder
{
  Tensor cam_start, order;
};

CamOrder camera_order(const Tensor & cam_idx, int64_t E, bool sorted)
{
  Tensor order = torch::empty({0}, cam_idx.options());
  Tensor cam_sorted = cam_idx;
  if (!sorted && cam_idx.size(0) > 0) {
    // stable: equal cameras keep the caller's order, so the sums' order is fixed by cam_idx alone
    auto [vals, idx] = at::sort(cam_idx, /*stable=*/true, /*dim=*/0, /*descending=*/false);
    cam_sorted = vals;
    order = idx.to(torch::kInt32);
  }
  // cam_start[c] = number of rays whose camera is below c
  Tensor cam_start = torch::searchsorted(
    cam_sorted, torch::arange(E + 1, cam_idx.options()), /*out_int32=*/true, /*right=*/false);
  return {cam_start, order};
}

// d(poses) in `shape` ([E,3|4,4]) of a batch's ray gradients: f2n_cam_pose_grad
Tensor launch_cam_pose_grad(
  const Tensor & K, const Tensor & dist, const Tensor & ij, const Tensor & d_o, const Tensor & d_d,
  const CamOrder & co, const std::vector<int64_t> & shape)
{
  const int64_t E = shape[0], n = ij.size(0);
  const int pose_ld = (int)(shape[1] * 4);
  Tensor ws = torch::empty({f2n_cam_pose_grad_workspace_floats(n, E)}, K.options());
  Tensor d_poses = torch::empty(shape, K.options());
  f2n::check(
    f2n_cam_pose_grad(
      K.data_ptr<float>(), f2n::fptr(dist), ij.data_ptr<int32_t>(), d_o.data_ptr<float>(),
      d_d.data_ptr<float>(), co.cam_start.data_ptr<int32_t>(),
      co.order.numel() ? co.order.data_ptr<int32_t>() : nullptr, d_poses.data_ptr<float>(), pose_ld,
      ws.data_ptr<float>(), n, E, f2n::current_stream(K)),
    "f2n_cam_pose_grad");
  return d_poses;
}

// launch_gen_rays with a camera per ray and a backward to the poses: the per-camera sums of
// f2n_cam_pose_grad.
class CamRaysFn : public torch::autograd::Function<CamRaysFn>
{
public:
  static torch::autograd::variable_list forward(
    torch::autograd::AutogradContext * ctx, Tensor poses, Tensor intrinsics, Tensor cam_idx,
    Tensor ij, Tensor dist, bool sorted)
  {
    if (dist.numel() == 0) dist = Tensor();
    dist = dist_rows(dist, poses.size(0), poses);
    const int64_t n = cam_idx.size(0), E = poses.size(0);
    Rays rays = launch_gen_rays(poses, intrinsics, cam_idx, ij, 0, 1, n, dist);
    const CamOrder co = camera_order(cam_idx, E, sorted);
    ctx->save_for_backward(
      {f2n::dev_f32(intrinsics, "intrinsics"), ij, dist, co.cam_start, co.order});
    ctx->saved_data["pose_shape"] = poses.sizes().vec();
    return {rays.origins, rays.dirs};
  }

  static torch::autograd::variable_list backward(
    torch::autograd::AutogradContext * ctx, torch::autograd::variable_list grad)
  {
    auto saved = ctx->get_saved_variables();
    const Tensor & K = saved[0];
    const Tensor & ij = saved[1];
    const int64_t n = ij.size(0);
    const auto opt = K.options();
    Tensor d_o = grad[0].defined() ? f2n::dev_f32(grad[0], "grad rays_o") : torch::zeros({n, 3}, opt);
    Tensor d_d = grad[1].defined() ? f2n::dev_f32(grad[1], "grad rays_d") : torch::zeros({n, 3}, opt);
    Tensor d_poses = launch_cam_pose_grad(
      K, saved[2], ij, d_o, d_d, {saved[3], saved[4]}, ctx->saved_data["pose_shape"].toIntVector());
    return {d_poses, Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

// CamRaysFn with the calibration as an input: the backward reaches the poses through
// f2n_cam_pose_grad (CamRaysFn's launch, the same bits) and the intrinsics and the coefficients
// through f2n_cam_intr_grad, each only if its input asks for it, over one shared cam_start / order.
// dist empty = pinhole cameras, which then have no coefficients to hand a gradient to.
class CalibratedCamRaysFn : public torch::autograd::Function<CalibratedCamRaysFn>
{
public:
  static torch::autograd::variable_list forward(
    torch::autograd::AutogradContext * ctx, Tensor poses, Tensor intrinsics, Tensor dist,
    Tensor cam_idx, Tensor ij, bool sorted)
  {
    ctx->saved_data["dist_shape"] = dist.sizes().vec();
    if (dist.numel() == 0) dist = Tensor();
    dist = dist_rows(dist, poses.size(0), poses);
    const int64_t n = cam_idx.size(0), E = poses.size(0);
    Rays rays = launch_gen_rays(poses, intrinsics, cam_idx, ij, 0, 1, n, dist);
    const CamOrder co = camera_order(cam_idx, E, sorted);
    auto [pose_rows, pose_ld] = pose_blocks(poses);
    (void)pose_ld;
    ctx->save_for_backward(
      {pose_rows, f2n::dev_f32(intrinsics, "intrinsics"), ij, dist, co.cam_start, co.order});
    return {rays.origins, rays.dirs};
  }

  static torch::autograd::variable_list backward(
    torch::autograd::AutogradContext * ctx, torch::autograd::variable_list grad)
  {
    auto saved = ctx->get_saved_variables();
    const Tensor & poses = saved[0];
    const Tensor & K = saved[1];
    const Tensor & ij = saved[2];
    const Tensor & dist = saved[3];
    const CamOrder co = {saved[4], saved[5]};
    const int64_t E = poses.size(0), n = ij.size(0);
    const auto opt = K.options();
    Tensor d_d = grad[1].defined() ? f2n::dev_f32(grad[1], "grad rays_d") : torch::zeros({n, 3}, opt);
    Tensor d_poses, d_K, d_dist;
    if (ctx->needs_input_grad(0)) {
      Tensor d_o =
        grad[0].defined() ? f2n::dev_f32(grad[0], "grad rays_o") : torch::zeros({n, 3}, opt);
      d_poses = launch_cam_pose_grad(K, dist, ij, d_o, d_d, co, poses.sizes().vec());
    }
    const bool want_K = ctx->needs_input_grad(1);
    const bool want_dist = dist.defined() && ctx->needs_input_grad(2);
    if (want_K || want_dist) {
      Tensor ws = torch::empty({f2n_cam_intr_grad_workspace_floats(n, E)}, opt);
      Tensor d_intr = torch::empty({E, 8}, opt);
      f2n::check(
        f2n_cam_intr_grad(
          poses.data_ptr<float>(), (int)(poses.size(1) * 4), K.data_ptr<float>(), f2n::fptr(dist),
          ij.data_ptr<int32_t>(), d_d.data_ptr<float>(), co.cam_start.data_ptr<int32_t>(),
          co.order.numel() ? co.order.data_ptr<int32_t>() : nullptr, d_intr.data_ptr<float>(),
          ws.data_ptr<float>(), n, E, f2n::current_stream(K)),
        "f2n_cam_intr_grad");
      if (want_K) {
        d_K = torch::zeros({E, 3, 3}, opt);
        d_K.select(1, 0).select(1, 0).copy_(d_intr.select(1, 0));
        d_K.select(1, 1).select(1, 1).copy_(d_intr.select(1, 1));
        d_K.select(1, 0).select(1, 2).copy_(d_intr.select(1, 2));
        d_K.select(1, 1).select(1, 2).copy_(d_intr.select(1, 3));
      }
      if (want_dist)
        d_dist = d_intr.slice(1, 4, 8).contiguous().view(ctx->saved_data["dist_shape"].toIntVector());
    }
    return {d_poses, d_K, d_dist, Tensor(), Tensor(), Tensor()};
  }
};

}  // namespace

CameraBatch draw_camera_batch(
  int64_t n_cameras, int h, int w, int64_t batch_size, const Tensor & cam_idx, const Tensor & ij,
  const torch::Device & device)
{
  const auto iopt = f2n::int_on(device);
  CameraBatch b;
  b.sorted = !cam_idx.defined();
  if (b.sorted) {
    // sorted values only: which ray gets which camera does not matter before the pixels are drawn
    b.cam = std::get<0>(torch::randint(n_cameras, {batch_size}, iopt).sort());
  } else {
    TORCH_CHECK(cam_idx.dim() == 1 && cam_idx.size(0) == batch_size, "cam_idx must be [batch_size]");
    b.cam = f2n::dev_i32(cam_idx, "cam_idx");
  }
  if (ij.defined()) {
    TORCH_CHECK(ij.dim() == 2 && ij.size(0) == batch_size && ij.size(1) == 2, "ij must be [n,2]");
    b.ij = f2n::dev_i32(ij, "ij");
  } else {
    Tensor i = torch::randint(0, h, {batch_size}, iopt);
    Tensor j = torch::randint(0, w, {batch_size}, iopt);
    b.ij = torch::stack({i, j}, -1).contiguous();
  }
  return b;
}

Tensor gather_colors(const Tensor & images, const CameraBatch & b, int h, int w)
{
  if (!images.defined()) return Tensor();
  Tensor flat = (b.cam.to(torch::kLong) * h + b.ij.select(1, 0).to(torch::kLong)) * w +
                b.ij.select(1, 1).to(torch::kLong);
  return images.view({-1, 3}).index({flat}).to(b.cam.device()).contiguous();
}

Rays get_rays_from_calibrated_cameras(
  const Tensor & poses, const Tensor & intrinsics, const Tensor & dist, const Tensor & cam_idx,
  const Tensor & ij, bool sorted)
{
  const bool grad_mode = torch::GradMode::is_enabled();
  const bool want_calib =
    grad_mode && (intrinsics.requires_grad() || (dist.defined() && dist.requires_grad()));
  // nothing for f2n_cam_intr_grad to do: today's route, the same graph
  if (!want_calib) return get_rays_from_cameras(poses, intrinsics, cam_idx, ij, dist, sorted);
  TORCH_CHECK(ij.dim() == 2 && ij.size(1) == 2, "ij must be [n,2]");
  TORCH_CHECK(cam_idx.dim() == 1 && cam_idx.size(0) == ij.size(0), "cam_idx must be [n]");
  TORCH_CHECK(poses.size(0) >= 1, "get_rays_from_calibrated_cameras: no cameras");
  Tensor cam = f2n::dev_i32(cam_idx, "cam_idx");
  Tensor ij32 = f2n::dev_i32(ij, "ij");
  const Tensor lens = dist.defined() ? dist : torch::empty({0}, f2n::float_on(poses.device()));
  auto out = CalibratedCamRaysFn::apply(poses, intrinsics, lens, cam, ij32, sorted);
  return {out[0], out[1]};
}

Rays get_rays_from_cameras(
  const Tensor & poses, const Tensor & intrinsics, const Tensor & cam_idx, const Tensor & ij,
  const Tensor & dist, bool sorted)
{
  TORCH_CHECK(ij.dim() == 2 && ij.size(1) == 2, "ij must be [n,2]");
  TORCH_CHECK(cam_idx.dim() == 1 && cam_idx.size(0) == ij.size(0), "cam_idx must be [n]");
  Tensor cam = f2n::dev_i32(cam_idx, "cam_idx");
  Tensor ij32 = f2n::dev_i32(ij, "ij");
  if (!(torch::GradMode::is_enabled() && poses.requires_grad()))
    return launch_gen_rays(poses, intrinsics, cam, ij32, 0, 1, cam.size(0), dist);
  TORCH_CHECK(poses.size(0) >= 1, "get_rays_from_cameras: no cameras");
  const Tensor lens =
    dist.defined() ? dist.detach() : torch::empty({0}, f2n::float_on(poses.device()));
  auto out = CamRaysFn::apply(poses, intrinsics.detach(), cam, ij32, lens, sorted);
  return {out[0], out[1]};
}

Rays get_rays_from_pose(
  const Tensor & pose, const Tensor & intrinsic, const Tensor & ij, const Tensor & dist)
{
  TORCH_CHECK(ij.dim() == 2 && ij.size(1) == 2, "ij must be [N,2]");
  const int64_t n = ij.size(0);
  TORCH_CHECK(
    pose.size(0) == 1 || pose.size(0) == n, "pose batch must be 1 or N (src/rays.cpp broadcast)");
  // the reference converts whatever ij holds with .to(kFloat32); pixel indices are exact either way
  Tensor ij32 = f2n::dev_i32(ij.to(torch::kInt32), "ij");
  return gen_rays(pose, intrinsic, ij32, 0, 1, n, dist);
}

Rays get_rays_from_poses(
  const Tensor & poses, const Tensor & intrinsic, const Tensor & ij, const Tensor & dist)
{
  TORCH_CHECK(ij.dim() == 2 && ij.size(1) == 2, "ij must be [K,2]");
  TORCH_CHECK(intrinsic.dim() == 2, "intrinsic must be [3,3]: the poses share one camera");
  Tensor ij32 = f2n::dev_i32(ij, "ij");
  const int64_t P = poses.size(0), K = ij32.size(0);
  Tensor cam = torch::arange(P * K, f2n::int_on(ij32.device())).floor_divide_(K);
  Tensor lens;
  if (dist.defined()) {
    TORCH_CHECK(dist.numel() == 4, "dist must be [4]: the poses share one camera");
    lens = dist.reshape({1, 4}).expand({P, 4});
  }
  return launch_gen_rays(
    poses, intrinsic.unsqueeze(0).expand({P, 3, 3}), cam, ij32.repeat({P, 1}), 0, 1, P * K, lens);
}

Rays get_view_rays(
  const Tensor & pose, const Tensor & intrinsic, int h, int w, const Tensor & dist)
{
  Tensor p = pose.dim() == 2 ? pose.unsqueeze(0) : pose;
  Tensor k = intrinsic.dim() == 2 ? intrinsic.unsqueeze(0) : intrinsic;
  TORCH_CHECK(p.size(0) == 1 && h > 0 && w > 0, "get_view_rays: one pose, a positive image size");
  return gen_rays(p, k, Tensor(), 0, w, (int64_t)h * w, dist);
}

std::tuple<Rays, Tensor, Tensor> sample_random_rays(
  const Tensor & poses, const Tensor & intrinsics, int h, int w, int64_t batch_size,
  const Tensor & images, const Tensor & dist)
{
  const auto iopt = torch::TensorOptions().dtype(torch::kInt32).device(poses.device());
  const int64_t n_images = poses.size(0);
  Tensor cam = torch::randint(n_images, {batch_size}, iopt);
  Tensor i = torch::randint(0, h, {batch_size}, iopt);
  Tensor j = torch::randint(0, w, {batch_size}, iopt);
  Tensor ij = torch::stack({i, j}, -1).contiguous();
  Rays rays = launch_gen_rays(poses, intrinsics, cam, ij, 0, 1, batch_size, dist);
  Tensor gt;
  if (images.defined()) {
    Tensor flat = (cam.to(torch::kLong) * h + i.to(torch::kLong)) * w + j.to(torch::kLong);
    gt = images.view({-1, 3}).index({flat}).to(poses.device()).contiguous();
  }
  return {rays, gt, cam};
}

std::tuple<Tensor, Tensor> project_points(
  const Tensor & points, const Tensor & pose, const Tensor & intrinsic, const Tensor & dist)
{
  Tensor pts = f2n::dev_f32(points, "points");
  TORCH_CHECK(pts.dim() == 2 && pts.size(1) == 3, "points must be [N,3]");
  const int64_t n = pts.size(0);
  auto [poses, pose_ld] = pose_blocks(pose.dim() == 2 ? pose.unsqueeze(0) : pose);
  const int64_t B = poses.size(0);
  TORCH_CHECK(B == 1 || B == n, "pose batch must be 1 or N");
  Tensor K = f2n::dev_f32(intrinsic.dim() == 2 ? intrinsic.unsqueeze(0) : intrinsic, "intrinsic");
  TORCH_CHECK(
    K.dim() == 3 && K.size(1) == 3 && K.size(2) == 3 && K.size(0) == B,
    "intrinsic must be [B,3,3] with the poses' B");
  TORCH_CHECK(
    poses.device() == pts.device() && K.device() == pts.device(),
    "points, pose and intrinsic must be on the same device");
  Tensor D = dist_rows(dist, B, poses);
  Tensor pix = torch::empty({n, 2}, pts.options());
  Tensor valid = torch::empty({n}, f2n::int_on(pts.device()));
  f2n::check(
    f2n_project_points(
      pts.data_ptr<float>(), poses.data_ptr<float>(), pose_ld, K.data_ptr<float>(), f2n::fptr(D), B,
      nullptr, pix.data_ptr<float>(), valid.data_ptr<int32_t>(), n, f2n::current_stream(pts)),
    "f2n_project_points");
  return {pix, valid};
}
