// localizer.cpp -- see localizer.hpp.
#include "localizer.hpp"

#include "common.hpp"
#include "scene_files.hpp"

using Tensor = torch::Tensor;

namespace
{
// rays per render call, the reference's chunk (src/localizer.cpp:172,234)
constexpr int kRayChunk = 1 << 16;
}  // namespace

// ---- the three kernels -----------------------------------------------------------------------------

Tensor f2n::perturb_poses(
  const Tensor & pose, const Tensor & noise, const std::array<float, 6> & s)
{
  Tensor p = f2n::dev_f32(pose, "pose");
  Tensor n = f2n::dev_f32(noise, "noise");
  TORCH_CHECK(
    p.dim() == 2 && p.size(1) == 4 && (p.size(0) == 3 || p.size(0) == 4),
    "pose must be [3,4] or [4,4]");
  TORCH_CHECK(n.dim() == 2 && n.size(1) == 6, "noise must be [P,6]");
  const int64_t P = n.size(0);
  Tensor poses = torch::empty({P, 3, 4}, p.options());
  f2n::check(
    f2n_perturb_poses(
      p.data_ptr<float>(), (int)(p.size(0) * 4), n.data_ptr<float>(), s[0], s[1], s[2], s[3], s[4],
      s[5], poses.data_ptr<float>(), (int)P, f2n::current_stream(p)),
    "f2n_perturb_poses");
  return poses;
}

std::pair<Tensor, Tensor> f2n::pose_scores(
  const Tensor & colors, const Tensor & image, const Tensor & ij)
{
  Tensor c = f2n::dev_f32(colors, "colors");
  Tensor img = f2n::dev_f32(image, "image");
  Tensor px = f2n::dev_i32(ij, "ij");
  TORCH_CHECK(img.dim() == 3 && img.size(2) == 3, "image must be [h,w,3]");
  TORCH_CHECK(px.dim() == 2 && px.size(1) == 2 && px.size(0) > 0, "ij must be [K,2], K > 0");
  const int64_t K = px.size(0);
  TORCH_CHECK(
    (c.dim() == 3 && c.size(1) == K && c.size(2) == 3) ||
      (c.dim() == 2 && c.size(1) == 3 && c.size(0) % K == 0),
    "colors must be [P,K,3] or [P*K,3] with the K of ij");
  TORCH_CHECK(
    img.device() == c.device() && px.device() == c.device(),
    "colors, image and ij must be on the same device");
  const int64_t P = c.numel() / (3 * K);
  Tensor loss = torch::empty({P}, c.options());
  Tensor weights = torch::empty({P}, c.options());
  Tensor ws = torch::empty({P}, c.options().dtype(torch::kFloat64));
  f2n::check(
    f2n_pose_scores(
      c.data_ptr<float>(), img.data_ptr<float>(), px.data_ptr<int32_t>(), loss.data_ptr<float>(),
      weights.data_ptr<float>(), ws.data_ptr<double>(), (int)P, (int)K, (int)img.size(0),
      (int)img.size(1), f2n::current_stream(c)),
    "f2n_pose_scores");
  return {loss, weights};
}

Tensor f2n::average_pose(const Tensor & poses, const Tensor & weights)
{
  Tensor p = f2n::dev_f32(poses, "poses");
  Tensor w = f2n::dev_f32(weights, "weights");
  TORCH_CHECK(p.dim() == 3 && p.size(1) == 3 && p.size(2) == 4, "poses must be [P,3,4]");
  TORCH_CHECK(w.dim() == 1 && w.size(0) == p.size(0) && p.size(0) > 0, "weights must be [P], P > 0");
  TORCH_CHECK(w.device() == p.device(), "poses and weights must be on the same device");
  Tensor out = torch::empty({3, 4}, p.options());
  f2n::check(
    f2n_average_pose(
      p.data_ptr<float>(), w.data_ptr<float>(), out.data_ptr<float>(), (int)p.size(0),
      f2n::current_stream(p)),
    "f2n_average_pose");
  return out;
}

// ---- Localizer -------------------------------------------------------------------------------------

Localizer::Localizer(const LocalizerParam & param) : param_(param)
{
  const f2n::InferenceParams ip = f2n::load_inference_params(param.train_result_dir);
  renderer_ = std::make_shared<Renderer>(ip.n_images);
  torch::load(renderer_, param.train_result_dir + "/checkpoints/latest/renderer.pt");
  init(ip.intrinsic, ip.height, ip.width, ip.normalizing_center, ip.normalizing_radius);
}

Localizer::Localizer(
  const LocalizerParam & param, std::shared_ptr<Renderer> renderer, const Tensor & intrinsic,
  int height, int width, const Tensor & center, float radius)
: param_(param), renderer_(std::move(renderer))
{
  TORCH_CHECK(renderer_ != nullptr, "Localizer needs a renderer");
  init(intrinsic, height, width, center, radius);
}

void Localizer::init(
  const Tensor & intrinsic, int height, int width, const Tensor & center, float radius)
{
  TORCH_CHECK(param_.resize_factor >= 1, "resize_factor must be >= 1");
  TORCH_CHECK(param_.render_pixel_num >= 1, "render_pixel_num must be >= 1");
  const torch::Device dev = renderer_->app_emb_.device();
  // the pose optimisation renders 65536-ray chunks of 1024 samples with rays that require grad:
  // they take the fused path (RendererOptions::fused_ray_grad)
  renderer_->options_.fused_ray_grad = true;
  if (param_.exact_ray_grad) renderer_->scene_field_->set_exact_point_grad(true);
  if (param_.level_alpha >= 0.) renderer_->set_coarse_to_fine(param_.level_alpha);
  if (param_.one_pass) {
    renderer_->set_one_pass(true);
    renderer_->set_one_pass_head(param_.one_pass_head);
  }
  // rows 0 and 1 (fx, skew, cx / fy, cy) scale with the image; row 2 stays [0, 0, 1]
  intrinsic_ = intrinsic.to(torch::kFloat32).reshape({3, 3}).to(dev).clone();
  intrinsic_.slice(0, 0, 2).div_(param_.resize_factor);
  const std::array<float, 4> & k = param_.dist_params;
  if (k[0] != 0.f || k[1] != 0.f || k[2] != 0.f || k[3] != 0.f)
    dist_ = torch::tensor({k[0], k[1], k[2], k[3]}).to(dev);
  center_ = center.to(torch::kFloat32).reshape({3}).to(dev);
  radius_ = radius;
  infer_height_ = height / param_.resize_factor;
  infer_width_ = width / param_.resize_factor;
  // Column j is the NeRF axis j (x right, y up, z back) written in the world frame (x front, y left,
  // z up): right = -left, up = up, back = -front.  A signed permutation, so products with it are exact.
  axes_ = torch::tensor({0.f, 0.f, -1.f, -1.f, 0.f, 0.f, 0.f, 1.f, 0.f}).view({3, 3}).to(dev);
}

void Localizer::set_level_alpha(double alpha)
{
  param_.level_alpha = alpha;
  if (alpha >= 0.)
    renderer_->set_coarse_to_fine(alpha);
  else
    renderer_->clear_level_weights();
}

std::array<float, 6> Localizer::noise_sigmas(float noise_coeff) const
{
  // the order of the axes differs: NeRF x <- world y, y <- z, z <- x (src/localizer.cpp:71-79)
  return {
    param_.noise_position_y * noise_coeff / radius_,
    param_.noise_position_z * noise_coeff / radius_,
    param_.noise_position_x * noise_coeff / radius_,
    param_.noise_rotation_y * noise_coeff,
    param_.noise_rotation_z * noise_coeff,
    param_.noise_rotation_x * noise_coeff};
}

std::pair<Tensor, Tensor> Localizer::random_search(
  const Tensor & initial_pose, const Tensor & image_tensor, int64_t particle_num,
  float noise_coeff, const Tensor & noise)
{
  torch::NoGradGuard no_grad;
  Tensor pose = f2n::dev_f32(initial_pose, "initial_pose");
  Tensor image = f2n::dev_f32(image_tensor, "image");
  TORCH_CHECK(particle_num >= 1, "particle_num must be >= 1");
  Tensor n = noise.defined() ? noise : torch::randn({particle_num, 6}, pose.options());
  TORCH_CHECK(n.dim() == 2 && n.size(0) == particle_num, "noise must be [particle_num, 6]");
  Tensor poses = f2n::perturb_poses(pose, n, noise_sigmas(noise_coeff));
  return {poses, evaluate_poses(poses, image)};
}

std::vector<Particle> Localizer::optimize_pose_by_random_search(
  Tensor initial_pose, Tensor image_tensor, int64_t particle_num, float noise_coeff,
  const Tensor & noise)
{
  auto [poses, weights] = random_search(initial_pose, image_tensor, particle_num, noise_coeff, noise);
  const Tensor host = weights.cpu();  // the one read
  const float * w = host.data_ptr<float>();
  std::vector<Particle> result;
  result.reserve(particle_num);
  for (int64_t i = 0; i < particle_num; i++) result.push_back({poses[i], w[i]});
  return result;
}

std::vector<Tensor> Localizer::optimize_pose_by_differential(
  Tensor initial_pose, Tensor image_tensor, int64_t iteration_num)
{
  f2n::dev_f32(initial_pose, "initial_pose");
  const Tensor target =
    f2n::dev_f32(image_tensor, "image").view({infer_height_, infer_width_, 3});
  const Tensor rotation0 = initial_pose.detach().slice(0, 0, 3).slice(1, 0, 3).clone();
  // the caller's tensor becomes the leaf that Adam moves, as with the reference's Localizer
  initial_pose.requires_grad_(true);
  torch::optim::Adam adam(std::vector<Tensor>{initial_pose}, torch::optim::AdamOptions(1e-4));
  std::vector<Tensor> steps;
  steps.reserve(iteration_num);
  for (int64_t it = 0; it < iteration_num; ++it) {
    adam.zero_grad();
    torch::mse_loss(render_image(initial_pose), target).backward();
    adam.step();
    // Adam moves all twelve numbers; a step reports the current translation under the INITIAL rotation
    Tensor step = initial_pose.detach().clone();
    step.slice(0, 0, 3).slice(1, 0, 3).copy_(rotation0);
    steps.push_back(step);
  }
  return steps;
}

Tensor Localizer::render_image(const Tensor & pose)
{
  f2n::dev_f32(pose, "pose");
  return std::get<0>(
    renderer_->render_image(pose, intrinsic_, infer_height_, infer_width_, kRayChunk, dist_));
}

Rays Localizer::pose_rays(const Tensor & poses, const Tensor & ij)
{
  Tensor p = f2n::dev_f32(poses, "poses");
  TORCH_CHECK(
    p.dim() == 3 && p.size(2) == 4 && (p.size(1) == 3 || p.size(1) == 4) && p.size(0) > 0,
    "poses must be [P,3,4] or [P,4,4], P > 0");
  return get_rays_from_poses(p, intrinsic_, ij, dist_);
}

Localizer::PoseScores Localizer::evaluate_poses_full(
  const Tensor & poses, const Tensor & image, const Tensor & ij)
{
  torch::NoGradGuard no_grad;
  Tensor p = f2n::dev_f32(poses, "poses");
  Tensor img = f2n::dev_f32(image, "image");
  TORCH_CHECK(
    img.numel() == (int64_t)infer_height_ * infer_width_ * 3,
    "image must be [infer_height, infer_width, 3]");
  img = img.view({infer_height_, infer_width_, 3});
  PoseScores out;
  if (ij.defined()) {
    out.ij = f2n::dev_i32(ij, "ij");
  } else {
    // pixels without replacement, drawn on the device (the reference shuffles h*w indices on the host)
    const int64_t n_pix = (int64_t)infer_height_ * infer_width_;
    const int64_t K = std::min<int64_t>(param_.render_pixel_num, n_pix);
    Tensor v = torch::randperm(n_pix, torch::TensorOptions().dtype(torch::kInt64).device(p.device()))
                 .index({Slc(0, K)});
    out.ij = torch::stack({v.floor_divide(infer_width_), v.remainder(infer_width_)}, -1)
               .to(torch::kInt32)
               .contiguous();
  }
  const int64_t P = p.size(0), K = out.ij.size(0);
  Rays rays = pose_rays(p, out.ij);
  out.colors =
    std::get<0>(renderer_->render_all_rays(rays.origins, rays.dirs, kRayChunk)).view({P, K, 3});
  std::tie(out.loss, out.weights) = f2n::pose_scores(out.colors, img, out.ij);
  return out;
}

Tensor Localizer::evaluate_poses(const Tensor & poses, const Tensor & image, const Tensor & ij)
{
  return evaluate_poses_full(poses, image, ij).weights;
}

Tensor Localizer::calc_average_pose(const Tensor & poses, const Tensor & weights)
{
  return f2n::average_pose(poses, weights);
}

Tensor Localizer::calc_average_pose(const std::vector<Particle> & particles)
{
  TORCH_CHECK(!particles.empty(), "calc_average_pose: no particles");
  std::vector<Tensor> poses;
  std::vector<float> weights;
  poses.reserve(particles.size());
  weights.reserve(particles.size());
  for (const Particle & particle : particles) {
    poses.push_back(f2n::dev_f32(particle.pose, "particle pose").index({Slc(0, 3), Slc(0, 4)}));
    weights.push_back(particle.weight);
  }
  Tensor stacked = torch::stack(poses);
  return f2n::average_pose(stacked, torch::tensor(weights).to(stacked.device()));
}

// A pose is [R | t]: camera axes and position in some frame.  Changing the frame of a world pose to
// the NeRF axes is the similarity R' = A^T R A with t' = A^T t (A = axes_); the field was trained on
// positions shifted by the centre and scaled by 1 / radius, so the translation is normalised as well.
Tensor Localizer::world2camera(const Tensor & pose_in_world)
{
  const Tensor w = f2n::dev_f32(pose_in_world, "pose_in_world");
  TORCH_CHECK(w.dim() == 2 && w.size(0) >= 3 && w.size(1) == 4, "pose_in_world must be [4,4] or [3,4]");
  const Tensor at = axes_.t();
  const Tensor rot = at.mm(w.slice(0, 0, 3).slice(1, 0, 3)).mm(axes_);
  const Tensor pos = (at.mv(w.slice(0, 0, 3).select(1, 3)) - center_) / radius_;
  return torch::cat({rot, pos.unsqueeze(1)}, 1);
}

// The inverse: [3,4] in the normalised NeRF frame -> [4,4] in the world frame.
Tensor Localizer::camera2world(const Tensor & pose_in_camera)
{
  const Tensor c = f2n::dev_f32(pose_in_camera, "pose_in_camera");
  TORCH_CHECK(c.dim() == 2 && c.size(0) >= 3 && c.size(1) == 4, "pose_in_camera must be [3,4] or [4,4]");
  const Tensor rot = axes_.mm(c.slice(0, 0, 3).slice(1, 0, 3)).mm(axes_.t());
  const Tensor pos = axes_.mv(c.slice(0, 0, 3).select(1, 3) * radius_ + center_);
  Tensor out = torch::zeros({4, 4}, c.options());
  out.slice(0, 0, 3).slice(1, 0, 3).copy_(rot);
  out.slice(0, 0, 3).select(1, 3).copy_(pos);
  out[3][3] = 1.f;
  return out;
}
