// pose_refiner.cpp -- see pose_refiner.hpp.
#include "pose_refiner.hpp"

#include "common.hpp"

using Tensor = torch::Tensor;

namespace
{

int pose_floats(const Tensor & base)
{
  TORCH_CHECK(
    base.dim() == 3 && base.size(2) == 4 && (base.size(1) == 3 || base.size(1) == 4),
    "base poses must be [E,3,4] or [E,4,4]");
  return (int)(base.size(1) * 4);
}

Tensor launch_compose(const Tensor & base, const Tensor & delta, const Tensor & fixed)
{
  const int pose_ld = pose_floats(base);
  const int64_t E = base.size(0);
  TORCH_CHECK(delta.dim() == 2 && delta.size(0) == E && delta.size(1) == 6, "delta must be [E,6]");
  TORCH_CHECK(!fixed.defined() || fixed.numel() == E, "fixed must be [E]");
  Tensor out = torch::empty({E, 3, 4}, base.options());
  f2n::check(
    f2n_pose_compose(
      base.data_ptr<float>(), pose_ld, delta.data_ptr<float>(), f2n::iptr(fixed),
      out.data_ptr<float>(), E, f2n::current_stream(base)),
    "f2n_pose_compose");
  return out;
}

// fixed empty = no fixed cameras (undefined tensors cannot pass through apply())
class PoseComposeFn : public torch::autograd::Function<PoseComposeFn>
{
public:
  static Tensor forward(
    torch::autograd::AutogradContext * ctx, Tensor delta, Tensor base, Tensor fixed)
  {
    if (fixed.numel() == 0) fixed = Tensor();
    Tensor d = f2n::dev_f32(delta, "delta");
    ctx->save_for_backward({d, base, fixed});
    return launch_compose(base, d, fixed);
  }

  static torch::autograd::variable_list backward(
    torch::autograd::AutogradContext * ctx, torch::autograd::variable_list grad)
  {
    auto saved = ctx->get_saved_variables();
    return {pose_compose_bwd(saved[1], saved[0], saved[2], grad[0]), Tensor(), Tensor()};
  }
};

}  // namespace

Tensor pose_compose(const Tensor & base, const Tensor & delta, const Tensor & fixed)
{
  Tensor b = f2n::dev_f32(base.detach(), "base");
  Tensor f = fixed.defined() ? f2n::dev_i32(fixed, "fixed") : Tensor();
  if (!(torch::GradMode::is_enabled() && delta.requires_grad()))
    return launch_compose(b, f2n::dev_f32(delta.detach(), "delta"), f);
  return PoseComposeFn::apply(delta, b, f.defined() ? f : torch::empty({0}, f2n::int_on(b.device())));
}

Tensor pose_compose_bwd(
  const Tensor & base, const Tensor & delta, const Tensor & fixed, const Tensor & d_out)
{
  Tensor b = f2n::dev_f32(base, "base");
  Tensor d = f2n::dev_f32(delta, "delta");
  Tensor g = f2n::dev_f32(d_out, "grad poses");
  const int pose_ld = pose_floats(b);
  const int64_t E = b.size(0);
  TORCH_CHECK(d.dim() == 2 && d.size(0) == E && d.size(1) == 6, "delta must be [E,6]");
  TORCH_CHECK(g.numel() == E * 12, "grad poses must be [E,3,4]");
  Tensor f = fixed.defined() && fixed.numel() ? f2n::dev_i32(fixed, "fixed") : Tensor();
  TORCH_CHECK(!f.defined() || f.numel() == E, "fixed must be [E]");
  Tensor d_delta = torch::empty({E, 6}, d.options());
  f2n::check(
    f2n_pose_compose_bwd(
      b.data_ptr<float>(), pose_ld, d.data_ptr<float>(), f2n::iptr(f), g.data_ptr<float>(),
      d_delta.data_ptr<float>(), E, f2n::current_stream(b)),
    "f2n_pose_compose_bwd");
  return d_delta;
}

PoseRefiner::PoseRefiner(const Tensor & base_poses)
{
  pose_floats(base_poses);
  TORCH_CHECK(base_poses.scalar_type() == torch::kFloat32, "base poses must be float32");
  Tensor rows = base_poses.detach().index({Slc(), Slc(0, 3), Slc()}).contiguous().clone();
  const int64_t E = rows.size(0);
  delta_ = register_parameter("delta", torch::zeros({E, 6}, rows.options()));
  base_ = register_buffer("base", rows);
  fixed_ = register_buffer("fixed", torch::zeros({E}, f2n::int_on(rows.device())));
}

Tensor PoseRefiner::poses() const { return pose_compose(base_, delta_, fixed_); }

void PoseRefiner::set_fixed(const Tensor & mask)
{
  TORCH_CHECK(mask.numel() == n_cameras(), "set_fixed: one entry per camera");
  torch::NoGradGuard no_grad;
  fixed_.copy_(mask.reshape({-1}).ne(0).to(torch::kInt32));
}

std::tuple<Rays, Tensor, Tensor> PoseRefiner::sample_random_rays(
  const Tensor & intrinsics, int h, int w, int64_t batch_size, const Tensor & images,
  const Tensor & dist, const Tensor & cam_idx, const Tensor & ij)
{
  const CameraBatch b =
    draw_camera_batch(n_cameras(), h, w, batch_size, cam_idx, ij, base_.device());
  Rays rays = get_rays_from_cameras(poses(), intrinsics, b.cam, b.ij, dist, b.sorted);
  return {rays, gather_colors(images, b, h, w), b.cam};
}

std::vector<torch::optim::OptimizerParamGroup> PoseRefiner::optim_param_groups(float lr)
{
  auto opt = std::make_unique<torch::optim::AdamOptions>(lr);
  opt->betas(std::make_tuple(0.9, 0.99)).eps(1e-15);
  std::vector<torch::optim::OptimizerParamGroup> groups;
  groups.emplace_back(std::vector<Tensor>{delta_}, std::move(opt));
  return groups;
}

Tensor PoseRefiner::correction_norms() const
{
  Tensor d = delta_.detach();
  return torch::stack(
    {d.index({Slc(), Slc(0, 3)}).norm(2, -1), d.index({Slc(), Slc(3, 6)}).norm(2, -1)}, -1);
}
