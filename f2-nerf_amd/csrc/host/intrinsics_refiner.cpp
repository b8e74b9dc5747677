// intrinsics_refiner.cpp -- see intrinsics_refiner.hpp.
#include "intrinsics_refiner.hpp"

#include "common.hpp"

using Tensor = torch::Tensor;

namespace
{

Tensor detached(const Tensor & t) { return t.defined() ? t.detach() : t; }

// the arguments as the entries take them; base_dist, learn: undefined stays undefined (NULL)
struct ComposeArgs
{
  Tensor K, dist, gamma, group, learn;
  int64_t E, G;
};

ComposeArgs compose_args(
  const Tensor & base_K, const Tensor & base_dist, const Tensor & gamma, const Tensor & group,
  const Tensor & learn)
{
  ComposeArgs a;
  a.K = f2n::dev_f32(base_K, "base_K");
  TORCH_CHECK(a.K.dim() == 3 && a.K.size(1) == 3 && a.K.size(2) == 3, "base_K must be [E,3,3]");
  a.E = a.K.size(0);
  a.gamma = f2n::dev_f32(gamma, "gamma");
  TORCH_CHECK(
    a.gamma.dim() == 2 && a.gamma.size(0) >= 1 && a.gamma.size(1) == 8, "gamma must be [G,8], G >= 1");
  a.G = a.gamma.size(0);
  a.group = f2n::dev_i32(group, "group");
  TORCH_CHECK(a.group.numel() == a.E, "group must be [E]");
  if (base_dist.defined() && base_dist.numel()) {
    a.dist = f2n::dev_f32(base_dist, "base_dist");
    TORCH_CHECK(a.dist.numel() == a.E * 4 && a.dist.size(-1) == 4, "base_dist must be [E,4]");
  }
  if (learn.defined() && learn.numel()) {
    a.learn = f2n::dev_i32(learn, "learn");
    TORCH_CHECK(a.learn.numel() == 8, "learn must be [8]");
  }
  return a;
}

// the one host read: a group past the table is the caller's error (the kernels only ignore it)
void check_groups(const Tensor & group, int64_t G)
{
  if (group.numel() == 0) return;
  TORCH_CHECK(
    group.max().item<int64_t>() < G, "group holds an entry >= ", G, ", the number of rows of gamma");
}

std::tuple<Tensor, Tensor> launch_compose(const ComposeArgs & a)
{
  Tensor out_K = torch::empty({a.E, 3, 3}, a.K.options());
  Tensor out_dist = torch::empty({a.E, 4}, a.K.options());
  f2n::check(
    f2n_intr_compose(
      a.K.data_ptr<float>(), f2n::fptr(a.dist), a.gamma.data_ptr<float>(),
      a.group.data_ptr<int32_t>(), out_K.data_ptr<float>(), out_dist.data_ptr<float>(), a.E, a.G,
      f2n::current_stream(a.K)),
    "f2n_intr_compose");
  return {out_K, out_dist};
}

Tensor launch_compose_bwd(const ComposeArgs & a, const Tensor & d_K, const Tensor & d_dist)
{
  Tensor gK, gD;
  if (d_K.defined()) {
    gK = f2n::dev_f32(d_K, "grad intrinsics");
    TORCH_CHECK(gK.numel() == a.E * 9, "grad intrinsics must be [E,3,3]");
  }
  if (d_dist.defined()) {
    gD = f2n::dev_f32(d_dist, "grad dist");
    TORCH_CHECK(gD.numel() == a.E * 4, "grad dist must be [E,4]");
  }
  Tensor d_gamma = torch::empty({a.G, 8}, a.gamma.options());
  f2n::check(
    f2n_intr_compose_bwd(
      a.K.data_ptr<float>(), f2n::fptr(a.dist), a.gamma.data_ptr<float>(),
      a.group.data_ptr<int32_t>(), f2n::iptr(a.learn), f2n::fptr(gK), f2n::fptr(gD),
      d_gamma.data_ptr<float>(), a.E, a.G, f2n::current_stream(a.K)),
    "f2n_intr_compose_bwd");
  return d_gamma;
}

// base_dist, learn empty = none (undefined tensors cannot pass through apply())
class IntrComposeFn : public torch::autograd::Function<IntrComposeFn>
{
public:
  static torch::autograd::variable_list forward(
    torch::autograd::AutogradContext * ctx, Tensor gamma, Tensor base_K, Tensor base_dist,
    Tensor group, Tensor learn)
  {
    const ComposeArgs a = compose_args(base_K, base_dist, gamma, group, learn);
    ctx->save_for_backward({a.gamma, base_K, base_dist, group, learn});
    auto [K, dist] = launch_compose(a);
    return {K, dist};
  }

  static torch::autograd::variable_list backward(
    torch::autograd::AutogradContext * ctx, torch::autograd::variable_list grad)
  {
    auto saved = ctx->get_saved_variables();
    const ComposeArgs a = compose_args(saved[1], saved[2], saved[0], saved[3], saved[4]);
    return {launch_compose_bwd(a, grad[0], grad[1]), Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

// intr_compose without the host read of check_groups
std::tuple<Tensor, Tensor> compose(
  const Tensor & base_K, const Tensor & base_dist, const Tensor & gamma, const Tensor & group,
  const Tensor & learn)
{
  if (!(torch::GradMode::is_enabled() && gamma.requires_grad()))
    return launch_compose(
      compose_args(base_K.detach(), detached(base_dist), gamma.detach(), group, learn));
  const auto none_f = torch::empty({0}, f2n::float_on(base_K.device()));
  const auto none_i = torch::empty({0}, f2n::int_on(base_K.device()));
  auto out = IntrComposeFn::apply(
    gamma, base_K.detach(), base_dist.defined() ? base_dist.detach() : none_f, group,
    learn.defined() ? learn : none_i);
  return {out[0], out[1]};
}

}  // namespace

std::tuple<Tensor, Tensor> intr_compose(
  const Tensor & base_K, const Tensor & base_dist, const Tensor & gamma, const Tensor & group,
  const Tensor & learn)
{
  TORCH_CHECK(gamma.dim() == 2, "gamma must be [G,8]");
  check_groups(group, gamma.size(0));
  return compose(base_K, base_dist, gamma, group, learn);
}

Tensor intr_compose_bwd(
  const Tensor & base_K, const Tensor & base_dist, const Tensor & gamma, const Tensor & group,
  const Tensor & learn, const Tensor & d_K, const Tensor & d_dist)
{
  const ComposeArgs a =
    compose_args(base_K.detach(), detached(base_dist), gamma.detach(), group, learn);
  check_groups(a.group, a.G);
  return launch_compose_bwd(a, d_K, d_dist);
}

IntrinsicsRefiner::IntrinsicsRefiner(
  const Tensor & base_intrinsics, const Tensor & base_dist, const Tensor & group)
{
  TORCH_CHECK(
    base_intrinsics.dim() == 3 && base_intrinsics.size(1) == 3 && base_intrinsics.size(2) == 3,
    "base intrinsics must be [E,3,3]");
  TORCH_CHECK(base_intrinsics.scalar_type() == torch::kFloat32, "base intrinsics must be float32");
  Tensor K = base_intrinsics.detach().contiguous().clone();
  const int64_t E = K.size(0);
  Tensor D = torch::zeros({E, 4}, K.options());
  if (base_dist.defined()) {
    TORCH_CHECK(
      base_dist.numel() == E * 4 && base_dist.size(-1) == 4 &&
        base_dist.scalar_type() == torch::kFloat32,
      "base dist must be float32 [E,4]");
    D.copy_(base_dist.detach().reshape({E, 4}));
  }
  Tensor g = torch::zeros({E}, f2n::int_on(K.device()));
  int64_t G = 1;
  if (group.defined()) {
    TORCH_CHECK(group.numel() == E, "group: one entry per image");
    g.copy_(group.reshape({-1}));
    // a negative entry -1 - g is a fixed image of camera g
    if (E > 0) G = torch::where(g < 0, -1 - g, g).max().item<int64_t>() + 1;
  }
  gamma_ = register_parameter("gamma", torch::zeros({G, 8}, K.options()));
  base_K_ = register_buffer("base_K", K);
  base_dist_ = register_buffer("base_dist", D);
  group_ = register_buffer("group", g);
  learn_ = register_buffer("learn", torch::ones({8}, f2n::int_on(K.device())));
}

std::tuple<Tensor, Tensor> IntrinsicsRefiner::calibration() const
{
  return compose(base_K_, base_dist_, gamma_, group_, learn_);
}

void IntrinsicsRefiner::set_learned(const std::array<bool, 8> & mask)
{
  Tensor m = torch::empty({8}, torch::kInt32);
  auto flags = m.accessor<int32_t, 1>();
  for (int k = 0; k < 8; k++) flags[k] = mask[k] ? 1 : 0;
  torch::NoGradGuard no_grad;
  learn_.copy_(m);
}

void IntrinsicsRefiner::set_fixed(const Tensor & mask)
{
  TORCH_CHECK(mask.numel() == n_images(), "set_fixed: one entry per image");
  torch::NoGradGuard no_grad;
  Tensor camera = torch::where(group_ < 0, -1 - group_, group_);
  Tensor fixed = mask.reshape({-1}).ne(0).to(group_.device());
  group_.copy_(torch::where(fixed, -1 - camera, camera));
}

std::tuple<Rays, Tensor, Tensor> IntrinsicsRefiner::sample_random_rays(
  const Tensor & poses, int h, int w, int64_t batch_size, const Tensor & images,
  const Tensor & cam_idx, const Tensor & ij)
{
  TORCH_CHECK(poses.dim() == 3 && poses.size(0) == n_images(), "poses: one per image");
  const CameraBatch b =
    draw_camera_batch(n_images(), h, w, batch_size, cam_idx, ij, base_K_.device());
  auto [K, D] = calibration();
  Rays rays = get_rays_from_calibrated_cameras(poses, K, D, b.cam, b.ij, b.sorted);
  return {rays, gather_colors(images, b, h, w), b.cam};
}

std::vector<torch::optim::OptimizerParamGroup> IntrinsicsRefiner::optim_param_groups(float lr)
{
  auto opt = std::make_unique<torch::optim::AdamOptions>(lr);
  opt->betas(std::make_tuple(0.9, 0.99)).eps(1e-15);
  std::vector<torch::optim::OptimizerParamGroup> groups;
  groups.emplace_back(std::vector<Tensor>{gamma_}, std::move(opt));
  return groups;
}

Tensor IntrinsicsRefiner::corrections() const
{
  torch::NoGradGuard no_grad;
  auto [K, D] = calibration();
  Tensor dK = K - base_K_;
  return torch::cat(
    {torch::stack(
       {dK.select(1, 0).select(1, 0), dK.select(1, 1).select(1, 1), dK.select(1, 0).select(1, 2),
        dK.select(1, 1).select(1, 2)},
       -1),
     D - base_dist_},
    1);
}
