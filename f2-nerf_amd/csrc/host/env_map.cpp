// env_map.cpp -- see env_map.hpp.
#include "env_map.hpp"

#include "common.hpp"

using Tensor = torch::Tensor;

namespace
{

int64_t face_resolution(const Tensor & texture)
{
  TORCH_CHECK(
    texture.dim() == 4 && texture.size(0) == 6 && texture.size(1) == texture.size(2) &&
      texture.size(3) == 3 && f2n_envmap_texels((int)texture.size(1)) > 0,
    "texture must be [6,R,R,3] with R in 2 .. 4096");
  return texture.size(1);
}

Tensor ray_dirs(const Tensor & dirs)
{
  Tensor d = f2n::dev_f32(dirs.detach(), "dirs");
  TORCH_CHECK(d.dim() == 2 && d.size(1) == 3 && d.size(0) <= INT32_MAX, "dirs must be [n,3]");
  return d;
}

// One node: texture -> bg.  dirs, acc and flags are constants of the node.
class EnvQueryFn : public torch::autograd::Function<EnvQueryFn>
{
public:
  static Tensor forward(
    torch::autograd::AutogradContext * ctx, Tensor texture, Tensor dirs, Tensor acc, Tensor flags)
  {
    Tensor bg = f2n::envmap_query(dirs, texture);
    // (an undefined upstream gradient stays undefined: the backward then launches nothing)
    ctx->set_materialize_grads(false);
    ctx->save_for_backward({dirs, bg});
    // (plain handles, not saved variables: the kernels write both behind autograd's back, and
    // EnvMap::flags() resets the flags in place between a forward and its backward)
    ctx->saved_data["acc"] = acc;
    ctx->saved_data["flags"] = flags;
    ctx->saved_data["R"] = texture.size(1);
    return bg;
  }

  static torch::autograd::variable_list backward(
    torch::autograd::AutogradContext * ctx, torch::autograd::variable_list grad)
  {
    if (!grad[0].defined()) return {Tensor(), Tensor(), Tensor(), Tensor()};
    auto sv = ctx->get_saved_variables();
    const int64_t R = ctx->saved_data["R"].toInt();
    Tensor acc = ctx->saved_data["acc"].toTensor();
    f2n::envmap_bwd(sv[0], sv[1], grad[0], R, acc, ctx->saved_data["flags"].toTensor());
    Tensor d_tex = torch::empty({6, R, R, 3}, sv[1].options());
    f2n::envmap_grad_apply(acc, R, d_tex, false);
    return {d_tex, Tensor(), Tensor(), Tensor()};
  }
};

}  // namespace

Tensor f2n::envmap_query(const Tensor & dirs, const Tensor & texture)
{
  Tensor d = ray_dirs(dirs);
  Tensor tex = f2n::dev_f32(texture.detach(), "texture");
  const int64_t R = face_resolution(tex);
  Tensor bg = torch::empty({d.size(0), 3}, d.options());
  if (d.size(0) == 0) return bg;  // (an empty tensor has no pointer to pass)
  f2n::check(
    f2n_envmap_fwd(
      d.data_ptr<float>(), tex.data_ptr<float>(), (int)R, bg.data_ptr<float>(), (int)d.size(0),
      f2n::current_stream(d)),
    "f2n_envmap_fwd");
  return bg;
}

void f2n::envmap_bwd(
  const Tensor & dirs, const Tensor & bg, const Tensor & d_bg, int64_t R, Tensor acc, Tensor flags)
{
  Tensor d = ray_dirs(dirs);
  Tensor b = f2n::dev_f32(bg.detach(), "bg");
  Tensor g = f2n::dev_f32(d_bg.detach(), "d_bg");
  const int64_t n = d.size(0);
  TORCH_CHECK(b.numel() == n * 3 && g.numel() == n * 3, "bg and d_bg must be [n,3]");
  TORCH_CHECK(f2n_envmap_texels((int)R) > 0, "R must be in 2 .. 4096");
  TORCH_CHECK(
    acc.is_cuda() && acc.scalar_type() == torch::kInt64 && acc.is_contiguous() &&
      acc.numel() == 3 * f2n_envmap_texels((int)R),
    "acc must be int64 [6*R*R*3] on the GPU");
  TORCH_CHECK(
    flags.is_cuda() && flags.scalar_type() == torch::kInt32 && flags.numel() == 1,
    "flags must be int32 [1] on the GPU");
  if (n == 0) return;
  f2n::check(
    f2n_envmap_bwd(
      d.data_ptr<float>(), b.data_ptr<float>(), g.data_ptr<float>(), (int)R, acc.data_ptr<int64_t>(),
      flags.data_ptr<int32_t>(), (int)n, f2n::current_stream(d)),
    "f2n_envmap_bwd");
}

void f2n::envmap_grad_apply(Tensor acc, int64_t R, Tensor d_tex, bool accumulate)
{
  TORCH_CHECK(f2n_envmap_texels((int)R) > 0, "R must be in 2 .. 4096");
  const int64_t n = 3 * f2n_envmap_texels((int)R);
  TORCH_CHECK(
    acc.is_cuda() && acc.scalar_type() == torch::kInt64 && acc.is_contiguous() && acc.numel() == n,
    "acc must be int64 [6*R*R*3] on the GPU");
  TORCH_CHECK(
    d_tex.is_cuda() && d_tex.scalar_type() == torch::kFloat32 && d_tex.is_contiguous() &&
      d_tex.numel() == n,
    "d_tex must be float32 [6,R,R,3] on the GPU");
  f2n::check(
    f2n_envmap_grad_apply(
      acc.data_ptr<int64_t>(), (int)R, d_tex.data_ptr<float>(), accumulate ? 1 : 0,
      f2n::current_stream(acc)),
    "f2n_envmap_grad_apply");
}

f2n::EnvMap::EnvMap(int64_t resolution, const torch::Device & device)
{
  TORCH_CHECK(
    resolution <= INT32_MAX && f2n_envmap_texels((int)resolution) > 0,
    "EnvMap: the face resolution must be in 2 .. 4096");
  texture_ = register_parameter(
    "texture", torch::zeros({6, resolution, resolution, 3}, f2n::float_on(device)));
  acc_ = torch::zeros(
    {18 * resolution * resolution}, torch::TensorOptions().dtype(torch::kInt64).device(device));
  flags_ = torch::zeros({1}, f2n::int_on(device));
}

Tensor f2n::EnvMap::query(const Tensor & dirs)
{
  if (!(torch::GradMode::is_enabled() && texture_.requires_grad()))
    return envmap_query(dirs, texture_);
  return EnvQueryFn::apply(texture_, ray_dirs(dirs), acc_, flags_);
}

std::vector<torch::optim::OptimizerParamGroup> f2n::EnvMap::optim_param_groups(float lr)
{
  auto opt = std::make_unique<torch::optim::AdamOptions>(lr);
  opt->betas(std::make_tuple(0.9, 0.99)).eps(1e-15);
  std::vector<torch::optim::OptimizerParamGroup> groups;
  groups.emplace_back(std::vector<Tensor>{texture_}, std::move(opt));
  return groups;
}

int f2n::EnvMap::flags()
{
  const int f = flags_.item<int>();
  flags_.zero_();
  return f;
}
