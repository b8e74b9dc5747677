// robust_loss.cpp -- see robust_loss.hpp
#include "robust_loss.hpp"

#include <algorithm>

#include "common.hpp"

namespace f2n
{

RobustWeights robust_weights(
  const Tensor & colors_in, const Tensor & target_in, const Tensor & ray_weight,
  const RobustLoss & opt)
{
  torch::NoGradGuard no_grad;
  const Tensor colors = dev_f32(colors_in.detach(), "colors");
  const Tensor target = dev_f32(target_in.detach(), "target");
  TORCH_CHECK(
    colors.dim() == 2 && colors.size(1) == 3 && colors.sizes() == target.sizes(),
    "robust_weights: colors and target must both be [n_rays, 3]");
  const int64_t n = colors.size(0);
  TORCH_CHECK(n >= 1 && n < (1 << 24), "robust_weights: 1 <= n_rays < 2^24");
  Tensor m;
  if (ray_weight.defined()) {
    m = dev_f32(ray_weight.detach(), "ray_weight").reshape({-1});
    TORCH_CHECK(m.numel() == n, "ray_weight must be [n_rays]");
  }
  const auto fopt = colors.options();
  RobustWeights out;
  out.weight = torch::empty({n}, fopt);
  out.omega = torch::empty({n}, fopt.dtype(torch::kUInt8));
  out.stats = torch::empty({4}, fopt);
  Tensor workspace =
    torch::empty({f2n_robust_workspace_words((int)n)}, fopt.dtype(torch::kInt32));
  check(
    f2n_robust_weights(
      colors.data_ptr<float>(), target.data_ptr<float>(), fptr(m), (int)n, opt.patch,
      opt.patch > 0 ? std::min(opt.nbhd, opt.patch) : opt.nbhd, std::min(opt.quantile, 1.f),
      opt.box_thresh, opt.nbhd_thresh, out.weight.data_ptr<float>(), out.omega.data_ptr<uint8_t>(),
      out.stats.data_ptr<float>(), (uint32_t *)workspace.data_ptr<int32_t>(),
      current_stream(colors)),
    "f2n_robust_weights");
  return out;
}

}  // namespace f2n
