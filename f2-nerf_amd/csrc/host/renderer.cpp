// renderer.cpp -- see renderer.hpp.  Arithmetic per reference src/renderer.cpp:18-197.
#include "renderer.hpp"

#include "kernel_timer.hpp"

#include "ragged_ops.hpp"
#include "rays.hpp"
#include "robust_loss.hpp"

#include <c10/hip/HIPGuard.h>
#include <hip/hip_runtime_api.h>

#include <limits>

using Tensor = torch::Tensor;

f2n::HostCount::~HostCount()
{
  if (event_) hipEventDestroy((hipEvent_t)event_);
  if (pinned_) hipHostFree(pinned_);
}

void f2n::HostCount::request(const torch::Tensor & device_int32, void * stream)
{
  TORCH_CHECK(
    device_int32.is_cuda() && device_int32.scalar_type() == torch::kInt32 && device_int32.numel() == 1,
    "HostCount: one int32 on the device");
  const int device = (int)device_int32.device().index();
  c10::hip::HIPGuard on_device(device);
  if (pending_) {  // a read nobody waited for (an exception between request and wait): drain it
    hipEventSynchronize((hipEvent_t)event_);
    pending_ = false;
  }
  if (!pinned_)
    TORCH_CHECK(hipHostMalloc((void **)&pinned_, sizeof(int32_t), hipHostMallocDefault) == hipSuccess,
                "HostCount: pinned allocation failed");
  if (!event_ || device_ != device) {
    // an event belongs to the device it was created on: a Renderer whose inputs moved to another
    // GPU gets a new one (the pinned word is host memory and stays)
    if (event_) hipEventDestroy((hipEvent_t)event_);
    hipEvent_t ev;
    TORCH_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess,
                "HostCount: event creation failed");
    event_ = ev;
    device_ = device;
  }
  TORCH_CHECK(
    hipMemcpyAsync(pinned_, device_int32.data_ptr<int32_t>(), sizeof(int32_t), hipMemcpyDeviceToHost,
                   (hipStream_t)stream) == hipSuccess &&
      hipEventRecord((hipEvent_t)event_, (hipStream_t)stream) == hipSuccess,
    "HostCount: copy failed");
  pending_ = true;
}

int64_t f2n::HostCount::wait()
{
  TORCH_CHECK(pending_, "HostCount: wait() without request()");
  TORCH_CHECK(hipEventSynchronize((hipEvent_t)event_) == hipSuccess, "HostCount: wait failed");
  pending_ = false;
  return (int64_t)*pinned_;
}

// ---- helpers and autograd nodes of the routes ----------------------------------------------------

namespace
{

// Exclusive scan of per-ray counts: bounds [n, 2] and their total [1], both left on the device.
std::pair<Tensor, Tensor> bounds_from_counts(const Tensor & counts, void * stream)
{
  const int n = (int)counts.size(0);
  Tensor bounds = torch::empty({n, 2}, counts.options()), total = torch::empty({1}, counts.options());
  f2n::check(
    f2n_bounds_from_counts(
      counts.data_ptr<int32_t>(), bounds.data_ptr<int32_t>(), total.data_ptr<int32_t>(), n, stream),
    "f2n_bounds_from_counts");
  return {bounds, total};
}

// colors [n,3], depths [n] and weights (ragged) of the bucketed order back into the caller's order:
// row i of the caller is row inv[i] of the bucketed storage; the backward is the inverse gather
// (map perm).  `rows`: every ray kept all S samples, the weights are plain [n, S] rows.  `per_ray`:
// one more float per ray that rides along (the distortion loss), or an empty tensor: nothing moves.
class RayUnpermuteFn : public torch::autograd::Function<RayUnpermuteFn>
{
public:
  static torch::autograd::variable_list forward(
    torch::autograd::AutogradContext * ctx, Tensor colors, Tensor depths, Tensor weights,
    Tensor per_ray, Tensor perm, Tensor inv, Tensor bounds_sorted, Tensor bounds_caller, int64_t S,
    bool rows)
  {
    colors = f2n::dev_f32(colors, "colors");
    depths = f2n::dev_f32(depths, "depths");
    weights = f2n::dev_f32(weights, "weights");
    per_ray = f2n::dev_f32(per_ray, "per-ray term");
    const int n = (int)perm.size(0);
    TORCH_CHECK(per_ray.numel() == 0 || per_ray.numel() == n, "per-ray term shape");
    void * s = f2n::current_stream(colors);
    Tensor c = torch::empty_like(colors), d = torch::empty_like(depths), w = torch::empty_like(weights);
    Tensor x = torch::empty_like(per_ray);
    gather(colors, depths, weights, c, d, w, inv, bounds_sorted, bounds_caller, n, S, rows, s);
    gather_per_ray(per_ray, x, inv, n, s);
    ctx->save_for_backward({perm, bounds_sorted, bounds_caller});
    ctx->saved_data["S"] = S;
    ctx->saved_data["rows"] = rows;
    // (the backward gathers the gradients that exist: no zeros made and moved for the others)
    ctx->set_materialize_grads(!f2n::lean_grads());
    return {c, d, w, x};
  }

  static torch::autograd::variable_list backward(
    torch::autograd::AutogradContext * ctx, torch::autograd::variable_list g)
  {
    auto saved = ctx->get_saved_variables();
    const Tensor & perm = saved[0];
    const int n = (int)perm.size(0);
    const int64_t S = ctx->saved_data["S"].toInt();
    const bool rows = ctx->saved_data["rows"].toBool();
    Tensor gc = g[0].defined() ? f2n::dev_f32(g[0], "grad colors") : Tensor();
    Tensor gd = g[1].defined() ? f2n::dev_f32(g[1], "grad depths") : Tensor();
    Tensor gw = g[2].defined() ? f2n::dev_f32(g[2], "grad weights") : Tensor();
    Tensor dc = gc.defined() ? torch::empty_like(gc) : Tensor();
    Tensor dd = gd.defined() ? torch::empty_like(gd) : Tensor();
    Tensor dw = gw.defined() ? torch::empty_like(gw) : Tensor();
    Tensor gx = g[3].defined() ? f2n::dev_f32(g[3], "grad per-ray term") : Tensor();
    Tensor dx = gx.defined() ? torch::empty_like(gx) : Tensor();
    void * s = f2n::current_stream(perm);
    gather(gc, gd, gw, dc, dd, dw, perm, saved[2], saved[1], n, S, rows, s);
    if (gx.defined()) gather_per_ray(gx, dx, perm, n, s);
    return {dc, dd, dw, dx, Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
  }

private:
  static void gather_per_ray(const Tensor & x, Tensor & x_out, const Tensor & map, int n, void * s)
  {
    if (x.numel() == 0) return;
    f2n::check(
      f2n_gather_rows(f2n::fptr(x), x_out.data_ptr<float>(), map.data_ptr<int32_t>(), n, 1, s),
      "f2n_gather_rows");
  }

  // dst = src through `map` for each defined pair; segment bounds src_b -> dst_b
  static void gather(
    const Tensor & c, const Tensor & d, const Tensor & w, Tensor & c_out, Tensor & d_out,
    Tensor & w_out, const Tensor & map, const Tensor & src_b, const Tensor & dst_b, int n, int64_t S,
    bool rows, void * s)
  {
    const int32_t * m = map.data_ptr<int32_t>();
    if (c.defined())
      f2n::check(f2n_gather_rows(f2n::fptr(c), c_out.data_ptr<float>(), m, n, 3, s), "f2n_gather_rows");
    if (d.defined())
      f2n::check(f2n_gather_rows(f2n::fptr(d), d_out.data_ptr<float>(), m, n, 1, s), "f2n_gather_rows");
    if (!w.defined()) return;
    if (rows)
      f2n::check(
        f2n_gather_rows(f2n::fptr(w), w_out.data_ptr<float>(), m, n, (int)S, s), "f2n_gather_rows");
    else
      f2n::check(
        f2n_gather_segments(
          f2n::fptr(w), f2n::iptr(src_b), w_out.data_ptr<float>(), f2n::iptr(dst_b), m, n, s),
        "f2n_gather_segments");
  }
};

// Per-ray rows [n, C] of the bucketed order back into the caller's order (the depth terms): row i of
// the caller is row inv[i] of the bucketed storage, the backward is the inverse gather (map perm).
class RayRowsUnpermuteFn : public torch::autograd::Function<RayRowsUnpermuteFn>
{
public:
  static torch::autograd::variable_list forward(
    torch::autograd::AutogradContext * ctx, Tensor rows, Tensor perm, Tensor inv)
  {
    rows = f2n::dev_f32(rows, "per-ray rows");
    TORCH_CHECK(rows.dim() == 2 && rows.size(0) == perm.size(0), "per-ray rows shape");
    ctx->save_for_backward({perm});
    ctx->set_materialize_grads(!f2n::lean_grads());
    return {gather(rows, inv)};
  }

  static torch::autograd::variable_list backward(
    torch::autograd::AutogradContext * ctx, torch::autograd::variable_list g)
  {
    if (!g[0].defined()) return {Tensor(), Tensor(), Tensor()};
    return {gather(f2n::dev_f32(g[0], "grad per-ray rows"), ctx->get_saved_variables()[0]), Tensor(),
            Tensor()};
  }

private:
  static Tensor gather(const Tensor & src, const Tensor & map)
  {
    Tensor dst = torch::empty_like(src);
    if (src.numel() > 0)
      f2n::check(
        f2n_gather_rows(
          f2n::fptr(src), dst.data_ptr<float>(), map.data_ptr<int32_t>(), (int)src.size(0),
          (int)src.size(1), f2n::current_stream(src)),
        "f2n_gather_rows");
    return dst;
  }
};

// Identity on the encoding of the kept samples whose backward also forms the rays' gradient from
// the encoding's (f2n_hash_rays_grad).  The encoding's gradient is handed on untouched, so the table
// gradient (Hash3DAnchoredFunction) and everything else upstream see exactly what they see without
// it.  pts / t / bounds: the kept samples (raw positions) and their segments, as the sampler made
// them from these rays.
class RayGradFn : public torch::autograd::Function<RayGradFn>
{
public:
  static torch::autograd::variable_list forward(
    torch::autograd::AutogradContext * ctx, Tensor enc, Tensor rays_o, Tensor rays_d, Tensor pts,
    Tensor t, Tensor bounds, torch::IValue hash3d_info)
  {
    Hash3DAnchored * field = hash3d_info.toCustomClass<Hash3DAnchoredInfo>()->hash3d_;
    ctx->saved_data["hash3d_info"] = hash3d_info;
    ctx->saved_data["n_rays"] = rays_o.size(0);
    ctx->saved_data["L_walk"] = (int64_t)field->walk_levels();  // the levels the encoding walked
    ctx->save_for_backward(
      {f2n::dev_f32(pts.detach(), "kept pts"), f2n::dev_f32(t.detach(), "kept t"),
       f2n::dev_i32(bounds, "kept bounds"), f2n::dev_f32(rays_d.detach(), "rays_d"),
       field->table_f16()});
    return {enc};
  }

  static torch::autograd::variable_list backward(
    torch::autograd::AutogradContext * ctx, torch::autograd::variable_list grad)
  {
    const Tensor & g_enc = grad[0];
    const bool want_o = ctx->needs_input_grad(1), want_d = ctx->needs_input_grad(2);
    Tensor d_o, d_d;
    if (want_o || want_d) {
      auto sv = ctx->get_saved_variables();
      const Tensor &pts = sv[0], &t = sv[1], &bounds = sv[2], &rays_d = sv[3], &table16 = sv[4];
      const int64_t n_rays = ctx->saved_data["n_rays"].toInt();
      d_o = torch::empty({n_rays, 3}, rays_d.options());
      d_d = torch::empty({n_rays, 3}, rays_d.options());
      if (!g_enc.defined()) {
        d_o.zero_();
        d_d.zero_();
      } else {
        Hash3DAnchored * field =
          ctx->saved_data["hash3d_info"].toCustomClass<Hash3DAnchoredInfo>()->hash3d_;
        const int64_t n = pts.size(0);
        const f2n::FieldArgs fa = field->kernel_args(table16);
        const int L_walk = (int)ctx->saved_data["L_walk"].toInt();
        const auto [g, ld_point, ld_chan] = f2n::encoding_grad_strides(g_enc, n, (int64_t)fa.L * fa.F);
        void * stream = f2n::current_stream(pts);
        if (field->options_.exact_point_grad) {
          // the encoding's true derivative instead of quirk Q5: same kept samples, same sums
          f2n::ScopedKernelTimer timer("hash_rays_grad_exact", stream, (double)n);
          f2n::check(
            f2n_hash_rays_grad_exact(
              pts.data_ptr<float>(), t.data_ptr<float>(), bounds.data_ptr<int32_t>(),
              rays_d.data_ptr<float>(), fa.table, fa.primes, fa.bias, fa.mul, g.data_ptr<float>(),
              ld_point, ld_chan, d_o.data_ptr<float>(), d_d.data_ptr<float>(), (int)n_rays, L_walk,
              fa.F, fa.T, fa.level_stride, stream),
            "f2n_hash_rays_grad_exact");
        } else {
          f2n::ScopedKernelTimer timer("hash_rays_grad", stream, (double)n);
          f2n::check(
            f2n_hash_rays_grad(
              pts.data_ptr<float>(), t.data_ptr<float>(), bounds.data_ptr<int32_t>(),
              rays_d.data_ptr<float>(), fa.table, fa.primes, fa.bias, fa.mul, g.data_ptr<float>(),
              ld_point, ld_chan, d_o.data_ptr<float>(), d_d.data_ptr<float>(), (int)n_rays, L_walk,
              fa.F, fa.T, fa.level_stride, 128.f /* hash_3d_anchored.cu:190 */, stream),
            "f2n_hash_rays_grad");
        }
      }
    }
    return {g_enc, want_o ? d_o : Tensor(), want_d ? d_d : Tensor(), Tensor(), Tensor(), Tensor(),
            Tensor()};
  }
};

}  // namespace

Tensor f2n::ray_order(const Tensor & rays_d_in)
{
  const Tensor rays_d = f2n::dev_f32(rays_d_in.detach(), "rays_d");
  TORCH_CHECK(rays_d.dim() == 2 && rays_d.size(1) == 3, "rays_d must be [n, 3]");
  const int n = (int)rays_d.size(0);
  Tensor keys = torch::empty({n}, f2n::int_on(rays_d.device()));
  f2n::check(
    f2n_ray_keys(rays_d.data_ptr<float>(), keys.data_ptr<int32_t>(), n, f2n::current_stream(rays_d)),
    "f2n_ray_keys");
  // stable: equal keys keep the caller's order, the permutation is deterministic
  return std::get<1>(keys.sort(/*stable=*/true, /*dim=*/0, /*descending=*/false));
}

Renderer::Renderer(int n_images, const RendererOptions & opt) : options_(opt)
{
  pts_sampler_ = std::make_shared<PtsSampler>(opt.sampler);

  scene_field_ = std::make_shared<Hash3DAnchored>(opt.field);
  register_module("scene_field", scene_field_);

  shader_ = std::make_shared<SHShader>(opt.field.device);
  register_module("shader", shader_);

  app_emb_ = torch::randn({n_images, 16}, f2n::float_on(opt.field.device)) * .1f;
  app_emb_.requires_grad_(true);
  register_parameter("app_emb", app_emb_);
}

RenderResult Renderer::render(
  const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx, RunningMode mode)
{
  return render(rays_o, rays_d, emb_idx, mode, Tensor(), Tensor());
}

RenderResult Renderer::render(
  const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx, RunningMode mode,
  const Tensor & noise_in, const Tensor & bg_in)
{
  return render_routed(rays_o, rays_d, emb_idx, mode, noise_in, bg_in, false, LossOutputs());
}

RenderResult Renderer::render_for_loss(
  const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx, RunningMode mode,
  const Tensor & noise_in, const Tensor & bg_in, const LossOutputs & want)
{
  return render_routed(rays_o, rays_d, emb_idx, mode, noise_in, bg_in, true, want);
}

RenderResult Renderer::render_routed(
  const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx, RunningMode mode,
  const Tensor & noise_in, const Tensor & bg_in, bool for_loss, const LossOutputs & want)
{
  const int64_t n_rays = rays_o.size(0);
  if (want.depth_target.defined()) {
    TORCH_CHECK(want.depth_target.numel() == n_rays, "depth_target must be [n_rays]");
    TORCH_CHECK(
      std::isfinite(want.depth_eps) && want.depth_eps >= 0.f, "depth_eps must be finite and >= 0");
  }
  const auto fopt = f2n::float_on(rays_o.device());
  // the uniform draw first, as ever (the generator stream does not depend on the route); the lean
  // dense route hands it to its sampler raw, every other route gets draw_noise's two passes over it
  Tensor raw = noise_in.defined() ? Tensor()
                                  : pts_sampler_->draw_noise_raw(n_rays, mode, rays_o.device());
  Tensor bg_color = background_or_default(bg_in, rays_d, mode, n_rays);
  if (n_rays <= 0) {
    record_kept(0);
    RenderResult none{
      bg_color, torch::zeros({n_rays}, fopt), torch::full({n_rays}, 512.f, fopt), Tensor()};
    if (want.dist) none.weight_dist = torch::zeros({n_rays}, fopt);
    if (want.depth_target.defined()) none.depth_terms = torch::zeros({n_rays, 3}, fopt);
    if (options_.normals) none.normals = torch::zeros({n_rays, 3}, fopt);
    if (want.opacity) none.opacity = torch::zeros({n_rays}, fopt);
    return none;
  }
  Route route = choose_route(rays_o, rays_d, bg_color);
  route.noise_raw = route.lean && raw.defined();
  route.want_var = route.lean && route.bucketed && for_loss;
  route.want = want;
  if (want.depth_target.defined())
    route.want.depth_target =
      f2n::dev_f32(want.depth_target.detach(), "depth_target").reshape({n_rays});
  const Tensor noise = noise_in.defined() ? noise_in
                       : route.noise_raw  ? raw
                                          : PtsSampler::cook_noise(raw);
  RenderResult res = route.first_pass == Route::OpByOp
                       ? render_op_by_op(rays_o, rays_d, emb_idx, mode, noise, bg_color, route)
                       : render_fused(rays_o, rays_d, emb_idx, mode, noise, bg_color, route);
  if (options_.check_finite) CHECK(std::isfinite(res.colors.mean().item<float>()));
  return res;
}

Tensor Renderer::background_or_default(
  const Tensor & bg_in, const Tensor & rays_d, RunningMode mode, int64_t n_rays) const
{
  if (bg_in.defined()) return bg_in;
  if (background_) return background_->query(rays_d);
  const auto fopt = f2n::float_on(rays_d.device());
  return (mode == RunningMode::TRAIN) ? torch::rand({n_rays, 3}, fopt)
                                      : torch::ones({n_rays, 3}, fopt) * .5f;
}

bool Renderer::fused_net_applies() const
{
  const auto & field = scene_field_->options_;
  return options_.fused_shade && f2n::shade_supported(field.n_levels * field.n_channels) &&
         field.mlp_out_dim == 16;
}

Renderer::Route Renderer::choose_route(
  const Tensor & rays_o, const Tensor & rays_d, const Tensor & bg_color) const
{
  Route route;
  const auto & field = scene_field_->options_;
  route.fused_net = fused_net_applies();
  const bool rays_need_grad =
    torch::GradMode::is_enabled() && (rays_o.requires_grad() || rays_d.requires_grad());
  // the fused kernels work on detached copies; shade() hands the encoding's gradient back to these
  if (rays_need_grad) route.grad_rays = Rays{rays_o, rays_d};
  if (!options_.fused || (rays_need_grad && !(options_.fused_ray_grad && route.fused_net)))
    route.first_pass = Route::OpByOp;
  else if (occupancy_)
    route.first_pass = Route::March;  // the dense pass encodes every sample: the cost a grid removes
  else if (route.fused_net && (options_.dense_first_pass == 1 ||
                               (options_.dense_first_pass < 0 && last_kept_fraction_ > 0.4f)))
    route.first_pass = Route::Dense;
  else
    route.first_pass = Route::March;
  // bg_color or rays that carry a gradient stay on the caller's order (the bucketed route
  // detaches them)
  route.bucketed = route.first_pass == Route::Dense &&
                   rays_o.size(0) >= options_.ray_order_min_rays &&
                   f2n_get_option(F2N_OPT_RAY_ORDER) == 0 && !rays_need_grad &&
                   !(torch::GradMode::is_enabled() && bg_color.requires_grad());
  const int64_t n_rays = rays_o.size(0), S = pts_sampler_->options_.max_samples;
  route.lean = route.first_pass == Route::Dense && f2n_get_option(F2N_OPT_DENSE_LEAN) == 0 &&
               !rays_need_grad && !(torch::GradMode::is_enabled() && bg_color.requires_grad()) &&
               f2n::shade_rays_applies(n_rays * S, n_rays, S);
  // normals need the kept samples' world positions, which neither of the two carries
  if (options_.normals) route.bucketed = route.lean = false;
  return route;
}

void Renderer::record_kept(int64_t n_kept, int64_t n_all)
{
  last_n_samples_ = n_kept;
  if (n_all >= 0) last_kept_fraction_ = n_all > 0 ? (float)n_kept / (float)n_all : 0.f;
}

// ---- op-by-op route (the reference's own sequence on the drop-in operators) ----------------------

RenderResult Renderer::render_op_by_op(
  const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx, RunningMode mode,
  const Tensor & noise, const Tensor & bg_color, const Route & route)
{
  const int64_t n_rays = rays_o.size(0);
  const int64_t S = pts_sampler_->options_.max_samples;
  // (rays with a gradient: the same samples, their positions differentiable in the rays)
  SampleResultFlex all = route.grad_rays.origins.defined()
                           ? pts_sampler_->get_samples_grad(rays_o, rays_d, noise)
                           : pts_sampler_->get_samples(rays_o, rays_d, noise);

  auto density_act = [](const Tensor & x) {
    return torch::autograd::TruncExp::apply(x - 3.f)[0];
  };

  SampleResultFlex kept;
  {
    Tensor scene_feat = scene_field_->query(all.pts);
    Tensor density = density_act(scene_feat.index({Slc(), Slc(0, 1)}));
    Tensor sec = density.index({Slc(), 0}) * all.dt;
    Tensor occupied;
    if (occupancy_) {
      occupied = occupancy_->occupied(all.pts);
      sec = sec * occupied.to(sec.scalar_type());
    }
    Tensor acc = FlexOps::AccumulateSum(sec, all.pts_idx_bounds, false);
    Tensor mask = torch::exp(-acc) > options_.early_stop_trans;
    if (occupancy_) mask = mask.logical_and(occupied);
    Tensor mask_idx = torch::where(mask)[0];
    kept.pts = all.pts.index({mask_idx}).contiguous();
    kept.dirs = all.dirs.index({mask_idx}).contiguous();
    kept.dt = all.dt.index({mask_idx}).contiguous();
    kept.t = all.t.index({mask_idx}).contiguous();
    Tensor num = mask.reshape({n_rays, S}).sum(1);
    Tensor cum = torch::cumsum(num, 0);
    kept.pts_idx_bounds = torch::stack({cum - num, cum}, 1).to(torch::kInt32).contiguous();
  }
  record_kept(kept.pts.size(0));

  Tensor scene_feat = scene_field_->query(kept.pts);
  Tensor density = density_act(scene_feat.index({Slc(), Slc(0, 1)}));
  Tensor sampled_colors = shade_aten(scene_feat, kept, emb_idx, mode);
  Tensor sampled_t = (kept.t + 1e-2f).contiguous();
  Tensor sec = density.index({Slc(), 0}) * kept.dt;
  Tensor alphas = 1.f - torch::exp(-sec);
  Tensor idx = kept.pts_idx_bounds;
  Tensor trans = torch::exp(-FlexOps::AccumulateSum(sec, idx, false));
  Tensor weights = trans * alphas;
  Tensor last_trans = torch::exp(-FlexOps::Sum(sec, idx));
  Tensor colors = FlexOps::Sum(weights.unsqueeze(-1) * sampled_colors, idx) +
                  last_trans.unsqueeze(-1) * bg_color;
  Tensor depths = FlexOps::Sum(weights * sampled_t, idx) / (1.f - last_trans + 1e-4f);
  RenderResult res{colors, depths, weights, idx};
  per_ray_terms(res, weights, kept, route);
  if (options_.normals) res.normals = ray_normals(kept, weights);
  return res;
}

// Where the kept samples' weights, t and dt lie side by side -- on every route, thinned by an
// occupancy grid or not; t and dt get no gradient.  The opacity of a ray is the plain sum of its kept
// samples' weights: the segment sum the op-by-op route composites with.
void Renderer::per_ray_terms(
  RenderResult & res, const Tensor & weights, const SampleResultFlex & kept, const Route & route)
{
  const Tensor & idx = kept.pts_idx_bounds;
  const LossOutputs & want = route.want;
  if (want.dist) res.weight_dist = CustomOps::WeightDist(weights, kept.t, kept.dt, idx);
  if (want.depth_target.defined())
    res.depth_terms =
      CustomOps::DepthSight(weights, kept.t, kept.dt, idx, want.depth_target, want.depth_eps);
  if (want.opacity) res.opacity = FlexOps::Sum(weights, idx);
}

// ---- fused routes --------------------------------------------------------------------------------

RenderResult Renderer::render_fused(
  const Tensor & rays_o_raw, const Tensor & rays_d_raw, const Tensor & emb_idx, RunningMode mode,
  const Tensor & noise_raw, const Tensor & bg_color, const Route & route)
{
  Tensor rays_o = f2n::dev_f32(rays_o_raw.detach(), "rays_o");
  Tensor rays_d = f2n::dev_f32(rays_d_raw.detach(), "rays_d");
  Tensor noise = noise_raw.defined() ? f2n::dev_f32(noise_raw, "noise") : Tensor();
  const int n_rays = (int)rays_o.size(0);
  const int S = pts_sampler_->options_.max_samples;
  TORCH_CHECK(!noise.defined() || noise.numel() == (int64_t)n_rays * S, "noise shape");
  if (route.first_pass == Route::Dense)
    return route.bucketed
             ? render_dense_bucketed(rays_o, rays_d, emb_idx, mode, noise, bg_color, route)
             : render_dense(rays_o, rays_d, emb_idx, mode, noise, bg_color, route);

  void * stream = f2n::current_stream(rays_o);
  Hash3DAnchored & field = *scene_field_;
  SampleResultFlex kept;
  {
    // First pass (renderer.cpp:58-90): density only, never differentiated by the loss.
    torch::NoGradGuard no_grad;
    Tensor table16 = field.table_f16();
    const f2n::FieldArgs g = field.kernel_args(table16);
    auto head = field.density_head();
    Tensor counts = torch::empty({n_rays}, f2n::int_on(rays_o.device()));
    Tensor len;  // with a grid: the prefix lengths the counts were thinned from
    if (occupancy_) {
      TORCH_CHECK(
        occupancy_->words().device() == rays_o.device(), "the occupancy grid lives on another device");
      len = torch::empty_like(counts);
      f2n::ScopedKernelTimer timer("density_march_occ", stream, (double)n_rays);
      f2n::check(
        f2n_density_march_occ(
          rays_o.data_ptr<float>(), rays_d.data_ptr<float>(), f2n::fptr(noise), g.table, g.primes,
          g.bias, g.mul, head.first.data_ptr<float>(), head.second.data_ptr<float>(),
          occupancy_->words_ptr(), (int)occupancy_->resolution(), counts.data_ptr<int32_t>(),
          len.data_ptr<int32_t>(), n_rays, S, pts_sampler_->options_.step, g.L_walk, g.F, g.T,
          g.level_stride, options_.early_stop_trans, 3.f, stream),
        "f2n_density_march_occ");
    } else {
      f2n::ScopedKernelTimer timer("density_march", stream, (double)n_rays);
      f2n::check(
      f2n_density_march(
        rays_o.data_ptr<float>(), rays_d.data_ptr<float>(), f2n::fptr(noise), g.table, g.primes,
        g.bias, g.mul, head.first.data_ptr<float>(), head.second.data_ptr<float>(),
        counts.data_ptr<int32_t>(), n_rays, S, pts_sampler_->options_.step, g.L_walk, g.F, g.T,
        g.level_stride, options_.early_stop_trans, 3.f, stream),
      "f2n_density_march");
    }
    auto [bounds, total] = bounds_from_counts(counts, stream);
    const int64_t n_kept = total.item<int>();  // the one host sync of this route (sizes tensors)
    record_kept(n_kept, (int64_t)n_rays * S);
    kept = compact_samples(rays_o, rays_d, noise, bounds, n_kept, len);
  }
  return shade_and_composite(kept, emb_idx, mode, bg_color, route);
}

// The dense pass on the rays sorted into pixel-compact bundles (f2n::ray_order): 64 consecutive rays
// are one ray tile of the encode, and a compact blob of pixels touches fewer table lines per gather
// than a row strip.  Every ray keeps its own noise row, background colour and image id, so each
// ray's samples, encoding, colour and weights are those of the caller's order; only their storage
// order differs, and the results are gathered back (bounds re-scanned in the caller's order).
RenderResult Renderer::render_dense_bucketed(
  const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx_in, RunningMode mode,
  const Tensor & noise, const Tensor & bg_in, const Route & route)
{
  const int n_rays = (int)rays_o.size(0);
  const int64_t S = pts_sampler_->options_.max_samples;
  const auto iopt = f2n::int_on(rays_o.device());
  void * stream = f2n::current_stream(rays_o);
  const Tensor emb_idx = (mode == RunningMode::TRAIN && emb_idx_in.defined())
                           ? f2n::dev_i32(emb_idx_in, "emb_idx") : Tensor();
  const Tensor bg = f2n::dev_f32(bg_in.detach(), "bg_color");
  TORCH_CHECK(bg.numel() == (int64_t)n_rays * 3, "bg_color shape");
  TORCH_CHECK(!emb_idx.defined() || emb_idx.numel() == n_rays, "emb_idx shape");

  const Tensor order = f2n::ray_order(rays_d);
  Tensor perm = torch::empty({n_rays}, iopt), inv = torch::empty({n_rays}, iopt);
  Tensor o_p = torch::empty_like(rays_o), d_p = torch::empty_like(rays_d), bg_p = torch::empty_like(bg);
  Tensor emb_p = emb_idx.defined() ? torch::empty_like(emb_idx) : Tensor();
  // (lean: the noise stays where it is, the sampler reads row perm[j] for bucketed ray j)
  const bool move_noise = noise.defined() && !route.lean;
  Tensor noise_p = move_noise ? torch::empty_like(noise) : Tensor();
  f2n::check(
    f2n_ray_permute(
      order.data_ptr<int64_t>(), n_rays, (int)S, rays_o.data_ptr<float>(), rays_d.data_ptr<float>(),
      f2n::iptr(emb_idx), bg.data_ptr<float>(), move_noise ? f2n::fptr(noise) : nullptr,
      perm.data_ptr<int32_t>(),
      o_p.data_ptr<float>(), d_p.data_ptr<float>(),
      emb_idx.defined() ? emb_p.data_ptr<int32_t>() : nullptr, bg_p.data_ptr<float>(),
      f2n::fptr_mut(noise_p), inv.data_ptr<int32_t>(), stream),
    "f2n_ray_permute");
  // a depth target travels with its ray: bucketed ray j is the caller's ray perm[j]
  Route route_p = route;
  if (route.want.depth_target.defined()) {
    route_p.want.depth_target = torch::empty_like(route.want.depth_target);
    f2n::check(
      f2n_gather_rows(
        route.want.depth_target.data_ptr<float>(), route_p.want.depth_target.data_ptr<float>(),
        perm.data_ptr<int32_t>(), n_rays, 1, stream),
      "f2n_gather_rows");
  }
  RenderResult r = route.lean
                     ? render_dense(o_p, d_p, emb_p, mode, noise, bg_p, route_p, perm)
                     : render_dense(o_p, d_p, emb_p, mode, noise_p, bg_p, route_p);

  // every ray kept all S samples (n_kept = n*S, counts <= S): the bounds {i*S, (i+1)*S} are the same
  // in both orders; otherwise the caller-order counts are scanned as the unbucketed route scans them
  const bool rows = r.weights.size(0) == (int64_t)n_rays * S;
  Tensor bounds = r.idx_start_end;
  if (!rows) {
    Tensor counts = torch::empty({n_rays}, iopt);
    f2n::check(
      f2n_counts_through(
        r.idx_start_end.data_ptr<int32_t>(), inv.data_ptr<int32_t>(), counts.data_ptr<int32_t>(),
        n_rays, stream),
      "f2n_counts_through");
    bounds = bounds_from_counts(counts, stream).first;
  }
  // the distortion loss was taken in composite(), where the weights, t and dt of the bucketed order
  // lie: one float per ray rides back (nothing, when it was not asked for)
  const Tensor dist = route.want.dist ? r.weight_dist : torch::empty({0}, rays_o.options());
  // ... and so do the depth terms, three floats per ray, through a node of their own: without a
  // target nothing here is launched or recorded
  const Tensor terms =
    r.depth_terms.defined() ? RayRowsUnpermuteFn::apply(r.depth_terms, perm, inv)[0] : Tensor();
  // ... and the opacity, one float per ray, the same way
  const Tensor opacity =
    r.opacity.defined()
      ? RayRowsUnpermuteFn::apply(r.opacity.unsqueeze(1), perm, inv)[0].squeeze(1)
      : Tensor();
  if (route.want_var) {
    // the variance is a per-ray quantity: taken where the weights lie, its [n_rays] result goes back
    // with colours and depths as rows of one float -- no [n, S] gather forward or backward
    Tensor var = CustomOps::WeightVar(r.weights, r.idx_start_end);
    auto out = RayUnpermuteFn::apply(
      r.colors, r.depths, var, dist, perm, inv, r.idx_start_end, bounds, /*S=*/1, /*rows=*/true);
    RenderResult res{
      out[0], out[1], Tensor(), bounds, out[2], route.want.dist ? out[3] : Tensor(), terms};
    res.opacity = opacity;
    return res;
  }
  auto out = RayUnpermuteFn::apply(
    r.colors, r.depths, r.weights, dist, perm, inv, r.idx_start_end, bounds, S, rows);
  RenderResult res{
    out[0], out[1], out[2], bounds, Tensor(), route.want.dist ? out[3] : Tensor(), terms};
  res.opacity = opacity;
  return res;
}

// Dense first pass: every sample is encoded once (level-major kernel), the keep-prefix comes from
// that encoding, and the shading pass reuses it -- same counts as the march, bit for bit.
RenderResult Renderer::render_dense(
  const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx, RunningMode mode,
  const Tensor & noise, const Tensor & bg_color, const Route & route, const Tensor & noise_rows)
{
  const int n_rays = (int)rays_o.size(0);
  const int S = pts_sampler_->options_.max_samples;
  void * stream = f2n::current_stream(rays_o);
  Hash3DAnchored & field = *scene_field_;
  // lean: contracted positions (all.x) and one direction per ray; all.pts / all.dirs stay undefined
  SampleResultFlex all =
    route.lean ? pts_sampler_->get_samples_dense(rays_o, rays_d, noise, noise_rows, route.noise_raw)
               : pts_sampler_->get_samples(rays_o, rays_d, noise);
  const int64_t n_all = all.dt.size(0);
  Tensor contracted_all, enc_all_cm;
  {
    torch::NoGradGuard no_grad;
    // the dense [n_rays, S] grid of the sampler: ray-tile mapping of the encode
    if (route.lean) {
      contracted_all = all.x;
      enc_all_cm = field.encode_contracted(all.x, S).t();
    } else {
      enc_all_cm = field.encode(all.pts, S, &contracted_all).t();  // [C, n_all] contiguous storage
    }
    TORCH_CHECK(enc_all_cm.is_contiguous(), "encode() must return channel-major storage");
  }
  // The number of survivors sizes everything downstream, so the host has to read it: one blocking
  // read per chunk.  When the previous chunk kept every sample the next one most likely does too
  // (no density yet, or validation of empty space), so that case is tried first and for free: the
  // shading pass is run over ALL samples (fresh buffers, nothing observable), the density logits
  // it produces anyway are summed per ray (f2n_density_margin: 67 MB instead of the 1 GB encoding
  // the exact scan reads) and a flag says whether some ray comes within a factor e^0.5 of the
  // early-stop threshold.  Flag clear = the exact scan would keep everything too (its logits
  // differ from these in the last bits only): the guess IS the result, and neither the scan
  // (0.22 ms per 8.4 M samples) nor an idle GPU across the read (the flag travels while
  // compositing runs) was paid.  Flag set = drop the guess, run the exact scan, compact.
  //   Small chunks (the 512-ray training batch) keep the exact scan instead -- there it costs
  // 20 us, less than the GPU would idle while the host waits for a flag that only exists after
  // the shading pass -- and hide ITS read-back behind the same guess.
  //   options_.deferred_check does without the read altogether.

  if (options_.deferred_check) {
    // (a) no host read: exact scan -> device-side "kept fewer than shaded" flag, all samples shaded
    Tensor total = scan_survivors(all, enc_all_cm, n_rays).second;
    if (!deferred_bad_.defined()) deferred_bad_ = torch::zeros({1}, total.options());
    deferred_bad_.add_(total.ne(n_all).to(torch::kInt32));  // (integers: nothing autograd records)
    record_kept(n_all, n_all);
    return shade_and_composite(all, emb_idx, mode, bg_color, route, enc_all_cm, contracted_all);
  }

  const bool may_guess = options_.speculate_dense && last_kept_fraction_ >= 1.f && n_all > 0;
  const bool large = n_all >= options_.margin_min_samples;
  if (may_guess && large) {
    // (b) accepted on the density-margin flag; a set flag falls through to (c) without a second guess
    if (auto guess = shade_all_unless_near_threshold(
          all, emb_idx, mode, bg_color, route, enc_all_cm, contracted_all)) {
      record_kept(n_all, n_all);
      if (options_.normals) guess->normals = ray_normals(all, guess->weights);
      return *guess;
    }
  }

  // (c) the exact scan and the read of its total
  auto [bounds, total] = scan_survivors(all, enc_all_cm, n_rays);
  survivors_.request(total, stream);
  RenderResult guess;
  const bool guessed = may_guess && !large;
  if (guessed)  // enqueued BEFORE the host waits for the count: the GPU does not idle across the read
    guess = shade_and_composite(
      all, emb_idx, mode, bg_color, route, enc_all_cm, contracted_all, /*final=*/false);
  const int64_t n_kept = survivors_.wait();
  record_kept(n_kept, n_all);
  if (guessed && n_kept == n_all) {
    if (options_.normals) guess.normals = ray_normals(all, guess.weights);
    return guess;
  }
  guess = RenderResult();  // a wrong guess is released before the compaction allocates
  if (n_kept == n_all) {
    // nothing terminated: the uncompacted arrays ARE the compacted ones, and so are their
    // contracted positions
    all.pts_idx_bounds = bounds;
    return shade_and_composite(all, emb_idx, mode, bg_color, route, enc_all_cm, contracted_all);
  }
  // rays terminate: from here on the existing kernels, which take the cooked noise in ray order
  Tensor noise_k = noise;
  if (route.lean && noise.defined()) {
    torch::NoGradGuard no_grad;
    if (route.noise_raw) noise_k = PtsSampler::cook_noise(noise);
    if (noise_rows.defined()) {
      Tensor rows = torch::empty_like(noise_k);
      f2n::check(
        f2n_gather_rows(
          noise_k.data_ptr<float>(), rows.data_ptr<float>(), noise_rows.data_ptr<int32_t>(), n_rays,
          S, stream),
        "f2n_gather_rows");
      noise_k = rows;
    }
  }
  SampleResultFlex kept = compact_samples(rays_o, rays_d, noise_k, bounds, n_kept);
  const int64_t C = enc_all_cm.size(0);
  Tensor enc_kept_cm = torch::empty({C, n_kept}, rays_o.options());
  f2n::check(
    f2n_compact_rows_cm(
      enc_all_cm.data_ptr<float>(), n_all, enc_kept_cm.data_ptr<float>(), n_kept, (int)C,
      bounds.data_ptr<int32_t>(), n_rays, S, stream),
    "f2n_compact_rows_cm");
  return shade_and_composite(kept, emb_idx, mode, bg_color, route, enc_kept_cm);
}

bool Renderer::deferred_check_ok()
{
  if (!deferred_bad_.defined()) return true;
  const bool ok = deferred_bad_.item<int32_t>() == 0;  // the caller's sync point
  deferred_bad_.zero_();
  return ok;
}

// ---- steps of the fused routes -------------------------------------------------------------------

// The exact keep-prefix of every ray from the dense encoding: {bounds [n_rays, 2], total [1]}.
std::pair<Tensor, Tensor> Renderer::scan_survivors(
  const SampleResultFlex & all, const Tensor & enc_all_cm, int n_rays)
{
  torch::NoGradGuard no_grad;
  void * stream = f2n::current_stream(enc_all_cm);
  auto head = scene_field_->density_head();
  Tensor counts = torch::empty({n_rays}, f2n::int_on(enc_all_cm.device()));
  {
    f2n::ScopedKernelTimer timer("density_scan", stream, (double)n_rays);
    f2n::check(
      f2n_density_scan(
        enc_all_cm.data_ptr<float>(), (int)enc_all_cm.size(0), all.dt.data_ptr<float>(),
        head.first.data_ptr<float>(), head.second.data_ptr<float>(), counts.data_ptr<int32_t>(),
        n_rays, pts_sampler_->options_.max_samples, options_.early_stop_trans, 3.f, stream),
      "f2n_density_scan");
  }
  return bounds_from_counts(counts, stream);
}

// The n_kept samples inside `bounds`, generated again from the rays (positions, directions, dt, t).
SampleResultFlex Renderer::compact_samples(
  const Tensor & rays_o, const Tensor & rays_d, const Tensor & noise, const Tensor & bounds,
  int64_t n_kept, const Tensor & len)
{
  const auto fopt = rays_o.options();
  SampleResultFlex kept{
    torch::empty({n_kept, 3}, fopt), torch::empty({n_kept, 3}, fopt), torch::empty({n_kept}, fopt),
    torch::empty({n_kept}, fopt), bounds};
  if (len.defined()) {
    f2n::check(
      f2n_sample_compact_occ(
        rays_o.data_ptr<float>(), rays_d.data_ptr<float>(), f2n::fptr(noise),
        bounds.data_ptr<int32_t>(), len.data_ptr<int32_t>(), occupancy_->words_ptr(),
        (int)occupancy_->resolution(), kept.pts.data_ptr<float>(), kept.dirs.data_ptr<float>(),
        kept.dt.data_ptr<float>(), kept.t.data_ptr<float>(), (int)rays_o.size(0),
        pts_sampler_->options_.max_samples, pts_sampler_->options_.step,
        f2n::current_stream(rays_o)),
      "f2n_sample_compact_occ");
    return kept;
  }
  f2n::check(
    f2n_sample_compact(
      rays_o.data_ptr<float>(), rays_d.data_ptr<float>(), f2n::fptr(noise),
      bounds.data_ptr<int32_t>(), kept.pts.data_ptr<float>(), kept.dirs.data_ptr<float>(),
      kept.dt.data_ptr<float>(), kept.t.data_ptr<float>(), (int)rays_o.size(0),
      pts_sampler_->options_.max_samples, pts_sampler_->options_.step,
      f2n::current_stream(rays_o)),
    "f2n_sample_compact");
  return kept;
}

// The large-chunk guess of render_dense: shade ALL samples (`all` is the sampler's dense
// [n_rays, max_samples] grid), and take that as the result unless some ray comes near the early-stop
// threshold.  The margin kernel sits between shade and composite so that its flag travels to the
// host while compositing runs.
std::optional<RenderResult> Renderer::shade_all_unless_near_threshold(
  const SampleResultFlex & all, const Tensor & emb_idx, RunningMode mode, const Tensor & bg_color,
  const Route & route, const Tensor & enc_cm, const Tensor & contracted)
{
  void * stream = f2n::current_stream(all.dt);
  Tensor near_threshold = torch::zeros({1}, f2n::int_on(all.dt.device()));
  Shaded shaded = shade(all, emb_idx, mode, route, enc_cm, contracted);
  const int S = pts_sampler_->options_.max_samples;
  const float limit = -std::log(options_.early_stop_trans) - 0.5f;
  f2n::check(
    f2n_density_margin(
      shaded.field_out.data_ptr<float>(), all.dt.data_ptr<float>(),
      near_threshold.data_ptr<int32_t>(), (int)(all.dt.size(0) / S), S, 3.f, limit, stream),
    "f2n_density_margin");
  survivors_.request(near_threshold, stream);
  RenderResult guess = composite(all, shaded, bg_color, route, /*final=*/false);
  if (survivors_.wait() != 0) return std::nullopt;
  return guess;
}

// Second pass on the survivors (renderer.cpp:92-118).
RenderResult Renderer::shade_and_composite(
  const SampleResultFlex & kept, const Tensor & emb_idx, RunningMode mode, const Tensor & bg_color,
  const Route & route, const Tensor & enc_cm, const Tensor & contracted, bool final)
{
  return composite(
    kept, shade(kept, emb_idx, mode, route, enc_cm, contracted), bg_color, route, final);
}

Renderer::Shaded Renderer::shade(
  const SampleResultFlex & kept, const Tensor & emb_idx, RunningMode mode, const Route & route,
  const Tensor & enc_cm, const Tensor & contracted)
{
  if (!route.fused_net) {
    Tensor scene_feat = scene_field_->query(kept.pts);  // [n, 16]: col 0 density logit, 1.. shading
    return {scene_feat, shade_aten(scene_feat, kept, emb_idx, mode)};
  }
  // hash encode -> one kernel for field head + embedding + SH + colour MLP
  const int64_t n_kept = kept.dt.size(0);
  Tensor enc = enc_cm.defined() ? scene_field_->encode_cached(kept.pts, enc_cm, contracted)
                                : scene_field_->encode(kept.pts);
  if (route.grad_rays.origins.defined()) {
    // enc passes through; the backward turns d(enc) into d(rays) (and, with the field frozen,
    // is what makes the shade backward form d(enc) at all)
    auto info = torch::make_intrusive<Hash3DAnchoredInfo>();
    info->hash3d_ = scene_field_.get();
    enc = RayGradFn::apply(
      enc, route.grad_rays.origins, route.grad_rays.dirs, kept.pts, kept.t, kept.pts_idx_bounds,
      torch::IValue(info))[0];
  }
  auto mlp = shader_->mlp_params();
  const Tensor emb = mode == RunningMode::TRAIN ? app_emb_ : Tensor();
  // The sampler's whole [n_rays, max_samples] grid (the dense first pass, or a march that kept
  // everything): the ray-uniform kernels, which take the image id per ray.  The rule looks at the
  // shape of the samples alone, so every route that hands over the same samples gets the same bits.
  const int64_t n_rays = kept.pts_idx_bounds.size(0), S = pts_sampler_->options_.max_samples;
  if (f2n::shade_rays_applies(n_kept, n_rays, S)) {
    const bool per_ray = kept.ray_dirs.defined();  // (the lean dense route)
    f2n::ShadeOut sh = f2n::shade_rays(
      enc, per_ray ? kept.ray_dirs : kept.dirs, mode == RunningMode::TRAIN ? emb_idx : Tensor(), S,
      scene_field_->head_weight(), scene_field_->mlp_->bias, mlp[0], mlp[1], mlp[2], mlp[3], emb,
      per_ray);
    return {sh.logit.unsqueeze(1), sh.rgb};
  }
  Tensor sample_img;
  if (mode == RunningMode::TRAIN)
    sample_img = CustomOps::ScatterIdx((int)n_kept, kept.pts_idx_bounds, emb_idx);
  f2n::ShadeOut sh = f2n::shade(
    enc, kept.dirs, sample_img, scene_field_->head_weight(), scene_field_->mlp_->bias, mlp[0],
    mlp[1], mlp[2], mlp[3], emb);
  return {sh.logit.unsqueeze(1), sh.rgb};
}

// The reference's per-sample colours from the field head's output (renderer.cpp:95-105): a ones
// column in place of the density logit, the image's appearance embedding added in TRAIN, SH + MLP.
Tensor Renderer::shade_aten(
  const Tensor & scene_feat, const SampleResultFlex & kept, const Tensor & emb_idx, RunningMode mode)
{
  const int64_t n_kept = kept.pts.size(0);
  Tensor shading_feat = torch::cat(
    {torch::ones({n_kept, 1}, scene_feat.options()),
     scene_feat.index({Slc(), Slc(1, torch::indexing::None)})},
    1);
  if (mode == RunningMode::TRAIN) {
    Tensor all_emb_idx = CustomOps::ScatterIdx((int)n_kept, kept.pts_idx_bounds, emb_idx);
    shading_feat = CustomOps::ScatterAdd(app_emb_, all_emb_idx, shading_feat);
  }
  return shader_->query(shading_feat, kept.dirs);
}

RenderResult Renderer::composite(
  const SampleResultFlex & kept, const Shaded & shaded, const Tensor & bg_color, const Route & route,
  bool final)
{
  // (the fused routes' kept.pts_idx_bounds comes from f2n_bounds_from_counts / the sampler: the
  // ranges tile [0, n))
  f2n::CompositeOut out = f2n::composite(
    shaded.field_out, shaded.rgb, kept.dt, kept.t, kept.pts_idx_bounds, bg_color, route.fused_net);
  RenderResult res{out.colors, out.depths, out.weights, kept.pts_idx_bounds};
  per_ray_terms(res, out.weights, kept, route);
  if (options_.normals && final) res.normals = ray_normals(kept, out.weights);
  return res;
}

Tensor Renderer::ray_normals(const SampleResultFlex & kept, const Tensor & weights_in)
{
  torch::NoGradGuard no_grad;
  TORCH_CHECK(kept.pts.defined(), "normals need the kept samples' world positions");
  const Tensor pts = f2n::dev_f32(kept.pts.detach(), "kept pts");
  const Tensor weights = f2n::dev_f32(weights_in.detach(), "weights");
  const Tensor bounds = f2n::dev_i32(kept.pts_idx_bounds, "kept bounds");
  const int64_t n_rays = bounds.size(0);
  TORCH_CHECK(weights.numel() == pts.size(0), "weights / kept samples mismatch");
  // nothing kept (an empty occupancy grid): every segment is empty, and an empty tensor has no pointer
  if (pts.size(0) == 0) return torch::zeros({n_rays, 3}, pts.options());
  Hash3DAnchored & field = *scene_field_;
  const Tensor table16 = field.table_f16();
  const f2n::FieldArgs g = field.kernel_args(table16);
  const Tensor w0 = field.density_head().first;
  Tensor normals = torch::empty({n_rays, 3}, pts.options());
  void * stream = f2n::current_stream(pts);
  f2n::ScopedKernelTimer timer("ray_normals", stream, (double)pts.size(0));
  f2n::check(
    f2n_ray_normals(
      pts.data_ptr<float>(), bounds.data_ptr<int32_t>(), weights.data_ptr<float>(), g.table,
      g.primes, g.bias, g.mul, w0.data_ptr<float>(), normals.data_ptr<float>(), (int)n_rays, g.L_walk,
      g.F, g.T, g.level_stride, stream),
    "f2n_ray_normals");
  return normals;
}

// ---- level weights -------------------------------------------------------------------------------

double f2n::CoarseToFine::alpha_at(double it, int64_t L) const
{
  double u = end > start ? (it - start) / (end - start) : (it >= start ? 1. : 0.);
  u = std::min(1., std::max(0., u));
  return base + ((double)L - base) * u;
}

std::pair<Tensor, int64_t> f2n::level_weights(double alpha, int64_t L)
{
  TORCH_CHECK(L >= 1 && L <= F2N_MAX_LEVELS, "level_weights: n_levels out of range");
  Tensor w = torch::empty({L}, torch::TensorOptions().dtype(torch::kFloat32));
  int l_active = 0;
  f2n::check(f2n_level_weights(alpha, (int)L, w.data_ptr<float>(), &l_active), "f2n_level_weights");
  return {w, (int64_t)l_active};
}

void Renderer::set_coarse_to_fine(double alpha)
{
  scene_field_->set_level_weights(f2n::level_weights(alpha, scene_field_->options_.n_levels).first);
}

// ---- one-pass inference render ---------------------------------------------------------------------

bool Renderer::one_pass_applies() const
{
  if (!options_.one_pass || !fused_net_applies()) return false;
  if (!torch::GradMode::is_enabled()) return true;
  for (const auto & p : parameters())
    if (p.requires_grad()) return false;
  return true;
}

void Renderer::set_one_pass_head(int n_head)
{
  TORCH_CHECK(
    n_head == 0 || n_head == -1 || (n_head > 0 && n_head % 64 == 0),
    "one_pass_head is 0 (one ray per wavefront), -1 (whole rays eight to a wavefront) or a positive "
    "multiple of 64 (head, then tail)");
  options_.one_pass_head = n_head;
}

void Renderer::render_rays_into(
  const Tensor & rays_o_raw, const Tensor & rays_d_raw, const Tensor & emb_idx_in, RunningMode mode,
  const Tensor & noise_raw, const Tensor & bg_raw, Tensor colors, Tensor depths, Tensor last_trans,
  Tensor kept)
{
  const Tensor rays_o = f2n::dev_f32(rays_o_raw.detach(), "rays_o");
  const Tensor rays_d = f2n::dev_f32(rays_d_raw.detach(), "rays_d");
  const Tensor noise = noise_raw.defined() ? f2n::dev_f32(noise_raw.detach(), "noise") : Tensor();
  const Tensor bg = f2n::dev_f32(bg_raw.detach(), "bg_color");
  const int n_rays = (int)rays_o.size(0);
  const int S = pts_sampler_->options_.max_samples;
  TORCH_CHECK(rays_o.numel() == (int64_t)n_rays * 3 && rays_d.numel() == (int64_t)n_rays * 3, "rays shape");
  TORCH_CHECK(!noise.defined() || noise.numel() == (int64_t)n_rays * S, "noise shape");
  TORCH_CHECK(bg.numel() == (int64_t)n_rays * 3, "bg_color shape");
  const bool train = mode == RunningMode::TRAIN;
  TORCH_CHECK(!train || emb_idx_in.defined(), "TRAIN mode needs emb_idx");
  const Tensor emb_idx = train ? f2n::dev_i32(emb_idx_in, "emb_idx") : Tensor();
  TORCH_CHECK(!emb_idx.defined() || emb_idx.numel() == n_rays, "emb_idx shape");
  TORCH_CHECK(
    colors.is_contiguous() && depths.is_contiguous() && last_trans.is_contiguous() &&
      kept.is_contiguous() && colors.numel() == (int64_t)n_rays * 3 && depths.numel() == n_rays &&
      last_trans.numel() == n_rays && kept.numel() == n_rays,
    "render_rays outputs");
  if (n_rays == 0) return;
  if (occupancy_)
    TORCH_CHECK(
      occupancy_->words().device() == rays_o.device(), "the occupancy grid lives on another device");
  Hash3DAnchored & field = *scene_field_;
  const Tensor table16 = field.table_f16();
  const f2n::FieldArgs g = field.kernel_args(table16);
  const Tensor w_h = f2n::dev_f32(field.head_weight().detach(), "field head weight");
  const Tensor b_h = f2n::dev_f32(field.mlp_->bias.detach(), "field head bias");
  auto mlp = shader_->mlp_params();
  const Tensor w1 = f2n::dev_f32(mlp[0].detach(), "shader w1"), b1 = f2n::dev_f32(mlp[1].detach(), "shader b1");
  const Tensor w2 = f2n::dev_f32(mlp[2].detach(), "shader w2"), b2 = f2n::dev_f32(mlp[3].detach(), "shader b2");
  const Tensor emb = train ? f2n::dev_f32(app_emb_.detach(), "app_emb") : Tensor();
  void * stream = f2n::current_stream(rays_o);
  // (the level-of-detail entries: g.L_walk == g.L is the entry without it, launch for launch)
  // 0: one launch; otherwise the head (n_head >= S: whole rays) and, for a shorter head, the tail
  const int head_opt = options_.one_pass_head;
  const int n_head = head_opt < 0 ? S : std::min(head_opt, S);
  void * state = nullptr;
  if (head_opt > 0 && n_head < S) {
    const int64_t words = f2n_render_rays_state_bytes(n_rays) / 4;
    if (
      !one_pass_state_.defined() || one_pass_state_.device() != rays_o.device() ||
      one_pass_state_.numel() < words)
      one_pass_state_ = torch::empty({words}, f2n::float_on(rays_o.device()));
    state = one_pass_state_.data_ptr<float>();
  }
  f2n::ScopedKernelTimer timer("render_rays", stream, (double)n_rays);
#define F2N_RENDER_RAYS_ARGS                                                                       \
  rays_o.data_ptr<float>(), rays_d.data_ptr<float>(), f2n::fptr(noise), g.table, g.primes, g.bias, \
    g.mul, w_h.data_ptr<float>(), b_h.data_ptr<float>(), w1.data_ptr<float>(),                     \
    b1.data_ptr<float>(), w2.data_ptr<float>(),                                                    \
    b2.data_ptr<float>(), f2n::fptr(emb), f2n::iptr(emb_idx),                                      \
    occupancy_ ? occupancy_->words_ptr() : nullptr,                                                \
    occupancy_ ? (int)occupancy_->resolution() : 0, bg.data_ptr<float>(),                          \
    colors.data_ptr<float>(), depths.data_ptr<float>(), last_trans.data_ptr<float>(),              \
    kept.data_ptr<int32_t>(), nullptr, n_rays, S, pts_sampler_->options_.step, g.L, g.L_walk, g.F, \
    g.T,                                                                                           \
    g.level_stride, options_.early_stop_trans, 3.f, 1e-2f
  if (head_opt == 0) {
    f2n::check(f2n_render_rays_lod(F2N_RENDER_RAYS_ARGS, stream), "f2n_render_rays_lod");
    return;
  }
  f2n::check(
    f2n_render_rays_head_lod(F2N_RENDER_RAYS_ARGS, n_head, state, stream),
    "f2n_render_rays_head_lod");
  if (n_head < S)
    f2n::check(
      f2n_render_rays_tail_lod(F2N_RENDER_RAYS_ARGS, n_head, state, stream),
      "f2n_render_rays_tail_lod");
#undef F2N_RENDER_RAYS_ARGS
}

std::tuple<Tensor, Tensor, Tensor, Tensor> Renderer::render_rays(
  const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx, RunningMode mode,
  const Tensor & noise_in, const Tensor & bg_in)
{
  torch::NoGradGuard no_grad;
  TORCH_CHECK(
    fused_net_applies(),
    "render_rays needs the fused per-sample network: n_levels * n_channels in {8, 16, 32, 64}, a "
    "16-wide field head and fused_shade");
  const int64_t n_rays = rays_o.size(0);
  const auto fopt = f2n::float_on(rays_o.device());
  Tensor noise = noise_in.defined() ? noise_in
                                    : pts_sampler_->draw_noise(n_rays, mode, rays_o.device());
  Tensor bg_color = background_or_default(bg_in, rays_d, mode, n_rays);
  Tensor colors = torch::empty({n_rays, 3}, fopt), depths = torch::empty({n_rays}, fopt);
  Tensor last_trans = torch::empty({n_rays}, fopt);
  Tensor kept = torch::empty({n_rays}, f2n::int_on(rays_o.device()));
  render_rays_into(rays_o, rays_d, emb_idx, mode, noise, bg_color, colors, depths, last_trans, kept);
  return {colors, depths, last_trans, kept};
}

// ---- whole-image helpers -------------------------------------------------------------------------

std::tuple<Tensor, Tensor> Renderer::render_all_rays(
  const Tensor & rays_o, const Tensor & rays_d, const int batch_size)
{
  const int64_t n_rays = rays_d.size(0);
  const bool rays_need_grad =
    torch::GradMode::is_enabled() && (rays_o.requires_grad() || rays_d.requires_grad());
  if (one_pass_applies() && !rays_need_grad && rays_d.is_cuda() && batch_size > 0) {
    // one launch per chunk, each into its rows of one output: nothing to concatenate
    torch::NoGradGuard no_grad;
    const auto fopt = f2n::float_on(rays_d.device());
    Tensor colors = torch::empty({n_rays, 3}, fopt), depths = torch::empty({n_rays, 1}, fopt);
    Tensor last_trans = torch::empty({n_rays}, fopt);
    Tensor kept = torch::empty({n_rays}, f2n::int_on(rays_d.device()));
    // (an attached background is looked up per chunk, one launch each; without one the constant)
    const Tensor bg = background_
                        ? Tensor()
                        : torch::ones({std::min<int64_t>(batch_size, n_rays), 3}, fopt) * .5f;
    for (int64_t lo = 0; lo < n_rays; lo += batch_size) {
      const int64_t hi = std::min<int64_t>(lo + batch_size, n_rays);
      render_rays_into(
        rays_o.slice(0, lo, hi), rays_d.slice(0, lo, hi), Tensor(), RunningMode::VALIDATE, Tensor(),
        background_ ? background_->query(rays_d.slice(0, lo, hi)) : bg.slice(0, 0, hi - lo),
        colors.slice(0, lo, hi), depths.slice(0, lo, hi), last_trans.slice(0, lo, hi),
        kept.slice(0, lo, hi));
    }
    return {colors, depths};
  }
  std::vector<Tensor> colors, depths;
  for (int64_t lo = 0; lo < n_rays; lo += batch_size) {
    const int64_t hi = std::min<int64_t>(lo + batch_size, n_rays);
    RenderResult r = render(
      rays_o.index({Slc(lo, hi)}).contiguous(), rays_d.index({Slc(lo, hi)}).contiguous(), Tensor(),
      RunningMode::VALIDATE);
    colors.push_back(r.colors);
    depths.push_back(r.depths.reshape({-1, 1}));
  }
  return {torch::cat(colors, 0), torch::cat(depths, 0)};
}

namespace
{
// The view's pixels in B x B tiles (row-major tiles, row-major inside a tile), int64 [h * w]; undefined
// when the tiles do not divide the view (row-major traversal).
Tensor pixel_tile_order(int h, int w, int B, const torch::Device & device)
{
  if (!(B > 1 && h % B == 0 && w % B == 0)) return Tensor();
  return torch::arange((int64_t)h * w, torch::TensorOptions().dtype(torch::kInt64).device(device))
    .view({h / B, B, w / B, B})
    .permute({0, 2, 1, 3})
    .reshape({-1});
}
}  // namespace

std::tuple<Tensor, Tensor> Renderer::render_image(
  const Tensor & pose, const Tensor & intrinsic, const int h, const int w, const int batch_size,
  const Tensor & dist)
{
  Rays rays = get_view_rays(pose, intrinsic, h, w, dist);  // pixel grid generated in the kernel
  // The view is traversed in B x B pixel tiles rather than row by row: the ray-tile encode takes 64
  // consecutive rays per workgroup, and an 8 x 8 block of pixels is a bundle 8 pixels wide both
  // ways instead of a strip 64 pixels long -- a third fewer distinct table lines per gather at the
  // middle levels (src/renderer.cpp:153-172 walks the image in row-major batches; the image that
  // comes out is the same).
  const Tensor order = pixel_tile_order(h, w, options_.pixel_tiles, pose.device());
  if (order.defined()) {
    rays.origins = rays.origins.index_select(0, order);
    rays.dirs = rays.dirs.index_select(0, order);
  }
  auto [colors, depths] = render_all_rays(rays.origins, rays.dirs, batch_size);
  if (order.defined()) {
    colors = torch::empty_like(colors).index_copy_(0, order, colors);
    depths = torch::empty_like(depths).index_copy_(0, order, depths);
  }
  colors = colors.reshape({h, w, 3}).clip(0.f, 1.f);
  depths = depths.reshape({h, w, 1}).repeat({1, 1, 3});
  return {colors, depths};
}

std::tuple<Tensor, Tensor, Tensor> Renderer::render_all_rays_with_normals(
  const Tensor & rays_o, const Tensor & rays_d, const int batch_size)
{
  TORCH_CHECK(batch_size > 0, "batch_size must be positive");
  const int64_t n_rays = rays_d.size(0);
  // the option is on for the duration of this call only, an exception included
  struct Restore
  {
    bool & flag;
    bool was;
    ~Restore() { flag = was; }
  } restore{options_.normals, options_.normals};
  options_.normals = true;
  std::vector<Tensor> colors, depths, normals;
  for (int64_t lo = 0; lo < n_rays; lo += batch_size) {
    const int64_t hi = std::min<int64_t>(lo + batch_size, n_rays);
    RenderResult r = render(
      rays_o.index({Slc(lo, hi)}).contiguous(), rays_d.index({Slc(lo, hi)}).contiguous(), Tensor(),
      RunningMode::VALIDATE);
    colors.push_back(r.colors);
    depths.push_back(r.depths.reshape({-1, 1}));
    normals.push_back(r.normals);
  }
  if (colors.empty()) {
    const auto fopt = f2n::float_on(rays_d.device());
    return {torch::empty({0, 3}, fopt), torch::empty({0, 1}, fopt), torch::empty({0, 3}, fopt)};
  }
  return {torch::cat(colors, 0), torch::cat(depths, 0), torch::cat(normals, 0)};
}

std::tuple<Tensor, Tensor, Tensor> Renderer::render_image_with_normals(
  const Tensor & pose, const Tensor & intrinsic, const int h, const int w, const int batch_size,
  const Tensor & dist)
{
  Rays rays = get_view_rays(pose, intrinsic, h, w, dist);
  const Tensor order = pixel_tile_order(h, w, options_.pixel_tiles, pose.device());  // as render_image
  if (order.defined()) {
    rays.origins = rays.origins.index_select(0, order);
    rays.dirs = rays.dirs.index_select(0, order);
  }
  auto [colors, depths, normals] = render_all_rays_with_normals(rays.origins, rays.dirs, batch_size);
  if (order.defined()) {
    colors = torch::empty_like(colors).index_copy_(0, order, colors);
    depths = torch::empty_like(depths).index_copy_(0, order, depths);
    normals = torch::empty_like(normals).index_copy_(0, order, normals);
  }
  colors = colors.reshape({h, w, 3}).clip(0.f, 1.f);
  depths = depths.reshape({h, w, 1}).repeat({1, 1, 3});
  normals = normals.reshape({h, w, 3});
  return {colors, depths, normals};
}

std::vector<torch::optim::OptimizerParamGroup> Renderer::optim_param_groups(float lr)
{
  std::vector<torch::optim::OptimizerParamGroup> groups;
  for (auto & g : scene_field_->optim_param_groups(lr)) groups.emplace_back(g);
  for (auto & g : shader_->optim_param_groups(lr)) groups.emplace_back(g);
  auto opt = std::make_unique<torch::optim::AdamOptions>(lr);
  opt->betas(std::make_tuple(0.9, 0.99)).eps(1e-15).weight_decay(1e-6);
  groups.emplace_back(std::vector<Tensor>{app_emb_}, std::move(opt));
  return groups;
}

// ---- training-step harness -----------------------------------------------------------------------

// The D-SSIM term of a batch of patches: loss + ssim_weight * sum_b m_b (1 - SSIM_b) / M on the
// colours viewed as [n, P, P, 3] against `target` (no gradient), M = sum_b m_b (1 when that is not
// positive; no host read).  The unweighted mean is left in last_ssim_loss_.
static Tensor add_patch_term(
  Renderer & renderer, const Tensor & loss, const Tensor & colors, const Tensor & target,
  const f2n::PatchLoss & pl)
{
  const int64_t P = pl.patch, n_rays = colors.size(0);
  TORCH_CHECK(
    P >= 11 && n_rays > 0 && n_rays % (P * P) == 0,
    "train_step: a PatchLoss needs n_patches * patch^2 rays in patch-major order, patch >= 11");
  const int64_t n = n_rays / (P * P);
  TORCH_CHECK(target.numel() == n_rays * 3, "train_step: the colour target must be [n_rays, 3]");
  const Tensor one_minus = 1.f - CustomOps::Ssim(
                                   colors.reshape({n, P, P, 3}),
                                   target.detach().reshape({n, P, P, 3}));  // [n]
  Tensor term;
  if (pl.patch_weight.defined()) {
    const Tensor m = f2n::dev_f32(pl.patch_weight.detach(), "patch_weight").reshape({-1});
    TORCH_CHECK(m.numel() == n, "train_step: patch_weight must be [n_rays / patch^2]");
    const Tensor sum_m = m.sum();
    const Tensor M = torch::where(sum_m.gt(0.f), sum_m, torch::ones_like(sum_m));
    term = (m * one_minus).sum() / M;
  } else {
    term = one_minus.mean();
  }
  renderer.last_ssim_loss_ = one_minus.detach().mean();
  return loss + pl.ssim_weight * term;
}

f2n::TrainStepResult f2n::train_step(
  Renderer & renderer, const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx,
  const Tensor & gt_colors, const LossTerms & terms, const Tensor & noise, const Tensor & bg_color,
  bool run_backward)
{
  const RaySupervision & sup = terms.sup;
  const int64_t n_rays = rays_o.size(0);
  // (a term that is off -- a zero weight, no target, quantile >= 1 -- is neither computed nor
  // differentiated: the step is the one without it, launch for launch)
  const bool want_dist = terms.want_dist(), want_depth = terms.want_depth();
  const bool want_opacity = sup.want_opacity(), want_robust = terms.robust.active();
  // per-ray weights (the caller's, or the robust loss's own): f2n::train_loss_sup and `* m` below;
  // none: f2n::train_loss, and no multiply is issued
  const bool weighted = terms.weighted();
  // composite_target off: the colour target is gt itself and alpha feeds the opacity term alone
  const bool plain_target = sup.alpha.defined() && !sup.composite_target;
  TORCH_CHECK(
    !sup.alpha.defined() || plain_target || bg_color.defined(),
    "train_step: an alpha target needs the bg_color the render blends in");
  Tensor m, alpha;
  if (sup.ray_weight.defined()) {
    m = f2n::dev_f32(sup.ray_weight.detach(), "ray_weight").reshape({-1});
    TORCH_CHECK(m.numel() == n_rays, "ray_weight must be [n_rays]");
  }
  if (sup.alpha.defined()) {
    alpha = f2n::dev_f32(sup.alpha.detach(), "alpha").reshape({-1});
    TORCH_CHECK(alpha.numel() == n_rays, "alpha must be [n_rays]");
  }
  // The per-batch constants of the depth term -- n_valid, counted on the device, and lambda_i /
  // n_valid -- are enqueued BEFORE the render, where the host runs ahead of the GPU: the dense route
  // reads one flag back per chunk, and small launches made between that read and the backward are on
  // the critical path.  One column sum, one dot product and one addition remain after it.
  Tensor depth_n_valid, depth_coef;
  LossOutputs want;
  want.dist = want_dist;
  want.opacity = want_opacity;
  if (want_depth) {
    torch::NoGradGuard no_grad;
    const Tensor z = f2n::dev_f32(terms.depth_target.detach(), "depth_target").reshape({-1});
    depth_n_valid = z.gt(0.f)
                      .logical_and(z.lt(std::numeric_limits<float>::infinity()))
                      .sum()
                      .to(torch::kFloat32)
                      .clamp_min(1.f);
    Tensor lambda = torch::empty({3}, z.options());  // (filled by launches: nothing is copied over)
    lambda.select(0, 0).fill_(terms.depth.empty);
    lambda.select(0, 1).fill_(terms.depth.near);
    lambda.select(0, 2).fill_(terms.depth.expected);
    depth_coef = lambda / depth_n_valid;
    want.depth_target = terms.depth_target;
    want.depth_eps = terms.depth.eps;
  }
  RenderResult res =
    renderer.render_for_loss(rays_o, rays_d, emb_idx, RunningMode::TRAIN, noise, bg_color, want);
  // the colour target the colour loss uses: a gt + (1 - a) bg when the alpha target composites
  // (formed where it is first needed, so that a step without the robust loss launches as before)
  Tensor target;
  const auto colour_target = [&]() {
    if (target.defined()) return target;
    target = gt_colors;
    if (alpha.defined() && !plain_target) {
      const Tensor a = alpha.unsqueeze(1);
      target = a * gt_colors.detach() + (1.f - a) * bg_color.detach();
    }
    return target;
  };
  // The robust loss: the render's own colours, detached, decide which rays the colour loss and the
  // regularisers see.  From here on its weight m_r omega_r stands wherever the caller's m_r stood --
  // train_loss_sup, the opacity, distortion and depth terms: a rejected ray regularises nothing.  The
  // D-SSIM term keeps the caller's patch_weight: it scores a patch as a whole and is not trimmed.
  TrainStepResult out;
  if (want_robust) {
    torch::NoGradGuard no_grad;
    RobustWeights rw = robust_weights(res.colors.detach(), colour_target(), m, terms.robust);
    m = out.robust_weight = rw.weight;
    out.robust_stats = rw.stats;
  }
  Tensor var = res.weight_var.defined() ? res.weight_var
                                        : CustomOps::WeightVar(res.weights, res.idx_start_end);
  // (a zero weight -- the reference's schedule starts there, train_manager.cpp:85-91 -- makes the
  // variance term's gradient exactly zero: its backward kernel is not run at all)
  if (terms.var_weight == 0.f) var = var.detach();
  Tensor loss, opacity_term;
  if (!weighted) {
    // colour loss + variance loss + squared error in two launches (f2n_loss_fwd; the ATen spelling of
    // the reference, train_manager.cpp:78-96, is ~23 launches of a few microseconds each)
    const Tensor stats = f2n::train_loss(res.colors, gt_colors, var, terms.var_weight);
    loss = stats[0];  // {loss, colour, var, sq}
    out.sq_err_sum = stats[3].detach();
  } else {
    // {loss, colour, var, opacity term, weighted squared error, sum of the weights}: three launches
    const Tensor stats =
      plain_target
        ? f2n::train_loss_sup(
            res.colors, gt_colors, var, Tensor(), m, Tensor(), Tensor(), terms.var_weight, 0.f)
        : f2n::train_loss_sup(
            res.colors, gt_colors, var, res.opacity, m, alpha,
            alpha.defined() ? bg_color.detach() : Tensor(), terms.var_weight, sup.opacity_weight);
    loss = stats[0];
    out.sq_err_sum = stats[4].detach();
    out.weight_sum = stats[5].detach();
    if (want_opacity && !plain_target) opacity_term = stats[3];
    // ... or the opacity term beside it, from the entry's own device scalar: W = sum m (1 when that
    // is not positive), d = O - a where m != 0 and exactly 0 elsewhere (the term and the opacity's
    // gradient of a masked ray are exact zeros), opac = sum m d^2 / W.  No host read.
    if (want_opacity && plain_target) {
      Tensor d = res.opacity - alpha;
      if (m.defined()) d = d.masked_fill(m.eq(0.f), 0.f);
      const Tensor sq = d * d;
      const Tensor W = torch::where(
        out.weight_sum.gt(0.f), out.weight_sum, torch::ones_like(out.weight_sum));
      opacity_term = (m.defined() ? m * sq : sq).sum() / W;
      loss = loss + sup.opacity_weight * opacity_term;
    }
  }
  renderer.last_opacity_loss_ = opacity_term.defined() ? opacity_term.detach() : Tensor();
  // the regularisers: a masked ray takes no part in them either (the per-ray terms are weighted
  // before their reductions, which keep their divisors)
  renderer.last_dist_loss_ = Tensor();
  if (want_dist && res.weight_dist.numel() > 0) {
    Tensor dist_loss = (m.defined() ? res.weight_dist * m : res.weight_dist).mean();
    loss = loss + terms.dist_weight * dist_loss;
    renderer.last_dist_loss_ = dist_loss.detach();
  }
  renderer.last_depth_loss_ = Tensor();
  if (want_depth && res.depth_terms.numel() > 0) {
    // invalid rays hold exact zeros: the sum over all rays is the sum over the valid ones
    const Tensor sums = (m.defined() ? res.depth_terms * m.unsqueeze(1) : res.depth_terms).sum(0);
    loss = loss + torch::dot(sums, depth_coef);
    renderer.last_depth_loss_ = sums.detach() / depth_n_valid;
  }
  renderer.last_ssim_loss_ = Tensor();
  if (terms.patch.active())
    loss = add_patch_term(renderer, loss, res.colors, colour_target(), terms.patch);
  out.loss = loss.detach();
  out.n_values = res.colors.numel();
  out.n_samples = renderer.last_n_samples_;
  if (sup.want_colors) out.colors = res.colors.detach();
  if (run_backward && loss.requires_grad()) loss.backward();
  return out;
}
