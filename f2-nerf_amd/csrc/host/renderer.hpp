// renderer.hpp -- Renderer: sampler + scene field + shader + per-image appearance embedding, and
// the volumetric render of a batch of rays.
//
// Public surface of reference src/renderer.hpp:15-49 (RenderResult, Renderer::render /
// render_all_rays / render_image / optim_param_groups); registered names "scene_field", "shader",
// "app_emb" kept so a reference checkpoint (renderer.pt) loads.
//
// render() picks one of three routes through the same arithmetic (reference src/renderer.cpp:33-123);
// Renderer::choose_route makes the choice once per call:
//   op-by-op          the reference's own sequence (sample all, query all, AccumulateSum, where,
//                     4x index, query survivors, Sum...) on the drop-in operators.  Used when
//                     RendererOptions::fused is off, when rays carry gradients (pose optimisation;
//                     unless RendererOptions::fused_ray_grad) and as the cross-check of the others;
//   fused, march      one wavefront-per-ray march finds each ray's kept prefix (early termination
//                     in-kernel), a scan turns counts into bounds, one kernel emits the compacted
//                     samples, the survivors are encoded and shaded, compositing is one kernel per
//                     direction;
//   fused, dense      every sample is encoded once, the kept prefix comes from that encoding and the
//                     shading pass reuses it (RendererOptions::dense_first_pass; the ways it avoids
//                     waiting for the survivor count are told in Renderer::render_dense).  Large
//                     chunks are rendered bucketed into pixel-compact ray bundles
//                     (Renderer::render_dense_bucketed) and handed back in the caller's order.
// With an occupancy grid attached (Renderer::set_occupancy) the density of every sample in an
// unoccupied cell counts as exactly zero and those samples are dropped: the march skips them
// (f2n_density_march_occ / f2n_sample_compact_occ), op-by-op masks them, the dense route is not
// taken (it encodes everything, which is the cost the grid removes).
//
// A loss asks for more than colours through one struct each: Renderer::render_for_loss takes a
// LossOutputs (the per-ray extras every route can hand back), f2n::train_step a LossTerms (the terms
// of the loss).  A field left at its default changes no launch and no bit.
#pragma once

#include <memory>
#include <optional>
#include <tuple>
#include <utility>
#include <vector>

#include "env_map.hpp"
#include "hash_3d_anchored.hpp"
#include "occupancy_grid.hpp"
#include "points_sampler.hpp"
#include "rays.hpp"
#include "robust_loss.hpp"
#include "sh_shader.hpp"

namespace f2n
{
// One int32 read back from the device without stalling the enqueue side: request() starts the copy
// into pinned memory behind everything already on the stream, wait() blocks on just that copy.
class HostCount
{
public:
  HostCount() = default;
  HostCount(const HostCount &) = delete;
  HostCount & operator=(const HostCount &) = delete;
  ~HostCount();
  void request(const torch::Tensor & device_int32, void * stream);
  int64_t wait();

private:
  int32_t * pinned_ = nullptr;
  void * event_ = nullptr;
  int device_ = -1;  // device the event belongs to (recreated when a request comes from another one)
  bool pending_ = false;
};
}  // namespace f2n

struct RenderResult
{
  using Tensor = torch::Tensor;
  Tensor colors;
  Tensor depths;
  Tensor weights;
  Tensor idx_start_end;
  // Renderer::render_for_loss only, and only when it says so: CustomOps::WeightVar of the weights,
  // [n_rays] in the caller's order; `weights` is then undefined
  Tensor weight_var;
  // Renderer::render_for_loss with LossOutputs::dist only: CustomOps::WeightDist of the kept
  // samples' weights, t and dt, [n_rays] in the caller's order, on every route; undefined otherwise
  Tensor weight_dist;
  // Renderer::render_for_loss with a depth target only: CustomOps::DepthSight of the kept samples'
  // weights, t and dt against that target, [n_rays, 3] = (empty space, near surface, expected depth)
  // in the caller's order, on every route; undefined otherwise
  Tensor depth_terms;
  // RendererOptions::normals only: N_r = sum_k w_k n^_k over the kept samples (f2n_ray_normals),
  // [n_rays, 3] in the caller's order, detached, not renormalised; undefined when the option is off
  Tensor normals;
  // Renderer::render_for_loss with LossOutputs::opacity only: FlexOps::Sum of the kept samples'
  // weights, [n_rays] in the caller's order, on every route (1 - the transmittance left behind the
  // last kept sample, to rounding), with the gradient going to the weights; undefined otherwise
  Tensor opacity;
};

// What Renderer::render_for_loss hands back beside colours, depths, weights and bounds.  Every field
// works on every route (op by op, march, dense, lean bucketed, with an occupancy grid attached): the
// term is taken where the kept samples' weights, t and dt lie, and on the bucketed routes its per-ray
// result rides back to the caller's order with colours and depths -- nothing per-sample is gathered
// for it.  A field left off launches nothing, and colours, depths, weights and bounds keep their bits
// whatever is asked for.
struct LossOutputs
{
  // RenderResult::weight_dist, the per-ray distortion loss.  t and dt get no gradient (sample
  // positions are data on every training route).
  bool dist = false;
  // defined: RenderResult::depth_terms against it.  [n_rays], each ray's target distance along the
  // ray, in the units of the rays (0, negative or non-finite: the ray has no return); on the bucketed
  // routes it is permuted with the rays.  It receives no gradient.
  torch::Tensor depth_target;
  float depth_eps = 0.f;  // >= 0: the half-width of the surface band around the target
  // RenderResult::opacity, O_r = sum_k w_k over the ray's kept samples (what an alpha target is
  // compared with), taken with f2n_seg_sum_fwd; the gradient goes to the weights.
  bool opacity = false;
};

struct RendererOptions
{
  Hash3DAnchoredOptions field;
  PtsSamplerOptions sampler;
  bool fused = true;
  bool fused_shade = true;         // per-sample network as one kernel (needs L*F in {8,16,32,64})
  // First-pass strategy of the fused path: -1 = adaptive (dense when the previous call kept more
  // than 40 % of its samples), 0 = always the early-terminating march, 1 = always dense.
  // dense: encode ALL samples once with the level-major kernel, derive the keep-prefix from that
  // encoding and hand the (compacted) encoding to the shading pass, so the field is evaluated once
  // instead of twice when little terminates; march: stop rays in-kernel, re-encode survivors.
  int dense_first_pass = -1;
  float early_stop_trans = 1e-4f;  // renderer.cpp:68
  int pixel_tiles = 8;             // render_image traverses the view in tiles of this many pixels squared (0: rows)
  // Dense first pass: when the previous chunk kept every sample, shade all samples first and accept
  // that as the result if no ray comes near the early-stop threshold (see Renderer::render_dense);
  // results are identical either way.
  bool speculate_dense = true;
  // ... chunks of at least this many samples accept the guess on the density-margin flag (no exact
  // scan at all), smaller ones run the scan and only hide its read-back behind the guess
  int64_t margin_min_samples = 2 << 20;
  // No host read at all (what a hipGraph capture of a training iteration needs; the reference
  // syncs at src/renderer.cpp:39-40,69,85-87,120): the dense first pass shades ALL samples and
  // returns that as the result without waiting for the survivor count; whether a ray would have
  // terminated early is ACCUMULATED on the device instead (deferred_bad_: += 1 for every render whose
  // exact scan kept fewer samples than it shaded) and the caller asks deferred_check_ok() whenever it
  // next synchronises anyway -- before it lets an optimiser consume the gradients.  A render whose
  // check fails produced colours that include samples the reference would have dropped (their
  // weights are below 1e-4 of the ray's, but not zero) and must be repeated without this option.
  bool deferred_check = false;
  bool check_finite = false;       // the reference's CHECK(isfinite(colors.mean())) host sync
  // Dense first pass of at least this many rays: render the rays bucketed into pixel-compact bundles
  // (f2n_ray_keys) and hand the results back in the caller's order, bit for bit the same
  // (F2N_OPT_RAY_ORDER = 1 switches it off).  The sort, permutes and gathers cost ~0.1 ms per chunk
  // (measured: +3.5 % at 65536-ray chunks of S = 128, L = 16; -15 % at 8192-ray chunks of S = 64, L = 4).
  int64_t ray_order_min_rays = 65536;
  // Rays that require grad (pose optimisation, reference src/localizer.cpp:142-167) take the fused
  // path too when the fused per-sample network applies (fused_shade, L*F in {8,16,32,64}, a 16-wide
  // field head): the kernels run on detached copies, the encoding's gradient d(enc) that the shade
  // backward forms anyway is turned into d(rays_o), d(rays_d) by one kernel (f2n_hash_rays_grad), and
  // the table, MLP and embedding gradients take exactly the kernels they take without it.  Off: such
  // rays go op by op.  The bucketed dense route is not used for them.
  bool fused_ray_grad = false;
  // Inference in one kernel (f2n_render_rays): render_all_rays / render_image take it when the fused
  // per-sample network applies and nothing can ask for a gradient (Renderer::one_pass_applies);
  // otherwise they do exactly what they do without it.  render() and train_step never take it: it
  // produces no per-sample weights and no gradients.
  bool one_pass = false;
  // How the one-pass render walks a ray (render_rays and everything that follows one_pass):
  //   0  one wavefront per ray, one launch (f2n_render_rays) -- the default;
  //  -1  the whole ray eight rays to a wavefront (f2n_render_rays_head with n_head >= S);
  //  a positive multiple of 64: the first one_pass_head samples eight rays to a wavefront, then the
  //      rays still alive one wavefront each (f2n_render_rays_head + f2n_render_rays_tail).
  // For scenes whose rays stop after a few samples.  Still no host read, O(n_rays)
  // memory (64 bytes of state per ray of a chunk, cached) and capturable in a hipGraph.
  int one_pass_head = 0;
  // Surface normals next to colours and depths: render() fills RenderResult::normals with the
  // weighted sum of the kept samples' unit normals -g/|g|, g the density logit's true spatial
  // gradient (f2n_ray_normals: one launch after compositing, on the kept samples and the weights the
  // route holds anyway).  No gradient flows through them.  While it is on, neither the bucketed nor
  // the lean dense route is taken (they carry no world positions -- the concession fused_ray_grad
  // makes); every other launch is the one made without it and colours, depths and weights keep their
  // bits on the route taken.  Ignored by render_rays and the one-pass path, which have no per-sample
  // weights: use render_all_rays_with_normals / render_image_with_normals.
  bool normals = false;
};

class Renderer : public torch::nn::Module
{
  using Tensor = torch::Tensor;

public:
  explicit Renderer(int n_images, const RendererOptions & opt = {});

  RenderResult render(
    const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx, RunningMode mode);

  // Same, with the device-side randomness supplied: `noise` [n_rays, max_samples] (undefined =
  // draw as the mode dictates), `bg_color` [n_rays, 3] (undefined = rand in TRAIN, 0.5 otherwise).
  RenderResult render(
    const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx, RunningMode mode,
    const Tensor & noise, const Tensor & bg_color);

  // render() for a caller that wants the weights only for their per-ray variance (f2n::train_step):
  // on the lean bucketed dense route the variance is taken from the weights where they lie and its
  // [n_rays] result travels back to the caller's order with colours and depths -- no [n, S] gather
  // either way.  There `weight_var` is defined and `weights` is not; everywhere else this is
  // render() and `weight_var` is undefined.  `want` adds the per-ray extras of LossOutputs.
  RenderResult render_for_loss(
    const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx, RunningMode mode,
    const Tensor & noise, const Tensor & bg_color, const LossOutputs & want = {});

  // The no-grad render as one kernel launch (f2n_render_rays): colours [n, 3], depths [n], last_trans
  // [n] (1 - opacity of the ray: an alpha mask) and kept [n] int32 (samples composited per ray).
  // mode, noise and bg_color as in render(); the attached occupancy grid is used.  Requires the fused
  // per-sample network (L*F in {8,16,32,64}, a 16-wide field head, fused_shade).  Nothing is read
  // back to the host and nothing per-sample is allocated, so the call can be captured in a hipGraph;
  // last_n_samples_ / last_kept_fraction_ (the adaptive route of render()) are left alone.
  std::tuple<Tensor, Tensor, Tensor, Tensor> render_rays(
    const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx, RunningMode mode,
    const Tensor & noise = Tensor(), const Tensor & bg_color = Tensor());

  void set_one_pass(bool on) { options_.one_pass = on; }
  // RendererOptions::one_pass_head: 0, -1 or a positive multiple of 64
  void set_one_pass_head(int n_head);
  // does render_all_rays / render_image take the one-kernel path right now?  (options_.one_pass, the
  // fused network applies, and grad mode is off or no parameter requires grad; rays that themselves
  // require grad under grad mode keep the default routes whatever this says)
  bool one_pass_applies() const;

  std::tuple<Tensor, Tensor> render_all_rays(
    const Tensor & rays_o, const Tensor & rays_d, const int batch_size);

  // dist: optional (k1, k2, p1, p2) of the view's camera, [4] or [1,4] (get_view_rays); undefined =
  // pinhole, as in the reference
  std::tuple<Tensor, Tensor> render_image(
    const torch::Tensor & pose, const torch::Tensor & intrinsic, const int h, const int w,
    const int batch_size, const torch::Tensor & dist = torch::Tensor());

  // render_all_rays / render_image with the per-ray normals as a third output ([n, 3] and [h, w, 3],
  // not clipped, not renormalised): the same chunk loop and pixel-tile traversal, every chunk through
  // render() with RendererOptions::normals on -- the default routes, whatever one_pass says.
  void set_normals(bool on) { options_.normals = on; }
  std::tuple<Tensor, Tensor, Tensor> render_all_rays_with_normals(
    const Tensor & rays_o, const Tensor & rays_d, const int batch_size);
  std::tuple<Tensor, Tensor, Tensor> render_image_with_normals(
    const torch::Tensor & pose, const torch::Tensor & intrinsic, const int h, const int w,
    const int batch_size, const torch::Tensor & dist = torch::Tensor());

  std::vector<torch::optim::OptimizerParamGroup> optim_param_groups(float lr);

  // Empty-space skipping: null = off (the default; same routes, same kernels, same bits as without
  // this call).  Not a parameter or buffer: renderer.pt keeps the reference's layout, the grid is
  // rebuilt from the field (OccupancyGrid::update).  The caller keeps it current.
  void set_occupancy(std::shared_ptr<OccupancyGrid> grid) { occupancy_ = std::move(grid); }
  const std::shared_ptr<OccupancyGrid> & occupancy() const { return occupancy_; }

  // A learned background: null = off (the default; same routes, same kernels, same bits as without
  // this call).  Attached, every render that is handed no bg_color blends background()->query(rays_d)
  // -- in the caller's ray order, in every mode -- where it would have blended rand (TRAIN) or 0.5:
  // render(), render_for_loss(), render_rays() and, through them, render_all_rays / render_image, their
  // _with_normals forms, the one-pass path and the Localizer.  A caller-supplied bg_color always wins.
  // Under grad mode the query carries a gradient to the texture, so choose_route keeps the dense
  // route in the caller's order and off its lean form (the known price).  Not a
  // parameter or buffer, like the occupancy grid: renderer.pt keeps the reference's layout.
  void set_background(std::shared_ptr<f2n::EnvMap> env) { background_ = std::move(env); }
  const std::shared_ptr<f2n::EnvMap> & background() const { return background_; }

  // Per-level weights of the field (Hash3DAnchored::set_level_weights): coarse-to-fine training and
  // level-of-detail renders.  Never set (the default): every route as without these calls, launch for
  // launch and bit for bit; all ones: the same bits.  Folded into the field head, so every route --
  // op by op, march, dense, lean bucketed, with an occupancy grid, train_step, render_rays and the
  // one-pass path (the f2n_render_rays_lod entries), normals, the mesh, the Localizer -- honours them.
  // set_coarse_to_fine(alpha): the weights of f2n_level_weights for a progress alpha in [1, L]
  // (f2n::CoarseToFine::alpha_at makes one from an iteration).  Values move in place: a captured
  // step stays valid while the number of active levels does not change.  Checkpoints hold the raw
  // parameters; the schedule's state stays with the caller.
  void set_level_weights(const Tensor & weights) { scene_field_->set_level_weights(weights); }
  void set_coarse_to_fine(double alpha);
  void clear_level_weights() { scene_field_->clear_level_weights(); }

  RendererOptions options_;
  std::shared_ptr<PtsSampler> pts_sampler_;
  std::shared_ptr<Hash3DAnchored> scene_field_;
  std::shared_ptr<SHShader> shader_;
  Tensor app_emb_;

  int64_t last_n_samples_ = 0;  // survivors of the most recent render() (bench bookkeeping)
  float last_kept_fraction_ = 0.f;
  f2n::HostCount survivors_;
  // f2n_render_rays_head's state for the largest chunk seen (one_pass_head > 0); grown outside graph
  // capture by the warm-up calls, reused afterwards
  Tensor one_pass_state_;

  // options_.deferred_check: renders since the last reset whose guess "nothing terminates" was wrong
  // (device int32, created on first use; stays valid across hipGraph replays).  deferred_check_ok()
  // reads it (a host sync) and resets it.
  Tensor deferred_bad_;
  bool deferred_check_ok();

  // mean over the rays of weight_dist in the most recent f2n::train_step with a distortion weight
  // (device scalar, detached, no host read); undefined after a step without one
  Tensor last_dist_loss_;
  // the three means over the valid rays (empty space, near surface, expected depth) of the most
  // recent f2n::train_step with a depth target and a non-zero DepthLossOptions weight ([3], device,
  // detached, no host read); undefined after a step without
  Tensor last_depth_loss_;
  // the weighted mean over the rays of (opacity - alpha)^2 in the most recent f2n::train_step with
  // an alpha target and the rendered opacity (device scalar, detached, no host read); undefined
  // after a step without
  Tensor last_opacity_loss_;
  // the unweighted mean over the patches of 1 - SSIM_b in the most recent f2n::train_step with an
  // active PatchLoss (device scalar, detached); undefined when the last step had none
  Tensor last_ssim_loss_;

private:
  // Everything the routes branch on, decided once per render() call (choose_route).
  struct Route
  {
    enum FirstPass { OpByOp, March, Dense };
    FirstPass first_pass = OpByOp;
    bool bucketed = false;   // Dense only: render_dense_bucketed instead of the caller's order
    bool fused_net = false;  // the fused per-sample network (f2n::shade) applies
    Rays grad_rays;          // the caller's rays when they carry a gradient, else undefined
    // Dense only, F2N_OPT_DENSE_LEAN = 0, the ray-uniform network kernels apply and neither rays nor
    // bg_color carry a gradient: f2n_sample_dense (contracted positions and one direction per ray;
    // no world positions, no per-sample directions, the noise read in place)
    bool lean = false;
    bool noise_raw = false;  // lean: the noise is the renderer's own uniform draw, cooked in the sampler
    bool want_var = false;   // lean and bucketed, render_for_loss: hand back weight_var, not weights
    // render_for_loss: the extras to hand back.  want.depth_target is [n_rays] f32 in the order of the
    // rays the route renders (render_dense_bucketed permutes it with them), else undefined
    LossOutputs want;
  };
  // What the shading pass hands to compositing: the field head's output ([n, 1] density logit of the
  // fused network, [n, 16] otherwise) and the colours [n, 3].
  struct Shaded
  {
    Tensor field_out, rgb;
  };

  Route choose_route(const Tensor & rays_o, const Tensor & rays_d, const Tensor & bg_color) const;
  RenderResult render_routed(
    const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx, RunningMode mode,
    const Tensor & noise, const Tensor & bg_color, bool for_loss, const LossOutputs & want);
  bool fused_net_applies() const;
  // f2n_render_rays -- or, by options_.one_pass_head, the head or head + tail -- into preallocated
  // outputs (rows of one chunk)
  void render_rays_into(
    const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx, RunningMode mode,
    const Tensor & noise, const Tensor & bg_color, Tensor colors, Tensor depths, Tensor last_trans,
    Tensor kept);

  // The routes.  render_fused: detached rays, then march / dense / dense bucketed.
  RenderResult render_op_by_op(
    const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx, RunningMode mode,
    const Tensor & noise, const Tensor & bg_color, const Route & route);
  RenderResult render_fused(
    const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx, RunningMode mode,
    const Tensor & noise, const Tensor & bg_color, const Route & route);
  // noise_rows (lean, bucketed): ray r's noise is row noise_rows[r] of `noise`, which stays in the
  // caller's order
  RenderResult render_dense(
    const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx, RunningMode mode,
    const Tensor & noise, const Tensor & bg_color, const Route & route,
    const Tensor & noise_rows = Tensor());
  RenderResult render_dense_bucketed(
    const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx, RunningMode mode,
    const Tensor & noise, const Tensor & bg_color, const Route & route);

  // The steps.  enc_cm / contracted: the samples' encoding (channel-major) and contracted positions
  // when a dense first pass has them already, else undefined (the shading pass encodes).
  std::pair<Tensor, Tensor> scan_survivors(
    const SampleResultFlex & all, const Tensor & enc_all_cm, int n_rays);
  // len: with an occupancy grid, the per-ray prefix lengths the bounds were thinned from
  SampleResultFlex compact_samples(
    const Tensor & rays_o, const Tensor & rays_d, const Tensor & noise, const Tensor & bounds,
    int64_t n_kept, const Tensor & len = Tensor());
  std::optional<RenderResult> shade_all_unless_near_threshold(
    const SampleResultFlex & all, const Tensor & emb_idx, RunningMode mode, const Tensor & bg_color,
    const Route & route, const Tensor & enc_cm, const Tensor & contracted);
  Shaded shade(
    const SampleResultFlex & kept, const Tensor & emb_idx, RunningMode mode, const Route & route,
    const Tensor & enc_cm, const Tensor & contracted);
  Tensor shade_aten(
    const Tensor & scene_feat, const SampleResultFlex & kept, const Tensor & emb_idx,
    RunningMode mode);
  // final = false: a guess of render_dense that may be thrown away -- RenderResult::normals is left
  // to the caller, who launches ray_normals once the guess is accepted
  RenderResult composite(
    const SampleResultFlex & kept, const Shaded & shaded, const Tensor & bg_color,
    const Route & route, bool final = true);
  RenderResult shade_and_composite(
    const SampleResultFlex & kept, const Tensor & emb_idx, RunningMode mode,
    const Tensor & bg_color, const Route & route, const Tensor & enc_cm = Tensor(),
    const Tensor & contracted = Tensor(), bool final = true);
  // RenderResult::weight_dist, depth_terms and opacity of the kept samples' weights, as route.want
  // asks: what render_op_by_op and composite share
  void per_ray_terms(
    RenderResult & res, const Tensor & weights, const SampleResultFlex & kept, const Route & route);
  // RenderResult::normals of the kept samples (raw positions) and their weights: one launch of
  // f2n_ray_normals, nothing recorded by autograd
  Tensor ray_normals(const SampleResultFlex & kept, const Tensor & weights);
  // n_all < 0: the kept fraction (what the adaptive first-pass choice reads) keeps its value
  void record_kept(int64_t n_kept, int64_t n_all = -1);

  // bg_in when defined, else the attached map's colours of rays_d, else rand (TRAIN) / 0.5
  Tensor background_or_default(
    const Tensor & bg_in, const Tensor & rays_d, RunningMode mode, int64_t n_rays) const;

  std::shared_ptr<OccupancyGrid> occupancy_;
  std::shared_ptr<f2n::EnvMap> background_;
};

namespace f2n
{

// The loss / backward segment of the reference's training loop
// (reference src/main_functions/train_manager.cpp:76-107 minus the optimiser step):
// render(TRAIN), Charbonnier colour loss, scheduled weight-variance loss, backward().
struct TrainStepResult
{
  Tensor loss;        // scalar
  Tensor sq_err_sum;  // scalar: sum over rays and channels of (pred - gt)^2
  int64_t n_values;   // n_rays * 3
  int64_t n_samples;  // surviving samples in this step
  // RaySupervision only: the sum of the ray weights as the loss formed it (device scalar, detached;
  // the number of rays when no weight was given); undefined without supervision
  Tensor weight_sum;
  // RaySupervision::want_colors only: the render's colours [n_rays, 3], detached (what
  // ErrorMap::accumulate takes); undefined otherwise
  Tensor colors;
  // RobustLoss only: the weight m_r omega_r the step's terms used ([n_rays], detached; what
  // ErrorMap::accumulate takes as its ray_weight, so that the map does not chase what the loss
  // rejected) and f2n_robust_weights' {T, N_c, sum of the pixel labels, sum of the final labels}
  // ([4], device); both undefined when the robust loss is off
  Tensor robust_weight, robust_stats;
};

// Caller indices of the rays sorted into pixel-compact bundles: the stable sort of their
// f2n_ray_keys, int64 [n].
Tensor ray_order(const Tensor & rays_d);

// The coarse-to-fine schedule of bundle-adjusting fields: the progress
//   alpha = base + (L - base) * clamp((it - start) / (end - start), 0, 1)
// that Renderer::set_coarse_to_fine takes.  end <= start: `base` before start, L from start on.
struct CoarseToFine
{
  double start = 0., end = 1., base = 1.;
  double alpha_at(double it, int64_t L) const;
};

// f2n_level_weights as a CPU tensor [L] and its number of active levels.
std::pair<Tensor, int64_t> level_weights(double alpha, int64_t L);

// Weights of the three line-of-sight depth terms (CustomOps::DepthSight) and the half-width of the
// surface band.  All three weights exactly 0: no depth term.  The schedule (URF shrinks eps while
// training) stays with the caller.
struct DepthLossOptions
{
  float empty = 0.f;     // lambda of E_r: weight in the free space before the return
  float near = 0.f;      // lambda of N_r: weight missing from the band around the return
  float expected = 0.f;  // lambda of X_r: squared error of the expected depth
  float eps = 0.f;       // half-width of the band, in the units of the rays
  bool active() const { return empty != 0.f || near != 0.f || expected != 0.f; }
};

// Per-ray supervision of a masked batch (f2n::sample_masked_rays makes one).  Both tensors undefined:
// no supervision.
struct RaySupervision
{
  Tensor ray_weight;           // [n_rays] m_r: 0 drops the ray from every term; undefined = 1
  Tensor alpha;                // [n_rays] a_r in [0, 1]: the ground truth's alpha; undefined = opaque
  float opacity_weight = 0.f;  // lambda of mean_r m_r (O_r - a_r)^2
  // hand the render's colours back in TrainStepResult::colors (a detached view of what the loss
  // read: no launch, and nothing else of the step changes)
  bool want_colors = false;
  // true: the colour target of a ray is a gt + (1 - a) bg (a sky ray's target is the background the
  // render blended in).  false: the colour target is gt unchanged and alpha feeds only the opacity
  // term -- what a learned background (Renderer::set_background) needs, or its texture never sees
  // the image; bg_color may then be left undefined.
  bool composite_target = true;
  bool weighted() const { return ray_weight.defined() || alpha.defined(); }
  bool want_opacity() const { return alpha.defined() && opacity_weight != 0.f; }
};

// A structural term on patches (f2n::sample_patch_rays makes such a batch; CustomOps::Ssim).
// patch == 0 or ssim_weight == 0: no term.
struct PatchLoss
{
  int patch = 0;             // P: the rays are n_patches * P^2, patch-major, row-major in a patch
  float ssim_weight = 0.f;   // lambda of sum_b m_b (1 - SSIM_b) / M
  Tensor patch_weight;       // [n_patches] m_b: 0 drops the patch; undefined = 1
  bool active() const { return patch != 0 && ssim_weight != 0.f; }
};

// The terms of f2n::train_step's loss beside the colour loss.  Each is off at its default, and a term
// that is off is neither computed nor differentiated: the step is then the one without it, launch for
// launch and bit for bit.  The schedules stay with the caller, like the reference's variance-loss
// ramp (src/main_functions/train_manager.cpp:85-91).
struct LossTerms
{
  float var_weight = 0.f;  // lambda of the weight-variance loss; 0: its backward kernel is not run
  // The distortion loss: loss += dist_weight * mean_r D_r (CustomOps::WeightDist; the mean is left in
  // Renderer::last_dist_loss_).  Exactly 0: off.
  float dist_weight = 0.f;
  // Depth supervision: `depth_target` [n_rays] as in LossOutputs, and
  //   loss += sum_i lambda_i * (sum over valid rays of term_i) / max(n_valid, 1),
  // n_valid counted on the device (no host read); the three means are left in
  // Renderer::last_depth_loss_.  An undefined target, or all three weights exactly 0: off.
  Tensor depth_target;
  DepthLossOptions depth;
  // Masked rays and alpha targets (f2n::train_loss_sup).  The colour target of a ray becomes
  // a gt + (1 - a) bg with the background colour the render blended in -- bg_color, which is then
  // required -- both means divide by W = sum_r m_r (1 when that is not positive; no host read), and
  //   loss = colour + var_weight * var + opacity_weight * sum_r m_r (O_r - a_r)^2 / W
  // with O_r the ray's rendered opacity (RenderResult::opacity; its mean term is left in
  // Renderer::last_opacity_loss_).  The distortion and depth terms are weighted by m_r as well, before
  // their reductions, which keep their divisors (n_rays, n_valid): a masked ray regularises nothing.
  // sq_err_sum is the weighted sum, weight_sum is sum_r m_r.  With ray_weight and alpha both undefined:
  // off, whatever opacity_weight says (want_colors then still fills TrainStepResult::colors, which
  // costs no launch).
  // With composite_target = false the colour and variance terms are f2n_loss_sup_fwd's without alpha
  // (gt' = gt), and the opacity term is formed in ATen from that entry's device scalar W:
  //   d = O - a on the rays with m != 0, else 0;  opac = sum_r m_r d_r^2 / W;  loss += opacity_weight opac
  // -- no host read, last_opacity_loss_ filled, a ray with m_r = 0 contributes exact zeros to the term
  // and to the opacity's gradient.
  RaySupervision sup;
  // A D-SSIM term on patches:
  //   loss += ssim_weight * sum_b m_b (1 - SSIM_b) / M,  M = sum_b m_b (1 when that is not positive;
  // no host read), SSIM_b the unclamped SSIM of the render's colours viewed as [n_patches, P, P, 3]
  // against the colour target the colour loss used (a gt + (1 - a) bg where the alpha target
  // composites).  The gradient reaches the colours through CustomOps::Ssim as the distortion term's
  // reaches the weights; a patch with m_b = 0 contributes exact zeros.  The unweighted mean of
  // 1 - SSIM_b is left in Renderer::last_ssim_loss_.  A ray count that is no multiple of P^2, P < 11
  // or a patch_weight of another length throws.  patch == 0 or ssim_weight == 0: off.
  PatchLoss patch;
  // A trimmed colour loss (robust_loss.hpp; f2n_robust_weights has the rule).  After the render, under
  // no-grad, the render's own detached colours and the colour target the colour loss uses (a gt +
  // (1 - a) bg where the alpha target composites) give per-ray weights m_r omega_r, and those stand
  // wherever m_r stands above: f2n::train_loss_sup and the opacity, distortion and depth terms -- a
  // rejected ray contributes exact zeros and regularises nothing.  The D-SSIM term keeps the caller's
  // patch_weight.  The weighted loss entry runs also when the caller gave neither ray_weight nor
  // alpha.  robust.patch is the P of the rule (0: scattered rays) and need not be PatchLoss::patch.
  // TrainStepResult::robust_weight and robust_stats are filled; no host read.  quantile >= 1: off.
  RobustLoss robust;

  bool want_dist() const { return dist_weight != 0.f; }
  bool want_depth() const { return depth_target.defined() && depth.active(); }
  // per-ray weights exist: the step goes through f2n::train_loss_sup, not f2n::train_loss
  bool weighted() const { return robust.active() || sup.weighted(); }
};

// One training step: render(TRAIN), the colour loss and the terms of `terms`, backward().  `noise` and
// `bg_color` as in Renderer::render.
TrainStepResult train_step(
  Renderer & renderer, const Tensor & rays_o, const Tensor & rays_d, const Tensor & emb_idx,
  const Tensor & gt_colors, const LossTerms & terms = {}, const Tensor & noise = {},
  const Tensor & bg_color = {}, bool run_backward = true);

}  // namespace f2n
