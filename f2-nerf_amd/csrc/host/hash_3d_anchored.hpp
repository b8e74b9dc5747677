// hash_3d_anchored.hpp -- Hash3DAnchored: the multi-resolution hash-grid scene field.
//
// Same public surface as the reference class (reference src/hash_3d_anchored.hpp:13-52): a
// torch::nn::Module with feat_pool_ / prim_pool_ / bias_pool_ / mlp_, query(points),
// optim_param_groups(lr), the Hash3DAnchoredInfo custom-class holder and
// torch::autograd::Hash3DAnchoredFunction(points, feat_pool, IValue info).  Parameter names and
// shapes are kept ("feat_pool", "prim_pool", "bias_pool", "mlp.*") so a reference checkpoint loads.
//
// What is different, by design:
//   * N_LEVELS / N_CHANNELS / table size are runtime options (defaults = the reference's
//     compile-time constants, hash_3d_anchored.hpp:10-11, hash_3d_anchored.cpp:21);
//   * the f16 working copy of the table is a persistent shadow refreshed only when feat_pool_
//     changes (the reference re-casts all 2^24 elements on every forward AND backward,
//     hash_3d_anchored.cu:169,198); the shadow is the same RNE cast of the same f32 master;
//   * the per-level scale table mul[l] is computed once on the host (exp2f) and passed to the kernels.
#pragma once

#include "common.hpp"

struct Hash3DAnchoredOptions
{
  int64_t n_levels = 16;     // N_LEVELS
  int64_t n_channels = 2;    // N_CHANNELS (features per level): 1, 2, 4 or 8
  int64_t log2_table = 19;   // rows per level = 2^log2_table (reference: pool = 2^19 * N_LEVELS)
  int64_t level_stride = 0;  // elements between level bases; 0 = reference behaviour (= rows per
                             // level, so adjacent levels overlap)
  int64_t mlp_out_dim = 16;
  bool binned_backward = true;  // large batches: f2n_hash_bwd_binned (needs a scratch workspace)
  // The table's gradient is 64 MiB.  Handed to autograd per backward call it costs a zero fill and,
  // from the second call of an iteration on (a view rendered in chunks), an accumulation pass over
  // all of it -- 48 us per call for a kernel that may take 180.  When feat_pool already has a
  // gradient, the kernels add into it directly and autograd is told "no gradient" for that input.
  // Tensor hooks on feat_pool do not see those calls; switch it off if you rely on them.
  bool accumulate_in_place = true;
  // Points (and rays) that require a gradient receive the encoding's true derivative -- the
  // interpolant differentiated with all three axes' weights, in f32 (f2n_hash_pts_grad_exact,
  // f2n_hash_rays_grad_exact) -- instead of the reference's point gradient (quirk Q5, about 4 times
  // a cell-centre derivative and rounded through f16): the magnitude changes, learning rates tuned
  // with it off do not carry over.  Off: every route launches what it always launched.
  bool exact_point_grad = false;
  // With level weights set (set_level_weights) whose tail is zero, the kernels that take L as a loop
  // bound are called with active_levels() instead: the levels the head multiplies by zero are not
  // gathered at all, forward or backward, and their rows of the encoding are zero-filled.  Off: every
  // level is walked and the fold alone applies the weights (the A/B arm; the same results).
  bool skip_masked_levels = true;
  torch::Device device = f2n::default_device();
};

namespace f2n
{

// The grid as every kernel entry of f2nerf_hip.h that walks it takes it (table, primes, bias, mul,
// ..., L, F, T, level_stride), already cast.  Pointers into tensors the caller keeps alive.
struct FieldArgs
{
  const uint16_t * table;
  const int32_t * primes;
  const float *bias, *mul;
  int L, F;
  uint32_t T;
  int64_t level_stride;
  int L_walk;  // the loop bound for entries that walk the levels: L, or fewer (Hash3DAnchored::walk_levels)
};

}  // namespace f2n

class Hash3DAnchored : public torch::nn::Module
{
  using Tensor = torch::Tensor;

public:
  explicit Hash3DAnchored(const Hash3DAnchoredOptions & opt = {});

  Tensor query(const Tensor & points);

  // contraction + hash encode only (no Linear): [n, L*F], stored channel-major.  The Renderer's
  // fused path feeds this straight into the fused per-sample network kernel.
  // samples_per_ray > 0 declares `points` a dense ray-major [n_rays, samples_per_ray] grid: the
  // forward then walks neighbouring rays per wavefront (f2n_hash_fwd_raytile), same results.
  // contracted_out, if given, receives the contracted points (to hand back to encode_cached).
  // Level weights (below) are NOT applied here: the features are the unweighted ones, with exact
  // zeros in the rows of the levels that skip_masked_levels leaves out.
  Tensor encode(const Tensor & points, int64_t samples_per_ray = 0, Tensor * contracted_out = nullptr);

  // encode() of positions that are contracted already (f2n_sample_dense writes them): `x` [n, 3] goes
  // to the hash encode as it is, no contraction node.  For positions that carry no gradient.
  Tensor encode_contracted(const Tensor & x, int64_t samples_per_ray = 0);

  // Same autograd node as encode(), but the forward result is supplied: `enc_cm` [L*F, n]
  // channel-major, the encoding of exactly these points computed earlier (the Renderer's first pass).
  // Only the backward (table gradient) runs a kernel.
  // `contracted`, if defined, is the contraction of exactly these points (from encode()); it is
  // used as is when the points carry no gradient.  `points` may be undefined when `contracted` is
  // given (a sampler that wrote contracted positions only).
  Tensor encode_cached(
    const Tensor & points, const Tensor & enc_cm, const Tensor & contracted = Tensor());

  // Row 0 of head_weight() and of mlp_'s bias (weight [L*F], bias [1]) as contiguous device tensors:
  // the density head the fused ray march evaluates in-kernel.
  std::pair<Tensor, Tensor> density_head() const;

  // ---- level weights: coarse-to-fine training and level-of-detail renders ----
  // lw[L] >= 0 scales what level l contributes to the head: h = b_h + sum_l lw[l] W_h[:, lF..lF+F) enc_l,
  // i.e. the head with its columns scaled.  The weights are FOLDED into the head (head_weight());
  // no encode kernel applies them, and d_enc = W_eff^T d_h carries them into every gradient.
  // encode() / encode_contracted() therefore return UNWEIGHTED features -- with exact zeros for the
  // levels skip_masked_levels leaves out.
  //   set_level_weights  a CPU or device [L] tensor of finite values >= 0, the last non-zero one
  //                      deciding active_levels().  Copied IN PLACE into one persistent device tensor:
  //                      a captured graph sees later values (it stays valid while walk_levels() does
  //                      not change).
  //   clear_level_weights  back to the field without weights, launch for launch.
  void set_level_weights(const Tensor & weights);
  void clear_level_weights() { has_level_weights_ = false; }
  bool has_level_weights() const { return has_level_weights_; }
  // the host copy [L] (undefined when none are set) / 1 + the index of the last non-zero weight (L
  // when none are set)
  Tensor level_weights() const { return has_level_weights_ ? level_weights_host_ : Tensor(); }
  int64_t active_levels() const { return has_level_weights_ ? active_levels_ : options_.n_levels; }
  // what the kernels that loop over levels are given: active_levels() under skip_masked_levels, else L
  int walk_levels() const
  {
    return (int)(options_.skip_masked_levels ? active_levels() : options_.n_levels);
  }
  // mlp_->weight itself when no weights are set; otherwise mlp_->weight * (lw (x) 1_F), one ATen
  // product that autograd differentiates (g_W_h = g_W_eff * cols).
  Tensor head_weight() const;

  // d(density logit)/d(position) at the raw points [n, 3] -> [n, 3]: the spatial gradient of the
  // trilinear interpolant query() evaluates, followed by row 0 of mlp_ and taken through the
  // contraction (f2n_density_grad).  Not the point gradient autograd returns for query(), which is
  // the reference's (quirk Q5: no interpolation weights of the other two axes).  No-grad, detached.
  Tensor density_grad(const Tensor & points);

  // Hash3DAnchoredOptions::exact_point_grad, for a field that exists already.  Both autograd nodes
  // that form a point gradient (Hash3DAnchoredFunction, the Renderer's RayGradFn) read it at
  // backward time.
  void set_exact_point_grad(bool on) { options_.exact_point_grad = on; }

  // f16 working copy of feat_pool_, refreshed if feat_pool_ was modified since the last call.
  Tensor table_f16();
  // f16 copy of an arbitrary table tensor (the shadow when it is feat_pool_ itself).
  Tensor table_for(const Tensor & feat_pool);
  // The grid for a kernel call, over `table16` (what table_f16() / table_for() returned).
  f2n::FieldArgs kernel_args(const Tensor & table16) const;

  // For an optimiser that rewrites the shadow itself while updating feat_pool_ (FusedAdam): the
  // shadow buffer (allocated on demand), and the call that declares it current.
  Tensor shadow_storage();
  void mark_shadow_fresh();

  std::vector<torch::optim::OptimizerParamGroup> optim_param_groups(float lr);

  Hash3DAnchoredOptions options_;
  int pool_size_;
  int local_size_;
  int64_t level_stride_;

  Tensor feat_pool_;  // [ pool_size_, n_channels ]
  Tensor prim_pool_;  // [ n_levels, 3 ] int32
  Tensor bias_pool_;  // [ n_levels, 3 ]
  Tensor level_mul_;  // [ n_levels ] f32, exp2f(7 l/(L-1) + 3)  (not a parameter)

  torch::nn::Linear mlp_ = nullptr;

private:
  Tensor feat_pool_f16_;
  const void * shadow_src_ = nullptr;
  uint32_t shadow_version_ = 0;

  bool has_level_weights_ = false;
  int64_t active_levels_ = 0;
  Tensor level_weights_host_;  // [L] f32, CPU
  Tensor level_cols_;          // [L*F] f32 on the device: lw (x) 1_F, rewritten in place
};

class Hash3DAnchoredInfo : public torch::CustomClassHolder
{
public:
  Hash3DAnchored * hash3d_ = nullptr;
  torch::Tensor precomputed_cm_;  // optional [L*F, n] encoding to return instead of computing it
  int64_t samples_per_ray_ = 0;   // > 0: points are a dense [n_rays, samples_per_ray] grid
};

namespace torch::autograd
{

class Hash3DAnchoredFunction : public Function<Hash3DAnchoredFunction>
{
public:
  static variable_list forward(
    AutogradContext * ctx, Tensor points, Tensor feat_pool_, IValue hash3d_info);

  static variable_list backward(AutogradContext * ctx, variable_list grad_output);
};

}  // namespace torch::autograd
