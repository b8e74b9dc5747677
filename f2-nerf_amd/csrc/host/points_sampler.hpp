// points_sampler.hpp -- PtsSampler: uniform jittered ray marching samples.
// Public surface of reference src/points_sampler.hpp:15-40 (SampleResultFlex, RunningMode,
// PtsSampler::get_samples); MAX_SAMPLE_PER_RAY / SAMPLE_L become runtime options whose defaults are
// the reference's constants (1024, 1/256).
#pragma once

#include "common.hpp"

constexpr int MAX_SAMPLE_PER_RAY = 1024;  // reference default (points_sampler.hpp:15)

struct SampleResultFlex
{
  using Tensor = torch::Tensor;
  Tensor pts;             // [ n_all_pts, 3 ]
  Tensor dirs;            // [ n_all_pts, 3 ]
  Tensor dt;              // [ n_all_pts ]
  Tensor t;               // [ n_all_pts ]
  Tensor pts_idx_bounds;  // [ n_rays, 2 ] start, end
  // PtsSampler::get_samples_dense only (pts and dirs stay undefined there):
  Tensor x;               // [ n_all_pts, 3 ] contracted positions
  Tensor ray_dirs;        // [ n_rays, 3 ] unit direction of each ray
};

enum RunningMode { TRAIN, VALIDATE };

struct PtsSamplerOptions
{
  int max_samples = MAX_SAMPLE_PER_RAY;
  float step = 1.0f / 256;  // SAMPLE_L (points_sampler.hpp:39)
};

class PtsSampler
{
  using Tensor = torch::Tensor;

public:
  explicit PtsSampler(const PtsSamplerOptions & opt = {});

  // One kernel instead of the reference's ~20 ATen launches (points_sampler.cpp:20-64).  Not
  // differentiable in the rays: use get_samples_grad() when rays carry gradients.
  SampleResultFlex get_samples(const Tensor & rays_o, const Tensor & rays_d, RunningMode mode);
  // Same, with the step-noise tensor [n_rays, max_samples] supplied (undefined = all ones).
  SampleResultFlex get_samples(const Tensor & rays_o, const Tensor & rays_d, const Tensor & noise);

  // The dense [n_rays, max_samples] grid for the hash encode and the ray-uniform network kernels, one
  // kernel (f2n_sample_dense): x (the contracted positions), dt, t, pts_idx_bounds and ray_dirs; no
  // world positions, no per-sample directions.  Same bits as get_samples + f2n_contract_fwd.
  //   noise      [n_rays, max_samples] or undefined (all ones)
  //   noise_rows [n_rays] int32 or undefined: ray r takes row noise_rows[r] of `noise`
  //   noise_raw  `noise` is draw_noise_raw()'s uniform draw, cooked in the kernel
  SampleResultFlex get_samples_dense(
    const Tensor & rays_o, const Tensor & rays_d, const Tensor & noise, const Tensor & noise_rows,
    bool noise_raw);

  // The reference's own ATen formulation (differentiable in rays_o / rays_d through autograd).  Its
  // positions differ from the kernel's in their last bit; no render route takes it any more.
  SampleResultFlex get_samples_aten(
    const Tensor & rays_o, const Tensor & rays_d, const Tensor & noise);

  // get_samples' own samples, bit for bit, with the positions differentiable in rays_o / rays_d:
  // pts = o + d^ t with d^ = d / |d|, so d_o = sum_k d_pts_k and d_d = (I - d^ d^T) / |d| sum_k t_k
  // d_pts_k.  dt = |d^| (t_k - t_{k-1}) and t do not depend on the rays.  The op-by-op route takes
  // this when rays carry a gradient, so that it renders the positions every other route renders.
  SampleResultFlex get_samples_grad(
    const Tensor & rays_o, const Tensor & rays_d, const Tensor & noise);

  // TRAIN: U[0,1) - 0.5 + 1 per sample (points_sampler.cpp:35); VALIDATE: undefined tensor (= ones).
  Tensor draw_noise(int64_t n_rays, RunningMode mode, const torch::Device & device) const;
  // The two halves of draw_noise: the uniform draw U[0,1) (the same torch::rand call, so the same
  // generator stream; undefined in VALIDATE), and draw_noise's two element-wise passes over it.
  Tensor draw_noise_raw(int64_t n_rays, RunningMode mode, const torch::Device & device) const;
  static Tensor cook_noise(const Tensor & raw);

  PtsSamplerOptions options_;
};
