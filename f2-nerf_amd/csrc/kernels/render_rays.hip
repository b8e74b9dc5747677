// render_rays.hip -- the no-grad render as ONE kernel: rays in, colours out.
//
// Replaces, for inference, the whole of Renderer::render (reference src/renderer.cpp:33-123) as
// render_all_rays (:125-151), render_image (:153-172) and Localizer::evaluate_poses
// (src/localizer.cpp:172) use it: the early-stop first pass, where() + four index() gathers, the second
// field query, the shader and the compositing sums.  The fused march route does the same work in six
// launches around a host read of the survivor count, evaluates the field twice on every kept sample
// and carries 180 bytes per kept sample through HBM.  Without gradients nothing per-sample has to
// outlive the 64-sample stride that produced it.
//
// Mapping: one wavefront per ray (persistent workgroups of kWaves waves walk the ray list), lanes =
// 64 consecutive samples, as in the march (sampler.hip).  Per stride:
//   1. make_stride, contract_point, the optional occupancy bit -- the march's;
//   2. the level loop of the march (density_chain).  Its F f16-rounded values per level go two ways:
//      into the march's density chain  logit_c = fmaf(enc, w_h[0][c], logit_c)  from b_h[0], same
//      order, same bits; and into a per-wave f16 LDS tile [C][kPitch], lane = sample;
//   3. the march's keep decision on logit_c (keep_step: scan, carry, ballot): the kept set EQUALS the
//      march's;
//   4. if the stride holds a kept, occupied sample: the tile is read back in the Q-layout of
//      shade_mfma.hip and the head, hidden and output layers of the ray-uniform forward run on the
//      matrix cores.  SH16(dir), the embedding row and b1 + w1[:, 16:32] . SH(dir) are formed once
//      per RAY.  h[0] is the density logit as f2n_shade_fwd computes it;
//   5. h[0] and the three pre-sigmoid colours go through a small LDS row back to lane = sample and
//      composite_fwd_kernel's stride runs on them (its own scan and carry, four fmaf accumulators).
// Two logits on purpose: the chain decides which samples exist, the matrix-core head weights them --
// what the existing route does with its two field evaluations.
//
// No workspace, no atomics: two launches give the same bits.
#include "render_rays.hiph"

#include <algorithm>

namespace
{

template <int C, int F, bool POW2>
__global__ __launch_bounds__(RShape<C>::kWaves * 64) void render_rays_kernel(
  F2N_RENDER_PARAMS, int corner_order, int L_active)
{
  using R = RShape<C>;
  using FS = typename R::FS;
  __shared__ __attribute__((aligned(16))) float lds_all[R::kLdsFloats];
  float * lds_w = lds_all;
  stage_fwd_weights<C, R::kWaves>(lds_w, p_w_h, p_b_h, p_w1, p_b1, p_w2, p_b2);
  __syncthreads();

  const int lane = lane_id();
  // the wave index in a scalar register: the ray, its origin, direction and image id are scalar loads
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool has_emb = (p_emb != nullptr) && (ray_img != nullptr);
  const bool has_grid = bits != nullptr;
  const float bias0 = p_b_h[0];
  const RenderArgs a = {rays_o, rays_d, noise,      table, primes,     bias,  mul, p_w_h,
                        p_emb,  ray_img, bits,      G,     bg,         colors, depths, last_trans,
                        kept,   len,     S,         step,  T,          level_stride, t_thresh,
                        density_shift,   t_shift, corner_order, L_active};
  const RayResume whole = {0, {0.f, 0.f, 0.f, 0.f}, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0, 0};
  __half * tile = reinterpret_cast<__half *>(lds_all + FS::kWFloats + wave * R::kWaveFloats);
  float * OUT = lds_all + FS::kWFloats + wave * R::kWaveFloats + R::kTileFloats;
  zero_tile_tail<C, F>(tile, L_active, lane);

  for (int r = (int)blockIdx.x * R::kWaves + wave; r < n_rays; r += (int)gridDim.x * R::kWaves)
    render_one_ray<C, F, POW2>(a, r, whole, lds_w, tile, OUT, lane, has_emb, has_grid, bias0);
}

}  // namespace

extern "C" int f2n_render_rays_lod(
  const float * rays_o, const float * rays_d, const float * noise, const uint16_t * table,
  const int32_t * primes, const float * bias, const float * mul, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, const int32_t * ray_img, const uint32_t * occ_bits, int G, const float * bg,
  float * colors, float * depths, float * last_trans, int32_t * kept, int32_t * len, int n_rays,
  int S, float step, int L, int L_active, int F, uint32_t T, int64_t level_stride, float t_thresh,
  float density_shift, float t_shift, void * stream)
{
  bool launch;
  const int st = render_args_status(F2N_RENDER_KARGS, L, F, L_active, S, nullptr, &launch);
  if (st != F2N_OK || !launch) return st;
  hipStream_t s = (hipStream_t)stream;
  // persistent workgroups: the weight operands are staged once per workgroup, not once per 8 rays
  f2n_dispatch_width_field(L, F, T, [&](auto cc, auto ff, auto p2) {
    using R = RShape<decltype(cc)::value>;
    const unsigned grid = std::min<unsigned>(f2n_div_up(n_rays, R::kWaves), 512u);
    hipLaunchKernelGGL(
      (render_rays_kernel<decltype(cc)::value, decltype(ff)::value, decltype(p2)::value>),
      dim3(grid), dim3(R::kWaves * 64), 0, s, F2N_RENDER_KARGS,
      f2n_get_option(F2N_OPT_GATHER_PAIRED), L_active);
  });
  return f2n_launch_status();
}

extern "C" int f2n_render_rays(
  const float * rays_o, const float * rays_d, const float * noise, const uint16_t * table,
  const int32_t * primes, const float * bias, const float * mul, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, const int32_t * ray_img, const uint32_t * occ_bits, int G, const float * bg,
  float * colors, float * depths, float * last_trans, int32_t * kept, int32_t * len, int n_rays,
  int S, float step, int L, int F, uint32_t T, int64_t level_stride, float t_thresh,
  float density_shift, float t_shift, void * stream)
{
  return f2n_render_rays_lod(
    rays_o, rays_d, noise, table, primes, bias, mul, w_h, b_h, w1, b1, w2, b2, app_emb, ray_img,
    occ_bits, G, bg, colors, depths, last_trans, kept, len, n_rays, S, step, L, L, F, T, level_stride,
    t_thresh, density_shift, t_shift, stream);
}
