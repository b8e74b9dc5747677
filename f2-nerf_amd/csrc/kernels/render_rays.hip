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
//   2. the level loop of density_march[_occ]_kernel.  Its F f16-rounded values per level go two ways:
//      into the march's density chain  logit_c = fmaf(enc, w_h[0][c], logit_c)  from b_h[0], same
//      order, same bits; and into a per-wave f16 LDS tile [C][kPitch], lane = sample;
//   3. the march's keep decision on logit_c (scan, carry, ballot): the kept set EQUALS the march's;
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
  const float * __restrict__ rays_o, const float * __restrict__ rays_d,
  const float * __restrict__ noise, const uint16_t * __restrict__ table,
  const int32_t * __restrict__ primes, const float * __restrict__ bias,
  const float * __restrict__ mul, const float * __restrict__ p_w_h,
  const float * __restrict__ p_b_h, const float * __restrict__ p_w1,
  const float * __restrict__ p_b1, const float * __restrict__ p_w2,
  const float * __restrict__ p_b2, const float * __restrict__ p_emb,
  const int32_t * __restrict__ ray_img, const uint32_t * __restrict__ bits, int G,
  const float * __restrict__ bg, float * __restrict__ colors, float * __restrict__ depths,
  float * __restrict__ last_trans, int32_t * __restrict__ kept, int32_t * __restrict__ len,
  int n_rays, int S, float step, uint32_t T, int64_t level_stride, float t_thresh,
  float density_shift, float t_shift)
{
  using R = RShape<C>;
  using FS = typename R::FS;
  constexpr int L = C / F, kS1 = FS::kS1, kPitch = R::kPitch;
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
                        density_shift,   t_shift};
  const RayResume whole = {0, {0.f, 0.f, 0.f, 0.f}, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0, 0};
  __half * tile = reinterpret_cast<__half *>(lds_all + FS::kWFloats + wave * R::kWaveFloats);
  float * OUT = lds_all + FS::kWFloats + wave * R::kWaveFloats + R::kTileFloats;

  for (int r = (int)blockIdx.x * R::kWaves + wave; r < n_rays; r += (int)gridDim.x * R::kWaves)
    render_one_ray<C, F, POW2>(a, r, whole, lds_w, tile, OUT, lane, has_emb, has_grid, bias0);
}

inline bool is_pow2(uint32_t v) { return v && !(v & (v - 1u)); }

}  // namespace

extern "C" int f2n_render_rays(
  const float * rays_o, const float * rays_d, const float * noise, const uint16_t * table,
  const int32_t * primes, const float * bias, const float * mul, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, const int32_t * ray_img, const uint32_t * occ_bits, int G, const float * bg,
  float * colors, float * depths, float * last_trans, int32_t * kept, int32_t * len, int n_rays,
  int S, float step, int L, int F, uint32_t T, int64_t level_stride, float t_thresh,
  float density_shift, float t_shift, void * stream)
{
  if (n_rays < 0 || S < 1 || L < 1 || T < 1 || level_stride < 0) return F2N_E_INVALID_ARG;
  if (F != 1 && F != 2 && F != 4 && F != 8) return F2N_E_UNSUPPORTED;
  const int64_t C = (int64_t)L * F;
  if (C != 8 && C != 16 && C != 32 && C != 64) return F2N_E_UNSUPPORTED;
  if (L > F2N_MAX_LEVELS) return F2N_E_UNSUPPORTED;  // (C = 64 at F = 1)
  if (level_stride % F) return F2N_E_INVALID_ARG;
  if (occ_bits && !f2n_occ_res_ok(G)) return F2N_E_INVALID_ARG;
  if ((app_emb == nullptr) != (ray_img == nullptr)) return F2N_E_INVALID_ARG;
  if (n_rays == 0) return F2N_OK;
  if (!rays_o || !rays_d || !table || !primes || !bias || !mul || !w_h || !b_h || !w1 || !b1 ||
      !w2 || !b2 || !bg || !colors || !depths || !last_trans || !kept)
    return F2N_E_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(table) % (2u * F)) return F2N_E_INVALID_ARG;
  // the embedding rows are read as float4
  if (app_emb && (reinterpret_cast<uintptr_t>(app_emb) & 15u)) return F2N_E_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const bool p2 = is_pow2(T);
  // persistent workgroups: the weight operands are staged once per workgroup, not once per 8 rays
#define F2N_RENDER(CC, FF, P2)                                                                     \
  {                                                                                                \
    using R = RShape<CC>;                                                                          \
    const unsigned grid = std::min<unsigned>(f2n_div_up(n_rays, R::kWaves), 512u);                 \
    hipLaunchKernelGGL(                                                                            \
      (render_rays_kernel<CC, FF, P2>), dim3(grid), dim3(R::kWaves * 64), 0, s, rays_o, rays_d,    \
      noise, table, primes, bias, mul, w_h, b_h, w1, b1, w2, b2, app_emb, ray_img, occ_bits, G,    \
      bg, colors, depths, last_trans, kept, len, n_rays, S, step, T, level_stride, t_thresh,       \
      density_shift, t_shift);                                                                     \
  }
#define F2N_RENDER_F(CC, FF)       \
  if (p2) F2N_RENDER(CC, FF, true) \
  else F2N_RENDER(CC, FF, false)
#define F2N_RENDER_C(CC, CASE_F1)                      \
  switch (F) {                                         \
    CASE_F1                                            \
    case 2: F2N_RENDER_F(CC, 2) break;                 \
    case 4: F2N_RENDER_F(CC, 4) break;                 \
    default: F2N_RENDER_F(CC, 8) break;                \
  }
#define F2N_RENDER_F1(CC) case 1: F2N_RENDER_F(CC, 1) break;
  switch ((int)C) {
    case 8: F2N_RENDER_C(8, F2N_RENDER_F1(8)) break;
    case 16: F2N_RENDER_C(16, F2N_RENDER_F1(16)) break;
    case 32: F2N_RENDER_C(32, F2N_RENDER_F1(32)) break;
    default: F2N_RENDER_C(64, ) break;  // (F = 1 would be 64 levels: refused above)
  }
#undef F2N_RENDER_F1
#undef F2N_RENDER_C
#undef F2N_RENDER_F
#undef F2N_RENDER
  return f2n_launch_status();
}
