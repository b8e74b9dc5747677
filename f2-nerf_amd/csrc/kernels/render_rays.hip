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
#include "occupancy.hiph"
#include "sampler.hiph"
#include "sh_basis.hiph"
#include "shade_fwd_mfma.hiph"

#include <algorithm>

namespace
{

template <int C>
struct RShape
{
  using FS = FShape<C, 8>;
  static constexpr int kWaves = 8;  // rays in flight per workgroup; two workgroups per CU at C <= 32
  // f16 tile [C][kPitch] per wave.  The Q-layout read takes, per quarter q, 16 consecutive halves
  // (8 banks) of row q * C/4 + t: the quarters' rows must start 8 or more banks apart.  Row pitch in
  // 32-bit words x C/4 rows, mod 64 banks: C = 8: 36 x 2 = 8; C = 16: 34 x 4 = 8; C = 32: 34 x 8 = 16;
  // C = 64: 33 x 16 = 16 -- conflict-free everywhere (34 words would be 2-way at C = 64).
  static constexpr int kPitch = (C == 8) ? 72 : (C == 64) ? 66 : 68;
  static constexpr int kTileFloats = C * kPitch / 2;
  static constexpr int kOutFloats = 4 * 64;  // [logit, r, g, b][sample] on the way back to lane = sample
  static constexpr int kWaveFloats = kTileFloats + kOutFloats;
  static constexpr int kLdsFloats = FS::kWFloats + kWaves * kWaveFloats;
  static_assert(kLdsFloats * 4 <= 80 * 1024 || C == 64, "two workgroups per CU");
  static_assert(kLdsFloats * 4 <= 160 * 1024, "LDS budget");
};

// round_f16 that also hands out the f16 itself (the value parked in the tile)
__device__ __forceinline__ float round_f16_keep(float v, __half & h)
{
  asm volatile("" : "+v"(v));  // (see round_f16: no v_fma_mixlo_f16)
  h = __float2half_rn(v);
  return __half2float(h);
}

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
  const int q = lane >> 4, m = lane & 15;
  __half * tile = reinterpret_cast<__half *>(lds_all + FS::kWFloats + wave * R::kWaveFloats);
  float * OUT = lds_all + FS::kWFloats + wave * R::kWaveFloats + R::kTileFloats;
  const float * wop = lds_w + lane;
  const bool has_emb = (p_emb != nullptr) && (ray_img != nullptr);
  const bool has_grid = bits != nullptr;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const float bias0 = p_b_h[0];

  for (int r = (int)blockIdx.x * R::kWaves + wave; r < n_rays; r += (int)gridDim.x * R::kWaves) {
    const RayFrame rf = load_ray(rays_o, rays_d, r);
    const float * nrow = noise ? noise + (int64_t)r * S : nullptr;

    // ---- once per ray: the embedding row and c = b1 + w1[:, 16:32] . SH(dir), the same in every
    // column (shade_fwd_mfma_body<.., RAYS>: once per stride there)
    f32x4 e4 = zero4;
    if (has_emb) e4 = *reinterpret_cast<const f32x4 *>(p_emb + (int64_t)ray_img[r] * kOut1 + 4 * q);
    f32x4 cM[4];
    {
      float sh[16], shq[4];
      sh_basis<4>(rf.dx, rf.dy, rf.dz, sh);
#pragma unroll
      for (int t = 0; t < 4; t++) shq[t] = pick4(q, sh[t], sh[4 + t], sh[8 + t], sh[12 + t]);
#pragma unroll
      for (int M = 0; M < 4; M++) {
        f32x4 c = *reinterpret_cast<const f32x4 *>(lds_w + FS::oB1 + 16 * M + 4 * q);
#pragma unroll
        for (int t = 4; t < 8; t++) c = mfma16(wop[(FS::oWA2 + M * 8 + t) * 64], shq[t - 4], c);
        cM[M] = c;
      }
    }

    StrideCarry carry = {0.f, 0.f, 0.f, 0.f};
    float depth_carry = 0.f;  // the march's optical depth (chain logit): decides which samples exist
    float comp_carry = 0.f;   // the compositing optical depth (head logit) over the kept samples
    float cr = 0.f, cg = 0.f, cb = 0.f, cd = 0.f;
    int n_kept = 0, n_len = 0;
    for (int k0 = 0; k0 < S; k0 += F2N_WAVE) {
      // ---- 1. sample and test
      const StrideSample sm = make_stride(rf, nrow, k0, S, step, carry, lane);
      float x = sm.px, y = sm.py, z = sm.pz;
      contract_point(x, y, z);
      const bool occ = sm.valid && (!has_grid || occ_test_contracted(x, y, z, bits, G));
      const unsigned long long om = __ballot(occ);
      // ---- 2. encode: the march's chain, and the values parked for the network
      float sec = 0.f;
      if (om != 0ull) {  // (wave-uniform: an empty stride costs no gathers at all)
        if (occ) {       // (no cross-lane move inside: the scans below run with every lane on)
          float logit = bias0;
#pragma unroll 1
          for (int l = 0; l < L; l++) {
            const LevelParams lp = load_level(primes, bias, mul, l);
            uint32_t row[8];
            float w[8], acc[F];
            corner_rows_and_weights<POW2>(x, y, z, lp, T, row, w);
            gather_blend<F>(table + level_stride * l, row, w, acc);
#pragma unroll
            for (int k = 0; k < F; k++) {
              __half hv;
              logit = fmaf(round_f16_keep(acc[k], hv), p_w_h[l * F + k], logit);
              tile[(l * F + k) * kPitch + lane] = hv;
            }
          }
          const float sigma = expf(logit - density_shift);
          sec = sigma * sm.dt;
        }
      }
      // ---- 3. the keep decision, exactly the march's
      const float incl = wave_incl_scan(sec);
      const float depth = depth_carry + wave_shift_up1(incl, 0.f);
      const float trans_c = expf(-depth);
      const bool keep = sm.valid && (trans_c > t_thresh);
      const unsigned long long km = __ballot(keep);
      n_len += __popcll(km);
      n_kept += __popcll(km & om);
      const bool use = keep && occ;  // this lane's sample is one of the ray's list
      const bool last = __popcll(km) < min(F2N_WAVE, S - k0);  // the mask is a prefix

      if ((km & om) != 0ull) {  // (wave-uniform)
        // ---- 4. the network on the stride, Q-layout.  Columns of lanes that did not gather hold
        // whatever the tile held: a column never leaves its own sample, and `use` drops it below.
        wave_lds_sync();
        f32x4 h[4];
#pragma unroll
        for (int TT = 0; TT < 4; TT++) h[TT] = *reinterpret_cast<const f32x4 *>(lds_w + FS::oBh + 4 * q);
#pragma unroll
        for (int t = 0; t < kS1; t++) {
          const float a = wop[(FS::oWA1 + t) * 64];
#pragma unroll
          for (int TT = 0; TT < 4; TT++)
            h[TT] = mfma16(a, __half2float(tile[(q * kS1 + t) * kPitch + 16 * TT + m]), h[TT]);
        }
        if (q == 0) {
#pragma unroll
          for (int TT = 0; TT < 4; TT++) OUT[16 * TT + m] = h[TT][0];
        }
        f32x4 Xh[4];
#pragma unroll
        for (int TT = 0; TT < 4; TT++) {
          Xh[TT] = h[TT];
          if (q == 0) Xh[TT][0] = 1.f;
          if (has_emb) Xh[TT] += e4;
        }
        f32x4 o[4];
#pragma unroll
        for (int TT = 0; TT < 4; TT++) {
          o[TT] = zero4;
          o[TT][0] = lds_w[FS::oB2 + q];
        }
#pragma unroll
        for (int M = 0; M < 4; M++) {
          f32x4 pre[4];
#pragma unroll
          for (int TT = 0; TT < 4; TT++) pre[TT] = cM[M];
#pragma unroll
          for (int t = 0; t < 4; t++) {
            const float a = wop[(FS::oWA2 + M * 8 + t) * 64];
#pragma unroll
            for (int TT = 0; TT < 4; TT++) pre[TT] = mfma16(a, Xh[TT][t], pre[TT]);
          }
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const float a = wop[(FS::oWA3 + M * 4 + rr) * 64];
#pragma unroll
            for (int TT = 0; TT < 4; TT++) o[TT] = mfma16(a, relu(pre[TT][rr]), o[TT]);
          }
        }
        if (q < 3) {  // output rows 0, 4, 8 = the colours, in lanes of quarters 0, 1, 2
#pragma unroll
          for (int TT = 0; TT < 4; TT++) OUT[(1 + q) * 64 + 16 * TT + m] = o[TT][0];
        }
        wave_lds_sync();
        // ---- 5. composite_fwd_kernel's stride, lane = sample
        const float hl = OUT[lane];
        const float o0 = OUT[64 + lane], o1 = OUT[128 + lane], o2 = OUT[192 + lane];
        wave_lds_sync();  // (the next stride's tile and OUT writes stay behind these reads)
        float sec2 = 0.f;
        if (use) sec2 = expf(hl - density_shift) * sm.dt;
        const float incl2 = wave_incl_scan(sec2);
        const float trans = expf(-(comp_carry + wave_shift_up1(incl2, 0.f)));
        if (use) {
          const float alpha = 1.f - expf(-sec2);
          const float w = trans * alpha;
          cr = fmaf(w, (1.f + 2.f * kEps) / (1.f + expf(-o0)) - kEps, cr);
          cg = fmaf(w, (1.f + 2.f * kEps) / (1.f + expf(-o1)) - kEps, cg);
          cb = fmaf(w, (1.f + 2.f * kEps) / (1.f + expf(-o2)) - kEps, cb);
          cd = fmaf(w, sm.t + t_shift, cd);
        }
        comp_carry += wave_bcast_last(incl2);
      }
      if (last) break;  // nothing later survives
      depth_carry += wave_bcast_last(incl);
    }
    // ---- 6. the ray's sums
    cr = wave_sum(cr);
    cg = wave_sum(cg);
    cb = wave_sum(cb);
    cd = wave_sum(cd);
    if (lane == 0) {
      const float tl = expf(-comp_carry);
      last_trans[r] = tl;
      colors[3 * r] = fmaf(tl, bg[3 * r], cr);
      colors[3 * r + 1] = fmaf(tl, bg[3 * r + 1], cg);
      colors[3 * r + 2] = fmaf(tl, bg[3 * r + 2], cb);
      depths[r] = cd / (1.f - tl + 1e-4f);
      kept[r] = n_kept;
      if (len) len[r] = n_len;
    }
  }
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
