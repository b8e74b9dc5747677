// render_rays_head.hip -- the one-pass render where rays are SHORT: eight rays to a wavefront.
//
// render_rays_kernel (render_rays.hip) gives one wavefront to one ray and walks it 64 samples at a
// time: a ray that keeps three samples still pays a 64-sample stride and a full pass of the network
// (an 800 x 800 view keeping 3.1 samples per ray: 16x the default route).  Here the HEAD of every ray
// -- its first n_head samples -- is walked with the eight-ray march's mapping (RayLanes<8>,
// sampler.hiph): a ray owns half a DPP row, g = lane >> 3 is the ray of the wave, m = lane & 7 the
// sample of an 8-sample stride.  Replaces the same reference sites as f2n_render_rays:
// Renderer::render (src/renderer.cpp:33-123) as render_all_rays (:125-151) and
// Localizer::evaluate_poses (src/localizer.cpp:172) use it.
//
//   f2n_render_rays_head  per 8-sample stride of 8 rays: sample, contract, occupancy bit, the level
//     loop with the march's chain logit (density_chain) and the f16 tile (column = lane), the
//     march's keep decision (keep_step, sampler.hiph: the 64-lane scan's additions, so kept / len
//     are the march's bit for bit), then -- if any of the 64 columns is a kept, occupied sample --
//     the network on the 64 columns and the compositing sums inside each 8-lane group.  Column c
//     belongs to ray c >> 3 for the whole life of the wave: SH16(dir) and the embedding row of the 8
//     rays sit in a small LDS block per wave, written once per ray group.  b1 + W1[:, 16:32] . SH is
//     RECOMPUTED per stride (4 more matrix instructions per 16 x 16 block, in the one-ray form's
//     order: the same bits per column): held per column it would be 64 registers and cost the
//     register class.  A ray that ends inside the head gets its outputs here; one that is still
//     alive at k0 == n_head leaves its state (below) and a pending flag.
//   f2n_render_rays_tail  render_one_ray (render_rays.hiph), resumed from that state at k0 = n_head
//     for the pending rays; the others are skipped on a scalar flag load.
//
// n_head is a multiple of 64 or >= S: the 64-lane scan's block boundary is where the half-row form's
// carries ARE the one-ray form's (carry + ((T3 + T2) + (T1 + T0))).
//
// State, 16 words (64 bytes) per ray, written by the head only when n_head < S:
//   [0] int32 pending (1: resume at n_head, 0: the ray's outputs are final)
//   [1] cumulative noise   [2..4] last sample point   [5] chain optical depth (the march's)
//   [6] compositing optical depth   [7..10] the partial sums r, g, b, depth (reduced over the group)
//   [11] int32 n_kept   [12] int32 n_len   [13..15] unused
// A ray that is not pending has only word 0 written.
//
// No atomics, no workspace but the state: two launches give the same bits.
#include "render_rays.hiph"

#include <algorithm>

namespace
{

constexpr int kStateWords = 16;

template <int C>
struct HShape
{
  using R = RShape<C>;
  using FS = typename R::FS;
  // ~150 registers (the half-row scans' state on top of the network's; capped at 128 the kernel
  // spills): three waves per SIMD, so ONE workgroup of 12 waves per CU rather than two of 8
  static constexpr int kWaves = 12;
  static constexpr int kRayFloats = 2 * 8 * 16;  // SH16(dir) and the embedding row of the wave's 8 rays
  static constexpr int kWaveFloats = R::kWaveFloats + kRayFloats;
  static constexpr int kLdsFloats = FS::kWFloats + kWaves * kWaveFloats;
  static_assert(kLdsFloats * 4 <= 160 * 1024, "LDS budget");
};

// inclusive scan inside the own 8-lane group, in lane order (every move by all lanes, then selected)
__device__ __forceinline__ float group_incl_scan(float v, int m)
{
  const float s1 = dpp_get<0x111, 0xf, 0xf>(v, 0.f);
  v += (m >= 1 ? s1 : 0.f);
  const float s2 = dpp_get<0x112, 0xf, 0xf>(v, 0.f);
  v += (m >= 2 ? s2 : 0.f);
  const float s4 = dpp_get<0x114, 0xf, 0xf>(v, 0.f);
  v += (m >= 4 ? s4 : 0.f);
  return v;
}

__device__ __forceinline__ float group_sum(float v, int m, int lane)
{
  return RayLanes<8>::last(group_incl_scan(v, m), lane);
}

template <int C, int F, bool POW2>
__global__ __launch_bounds__(HShape<C>::kWaves * 64) void render_rays_head_kernel(
  F2N_RENDER_PARAMS, float * __restrict__ state, int n_head, int corner_order,
  int L_active)
{
  using H = HShape<C>;
  using R = RShape<C>;
  using FS = typename R::FS;
  using RL = RayLanes<8>;
  constexpr int kS1 = FS::kS1, kPitch = R::kPitch;
  __shared__ __attribute__((aligned(16))) float lds_all[H::kLdsFloats];
  float * lds_w = lds_all;
  stage_fwd_weights<C, H::kWaves>(lds_w, p_w_h, p_b_h, p_w1, p_b1, p_w2, p_b2);
  __syncthreads();

  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int q = lane >> 4, mq = lane & 15;  // the matrix layout: quarter, column of a 16-wide block
  const int g = lane >> 3, m = lane & 7;    // the march's: ray of the wave, sample of the stride
  float * wave_lds = lds_all + FS::kWFloats + wave * H::kWaveFloats;
  __half * tile = reinterpret_cast<__half *>(wave_lds);
  float * OUT = wave_lds + R::kTileFloats;
  float * SHT = OUT + R::kOutFloats;  // [8 rays][16]
  float * EMB = SHT + 8 * 16;         // [8 rays][16]
  const float * wop = lds_w + lane;
  const bool has_emb = (p_emb != nullptr) && (ray_img != nullptr);
  const bool has_grid = bits != nullptr;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const float bias0 = p_b_h[0];
  const bool hand_over = n_head < S;  // (then n_head is a multiple of 64)
  const int k_end = hand_over ? n_head : S;
  const int n_groups = (n_rays + 7) >> 3;
  zero_tile_tail<C, F>(tile, L_active, lane);

  for (int w8 = (int)blockIdx.x * H::kWaves + wave; w8 < n_groups; w8 += (int)gridDim.x * H::kWaves) {
    const int r_raw = (w8 << 3) + g;
    const bool has_ray = r_raw < n_rays;
    const int r = has_ray ? r_raw : n_rays - 1;  // (spare groups of the last wave: idle)
    const RayFrame rf = load_ray(rays_o, rays_d, r);
    const float * nrow = noise ? noise + (int64_t)r * S : nullptr;

    // ---- once per ray group: SH16(dir) and the embedding row of the 8 rays, for the columns to read
    wave_lds_sync();  // (the previous group's last reads stay in front)
    {
      float sh[16];
      sh_basis<4>(rf.dx, rf.dy, rf.dz, sh);
      if (m == 0) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
          const f32x4 v = {sh[4 * t], sh[4 * t + 1], sh[4 * t + 2], sh[4 * t + 3]};
          *reinterpret_cast<f32x4 *>(SHT + g * 16 + 4 * t) = v;
        }
      }
      if (has_emb && m < 4)
        *reinterpret_cast<f32x4 *>(EMB + g * 16 + 4 * m) =
          *reinterpret_cast<const f32x4 *>(p_emb + (int64_t)ray_img[r] * kOut1 + 4 * m);
    }
    wave_lds_sync();

    StrideState<8> carry = {};
    DepthState<8> ds = {};
    float comp_carry = 0.f;              // the compositing optical depth (head logit), per ray
    float cr = 0.f, cg = 0.f, cb = 0.f, cd = 0.f;
    int n_kept = 0, n_len = 0;
    bool done = !has_ray;
    for (int k0 = 0; k0 < k_end; k0 += 8) {
      // ---- 1. sample and test
      const StrideSample sm = make_stride(rf, nrow, k0, S, step, carry, lane);
      float x = sm.px, y = sm.py, z = sm.pz;
      contract_point(x, y, z);
      // finished, absent and unoccupied samples do not gather
      const bool occ = sm.valid && !done && (!has_grid || occ_test_contracted(x, y, z, bits, G));
      const unsigned long long om = __ballot(occ);
      // ---- 2. encode: the march's chain, and the values parked for the network
      float sec = 0.f;
      if (om != 0ull) {  // (wave-uniform)
        if (occ) {       // (no cross-lane move inside)
          const float logit = density_chain<F, POW2>(
            x, y, z, table, primes, bias, mul, p_w_h, bias0, L_active, T, level_stride, corner_order,
            [&](int c, __half hv) { tile[c * kPitch + lane] = hv; });
          const float sigma = expf(logit - density_shift);
          sec = sigma * sm.dt;
        }
      }
      // ---- 3. the keep decision, the march's (unoccupied lanes feed 0.f, outside any branch)
      const KeepStep ks = keep_step(sec, sm.valid && !done, k0, S, t_thresh, ds, lane);
      const unsigned long long km = ks.mask;
      const bool use = ks.keep && occ;  // this lane's sample is one of its ray's list
      if (!done) {
        n_len += ks.n;
        n_kept += RL::count(km & om, lane);
        done = ks.ends;  // nothing later survives
      }

      if ((km & om) != 0ull) {  // (wave-uniform)
        // ---- 4. the network on the 64 columns, Q-layout.  A column that did not gather holds
        // whatever the tile held: it never leaves its own lane, and `use` drops it below.
        wave_lds_sync();
        f32x4 hh[4];
#pragma unroll
        for (int TT = 0; TT < 4; TT++) hh[TT] = *reinterpret_cast<const f32x4 *>(lds_w + FS::oBh + 4 * q);
#pragma unroll
        for (int t = 0; t < kS1; t++) {
          const float a = wop[(FS::oWA1 + t) * 64];
#pragma unroll
          for (int TT = 0; TT < 4; TT++)
            hh[TT] = mfma16(a, __half2float(tile[(q * kS1 + t) * kPitch + 16 * TT + mq]), hh[TT]);
        }
        if (q == 0) {
#pragma unroll
          for (int TT = 0; TT < 4; TT++) OUT[16 * TT + mq] = hh[TT][0];
        }
        // column 16 TT + mq is ray 2 TT + (mq >> 3) of the wave
        f32x4 Xh[4], shv[4];
#pragma unroll
        for (int TT = 0; TT < 4; TT++) {
          const int cray = 2 * TT + (mq >> 3);
          shv[TT] = *reinterpret_cast<const f32x4 *>(SHT + cray * 16 + 4 * q);
          Xh[TT] = hh[TT];
          if (q == 0) Xh[TT][0] = 1.f;
          if (has_emb) Xh[TT] += *reinterpret_cast<const f32x4 *>(EMB + cray * 16 + 4 * q);
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
          const f32x4 b1v = *reinterpret_cast<const f32x4 *>(lds_w + FS::oB1 + 16 * M + 4 * q);
#pragma unroll
          for (int TT = 0; TT < 4; TT++) pre[TT] = b1v;
          // b1 + w1[:, 16:32] . SH(dir of the column's ray) first, as the one-ray form sums it
#pragma unroll
          for (int t = 4; t < 8; t++) {
            const float a = wop[(FS::oWA2 + M * 8 + t) * 64];
#pragma unroll
            for (int TT = 0; TT < 4; TT++) pre[TT] = mfma16(a, shv[TT][t - 4], pre[TT]);
          }
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
          for (int TT = 0; TT < 4; TT++) OUT[(1 + q) * 64 + 16 * TT + mq] = o[TT][0];
        }
        wave_lds_sync();
        // ---- 5. compositing, per ray inside its 8-lane group
        const float hl = OUT[lane];
        const float o0 = OUT[64 + lane], o1 = OUT[128 + lane], o2 = OUT[192 + lane];
        wave_lds_sync();  // (the next stride's tile and OUT writes stay behind these reads)
        float sec2 = 0.f;
        if (use) sec2 = expf(hl - density_shift) * sm.dt;
        const float incl2 = group_incl_scan(sec2, m);
        const float trans = expf(-(comp_carry + RL::prev(incl2, 0.f, lane)));
        if (use) {
          const float alpha = 1.f - expf(-sec2);
          const float w = trans * alpha;
          cr = fmaf(w, (1.f + 2.f * kEps) / (1.f + expf(-o0)) - kEps, cr);
          cg = fmaf(w, (1.f + 2.f * kEps) / (1.f + expf(-o1)) - kEps, cg);
          cb = fmaf(w, (1.f + 2.f * kEps) / (1.f + expf(-o2)) - kEps, cb);
          cd = fmaf(w, sm.t + t_shift, cd);
        }
        comp_carry += RL::last(incl2, lane);
      }
      if (__ballot(!done) == 0ull) break;
    }
    // ---- 6. per ray: its outputs, or the state the tail resumes from
    cr = group_sum(cr, m, lane);
    cg = group_sum(cg, m, lane);
    cb = group_sum(cb, m, lane);
    cd = group_sum(cd, m, lane);
    if (has_ray && m == 0) {
      const bool pending = hand_over && !done;
      if (!pending) {
        const float tl = expf(-comp_carry);
        last_trans[r] = tl;
        colors[3 * r] = fmaf(tl, bg[3 * r], cr);
        colors[3 * r + 1] = fmaf(tl, bg[3 * r + 1], cg);
        colors[3 * r + 2] = fmaf(tl, bg[3 * r + 2], cb);
        depths[r] = cd / (1.f - tl + 1e-4f);
        kept[r] = n_kept;
        if (len) len[r] = n_len;
        if (hand_over) state[(int64_t)r * kStateWords] = __int_as_float(0);
      } else {
        f32x4 * st = reinterpret_cast<f32x4 *>(state + (int64_t)r * kStateWords);
        const f32x4 s0 = {__int_as_float(1), carry.noise, carry.lx, carry.ly};
        const f32x4 s1 = {carry.lz, ds.carry, comp_carry, cr};
        const f32x4 s2 = {cg, cb, cd, __int_as_float(n_kept)};
        const f32x4 s3 = {__int_as_float(n_len), 0.f, 0.f, 0.f};
        st[0] = s0;
        st[1] = s1;
        st[2] = s2;
        st[3] = s3;
      }
    }
  }
}

template <int C, int F, bool POW2>
__global__ __launch_bounds__(RShape<C>::kWaves * 64) void render_rays_tail_kernel(
  F2N_RENDER_PARAMS, const float * __restrict__ state, int n_head, int corner_order,
  int L_active)
{
  using R = RShape<C>;
  using FS = typename R::FS;
  __shared__ __attribute__((aligned(16))) float lds_all[R::kLdsFloats];
  float * lds_w = lds_all;
  stage_fwd_weights<C, R::kWaves>(lds_w, p_w_h, p_b_h, p_w1, p_b1, p_w2, p_b2);
  __syncthreads();

  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool has_emb = (p_emb != nullptr) && (ray_img != nullptr);
  const bool has_grid = bits != nullptr;
  const float bias0 = p_b_h[0];
  const RenderArgs a = {rays_o, rays_d, noise,      table, primes,     bias,  mul, p_w_h,
                        p_emb,  ray_img, bits,      G,     bg,         colors, depths, last_trans,
                        kept,   len,     S,         step,  T,          level_stride, t_thresh,
                        density_shift,   t_shift, corner_order, L_active};
  __half * tile = reinterpret_cast<__half *>(lds_all + FS::kWFloats + wave * R::kWaveFloats);
  float * OUT = lds_all + FS::kWFloats + wave * R::kWaveFloats + R::kTileFloats;
  zero_tile_tail<C, F>(tile, L_active, lane);

  for (int r = (int)blockIdx.x * R::kWaves + wave; r < n_rays; r += (int)gridDim.x * R::kWaves) {
    // (r lives in scalar registers: the state is fetched with scalar loads, the skip is wave-uniform)
    const float * st = state + (int64_t)r * kStateWords;
    if (__float_as_int(st[0]) == 0) continue;
    const RayResume rs = {n_head, {st[1], st[2], st[3], st[4]}, st[5], st[6], st[7], st[8], st[9],
                          st[10], __float_as_int(st[11]), __float_as_int(st[12])};
    render_one_ray<C, F, POW2>(a, r, rs, lds_w, tile, OUT, lane, has_emb, has_grid, bias0);
  }
}

}  // namespace

extern "C" int64_t f2n_render_rays_state_bytes(int n_rays)
{
  return n_rays < 0 ? -1 : (int64_t)n_rays * kStateWords * 4;
}

extern "C" int f2n_render_rays_head_lod(
  const float * rays_o, const float * rays_d, const float * noise, const uint16_t * table,
  const int32_t * primes, const float * bias, const float * mul, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, const int32_t * ray_img, const uint32_t * occ_bits, int G, const float * bg,
  float * colors, float * depths, float * last_trans, int32_t * kept, int32_t * len, int n_rays,
  int S, float step, int L, int L_active, int F, uint32_t T, int64_t level_stride, float t_thresh,
  float density_shift, float t_shift, int n_head, void * state, void * stream)
{
  bool launch;
  const int st = render_args_status(F2N_RENDER_KARGS, L, F, L_active, n_head, state, &launch);
  if (st != F2N_OK || !launch) return st;
  hipStream_t s = (hipStream_t)stream;
  // persistent workgroups, 12 waves of 8 rays each, one per CU
  f2n_dispatch_width_field(L, F, T, [&](auto cc, auto ff, auto p2) {
    using H = HShape<decltype(cc)::value>;
    const unsigned grid = std::min<unsigned>(f2n_div_up(f2n_div_up(n_rays, 8), H::kWaves), 256u);
    hipLaunchKernelGGL(
      (render_rays_head_kernel<decltype(cc)::value, decltype(ff)::value, decltype(p2)::value>),
      dim3(grid), dim3(H::kWaves * 64), 0, s, F2N_RENDER_KARGS, static_cast<float *>(state),
      n_head, f2n_get_option(F2N_OPT_GATHER_PAIRED), L_active);
  });
  return f2n_launch_status();
}

extern "C" int f2n_render_rays_tail_lod(
  const float * rays_o, const float * rays_d, const float * noise, const uint16_t * table,
  const int32_t * primes, const float * bias, const float * mul, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, const int32_t * ray_img, const uint32_t * occ_bits, int G, const float * bg,
  float * colors, float * depths, float * last_trans, int32_t * kept, int32_t * len, int n_rays,
  int S, float step, int L, int L_active, int F, uint32_t T, int64_t level_stride, float t_thresh,
  float density_shift, float t_shift, int n_head, const void * state, void * stream)
{
  bool launch;
  const int st = render_args_status(F2N_RENDER_KARGS, L, F, L_active, n_head, state, &launch);
  if (st != F2N_OK || !launch) return st;
  if (n_head >= S) return F2N_OK;  // the head rendered every ray whole: nothing is pending
  hipStream_t s = (hipStream_t)stream;
  f2n_dispatch_width_field(L, F, T, [&](auto cc, auto ff, auto p2) {
    using R = RShape<decltype(cc)::value>;
    const unsigned grid = std::min<unsigned>(f2n_div_up(n_rays, R::kWaves), 512u);
    hipLaunchKernelGGL(
      (render_rays_tail_kernel<decltype(cc)::value, decltype(ff)::value, decltype(p2)::value>),
      dim3(grid), dim3(R::kWaves * 64), 0, s, F2N_RENDER_KARGS, static_cast<const float *>(state),
      n_head, f2n_get_option(F2N_OPT_GATHER_PAIRED), L_active);
  });
  return f2n_launch_status();
}

extern "C" int f2n_render_rays_head(
  const float * rays_o, const float * rays_d, const float * noise, const uint16_t * table,
  const int32_t * primes, const float * bias, const float * mul, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, const int32_t * ray_img, const uint32_t * occ_bits, int G, const float * bg,
  float * colors, float * depths, float * last_trans, int32_t * kept, int32_t * len, int n_rays,
  int S, float step, int L, int F, uint32_t T, int64_t level_stride, float t_thresh,
  float density_shift, float t_shift, int n_head, void * state, void * stream)
{
  return f2n_render_rays_head_lod(
    rays_o, rays_d, noise, table, primes, bias, mul, w_h, b_h, w1, b1, w2, b2, app_emb, ray_img,
    occ_bits, G, bg, colors, depths, last_trans, kept, len, n_rays, S, step, L, L, F, T, level_stride,
    t_thresh, density_shift, t_shift, n_head, state, stream);
}

extern "C" int f2n_render_rays_tail(
  const float * rays_o, const float * rays_d, const float * noise, const uint16_t * table,
  const int32_t * primes, const float * bias, const float * mul, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, const int32_t * ray_img, const uint32_t * occ_bits, int G, const float * bg,
  float * colors, float * depths, float * last_trans, int32_t * kept, int32_t * len, int n_rays,
  int S, float step, int L, int F, uint32_t T, int64_t level_stride, float t_thresh,
  float density_shift, float t_shift, int n_head, const void * state, void * stream)
{
  return f2n_render_rays_tail_lod(
    rays_o, rays_d, noise, table, primes, bias, mul, w_h, b_h, w1, b1, w2, b2, app_emb, ray_img,
    occ_bits, G, bg, colors, depths, last_trans, kept, len, n_rays, S, step, L, L, F, T, level_stride,
    t_thresh, density_shift, t_shift, n_head, state, stream);
}
