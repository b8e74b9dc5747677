// sampler.hip -- ray sampling, the fused early-termination march and sample compaction
// (SURVEY.md rows A4, A5).
//
// Replaces PtsSampler::get_samples (about 20 ATen launches, reference src/points_sampler.cpp:20-64)
// and the early-stop block of Renderer::render (src/renderer.cpp:58-90), which in the reference
// evaluates the whole field on all n_rays*S samples only to build a keep-mask and then runs
// where() + four index() gathers.
//
// Mapping: one 64-lane wavefront per ray, lanes = 64 consecutive samples (a "stride").  Cumulative
// step noise and the exclusive optical-depth scan are DPP wave scans with a scalar carry between
// strides; the keep-mask is a wave ballot; a ray whose transmittance has dropped to <= t_thresh
// stops issuing strides, so a terminated ray costs ceil(kept/64) strides, not S/64.
#include "hash_grid.hiph"
#include "occupancy.hiph"
#include "sampler.hiph"

namespace
{

__device__ __forceinline__ int ray_of_wave()
{
  return (int)blockIdx.x * F2N_WAVES_PER_BLOCK + (int)(threadIdx.x >> 6);
}

// sample i of the output arrays: what f2n_sample_rays and f2n_sample_compact[_occ] write per sample
__device__ __forceinline__ void store_sample(
  float * __restrict__ pts, float * __restrict__ dirs, float * __restrict__ dt,
  float * __restrict__ t, int64_t i, const RayFrame & rf, const StrideSample & sm)
{
  pts[3 * i] = sm.px;
  pts[3 * i + 1] = sm.py;
  pts[3 * i + 2] = sm.pz;
  dirs[3 * i] = rf.dx;
  dirs[3 * i + 1] = rf.dy;
  dirs[3 * i + 2] = rf.dz;
  dt[i] = sm.dt;
  t[i] = sm.t;
}

// ---- f2n_sample_rays ----------------------------------------------------------------------------

__global__ __launch_bounds__(F2N_BLOCK) void sample_rays_kernel(
  const float * __restrict__ rays_o, const float * __restrict__ rays_d,
  const float * __restrict__ noise, float * __restrict__ pts, float * __restrict__ dirs,
  float * __restrict__ dt, float * __restrict__ t, int32_t * __restrict__ bounds, int n_rays, int S,
  float step)
{
  const int r = ray_of_wave();
  if (r >= n_rays) return;
  const int lane = lane_id();
  const RayFrame rf = load_ray(rays_o, rays_d, r);
  const float * nrow = noise ? noise + (int64_t)r * S : nullptr;
  StrideCarry carry = {0.f, 0.f, 0.f, 0.f};
  const int64_t base = (int64_t)r * S;
  for (int k0 = 0; k0 < S; k0 += F2N_WAVE) {
    const StrideSample sm = make_stride(rf, nrow, k0, S, step, carry, lane);
    if (sm.valid) store_sample(pts, dirs, dt, t, base + k0 + lane, rf, sm);
  }
  if (lane == 0) {
    bounds[2 * r] = (int32_t)base;
    bounds[2 * r + 1] = (int32_t)(base + S);
  }
}

// ---- f2n_sample_dense ---------------------------------------------------------------------------
// sample_rays_kernel for a dense grid that goes straight to the encode: the contracted position is
// written instead of the world position (contract_point on the registers make_stride filled: what
// f2n_contract_fwd computes from the stored point), the direction once per ray instead of once per
// sample, and the noise row is read where it lies -- through `noise_row` when the rays were
// reordered, and as the raw uniform draw u when `affine` (the step multiplier (u - .5f) + 1.f, two
// f32 roundings as the two ATen passes of PtsSampler::draw_noise make them).
__global__ __launch_bounds__(F2N_BLOCK) void sample_dense_kernel(
  const float * __restrict__ rays_o, const float * __restrict__ rays_d,
  const float * __restrict__ noise, const int32_t * __restrict__ noise_row, int affine,
  float * __restrict__ x, float * __restrict__ dt, float * __restrict__ t,
  int32_t * __restrict__ bounds, float * __restrict__ ray_dirs, int n_rays, int S, float step)
{
  const int r = ray_of_wave();
  if (r >= n_rays) return;
  const int lane = lane_id();
  const RayFrame rf = load_ray(rays_o, rays_d, r);
  // (a map entry outside [0, n_rays) is clamped: no read leaves the noise array)
  const int nr = noise_row ? min(max(noise_row[r], 0), n_rays - 1) : r;
  const float * nrow = noise ? noise + (int64_t)nr * S : nullptr;
  StrideCarry carry = {0.f, 0.f, 0.f, 0.f};
  const int64_t base = (int64_t)r * S;
  for (int k0 = 0; k0 < S; k0 += F2N_WAVE) {
    float nz = 0.f;
    if (nrow && k0 + lane < S) {
      nz = nrow[k0 + lane];
      if (affine) nz = (nz - .5f) + 1.f;
    }
    const StrideSample sm = make_stride_from(rf, nrow != nullptr, nz, k0, S, step, carry, lane);
    if (sm.valid) {
      const int64_t i = base + k0 + lane;
      float cx = sm.px, cy = sm.py, cz = sm.pz;
      contract_point(cx, cy, cz);
      x[3 * i] = cx;
      x[3 * i + 1] = cy;
      x[3 * i + 2] = cz;
      dt[i] = sm.dt;
      t[i] = sm.t;
    }
  }
  if (lane == 0) {
    bounds[2 * r] = (int32_t)base;
    bounds[2 * r + 1] = (int32_t)(base + S);
    ray_dirs[3 * r] = rf.dx;
    ray_dirs[3 * r + 1] = rf.dy;
    ray_dirs[3 * r + 2] = rf.dz;
  }
}

// ---- f2n_sample_compact, f2n_sample_compact_occ -------------------------------------------------
// The kept samples of every ray, re-created where the compacted list wants them.  OCC: the ray list
// was thinned by the occupancy bitfield, the ray's samples are {k < len_r : occupied(p_k)} in order of
// k.  Walks the same strides as the march, tests the same bit on the same point, and writes sample k
// at start + rank (rank = occupied samples before it).  Without a grid the rank is k itself.
template <bool OCC>
__device__ __forceinline__ void sample_compact_rays(
  const float * __restrict__ rays_o, const float * __restrict__ rays_d,
  const float * __restrict__ noise, const int32_t * __restrict__ bounds,
  const int32_t * __restrict__ len, const uint32_t * __restrict__ bits, int G,
  float * __restrict__ pts, float * __restrict__ dirs, float * __restrict__ dt,
  float * __restrict__ t, int n_rays, int S, float step)
{
  const int r = ray_of_wave();
  if (r >= n_rays) return;
  const int lane = lane_id();
  const int start = bounds[2 * r];
  const int cnt = bounds[2 * r + 1] - start;
  const int n_len = OCC ? min(len[r], S) : cnt;
  if (cnt <= 0 || n_len <= 0) return;
  const RayFrame rf = load_ray(rays_o, rays_d, r);
  const float * nrow = noise ? noise + (int64_t)r * S : nullptr;
  StrideCarry carry = {0.f, 0.f, 0.f, 0.f};
  int base = 0;  // samples written by the earlier strides
  for (int k0 = 0; k0 < n_len && base < cnt; k0 += F2N_WAVE) {
    const StrideSample sm = make_stride(rf, nrow, k0, S, step, carry, lane);
    bool mine = k0 + lane < n_len;
    int rank = k0 + lane;
    if constexpr (OCC) {
      mine = mine && occ_test_point(sm.px, sm.py, sm.pz, bits, G);
      const unsigned long long m = __ballot(mine);
      rank = base + __popcll(m & ((1ull << lane) - 1ull));
      base += __popcll(m);
    } else {
      base += F2N_WAVE;
    }
    // (rank < cnt always when bounds and len come from the same grid)
    if (mine && rank < cnt) store_sample(pts, dirs, dt, t, (int64_t)start + rank, rf, sm);
  }
}

__global__ __launch_bounds__(F2N_BLOCK) void sample_compact_kernel(
  const float * __restrict__ rays_o, const float * __restrict__ rays_d,
  const float * __restrict__ noise, const int32_t * __restrict__ bounds, float * __restrict__ pts,
  float * __restrict__ dirs, float * __restrict__ dt, float * __restrict__ t, int n_rays, int S,
  float step)
{
  sample_compact_rays<false>(
    rays_o, rays_d, noise, bounds, nullptr, nullptr, 0, pts, dirs, dt, t, n_rays, S, step);
}

__global__ __launch_bounds__(F2N_BLOCK) void sample_compact_occ_kernel(
  const float * __restrict__ rays_o, const float * __restrict__ rays_d,
  const float * __restrict__ noise, const int32_t * __restrict__ bounds,
  const int32_t * __restrict__ len, const uint32_t * __restrict__ bits, int G,
  float * __restrict__ pts, float * __restrict__ dirs, float * __restrict__ dt,
  float * __restrict__ t, int n_rays, int S, float step)
{
  sample_compact_rays<true>(
    rays_o, rays_d, noise, bounds, len, bits, G, pts, dirs, dt, t, n_rays, S, step);
}

// ---- f2n_density_march, f2n_density_march_occ ---------------------------------------------------
// One body for every lane mapping (RayLanes<W>, sampler.hiph: W = 64, 16 or 8 lanes to a ray) and for
// the march with and without the occupancy grid.  Per stride: make_stride, contract_point, the density
// chain, keep_step.
//
// OCC: the density of every sample in an unoccupied cell is exactly zero.  The lane tests its bit
// before the level loop, a stride without an occupied sample skips the level loop as a whole
// (wave-uniform) and only advances make_stride's carries, and unoccupied lanes feed 0.f into the same
// scan -- the scan's additions stay those of the plain march, so an all-ones grid gives its counts
// bit for bit.  len[r] = leading samples with T above t_thresh (still a prefix), kept[r] = the occupied
// ones among them.  Without OCC the grid test compiles away and kept[r] = that prefix.
//
// W < 64: a ray that stops after a handful of samples (a trained scene seen from close by; the
// bench's terminating regime keeps 3.5 samples per ray) costs a 16- or 8-sample stride instead of a
// 64-sample one -- the wave scans are row scans anyway, and the gathers of a stride touch as many
// lines either way.  Same counts whatever W, bit for bit (tests/test_gpu_fused.py).
template <int F, bool POW2, int W, bool OCC>
__device__ __forceinline__ void march_rays(
  const float * __restrict__ rays_o, const float * __restrict__ rays_d,
  const float * __restrict__ noise, const uint16_t * __restrict__ table,
  const int32_t * __restrict__ primes, const float * __restrict__ bias,
  const float * __restrict__ mul, const float * __restrict__ w0, const float * __restrict__ b0,
  const uint32_t * __restrict__ bits, int G, int32_t * __restrict__ kept,
  int32_t * __restrict__ len, int n_rays, int S, float step, int L, uint32_t T,
  int64_t level_stride, float t_thresh, float density_shift, int corner_order)
{
  using RL = RayLanes<W>;
  const int r0 = ray_of_wave() * RL::kRays;
  if (r0 >= n_rays) return;
  const int lane = lane_id();
  const int r_raw = r0 + RL::group(lane);
  const bool has_ray = r_raw < n_rays;
  const int r = has_ray ? r_raw : n_rays - 1;  // (the spare groups of the last wave redo the last ray)
  const RayFrame rf = load_ray(rays_o, rays_d, r);
  const float * nrow = noise ? noise + (int64_t)r * S : nullptr;
  const float bias0 = b0[0];
  StrideState<W> carry = {};
  DepthState<W> ds = {};
  int n_kept = 0, n_len = 0;
  bool done = !has_ray;
  for (int k0 = 0; k0 < S; k0 += W) {
    const StrideSample sm = make_stride(rf, nrow, k0, S, step, carry, lane);
    float x = sm.px, y = sm.py, z = sm.pz;
    contract_point(x, y, z);
    bool occ = true;
    unsigned long long om = ~0ull;
    if constexpr (OCC) {
      occ = sm.valid && occ_test_contracted(x, y, z, bits, G);
      om = __ballot(occ);
    }
    float sec = 0.f;
    if (om != 0ull) {  // (wave-uniform: an empty stride costs no gathers at all)
      if (occ) {       // (no cross-lane move inside: the scan below runs with every lane on)
        const float logit = density_chain<F, POW2>(
          x, y, z, table, primes, bias, mul, w0, bias0, L, T, level_stride, corner_order,
          [](int, __half) {});
        const float sigma = expf(logit - density_shift);   // TruncExp forward
        sec = sm.valid ? sigma * sm.dt : 0.f;               // sigma * dt
      }
    }
    const KeepStep ks = keep_step(sec, sm.valid && !done, k0, S, t_thresh, ds, lane);
    if (!done) {
      n_len += ks.n;
      n_kept += RL::count(ks.mask & om, lane);
      done = ks.ends;  // nothing later survives
    }
    if (__ballot(!done) == 0ull) break;
  }
  if (has_ray && RL::sample(lane) == 0) {
    kept[r_raw] = n_kept;
    if constexpr (OCC) len[r_raw] = n_len;
  }
}

#define F2N_MARCH_PARAMS                                                                           \
  const float * __restrict__ rays_o, const float * __restrict__ rays_d,                            \
    const float * __restrict__ noise, const uint16_t * __restrict__ table,                         \
    const int32_t * __restrict__ primes, const float * __restrict__ bias,                          \
    const float * __restrict__ mul, const float * __restrict__ w0, const float * __restrict__ b0
#define F2N_MARCH_TAIL_PARAMS                                                                      \
  int n_rays, int S, float step, int L, uint32_t T, int64_t level_stride, float t_thresh,          \
    float density_shift, int corner_order
#define F2N_MARCH_HEAD_ARGS rays_o, rays_d, noise, table, primes, bias, mul, w0, b0
#define F2N_MARCH_TAIL_ARGS                                                                        \
  n_rays, S, step, L, T, level_stride, t_thresh, density_shift, corner_order

// one ray per wavefront (F2N_OPT_MARCH = 1)
template <int F, bool POW2>
__global__ __launch_bounds__(F2N_BLOCK) void density_march_kernel(
  F2N_MARCH_PARAMS, int32_t * __restrict__ kept, F2N_MARCH_TAIL_PARAMS)
{
  march_rays<F, POW2, 64, false>(
    F2N_MARCH_HEAD_ARGS, nullptr, 0, kept, nullptr, F2N_MARCH_TAIL_ARGS);
}

template <int F, bool POW2>
__global__ __launch_bounds__(F2N_BLOCK) void density_march_occ_kernel(
  F2N_MARCH_PARAMS, const uint32_t * __restrict__ bits, int G, int32_t * __restrict__ kept,
  int32_t * __restrict__ len, F2N_MARCH_TAIL_PARAMS)
{
  march_rays<F, POW2, 64, true>(F2N_MARCH_HEAD_ARGS, bits, G, kept, len, F2N_MARCH_TAIL_ARGS);
}

// four rays per wavefront (F2N_OPT_MARCH = 2)
template <int F, bool POW2>
__global__ __launch_bounds__(F2N_BLOCK) void density_march16_kernel(
  F2N_MARCH_PARAMS, int32_t * __restrict__ kept, F2N_MARCH_TAIL_PARAMS)
{
  march_rays<F, POW2, 16, false>(
    F2N_MARCH_HEAD_ARGS, nullptr, 0, kept, nullptr, F2N_MARCH_TAIL_ARGS);
}

// eight rays per wavefront (the default)
template <int F, bool POW2>
__global__ __launch_bounds__(F2N_BLOCK) void density_march8_kernel(
  F2N_MARCH_PARAMS, int32_t * __restrict__ kept, F2N_MARCH_TAIL_PARAMS)
{
  march_rays<F, POW2, 8, false>(
    F2N_MARCH_HEAD_ARGS, nullptr, 0, kept, nullptr, F2N_MARCH_TAIL_ARGS);
}

// ---- f2n_density_scan ---------------------------------------------------------------------------
// The keep-prefix of every ray from an ALREADY COMPUTED encoding of all its samples (channel-major
// [C, n_all]): same logit FMA chain as density_chain and the march's own keep_step, so both give
// identical counts.  Used when most samples survive anyway: the encoding is then computed
// once by the level-major f2n_hash_fwd (L2-resident table levels) and reused by the shading pass,
// instead of being evaluated by the march and again by the second pass.
template <int C>
__global__ __launch_bounds__(F2N_BLOCK) void density_scan_kernel(
  const float * __restrict__ enc, const float * __restrict__ dt, const float * __restrict__ w0,
  const float * __restrict__ b0, int32_t * __restrict__ kept, int n_rays, int S, int64_t n_all,
  float t_thresh, float density_shift)
{
  const int r = ray_of_wave();
  if (r >= n_rays) return;
  const int lane = lane_id();
  const float bias0 = b0[0];
  const int64_t base = (int64_t)r * S;
  DepthState<64> ds = {};
  int n_kept = 0;
  for (int k0 = 0; k0 < S; k0 += F2N_WAVE) {
    const int k = k0 + lane;
    const bool valid = k < S;
    const int64_t i = base + (valid ? k : S - 1);
    float logit = bias0;
#pragma unroll
    for (int c = 0; c < C; c++) logit = fmaf(enc[(int64_t)c * n_all + i], w0[c], logit);
    const float sigma = expf(logit - density_shift);
    const float sec = valid ? sigma * dt[i] : 0.f;
    const KeepStep ks = keep_step(sec, valid, k0, S, t_thresh, ds, lane);
    n_kept += ks.n;
    if (ks.ends) break;
  }
  if (lane == 0) kept[r] = n_kept;
}

// ---- f2n_density_margin -------------------------------------------------------------------------
// Does every ray of a dense [n_rays, S] grid keep all its samples with room to spare?  One wavefront
// per ray sums the optical depth of its S density logits; a ray whose total reaches `depth_limit`
// (or is not a number) sets flag[0].  The caller chooses depth_limit = -ln(threshold) - margin, so a
// clear flag means the exact early-stop scan (f2n_density_scan, whose FMA order differs in the last
// bits) would keep everything too.
__global__ __launch_bounds__(F2N_BLOCK) void density_margin_kernel(
  const float * __restrict__ logit, const float * __restrict__ dt, int32_t * __restrict__ flag,
  int n_rays, int S, float density_shift, float depth_limit)
{
  const int r = ray_of_wave();
  if (r >= n_rays) return;
  const int lane = lane_id();
  const int64_t base = (int64_t)r * S;
  float sum = 0.f;
  for (int k = lane; k < S; k += F2N_WAVE) sum += expf(logit[base + k] - density_shift) * dt[base + k];
  sum = wave_sum(sum);
  if (lane == 0 && !(sum < depth_limit)) atomicOr(flag, 1);
}

// ---- f2n_compact_rows_cm ------------------------------------------------------------------------
// Channel-major compaction of per-ray prefixes: dst[c, new_start_r + k] = src[c, r*S + k], k < cnt_r.
__global__ __launch_bounds__(F2N_BLOCK) void compact_rows_cm_kernel(
  const float * __restrict__ src, int64_t n_src, float * __restrict__ dst, int64_t n_dst, int C,
  const int32_t * __restrict__ bounds, int n_rays, int S)
{
  const int r = ray_of_wave();
  if (r >= n_rays) return;
  const int lane = lane_id();
  const int start = bounds[2 * r];
  const int cnt = bounds[2 * r + 1] - start;
  const int64_t sbase = (int64_t)r * S;
  for (int k = lane; k < cnt; k += F2N_WAVE)
    for (int c = 0; c < C; c++)
      dst[(int64_t)c * n_dst + start + k] = src[(int64_t)c * n_src + sbase + k];
}

// ---- f2n_bounds_from_counts ---------------------------------------------------------------------

constexpr int kScanBlock = 1024;
constexpr int kScanItems = 16;  // per thread and pass: the single workgroup is bound by the latency of
                                // its passes (65 536 rays: 4 passes instead of 16, 39 -> ~12 us)

__global__ __launch_bounds__(kScanBlock) void bounds_from_counts_kernel(
  const int32_t * __restrict__ kept, int32_t * __restrict__ bounds, int32_t * __restrict__ total,
  int n_rays)
{
  __shared__ int wave_tot[kScanBlock / F2N_WAVE];
  __shared__ int tile_tot;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const bool pair_aligned = (reinterpret_cast<uintptr_t>(bounds) & 7u) == 0;
  int carry = 0;
  for (int base = 0; base < n_rays; base += kScanBlock * kScanItems) {
    const int i0 = base + tid * kScanItems;
    int v[kScanItems];
    int local = 0;
    if (i0 + kScanItems <= n_rays && (reinterpret_cast<uintptr_t>(kept) & 15u) == 0) {
#pragma unroll
      for (int j = 0; j < kScanItems; j += 4) {
        const int4 q = *reinterpret_cast<const int4 *>(kept + i0 + j);
        v[j] = q.x;
        v[j + 1] = q.y;
        v[j + 2] = q.z;
        v[j + 3] = q.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < kScanItems; j++) v[j] = (i0 + j < n_rays) ? kept[i0 + j] : 0;
    }
#pragma unroll
    for (int j = 0; j < kScanItems; j++) local += v[j];
    const int incl = wave_incl_scan_i32(local);
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    if (wv == 0) {
      const int wt = (lane < kScanBlock / F2N_WAVE) ? wave_tot[lane] : 0;
      const int wi = wave_incl_scan_i32(wt);
      if (lane < kScanBlock / F2N_WAVE) wave_tot[lane] = wi - wt;  // exclusive wave offsets
      if (lane == 63) tile_tot = wi;
    }
    __syncthreads();
    int run = carry + wave_tot[wv] + (incl - local);
#pragma unroll
    for (int j = 0; j < kScanItems; j++) {
      if (i0 + j < n_rays) {
        if (pair_aligned) {
          *reinterpret_cast<int2 *>(bounds + 2 * (i0 + j)) = make_int2(run, run + v[j]);
        } else {
          bounds[2 * (i0 + j)] = run;
          bounds[2 * (i0 + j) + 1] = run + v[j];
        }
      }
      run += v[j];
    }
    carry += tile_tot;
    __syncthreads();
  }
  if (tid == 0 && total) total[0] = carry;
}

// Up to 2^17 rays: one workgroup per 1024 rays.  Each re-derives its own offset -- the sum of all
// counts before its rays, read straight from `kept` (256 KiB for 65 536 rays: L2-resident; 8 MB of L2
// reads over all workgroups) -- so there is neither a second launch nor a hand-off between
// workgroups, and the 0.75 MB of loads and stores no longer pass through one CU (65 536 rays:
// 42 -> ~6 us).  Integer sums: the same bounds whatever the order.
constexpr int kMultiScanBlock = 256, kMultiScanItems = 4;
constexpr int kMultiScanRays = kMultiScanBlock * kMultiScanItems;
constexpr int kMultiScanMaxRays = 1 << 17;

__global__ __launch_bounds__(kMultiScanBlock) void bounds_from_counts_multi_kernel(
  const int32_t * __restrict__ kept, int32_t * __restrict__ bounds, int32_t * __restrict__ total,
  int n_rays)
{
  constexpr int kWaves = kMultiScanBlock / F2N_WAVE;
  __shared__ int wave_part[kWaves], wave_tot[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int first = (int)blockIdx.x * kMultiScanRays;  // (a multiple of 1024: int4 loads stay aligned)
  const bool vec = (reinterpret_cast<uintptr_t>(kept) & 15u) == 0;
  // ---- everything before this workgroup's rays
  int before = 0;
  if (vec) {
    for (int i = 4 * tid; i < first; i += 4 * kMultiScanBlock) {
      const int4 q = *reinterpret_cast<const int4 *>(kept + i);
      before += (q.x + q.y) + (q.z + q.w);
    }
  } else {
    for (int i = tid; i < first; i += kMultiScanBlock) before += kept[i];
  }
  before = __builtin_amdgcn_readlane(wave_incl_scan_i32(before), 63);
  // ---- this workgroup's rays
  const int i0 = first + tid * kMultiScanItems;
  int v[kMultiScanItems];
  int local = 0;
#pragma unroll
  for (int j = 0; j < kMultiScanItems; j++) {
    v[j] = (i0 + j < n_rays) ? kept[i0 + j] : 0;
    local += v[j];
  }
  const int incl = wave_incl_scan_i32(local);
  if (lane == 63) wave_tot[wv] = incl;
  if (lane == 0) wave_part[wv] = before;
  __syncthreads();
  int offset = 0, lower = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kWaves; w++) {
    offset += wave_part[w];
    if (w < wv) lower += wave_tot[w];
    all += wave_tot[w];
  }
  int run = offset + lower + (incl - local);
  const bool pair_aligned = (reinterpret_cast<uintptr_t>(bounds) & 7u) == 0;
#pragma unroll
  for (int j = 0; j < kMultiScanItems; j++) {
    if (i0 + j < n_rays) {
      if (pair_aligned) {
        *reinterpret_cast<int2 *>(bounds + 2 * (i0 + j)) = make_int2(run, run + v[j]);
      } else {
        bounds[2 * (i0 + j)] = run;
        bounds[2 * (i0 + j) + 1] = run + v[j];
      }
    }
    run += v[j];
  }
  if (total && blockIdx.x == gridDim.x - 1 && tid == 0) total[0] = offset + all;
}

}  // namespace

extern "C" int f2n_sample_rays(
  const float * rays_o, const float * rays_d, const float * noise, float * pts, float * dirs,
  float * dt, float * t, int32_t * bounds, int n_rays, int S, float step, void * stream)
{
  if (n_rays < 0 || S < 1) return F2N_E_INVALID_ARG;
  if ((int64_t)n_rays * S > INT32_MAX) return F2N_E_INVALID_ARG;  // bounds are int32
  if (n_rays == 0) return F2N_OK;
  if (!rays_o || !rays_d || !pts || !dirs || !dt || !t || !bounds) return F2N_E_INVALID_ARG;
  hipLaunchKernelGGL(
    sample_rays_kernel, dim3(f2n_div_up(n_rays, F2N_WAVES_PER_BLOCK)), dim3(F2N_BLOCK), 0,
    (hipStream_t)stream, rays_o, rays_d, noise, pts, dirs, dt, t, bounds, n_rays, S, step);
  return f2n_launch_status();
}

extern "C" int f2n_sample_dense(
  const float * rays_o, const float * rays_d, const float * noise, const int32_t * noise_row,
  int noise_affine, float * x, float * dt, float * t, int32_t * bounds, float * ray_dirs,
  int n_rays, int S, float step, void * stream)
{
  if (n_rays < 0 || S < 1 || (noise_affine != 0 && noise_affine != 1)) return F2N_E_INVALID_ARG;
  if ((int64_t)n_rays * S > INT32_MAX) return F2N_E_INVALID_ARG;  // bounds are int32
  if (n_rays == 0) return F2N_OK;
  if (!rays_o || !rays_d || !x || !dt || !t || !bounds || !ray_dirs) return F2N_E_INVALID_ARG;
  hipLaunchKernelGGL(
    sample_dense_kernel, dim3(f2n_div_up(n_rays, F2N_WAVES_PER_BLOCK)), dim3(F2N_BLOCK), 0,
    (hipStream_t)stream, rays_o, rays_d, noise, noise_row, noise_affine, x, dt, t, bounds, ray_dirs,
    n_rays, S, step);
  return f2n_launch_status();
}

extern "C" int f2n_sample_compact(
  const float * rays_o, const float * rays_d, const float * noise, const int32_t * bounds,
  float * pts, float * dirs, float * dt, float * t, int n_rays, int S, float step, void * stream)
{
  if (n_rays < 0 || S < 1) return F2N_E_INVALID_ARG;
  if (n_rays == 0) return F2N_OK;
  if (!rays_o || !rays_d || !bounds) return F2N_E_INVALID_ARG;
  hipLaunchKernelGGL(
    sample_compact_kernel, dim3(f2n_div_up(n_rays, F2N_WAVES_PER_BLOCK)), dim3(F2N_BLOCK), 0,
    (hipStream_t)stream, rays_o, rays_d, noise, bounds, pts, dirs, dt, t, n_rays, S, step);
  return f2n_launch_status();
}

extern "C" int f2n_density_march(
  const float * rays_o, const float * rays_d, const float * noise, const uint16_t * table_f16,
  const int32_t * primes, const float * bias, const float * mul, const float * w0, const float * b0,
  int32_t * kept, int n_rays, int S, float step, int L, int F, uint32_t T, int64_t level_stride,
  float t_thresh, float density_shift, void * stream)
{
  if (n_rays < 0 || S < 1 || L > F2N_MAX_LEVELS) return F2N_E_INVALID_ARG;
  if (const int st = f2n_field_args_status(L, F, T, level_stride)) return st;
  if (n_rays == 0) return F2N_OK;
  if (!rays_o || !rays_d || !table_f16 || !primes || !bias || !mul || !w0 || !b0 || !kept)
    return F2N_E_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(table_f16) % (2u * F)) return F2N_E_INVALID_ARG;
  // eight rays per wavefront (8-sample strides) unless F2N_OPT_MARCH asks for one (1: 64-sample
  // strides, round 2) or four (2: 16-sample strides)
  const int route = f2n_get_option(F2N_OPT_MARCH);
  const int corner_order = f2n_get_option(F2N_OPT_GATHER_PAIRED);
  const bool rows = route == 2;
  const int rays_per_wave = route == 1 ? 1 : route == 2 ? 4 : 8;
  const dim3 grid(f2n_div_up(n_rays, F2N_WAVES_PER_BLOCK * rays_per_wave)), block(F2N_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  f2n_dispatch_field(F, T, [&](auto ff, auto p2) {
    constexpr int FF = decltype(ff)::value;
    constexpr bool P2 = decltype(p2)::value;
    const auto kernel = route == 0 ? density_march8_kernel<FF, P2>
                        : rows     ? density_march16_kernel<FF, P2>
                                   : density_march_kernel<FF, P2>;
    hipLaunchKernelGGL(
      kernel, grid, block, 0, s, rays_o, rays_d, noise, table_f16, primes, bias, mul, w0, b0, kept,
      n_rays, S, step, L, T, level_stride, t_thresh, density_shift, corner_order);
  });
  return f2n_launch_status();
}

extern "C" int f2n_density_march_occ(
  const float * rays_o, const float * rays_d, const float * noise, const uint16_t * table_f16,
  const int32_t * primes, const float * bias, const float * mul, const float * w0, const float * b0,
  const uint32_t * bits, int G, int32_t * kept, int32_t * len, int n_rays, int S, float step, int L,
  int F, uint32_t T, int64_t level_stride, float t_thresh, float density_shift, void * stream)
{
  if (n_rays < 0 || S < 1 || L > F2N_MAX_LEVELS || !f2n_occ_res_ok(G)) return F2N_E_INVALID_ARG;
  if (const int st = f2n_field_args_status(L, F, T, level_stride)) return st;
  if (n_rays == 0) return F2N_OK;
  if (!rays_o || !rays_d || !table_f16 || !primes || !bias || !mul || !w0 || !b0 || !bits ||
      !kept || !len)
    return F2N_E_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(table_f16) % (2u * F)) return F2N_E_INVALID_ARG;
  const dim3 grid(f2n_div_up(n_rays, F2N_WAVES_PER_BLOCK)), block(F2N_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  const int corner_order = f2n_get_option(F2N_OPT_GATHER_PAIRED);
  f2n_dispatch_field(F, T, [&](auto ff, auto p2) {
    hipLaunchKernelGGL(
      (density_march_occ_kernel<decltype(ff)::value, decltype(p2)::value>), grid, block, 0, s,
      rays_o, rays_d, noise, table_f16, primes, bias, mul, w0, b0, bits, G, kept, len, n_rays, S,
      step, L, T, level_stride, t_thresh, density_shift, corner_order);
  });
  return f2n_launch_status();
}

extern "C" int f2n_sample_compact_occ(
  const float * rays_o, const float * rays_d, const float * noise, const int32_t * bounds,
  const int32_t * len, const uint32_t * bits, int G, float * pts, float * dirs, float * dt,
  float * t, int n_rays, int S, float step, void * stream)
{
  if (n_rays < 0 || S < 1 || !f2n_occ_res_ok(G)) return F2N_E_INVALID_ARG;
  if (n_rays == 0) return F2N_OK;
  if (!rays_o || !rays_d || !bounds || !len || !bits) return F2N_E_INVALID_ARG;
  hipLaunchKernelGGL(
    sample_compact_occ_kernel, dim3(f2n_div_up(n_rays, F2N_WAVES_PER_BLOCK)), dim3(F2N_BLOCK), 0,
    (hipStream_t)stream, rays_o, rays_d, noise, bounds, len, bits, G, pts, dirs, dt, t, n_rays, S,
    step);
  return f2n_launch_status();
}

extern "C" int f2n_density_scan(
  const float * enc_cm, int C, const float * dt, const float * w0, const float * b0, int32_t * kept,
  int n_rays, int S, float t_thresh, float density_shift, void * stream)
{
  if (n_rays < 0 || S < 1) return F2N_E_INVALID_ARG;
  if (C != 8 && C != 16 && C != 32 && C != 64 && C != 128) return F2N_E_UNSUPPORTED;
  if (n_rays == 0) return F2N_OK;
  if (!enc_cm || !dt || !w0 || !b0 || !kept) return F2N_E_INVALID_ARG;
  const dim3 grid(f2n_div_up(n_rays, F2N_WAVES_PER_BLOCK)), block(F2N_BLOCK);
  const int64_t n_all = (int64_t)n_rays * S;
  hipStream_t s = (hipStream_t)stream;
#define F2N_SCAN(CC)                                                                              \
  hipLaunchKernelGGL(                                                                             \
    (density_scan_kernel<CC>), grid, block, 0, s, enc_cm, dt, w0, b0, kept, n_rays, S, n_all,     \
    t_thresh, density_shift)
  switch (C) {
    case 8: F2N_SCAN(8); break;
    case 16: F2N_SCAN(16); break;
    case 32: F2N_SCAN(32); break;
    case 64: F2N_SCAN(64); break;
    default: F2N_SCAN(128); break;
  }
#undef F2N_SCAN
  return f2n_launch_status();
}

extern "C" int f2n_density_margin(
  const float * logit, const float * dt, int32_t * flag, int n_rays, int S, float density_shift,
  float depth_limit, void * stream)
{
  if (n_rays < 0 || S < 1) return F2N_E_INVALID_ARG;
  if (n_rays == 0) return F2N_OK;
  if (!logit || !dt || !flag) return F2N_E_INVALID_ARG;
  hipLaunchKernelGGL(
    density_margin_kernel, dim3(f2n_div_up(n_rays, F2N_WAVES_PER_BLOCK)), dim3(F2N_BLOCK), 0,
    (hipStream_t)stream, logit, dt, flag, n_rays, S, density_shift, depth_limit);
  return f2n_launch_status();
}

extern "C" int f2n_compact_rows_cm(
  const float * src, int64_t n_src, float * dst, int64_t n_dst, int C, const int32_t * bounds,
  int n_rays, int S, void * stream)
{
  if (n_rays < 0 || S < 1 || C < 1 || n_src < 0 || n_dst < 0) return F2N_E_INVALID_ARG;
  if (n_rays == 0 || n_dst == 0) return F2N_OK;
  if (!src || !dst || !bounds) return F2N_E_INVALID_ARG;
  hipLaunchKernelGGL(
    compact_rows_cm_kernel, dim3(f2n_div_up(n_rays, F2N_WAVES_PER_BLOCK)), dim3(F2N_BLOCK), 0,
    (hipStream_t)stream, src, n_src, dst, n_dst, C, bounds, n_rays, S);
  return f2n_launch_status();
}

extern "C" int f2n_bounds_from_counts(
  const int32_t * kept, int32_t * bounds, int32_t * total, int n_rays, void * stream)
{
  if (n_rays < 0 || n_rays > (1 << 24)) return F2N_E_INVALID_ARG;
  if (n_rays > 0 && (!kept || !bounds)) return F2N_E_INVALID_ARG;
  if (n_rays > kMultiScanRays && n_rays <= kMultiScanMaxRays)
    hipLaunchKernelGGL(
      bounds_from_counts_multi_kernel, dim3(f2n_div_up(n_rays, kMultiScanRays)),
      dim3(kMultiScanBlock), 0, (hipStream_t)stream, kept, bounds, total, n_rays);
  else
    hipLaunchKernelGGL(
      bounds_from_counts_kernel, dim3(1), dim3(kScanBlock), 0, (hipStream_t)stream, kept, bounds,
      total, n_rays);
  return f2n_launch_status();
}
