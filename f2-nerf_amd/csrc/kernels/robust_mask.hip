// robust_mask.hip -- per-ray weights of a trimmed colour loss with patch-smoothed inlier masks
// (include/f2nerf_hip.h has the entry).  The idea and the defaults are those of RobustNeRF (Sabour et
// al., CVPR 2023, section 3.2): rank the rays of a batch by colour residual, keep those below a
// quantile, smooth that mask over image patches so that sharp but static detail is let back in while
// coherent blobs stay out.  The reference has no such loss: src/main_functions/train_manager.cpp:78-96
// averages over every ray of the batch.  The exact rule below is this project's; integers decide
// everything after the residual, there is no host read and no float atomic: the same bits on every run.
//
// THE RULE (tests/robust_model.py follows these steps by number).  m_r is ray_weight[r], 1 when
// ray_weight is null.
//   1. Considered rays.  Ray r is considered iff m_r != 0.  A ray that is not considered gets
//      weight_out = +0, omega = 0, takes no part in the quantile or in any count, and its colours are
//      not read (f2n_loss_sup_fwd's rule: they may hold anything, NaN included).
//   2. Residual, f32, no contraction (-ffp-contract=off):
//        d_c = colors[r][c] - target[r][c]            one rounding each
//        eps = (d0*d0 + d1*d1) + d2*d2                three products, two adds, in this order
//      A non-finite eps becomes +inf.  eps is never negative, so its bits order like its value.
//   3. Threshold.  N_c = the number of considered rays;
//        k = min(N_c, max(1, (int64)ceil((double)quantile * N_c)))      on the device
//      T = the k-th smallest eps among the considered rays, found exactly by radix selection on the
//      u32 bits of eps: four passes of 8 bits from the top, a 256-bin LDS histogram of integer atomics
//      per pass over the rays that match the prefix chosen so far, the bin holding the k-th element
//      picked by an integer prefix sum.  One workgroup strides over the rays and keeps the prefix in
//      LDS; nothing is read on the host.  N_c == 0: T = 0 and every output is zero.
//   4. Pixel label.  w0_r = isfinite(eps_r) && eps_r <= T, on the bits.  Every tie at T is an inlier,
//      so sum w0 may exceed k; an infinite eps is an outlier even when T = inf.
//   5. Box diffusion (P > 0).  Pixel (u, v) of patch b is ray b P^2 + u P + v (f2n_draw_patches).  Over
//      the considered pixels of the 3 x 3 window clipped to the patch: cnt of them, s of those with
//      w0 = 1;  W_r = cnt > 0 && (float)s >= box_thresh * (float)cnt, the product rounded once in f32.
//   6. Neighbourhood vote (P > 0).  The patch is tiled from its top-left corner into blocks of
//      nbhd x nbhd pixels, edge blocks being whatever is left (P = 11, nbhd = 8: 8 + 3).  Per block,
//      cnt considered pixels, s of them with W = 1;
//        R_block = cnt > 0 && (float)s >= nbhd_thresh * (float)cnt.
//   7. Final label.  omega_r = w0_r | W_r | R_block(r) for a considered ray; weight_out = m_r where
//      omega_r is set (1 without ray_weight), else +0.  P = 0: steps 5 and 6 are skipped, omega = w0.
//   stats4 = {T, N_c, sum w0, sum omega}: the three counts are integer sums in a fixed tree (a DPP scan
//   per wavefront, the wave totals added in order), below 2^24 and so exact as f32.
//
// LAUNCHES.  P = 0: one (the selecting workgroup also writes the labels).  P > 0: three -- select, one
// workgroup per patch for steps 4 to 7 with the patch's labels as bytes in LDS and a packed
// (cnt | s << 16) counter per block, and one workgroup that adds the patches' counts.  No workgroup
// waits on another.
// WORKSPACE, u32 words: [0] the bits of T, [1] N_c, [2..7] unused, [8 .. 8 + n) the residuals' bits
// (kNotConsidered for a ray that is not considered), then two counts per patch.
#include "common.hiph"

namespace
{

constexpr int kSelBlock = 1024;          // the selecting workgroup
constexpr int kPatchBlock = 256;         // one workgroup per patch
constexpr int kMaxP = 64;
constexpr int kHeaderWords = 8;
constexpr uint32_t kInfBits = 0x7f800000u;
constexpr uint32_t kNotConsidered = 0xffffffffu;  // no residual has the sign bit

// sum of v over the workgroup, valid in every thread; smem holds blockDim.x / 64 + 1 ints
__device__ __forceinline__ int block_sum_i32(int v, int * smem)
{
  const int scan = wave_incl_scan_i32(v);
  const int lane = lane_id(), wave = (int)(threadIdx.x >> 6), n_waves = (int)(blockDim.x >> 6);
  __syncthreads();
  if (lane == 63) smem[wave] = scan;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int i = 0; i < n_waves; i++) t += smem[i];
    smem[n_waves] = t;
  }
  __syncthreads();
  return smem[n_waves];
}

__device__ __forceinline__ bool label_w0(uint32_t key, uint32_t t_bits)
{
  return key < kInfBits && key <= t_bits;  // (kNotConsidered fails the first test)
}

// steps 1 to 3, and with P == 0 steps 4 and 7 as well
__global__ __launch_bounds__(kSelBlock) void robust_select_kernel(
  const float * __restrict__ colors, const float * __restrict__ target,
  const float * __restrict__ ray_weight, int n_rays, float quantile, int scattered,
  float * __restrict__ weight_out, uint8_t * __restrict__ omega_out, float * __restrict__ stats4,
  uint32_t * __restrict__ workspace)
{
  __shared__ int s_red[kSelBlock / 64 + 1];
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_prefix;
  __shared__ int s_k;
  uint32_t * keys = workspace + kHeaderWords;
  const int tid = (int)threadIdx.x;

  // steps 1 and 2
  int n_c = 0;
  for (int r = tid; r < n_rays; r += kSelBlock) {
    uint32_t key = kNotConsidered;
    const bool considered = ray_weight ? ray_weight[r] != 0.f : true;
    if (considered) {
      const float d0 = colors[3 * r] - target[3 * r], d1 = colors[3 * r + 1] - target[3 * r + 1],
                  d2 = colors[3 * r + 2] - target[3 * r + 2];
      const float eps = (d0 * d0 + d1 * d1) + d2 * d2;
      key = (__float_as_uint(eps) & 0x7fffffffu) < kInfBits ? __float_as_uint(eps) : kInfBits;
      n_c++;
    }
    keys[r] = key;
  }
  n_c = block_sum_i32(n_c, s_red);  // (its barriers also order the keys' stores before the reads below)

  // step 3
  uint32_t t_bits = 0u;
  if (n_c > 0) {
    if (tid == 0) {
      int64_t k = (int64_t)ceil((double)quantile * (double)n_c);
      if (k < 1) k = 1;
      if (k > n_c) k = n_c;
      s_k = (int)k;
      s_prefix = 0u;
    }
#pragma unroll
    for (int pass = 0; pass < 4; pass++) {
      const int shift = 24 - 8 * pass;
      if (tid < 256) s_hist[tid] = 0u;
      __syncthreads();
      const uint32_t prefix = s_prefix;
      for (int r = tid; r < n_rays; r += kSelBlock) {
        const uint32_t key = keys[r];
        if (key == kNotConsidered) continue;
        if (pass == 0 || (key >> ((shift + 8) & 31)) == prefix)
          atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid < 64) {
        // lane l owns bins 4 l .. 4 l + 3; the lane whose span holds the k-th element walks its four
        const int k = s_k;
        const int h0 = (int)s_hist[4 * tid], h1 = (int)s_hist[4 * tid + 1],
                  h2 = (int)s_hist[4 * tid + 2], h3 = (int)s_hist[4 * tid + 3];
        const int mine = (h0 + h1) + (h2 + h3);
        const int incl = wave_incl_scan_i32(mine), excl = incl - mine;
        if (excl < k && k <= incl) {
          int below = excl, bin = 4 * tid;
          if (below + h0 < k) {
            below += h0;
            bin++;
            if (below + h1 < k) {
              below += h1;
              bin++;
              if (below + h2 < k) {
                below += h2;
                bin++;
              }
            }
          }
          s_prefix = (prefix << 8) | (uint32_t)bin;
          s_k = k - below;
        }
      }
      __syncthreads();
    }
    t_bits = s_prefix;
  }
  if (tid == 0) {
    workspace[0] = t_bits;
    workspace[1] = (uint32_t)n_c;
    stats4[0] = __uint_as_float(t_bits);
    stats4[1] = (float)n_c;
  }
  if (!scattered) return;

  // steps 4 and 7 without patches: omega = w0
  int n_in = 0;
  for (int r = tid; r < n_rays; r += kSelBlock) {
    const bool in = label_w0(keys[r], t_bits);
    weight_out[r] = in ? (ray_weight ? ray_weight[r] : 1.f) : 0.f;
    if (omega_out) omega_out[r] = in ? 1 : 0;
    n_in += in ? 1 : 0;
  }
  n_in = block_sum_i32(n_in, s_red);
  if (tid == 0) stats4[2] = stats4[3] = (float)n_in;
}

// steps 4 to 7 of one patch
__global__ __launch_bounds__(kPatchBlock) void robust_patch_kernel(
  const float * __restrict__ ray_weight, int P, int nbhd, float box_thresh, float nbhd_thresh,
  float * __restrict__ weight_out, uint8_t * __restrict__ omega_out,
  const uint32_t * __restrict__ workspace, uint32_t * __restrict__ counts)
{
  __shared__ uint8_t s_px[kMaxP * kMaxP];      // bit 0 considered, bit 1 w0
  __shared__ uint8_t s_box[kMaxP * kMaxP];     // W
  __shared__ uint32_t s_block[kMaxP * kMaxP];  // cnt | s << 16, both at most 4096
  __shared__ int s_red[kPatchBlock / 64 + 1];
  const int tid = (int)threadIdx.x, PP = P * P;
  const int64_t base = (int64_t)blockIdx.x * PP;
  const uint32_t * keys = workspace + kHeaderWords + base;
  const uint32_t t_bits = workspace[0];
  const int nb = (P + nbhd - 1) / nbhd;

  // step 4
  for (int p = tid; p < PP; p += kPatchBlock) {
    const uint32_t key = keys[p];
    s_px[p] = (uint8_t)((key != kNotConsidered ? 1 : 0) | (label_w0(key, t_bits) ? 2 : 0));
  }
  for (int b = tid; b < nb * nb; b += kPatchBlock) s_block[b] = 0u;
  __syncthreads();
  // step 5, and the counts of step 6
  for (int p = tid; p < PP; p += kPatchBlock) {
    const int u = p / P, v = p - u * P;
    int cnt = 0, s = 0;
    for (int du = -1; du <= 1; du++) {
      const int uu = u + du;
      if (uu < 0 || uu >= P) continue;
      for (int dv = -1; dv <= 1; dv++) {
        const int vv = v + dv;
        if (vv < 0 || vv >= P) continue;
        const int f = s_px[uu * P + vv];
        cnt += f & 1;
        s += (f >> 1) & 1;
      }
    }
    const bool W = cnt > 0 && (float)s >= box_thresh * (float)cnt;
    s_box[p] = W ? 1 : 0;
    if (s_px[p] & 1) atomicAdd(&s_block[(u / nbhd) * nb + v / nbhd], 1u | (W ? 1u << 16 : 0u));
  }
  __syncthreads();
  // the vote of step 6, and step 7
  int n_w0 = 0, n_omega = 0;
  for (int p = tid; p < PP; p += kPatchBlock) {
    const int f = s_px[p];
    const int u = p / P, v = p - u * P;
    const uint32_t c = s_block[(u / nbhd) * nb + v / nbhd];
    const int cnt = (int)(c & 0xffffu), s = (int)(c >> 16);
    const bool R = cnt > 0 && (float)s >= nbhd_thresh * (float)cnt;
    const bool omega = (f & 1) && ((f & 2) || s_box[p] || R);
    const int64_t r = base + p;
    weight_out[r] = omega ? (ray_weight ? ray_weight[r] : 1.f) : 0.f;
    if (omega_out) omega_out[r] = omega ? 1 : 0;
    n_w0 += (f >> 1) & 1;
    n_omega += omega ? 1 : 0;
  }
  n_w0 = block_sum_i32(n_w0, s_red);
  n_omega = block_sum_i32(n_omega, s_red);
  if (tid == 0) {
    counts[2 * blockIdx.x] = (uint32_t)n_w0;
    counts[2 * blockIdx.x + 1] = (uint32_t)n_omega;
  }
}

// the patches' counts: thread t adds patches t, t + 256, ... in ascending order, then the tree
__global__ __launch_bounds__(kPatchBlock) void robust_counts_kernel(
  const uint32_t * __restrict__ counts, int n_patches, float * __restrict__ stats4)
{
  __shared__ int s_red[kPatchBlock / 64 + 1];
  int a = 0, b = 0;
  for (int i = (int)threadIdx.x; i < n_patches; i += kPatchBlock) {
    a += (int)counts[2 * i];
    b += (int)counts[2 * i + 1];
  }
  a = block_sum_i32(a, s_red);
  b = block_sum_i32(b, s_red);
  if (threadIdx.x == 0) {
    stats4[2] = (float)a;
    stats4[3] = (float)b;
  }
}

bool robust_sizes_ok(int n_rays) { return n_rays >= 1 && n_rays < (1 << 24); }

}  // namespace

extern "C" int64_t f2n_robust_workspace_words(int n_rays)
{
  if (!robust_sizes_ok(n_rays)) return 0;
  // header, one word per ray, two per patch of the smallest side (3 x 3)
  return kHeaderWords + (int64_t)n_rays + 2 * ((int64_t)n_rays / 9 + 1);
}

extern "C" int f2n_robust_weights(
  const float * colors, const float * target, const float * ray_weight, int n_rays, int P, int nbhd,
  float quantile, float box_thresh, float nbhd_thresh, float * weight_out, uint8_t * omega_out,
  float * stats4, uint32_t * workspace, void * stream)
{
  if (!colors || !target || !weight_out || !stats4 || !workspace) return F2N_E_INVALID_ARG;
  if (!robust_sizes_ok(n_rays)) return F2N_E_INVALID_ARG;
  if (P != 0 && (P < 3 || P > kMaxP || n_rays % (P * P) != 0 || nbhd < 1 || nbhd > P))
    return F2N_E_INVALID_ARG;
  // (written so that NaN fails)
  if (!(quantile > 0.f && quantile <= 1.f) || !(box_thresh >= 0.f && box_thresh <= 1.f) ||
      !(nbhd_thresh >= 0.f && nbhd_thresh <= 1.f))
    return F2N_E_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(
    robust_select_kernel, dim3(1), dim3(kSelBlock), 0, s, colors, target, ray_weight, n_rays,
    quantile, P == 0 ? 1 : 0, weight_out, omega_out, stats4, workspace);
  if (P != 0) {
    const int n_patches = n_rays / (P * P);
    uint32_t * counts = workspace + kHeaderWords + n_rays;
    hipLaunchKernelGGL(
      robust_patch_kernel, dim3(n_patches), dim3(kPatchBlock), 0, s, ray_weight, P, nbhd, box_thresh,
      nbhd_thresh, weight_out, omega_out, workspace, counts);
    hipLaunchKernelGGL(
      robust_counts_kernel, dim3(1), dim3(kPatchBlock), 0, s, counts, n_patches, stats4);
  }
  return f2n_launch_status();
}
