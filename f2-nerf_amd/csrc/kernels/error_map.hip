// error_map.hip -- error-guided ray sampling: a per-image grid of running colour errors, its CDF and
// the training-batch draw that follows it (include/f2nerf_hip.h has the contracts).  They stand beside
// the reference's Dataset::sample_random_rays (src/dataset.cpp:150-171), which draws uniformly over
// pixels, and beside f2n_draw_pixels_masked (pixel_mask.hip), which draws uniformly over valid pixels.
// The idea is the per-image error map of instant-ngp's training loop (Mueller et al., SIGGRAPH 2022).
// Wherever a sum or a comparison decides something it is an integer, so the state after any number
// of steps is the same on every run.
//
// GEOMETRY (integers; host, kernels and the numpy model share it).  E images of h x w pixels, gh x gw
// cells per image, 1 <= gh <= h, 1 <= gw <= w.  Pixel (e, i, j) lies in cell
//     c = (e*gh + (i*gh)/h)*gw + (j*gw)/w
// and cell row a covers pixel rows ceil(a*h/gh) .. ceil((a+1)*h/gh) - 1, columns alike: i*gh/h == a
// iff a*h <= i*gh < (a+1)*h.  gh <= h makes every cell row at least one pixel high.  Limits:
// n_cells = E*gh*gw < 2^24, h*w < 2^31 and E*h*w < 2^36 (f2n_mask_pack's limit, which also keeps the
// cdf below 2^60).
//
// COUNTS.  One wavefront per cell, lanes over the cell's pixels in strides of 64, one bit test each;
// the 64 lane counts are added by the integer DPP scan of common.hiph.  No atomics.
//
// ACCUMULATE.  One lane per ray.  EVALUATION ORDER, all f64 on the f32 inputs (the library is built
// with -ffp-contract=off: nothing below is fused):
//     per channel c, alpha given:   om = 1.0 - a;  g = a * gt_c + om * bg_c     (else g = gt_c)
//     d_c = C_c - g
//     e = (d_0 * d_0 + d_1 * d_1) + d_2 * d_2
//     q = llrint(min(e, 4.0) * 1048576.0)            round half to even; 0 <= q <= 2^22
// A ray is skipped when its weight is given and zero, when e is not finite, and when (cam, i, j) lies
// outside the set; otherwise acc_sum[c] += q (u64) and acc_cnt[c] += 1 (u32), two integer atomicAdd
// in global memory -- the only atomics of the feature; integer sums do not depend on their order.
// Lanes of a wavefront hit unrelated cells (the batch is a random draw), which is the access shape
// atomics like least; at 65 536 rays that is 131 072 of them per step, against the millions of
// float atomics of a table gradient.
//
// APPLY.  One lane per cell with cnt > 0, f64:
//     mean = (double)sum / (1048576.0 * (double)cnt)
//     value = (float)(decay * value + (1.0 - decay) * mean)
// and both accumulators are left at zero.
//
// CDF.  mass[c] = quant(value[c]) * counts[c] in u64 with
//     quant(v) = 1 when v is not finite, else clamp(llrint((double)v * 65536.0), 1, 2^24)
// (the clamp is applied to the double before the conversion, so no value overflows it).  cdf is the
// inclusive prefix sum, at most 2^24 * E*h*w < 2^60.  Three launches, none of which waits on
// another workgroup: (1) one sum per tile of 2048 cells (256 lanes x 8 consecutive cells, a
// Hillis-Steele scan of the 256 lane totals in LDS), (2) one workgroup turns the tile sums into
// exclusive offsets (each lane a contiguous run of them, the same LDS scan across lanes), (3) every
// tile scans its cells again and adds its offset.  Integer sums: any scan structure gives these bits.
//
// DRAW.  One lane per ray r.  (x0, x1, x2, x3) = Philox4x32-10, key (seed_lo, seed_hi), counter
// (r, 0, 0, 0): the block the masked draw takes for attempt 0, of which it leaves x3 unused (the
// generator is specified in pixel_mask.hip).  T = llrint(uniform_fraction * 2^32), u = T / 2^32,
// total = cdf[n_cells - 1].
//   uniform branch ((uint64)x3 < T, or total == 0): f2n_draw_pixels_masked exactly -- attempts
//     a = 0 .. A-1 with counter (r, a, 0, 0), cam = mulhi(x0, E), i = mulhi(x1, h), j = mulhi(x2, w).
//   guided branch: t = mulhi64((x0 << 32) | x1, total) < total; the cell is the first c with
//     cdf[c] > t (binary search; a cell of mass 0 has cdf[c] == cdf[c-1] and is never the first);
//     attempts a = 0 .. A-1 with counter (r, a, 1, 0): i = i0 + mulhi(y0, rows),
//     j = j0 + mulhi(y1, cols) inside that cell.
//   The first attempt whose bit is set is kept (no bits: every pixel is valid); tries = a + 1, or 0
//   with the last attempt left in cam / ij.
//   ray_weight = 0 when tries == 0, else, with q = quant(value[cell of the kept pixel]) and
//   N = n_valid[0], in f64 and in this order:
//     den = (((1.0 - u) * (double)q) * (double)N) / (double)total + u;   weight = (float)(1.0 / den)
//   -- the uniform pdf 1 / N over the pdf used, (1 - u) q / total + u / N: its expectation under the
//   draw is 1, it never exceeds 1 / u, and at u = 1 it is exactly 1.
//   (The entry takes counts with value and cdf, the triple that belongs together, and checks it for
//   null; the kernel itself needs only value and cdf: a cell's count is already inside its mass.)
//
// DIVERGENCE.  The uniform branch diverges as the masked draw does (pixel_mask.hip: geometric in the
// valid fraction f, a wavefront runs as long as its unluckiest lane).  The guided branch's attempts
// are geometric in the valid fraction of the CHOSEN cell, and cells are chosen in proportion to their
// valid pixels, so a half-masked set costs about the masked draw's 7.3 attempts per wavefront at
// f = 0.5; a cell that is nearly all invalid but carries a large error is the bad case (its lanes run
// to the cap and lose the ray: ray weight 0).  With 0 < u < 1 a wavefront holds lanes of both
// branches and runs them one after the other: the sum of the two maxima.  Per attempt both branches
// cost one Philox block (~40 integer instructions) and one 4-byte load.
// The binary search is ceil(log2 n_cells) <= 24 dependent 8-byte loads per lane on an array of at most
// 128 MB.  At 200 x 32 x 32 cells the cdf is 1.6 MB (value and counts 0.8 MB each): it fits the 4 MiB
// L2 of every XCD several times over, the first steps of every search touch the same few lines in
// every lane, and only the last five or six steps are scattered -- L2 hits after the first batch, so
// about 18 x an L2 round trip per wavefront, a few microseconds, hidden by the other wavefronts.  At
// the 2^24-cell limit (128 MB) the array still fits the 256 MiB Infinity Cache but not L2, and the
// last ten steps of a search go there.  Alias tables would flatten both costs; not attempted here.
#include "common.hiph"
#include "philox.hiph"

namespace
{

constexpr int kEmBlock = 256;
constexpr int kScanItems = 8;
constexpr int kScanTile = kEmBlock * kScanItems;  // 2048 cells per workgroup
constexpr int64_t kMaxCells = (int64_t)1 << 24;
constexpr int64_t kMaxImagePixels = (int64_t)1 << 31;
constexpr int64_t kMaxMaskPixels = (int64_t)1 << 36;  // f2n_mask_pack's limit
constexpr uint32_t kQuantCap = 1u << 24;

// first pixel row (column) of cell row (column) a: ceil(a * h / gh)
__host__ __device__ __forceinline__ int cell_first(int a, int h, int gh)
{
  return (int)(((int64_t)a * h + gh - 1) / gh);
}

// cell row (column) of pixel row (column) i
__host__ __device__ __forceinline__ int cell_of(int i, int h, int gh)
{
  return (int)(((int64_t)i * gh) / h);
}

__device__ __forceinline__ uint32_t quant_value(float v)
{
  if (!isfinite(v)) return 1u;
  const double x = (double)v * 65536.0;
  if (!(x > 1.0)) return 1u;
  if (x >= (double)kQuantCap) return kQuantCap;
  return (uint32_t)llrint(x);  // >= 1
}

__device__ __forceinline__ bool pixel_valid(const uint32_t * __restrict__ bits, int64_t g)
{
  return !bits || ((bits[g >> 5] >> (uint32_t)(g & 31)) & 1u);
}

__global__ __launch_bounds__(kEmBlock) void mask_cell_counts_kernel(
  const uint32_t * __restrict__ bits, int h, int w, int gh, int gw, int n_cells,
  int32_t * __restrict__ counts)
{
  // (the cell is the same for all 64 lanes: a wavefront leaves whole, and every lane scans)
  const int c = blockIdx.x * (kEmBlock / 64) + (int)(threadIdx.x >> 6);
  if (c >= n_cells) return;
  const int lane = lane_id();
  const int b = c % gw, a = (c / gw) % gh, e = c / (gw * gh);
  const int i0 = cell_first(a, h, gh), rows = cell_first(a + 1, h, gh) - i0;
  const int j0 = cell_first(b, w, gw), cols = cell_first(b + 1, w, gw) - j0;
  const int n_px = rows * cols;  // <= h*w < 2^31
  if (!bits) {
    if (lane == 0) counts[c] = n_px;
    return;
  }
  int count = 0;
  for (uint32_t p = (uint32_t)lane; p < (uint32_t)n_px; p += 64u) {  // n_px < 2^31: no wrap
    const int i = i0 + (int)(p / (uint32_t)cols), j = j0 + (int)(p % (uint32_t)cols);
    const int64_t g = ((int64_t)e * h + i) * w + j;
    count += (int)((bits[g >> 5] >> (uint32_t)(g & 31)) & 1u);
  }
  count = wave_incl_scan_i32(count);
  if (lane == 63) counts[c] = count;
}

__global__ __launch_bounds__(kEmBlock) void error_map_accum_kernel(
  const float * __restrict__ colors, const float * __restrict__ gt, const float * __restrict__ alpha,
  const float * __restrict__ bg, const float * __restrict__ ray_weight,
  const int32_t * __restrict__ cam, const int32_t * __restrict__ ij, int n, int E, int h, int w,
  int gh, int gw, unsigned long long * __restrict__ acc_sum, uint32_t * __restrict__ acc_cnt)
{
  const int r = blockIdx.x * kEmBlock + threadIdx.x;
  if (r >= n) return;
  if (ray_weight && ray_weight[r] == 0.f) return;
  const int e = cam[r], i = ij[2 * r], j = ij[2 * r + 1];
  if (e < 0 || e >= E || i < 0 || i >= h || j < 0 || j >= w) return;
  const double a = alpha ? (double)alpha[r] : 1.0;
  const double om = 1.0 - a;
  double d2[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    double g = (double)gt[3 * r + c];
    if (alpha) g = a * g + om * (double)bg[3 * r + c];
    const double d = (double)colors[3 * r + c] - g;
    d2[c] = d * d;
  }
  const double err = (d2[0] + d2[1]) + d2[2];
  if (!isfinite(err)) return;
  const unsigned long long q = (unsigned long long)llrint(fmin(err, 4.0) * 1048576.0);
  const int cell = (e * gh + cell_of(i, h, gh)) * gw + cell_of(j, w, gw);  // < n_cells < 2^24
  atomicAdd(acc_sum + cell, q);
  atomicAdd(acc_cnt + cell, 1u);
}

__global__ __launch_bounds__(kEmBlock) void error_map_apply_kernel(
  float * __restrict__ value, unsigned long long * __restrict__ acc_sum,
  uint32_t * __restrict__ acc_cnt, int n_cells, float decay)
{
  const int c = blockIdx.x * kEmBlock + threadIdx.x;
  if (c >= n_cells) return;
  const uint32_t cnt = acc_cnt[c];
  if (cnt == 0u) return;  // (its sum is zero as well: nothing was added)
  const double mean = (double)acc_sum[c] / (1048576.0 * (double)cnt);
  const double d = (double)decay;
  value[c] = (float)(d * (double)value[c] + (1.0 - d) * mean);
  acc_sum[c] = 0ull;
  acc_cnt[c] = 0u;
}

// Inclusive scan of one u64 per lane over the workgroup's 256 lanes (Hillis-Steele in LDS, two
// buffers); every lane calls it.  Returns the lane's inclusive sum; smem[2 * kEmBlock].
__device__ __forceinline__ uint64_t block_incl_scan(uint64_t v, uint64_t * smem)
{
  const int t = (int)threadIdx.x;
  int cur = 0;
  smem[t] = v;
  __syncthreads();
#pragma unroll
  for (int off = 1; off < kEmBlock; off <<= 1) {
    const uint64_t mine = smem[cur * kEmBlock + t];
    const uint64_t left = t >= off ? smem[cur * kEmBlock + t - off] : 0ull;
    cur ^= 1;
    smem[cur * kEmBlock + t] = mine + left;
    __syncthreads();
  }
  const uint64_t out = smem[cur * kEmBlock + t];
  __syncthreads();  // (the buffers may be written again at once)
  return out;
}

// the masses of this lane's kScanItems consecutive cells (0 past the end) and their sum
__device__ __forceinline__ uint64_t lane_masses(
  const float * __restrict__ value, const int32_t * __restrict__ counts, int n_cells,
  uint64_t (&mass)[kScanItems])
{
  const int64_t first = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  uint64_t sum = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; k++) {
    const int64_t c = first + k;
    uint64_t m = 0;
    if (c < n_cells) {
      const int32_t cnt = counts[c];
      m = (uint64_t)quant_value(value[c]) * (uint64_t)(cnt > 0 ? cnt : 0);
    }
    mass[k] = m;
    sum += m;
  }
  return sum;
}

__global__ __launch_bounds__(kEmBlock) void error_cdf_tile_sums_kernel(
  const float * __restrict__ value, const int32_t * __restrict__ counts, int n_cells,
  uint64_t * __restrict__ partial)
{
  __shared__ uint64_t smem[2 * kEmBlock];
  uint64_t mass[kScanItems];
  const uint64_t incl = block_incl_scan(lane_masses(value, counts, n_cells, mass), smem);
  if (threadIdx.x == kEmBlock - 1) partial[blockIdx.x] = incl;
}

// tile sums -> exclusive offsets, in place, by one workgroup
__global__ __launch_bounds__(kEmBlock) void error_cdf_offsets_kernel(
  uint64_t * __restrict__ partial, int n_tiles)
{
  __shared__ uint64_t smem[2 * kEmBlock];
  const int per = (n_tiles + kEmBlock - 1) / kEmBlock;  // <= 32
  const int first = (int)threadIdx.x * per;
  uint64_t sum = 0;
  for (int k = 0; k < per; k++)
    if (first + k < n_tiles) sum += partial[first + k];
  uint64_t run = block_incl_scan(sum, smem) - sum;  // exclusive
  for (int k = 0; k < per; k++) {
    if (first + k < n_tiles) {
      const uint64_t v = partial[first + k];
      partial[first + k] = run;
      run += v;
    }
  }
}

__global__ __launch_bounds__(kEmBlock) void error_cdf_write_kernel(
  const float * __restrict__ value, const int32_t * __restrict__ counts, int n_cells,
  const uint64_t * __restrict__ partial, uint64_t * __restrict__ cdf)
{
  __shared__ uint64_t smem[2 * kEmBlock];
  uint64_t mass[kScanItems];
  const uint64_t sum = lane_masses(value, counts, n_cells, mass);
  uint64_t run = partial[blockIdx.x] + (block_incl_scan(sum, smem) - sum);
  const int64_t first = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
#pragma unroll
  for (int k = 0; k < kScanItems; k++) {
    run += mass[k];
    if (first + k < n_cells) cdf[first + k] = run;
  }
}

__global__ __launch_bounds__(kEmBlock) void draw_pixels_guided_kernel(
  const uint32_t * __restrict__ bits, const float * __restrict__ value,
  const uint64_t * __restrict__ cdf, const int64_t * __restrict__ n_valid, int E, int h, int w,
  int gh, int gw, uint32_t seed_lo, uint32_t seed_hi, int attempts, uint64_t T,
  int32_t * __restrict__ cam, int32_t * __restrict__ ij, int32_t * __restrict__ tries,
  float * __restrict__ ray_weight, int n)
{
  const int r = blockIdx.x * kEmBlock + threadIdx.x;
  if (r >= n) return;
  const int n_cells = E * gh * gw;
  const uint64_t total = cdf[n_cells - 1];
  const Philox4 x = philox4x32_10((uint32_t)r, 0u, 0u, 0u, seed_lo, seed_hi);
  uint32_t c = 0, i = 0, j = 0;
  int used = 0;
  if (total == 0ull || (uint64_t)x.x3 < T) {
    // the masked draw (pixel_mask.hip)
    for (int a = 0; a < attempts; a++) {
      const Philox4 y = philox4x32_10((uint32_t)r, (uint32_t)a, 0u, 0u, seed_lo, seed_hi);
      c = __umulhi(y.x0, (uint32_t)E);  // < E
      i = __umulhi(y.x1, (uint32_t)h);  // < h
      j = __umulhi(y.x2, (uint32_t)w);  // < w: g < E*h*w, inside the words
      if (pixel_valid(bits, ((int64_t)c * h + i) * w + j)) {
        used = a + 1;
        break;
      }
    }
  } else {
    const uint64_t t = __umul64hi(((uint64_t)x.x0 << 32) | (uint64_t)x.x1, total);  // < total
    int lo = 0, hi = n_cells - 1;  // the answer lies in [lo, hi]: cdf[n_cells - 1] = total > t
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (cdf[mid] > t)
        hi = mid;
      else
        lo = mid + 1;
    }
    const int b = lo % gw, a_row = (lo / gw) % gh;
    c = (uint32_t)(lo / (gw * gh));  // < E
    const int i0 = cell_first(a_row, h, gh), rows = cell_first(a_row + 1, h, gh) - i0;
    const int j0 = cell_first(b, w, gw), cols = cell_first(b + 1, w, gw) - j0;
    for (int a = 0; a < attempts; a++) {
      const Philox4 y = philox4x32_10((uint32_t)r, (uint32_t)a, 1u, 0u, seed_lo, seed_hi);
      i = (uint32_t)i0 + __umulhi(y.x0, (uint32_t)rows);  // < i0 + rows <= h
      j = (uint32_t)j0 + __umulhi(y.x1, (uint32_t)cols);  // < j0 + cols <= w
      if (pixel_valid(bits, ((int64_t)c * h + i) * w + j)) {
        used = a + 1;
        break;
      }
    }
  }
  cam[r] = (int32_t)c;
  ij[2 * r] = (int32_t)i;
  ij[2 * r + 1] = (int32_t)j;
  tries[r] = used;
  float weight = 0.f;
  if (used > 0) {
    weight = 1.f;
    if (total != 0ull) {
      const int cell = ((int)c * gh + cell_of((int)i, h, gh)) * gw + cell_of((int)j, w, gw);
      const double u = (double)T * (1.0 / 4294967296.0);
      const double den =
        (((1.0 - u) * (double)quant_value(value[cell])) * (double)n_valid[0]) / (double)total + u;
      weight = (float)(1.0 / den);
    }
  }
  ray_weight[r] = weight;
}

// the limits of the GEOMETRY paragraph, without overflow on the way
inline bool grid_ok(int E, int h, int w, int gh, int gw)
{
  if (E <= 0 || h <= 0 || w <= 0 || gh < 1 || gw < 1 || gh > h || gw > w) return false;
  if ((int64_t)h * w >= kMaxImagePixels) return false;
  const int64_t per_image = (int64_t)gh * gw;  // <= h*w < 2^31
  if (per_image >= kMaxCells || (int64_t)E > (kMaxCells - 1) / per_image) return false;
  return (int64_t)E * ((int64_t)h * w) < kMaxMaskPixels;  // E < 2^24, h*w < 2^31: no overflow
}

inline bool unit_ok(float x) { return x >= 0.f && x <= 1.f; }  // false for NaN

}  // namespace

extern "C" int f2n_mask_cell_counts(
  const uint32_t * bits, int E, int h, int w, int gh, int gw, int32_t * counts, void * stream)
{
  if (!counts || !grid_ok(E, h, w, gh, gw)) return F2N_E_INVALID_ARG;
  const int n_cells = E * gh * gw;
  hipLaunchKernelGGL(
    mask_cell_counts_kernel, dim3(f2n_div_up(n_cells, kEmBlock / 64)), dim3(kEmBlock), 0,
    (hipStream_t)stream, bits, h, w, gh, gw, n_cells, counts);
  return f2n_launch_status();
}

extern "C" int f2n_error_map_accum(
  const float * colors, const float * gt, const float * alpha, const float * bg,
  const float * ray_weight, const int32_t * cam, const int32_t * ij, int n, int E, int h, int w,
  int gh, int gw, uint64_t * acc_sum, uint32_t * acc_cnt, void * stream)
{
  if (!colors || !gt || !cam || !ij || !acc_sum || !acc_cnt || n < 0 || !grid_ok(E, h, w, gh, gw))
    return F2N_E_INVALID_ARG;
  if (alpha && !bg) return F2N_E_INVALID_ARG;
  if (n == 0) return F2N_OK;
  hipLaunchKernelGGL(
    error_map_accum_kernel, dim3(f2n_div_up(n, kEmBlock)), dim3(kEmBlock), 0, (hipStream_t)stream,
    colors, gt, alpha, bg, ray_weight, cam, ij, n, E, h, w, gh, gw, (unsigned long long *)acc_sum,
    acc_cnt);
  return f2n_launch_status();
}

extern "C" int f2n_error_map_apply(
  float * value, uint64_t * acc_sum, uint32_t * acc_cnt, int n_cells, float decay, void * stream)
{
  if (!value || !acc_sum || !acc_cnt || n_cells < 1 || n_cells >= kMaxCells || !unit_ok(decay))
    return F2N_E_INVALID_ARG;
  hipLaunchKernelGGL(
    error_map_apply_kernel, dim3(f2n_div_up(n_cells, kEmBlock)), dim3(kEmBlock), 0,
    (hipStream_t)stream, value, (unsigned long long *)acc_sum, acc_cnt, n_cells, decay);
  return f2n_launch_status();
}

extern "C" int64_t f2n_error_cdf_workspace_words(int n_cells)
{
  if (n_cells < 1 || n_cells >= kMaxCells) return 0;
  return (n_cells + kScanTile - 1) / kScanTile;
}

extern "C" int f2n_error_cdf(
  const float * value, const int32_t * counts, int n_cells, uint64_t * cdf, uint64_t * partial,
  void * stream)
{
  if (!value || !counts || !cdf || !partial || n_cells < 1 || n_cells >= kMaxCells)
    return F2N_E_INVALID_ARG;
  const int n_tiles = (n_cells + kScanTile - 1) / kScanTile;  // <= 8192
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(
    error_cdf_tile_sums_kernel, dim3(n_tiles), dim3(kEmBlock), 0, s, value, counts, n_cells, partial);
  hipLaunchKernelGGL(error_cdf_offsets_kernel, dim3(1), dim3(kEmBlock), 0, s, partial, n_tiles);
  hipLaunchKernelGGL(
    error_cdf_write_kernel, dim3(n_tiles), dim3(kEmBlock), 0, s, value, counts, n_cells, partial, cdf);
  return f2n_launch_status();
}

extern "C" int f2n_draw_pixels_guided(
  const uint32_t * bits, const int32_t * counts, const float * value, const uint64_t * cdf,
  const int64_t * n_valid, int E, int h, int w, int gh, int gw, uint32_t seed_lo, uint32_t seed_hi,
  int attempts, float uniform_fraction, int32_t * cam, int32_t * ij, int32_t * tries,
  float * ray_weight, int n, void * stream)
{
  if (!counts || !value || !cdf || !n_valid || !cam || !ij || !tries || !ray_weight || n < 0 ||
      !grid_ok(E, h, w, gh, gw) || attempts < 1 || attempts > 64 ||
      !unit_ok(uniform_fraction))
    return F2N_E_INVALID_ARG;
  if (n == 0) return F2N_OK;
  const uint64_t T = (uint64_t)llrint((double)uniform_fraction * 4294967296.0);  // 0 .. 2^32
  hipLaunchKernelGGL(
    draw_pixels_guided_kernel, dim3(f2n_div_up(n, kEmBlock)), dim3(kEmBlock), 0, (hipStream_t)stream,
    bits, value, cdf, n_valid, E, h, w, gh, gw, seed_lo, seed_hi, attempts, T, cam, ij, tries,
    ray_weight, n);
  return f2n_launch_status();
}
