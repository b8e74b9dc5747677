// ray_order.hip -- pixel-compact ray bundles for the dense first pass (Renderer::render_fused).
//
// The hash-grid gather of f2n_hash_fwd_raytile costs what the number of distinct 128-byte table
// lines per wave instruction costs, and that number depends only on how close together the 64 rays
// of a tile are.  A chunk handed over row by row makes each tile a 64x1 pixel strip; sorted by the
// key below, the same rays form compact blobs of about 10x11 pixels (the mean bounding box over
// the benchmark's views).
//
// Key: the ray direction projected on the face of the unit cube it points through (gnomonic
// projection: pixel rows and columns of a camera stay straight lines, nearly axis-aligned for an
// upright camera), each face coordinate quantised to 14 bits, the pair ordered along a Hilbert
// curve (consecutive cells are neighbours: a run of 64 rays is one connected blob, where a Morton
// order jumps); face id in bits 28-30.  One thread per ray, no reduction over the chunk: the key of
// a ray depends on its direction alone.  Rays of one view share their origin, so direction is what
// decides neighbourhood; a random batch has no locality to find and only pays for the sort.
//
// Sort: the host sorts the keys stably (at::sort), so ties keep the caller's order and the
// permutation is a deterministic function of the directions.
#include "common.hiph"

namespace
{

constexpr int kCellBits = 14;

__device__ __forceinline__ uint32_t hilbert_index(uint32_t x, uint32_t y)
{
  uint32_t d = 0;
#pragma unroll
  for (uint32_t s = 1u << (kCellBits - 1); s > 0; s >>= 1) {
    const uint32_t rx = (x & s) ? 1u : 0u;
    const uint32_t ry = (y & s) ? 1u : 0u;
    d += s * s * ((3u * rx) ^ ry);
    if (ry == 0) {
      if (rx == 1) {  // reflect; later steps read only the bits below s
        x ^= s - 1;
        y ^= s - 1;
      }
      const uint32_t t = x;
      x = y;
      y = t;
    }
  }
  return d;
}

__device__ __forceinline__ uint32_t quantise(float u)
{
  const float q = fminf(fmaxf((u * .5f + .5f) * (float)(1u << kCellBits), 0.f),
                        (float)((1u << kCellBits) - 1));
  return (uint32_t)q;
}

__global__ __launch_bounds__(F2N_BLOCK) void ray_key_kernel(
  const float * __restrict__ rays_d, int32_t * __restrict__ keys, int n)
{
  const int r = blockIdx.x * F2N_BLOCK + threadIdx.x;
  if (r >= n) return;
  const float d[3] = {rays_d[3 * r], rays_d[3 * r + 1], rays_d[3 * r + 2]};
  const float a[3] = {fabsf(d[0]), fabsf(d[1]), fabsf(d[2])};
  const int ax = (a[0] >= a[1] && a[0] >= a[2]) ? 0 : (a[1] >= a[2] ? 1 : 2);
  const float m = a[ax];
  uint32_t key = 0;
  // zero, infinite or NaN directions: key 0 (the order is a hint).  A NaN loses every >=, so it is
  // never the component picked above: (NaN, 1, 0) has m = 1, and the sum is what sees it.
  const float all3 = a[0] + a[1] + a[2];  // NaN exactly when a component is
  if (m > 0.f && m <= 3.4e38f && all3 == all3) {
    const float u = d[(ax + 1) % 3] / m, v = d[(ax + 2) % 3] / m;
    const uint32_t face = 2u * (uint32_t)ax + (d[ax] < 0.f ? 1u : 0u);
    key = (face << (2 * kCellBits)) | hilbert_index(quantise(u), quantise(v));
  }
  keys[r] = (int32_t)key;  // < 6 * 2^28: non-negative
}

// Per ray j of the bucketed order: its inputs from caller ray order[j]; perm[j] = order[j] as int32,
// inv[order[j]] = j.
__global__ __launch_bounds__(F2N_BLOCK) void ray_permute_kernel(
  const int64_t * __restrict__ order, int32_t * __restrict__ perm, const float * __restrict__ rays_o,
  const float * __restrict__ rays_d, const int32_t * __restrict__ emb, const float * __restrict__ bg,
  float * __restrict__ rays_o_p, float * __restrict__ rays_d_p, int32_t * __restrict__ emb_p,
  float * __restrict__ bg_p, int32_t * __restrict__ inv, int n)
{
  const int j = blockIdx.x * F2N_BLOCK + threadIdx.x;
  if (j >= n) return;
  const int r = (int)order[j];
  perm[j] = r;
  inv[r] = j;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    rays_o_p[3 * j + a] = rays_o[3 * r + a];
    rays_d_p[3 * j + a] = rays_d[3 * r + a];
    if (bg) bg_p[3 * j + a] = bg[3 * r + a];
  }
  if (emb) emb_p[j] = emb[r];
}

// dst row i = src row map[i]; one thread per 16-byte (or 4-byte) word of the destination.
template <typename W>
__global__ __launch_bounds__(F2N_BLOCK) void gather_rows_kernel(
  const W * __restrict__ src, W * __restrict__ dst, const int32_t * __restrict__ map, int n,
  int row_words)
{
  const int64_t e = (int64_t)blockIdx.x * F2N_BLOCK + threadIdx.x;
  if (e >= (int64_t)n * row_words) return;
  const int i = (int)(e / row_words), w = (int)(e - (int64_t)i * row_words);
  dst[e] = src[(int64_t)map[i] * row_words + w];
}

// dst segment of ray i = src segment of ray map[i] (equal lengths); one wavefront per ray.
__global__ __launch_bounds__(F2N_BLOCK) void gather_segments_kernel(
  const float * __restrict__ src, const int32_t * __restrict__ src_bounds, float * __restrict__ dst,
  const int32_t * __restrict__ dst_bounds, const int32_t * __restrict__ map, int n_rays)
{
  const int i = blockIdx.x * F2N_WAVES_PER_BLOCK + threadIdx.x / F2N_WAVE;
  if (i >= n_rays) return;
  const int lane = threadIdx.x % F2N_WAVE;
  const int j = map[i];
  const int s0 = src_bounds[2 * j], d0 = dst_bounds[2 * i];
  const int len = dst_bounds[2 * i + 1] - d0;
  for (int k = lane; k < len; k += F2N_WAVE) dst[d0 + k] = src[s0 + k];
}

__global__ __launch_bounds__(F2N_BLOCK) void counts_through_kernel(
  const int32_t * __restrict__ bounds, const int32_t * __restrict__ map, int32_t * __restrict__ counts,
  int n)
{
  const int i = blockIdx.x * F2N_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int j = map[i];
  counts[i] = bounds[2 * j + 1] - bounds[2 * j];
}

}  // namespace

extern "C" int f2n_ray_keys(const float * rays_d, int32_t * keys, int n, void * stream)
{
  if (!rays_d || !keys || n < 0) return F2N_E_INVALID_ARG;
  if (n == 0) return F2N_OK;
  hipLaunchKernelGGL(
    ray_key_kernel, dim3(f2n_div_up(n, F2N_BLOCK)), dim3(F2N_BLOCK), 0, (hipStream_t)stream, rays_d,
    keys, n);
  return f2n_launch_status();
}

extern "C" int f2n_ray_permute(
  const int64_t * order, int n, int S, const float * rays_o, const float * rays_d,
  const int32_t * emb_idx, const float * bg, const float * noise, int32_t * perm, float * rays_o_p,
  float * rays_d_p, int32_t * emb_idx_p, float * bg_p, float * noise_p, int32_t * inv,
  void * stream)
{
  if (!order || !perm || !rays_o || !rays_d || !rays_o_p || !rays_d_p || !inv || n < 0 || S <= 0)
    return F2N_E_INVALID_ARG;
  if ((emb_idx && !emb_idx_p) || (bg && !bg_p) || (noise && !noise_p)) return F2N_E_INVALID_ARG;
  if (n == 0) return F2N_OK;
  hipLaunchKernelGGL(
    ray_permute_kernel, dim3(f2n_div_up(n, F2N_BLOCK)), dim3(F2N_BLOCK), 0, (hipStream_t)stream,
    order, perm, rays_o, rays_d, emb_idx, bg, rays_o_p, rays_d_p, emb_idx_p, bg_p, inv, n);
  if (f2n_launch_status() != F2N_OK) return F2N_E_LAUNCH;
  if (noise) return f2n_gather_rows(noise, noise_p, perm, n, S, stream);
  return F2N_OK;
}

extern "C" int f2n_gather_rows(
  const float * src, float * dst, const int32_t * map, int n, int row_floats, void * stream)
{
  if (!src || !dst || !map || n < 0 || row_floats <= 0) return F2N_E_INVALID_ARG;
  if (n == 0) return F2N_OK;
  const bool vec = row_floats % 4 == 0 && (reinterpret_cast<uintptr_t>(src) % 16) == 0 &&
                   (reinterpret_cast<uintptr_t>(dst) % 16) == 0;
  if (vec) {
    const int w = row_floats / 4;
    hipLaunchKernelGGL(
      gather_rows_kernel<float4>, dim3(f2n_div_up((int64_t)n * w, F2N_BLOCK)), dim3(F2N_BLOCK), 0,
      (hipStream_t)stream, reinterpret_cast<const float4 *>(src), reinterpret_cast<float4 *>(dst),
      map, n, w);
  } else {
    hipLaunchKernelGGL(
      gather_rows_kernel<float>, dim3(f2n_div_up((int64_t)n * row_floats, F2N_BLOCK)),
      dim3(F2N_BLOCK), 0, (hipStream_t)stream, src, dst, map, n, row_floats);
  }
  return f2n_launch_status();
}

extern "C" int f2n_gather_segments(
  const float * src, const int32_t * src_bounds, float * dst, const int32_t * dst_bounds,
  const int32_t * map, int n_rays, void * stream)
{
  if (!src_bounds || !dst_bounds || !map || n_rays < 0) return F2N_E_INVALID_ARG;
  if (n_rays == 0) return F2N_OK;
  if (!src || !dst) return F2N_E_INVALID_ARG;
  hipLaunchKernelGGL(
    gather_segments_kernel, dim3(f2n_div_up(n_rays, F2N_WAVES_PER_BLOCK)), dim3(F2N_BLOCK), 0,
    (hipStream_t)stream, src, src_bounds, dst, dst_bounds, map, n_rays);
  return f2n_launch_status();
}

extern "C" int f2n_counts_through(
  const int32_t * bounds, const int32_t * map, int32_t * counts, int n_rays, void * stream)
{
  if (!bounds || !map || !counts || n_rays < 0) return F2N_E_INVALID_ARG;
  if (n_rays == 0) return F2N_OK;
  hipLaunchKernelGGL(
    counts_through_kernel, dim3(f2n_div_up(n_rays, F2N_BLOCK)), dim3(F2N_BLOCK), 0,
    (hipStream_t)stream, bounds, map, counts, n_rays);
  return f2n_launch_status();
}
