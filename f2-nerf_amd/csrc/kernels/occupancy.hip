// occupancy.hip -- maintenance and public lookup of the occupancy bitfield (occupancy.hiph).
//
// The reference fork stripped upstream's occupancy grid and left only its trace
// (src/main_functions/train_manager.cpp:102); the early-stop block of Renderer::render
// (src/renderer.cpp:58-90) therefore evaluates the field on every sample in front of the first
// surface.  The grid marks the cells of contracted space whose density has been seen above a
// threshold; the march (sampler.hip) encodes only samples that fall into such cells.
#include "occupancy.hiph"

namespace
{

// One thread per cell, x fastest: the 64 lanes of a wavefront are 64 consecutive bit indices, i.e.
// two whole words of the bitfield, which lanes 0 and 32 write from one ballot.  The density of the
// cell's probe point takes the gather, f16 rounding and level-ordered FMA chain of
// density_march_kernel (sampler.hip); the probe is a contracted-space point already.
template <int F, bool POW2>
__global__ __launch_bounds__(F2N_BLOCK) void occ_update_kernel(
  const uint16_t * __restrict__ table, const int32_t * __restrict__ primes,
  const float * __restrict__ bias, const float * __restrict__ mul, const float * __restrict__ w0,
  const float * __restrict__ b0, const float * __restrict__ probe_u, float * __restrict__ density,
  uint32_t * __restrict__ bits, int G, int log2_g, int L, uint32_t T, int64_t level_stride,
  float density_shift, float threshold, float decay)
{
  // (G^3 is a multiple of the block size: every thread owns a cell, no wave is partial)
  const uint32_t i = blockIdx.x * (uint32_t)F2N_BLOCK + threadIdx.x;
  const uint32_t cx = i & (uint32_t)(G - 1), cy = (i >> log2_g) & (uint32_t)(G - 1),
                 cz = i >> (2 * log2_g);
  float ux = 0.5f, uy = 0.5f, uz = 0.5f;
  if (probe_u) {
    ux = probe_u[3 * (int64_t)i];
    uy = probe_u[3 * (int64_t)i + 1];
    uz = probe_u[3 * (int64_t)i + 2];
  }
  const float cell = 4.f / (float)G;  // a power of two: the products below are exact
  const float x = ((float)cx + ux) * cell - 2.f;
  const float y = ((float)cy + uy) * cell - 2.f;
  const float z = ((float)cz + uz) * cell - 2.f;
  float logit = b0[0];
  for (int l = 0; l < L; l++) {
    const LevelParams lp = load_level(primes, bias, mul, l);
    uint32_t row[8];
    float w[8], acc[F];
    corner_rows_and_weights<POW2>(x, y, z, lp, T, row, w);
    gather_blend<F>(table + level_stride * l, row, w, acc);
#pragma unroll
    for (int k = 0; k < F; k++) logit = fmaf(round_f16(acc[k]), w0[l * F + k], logit);
  }
  const float sigma = expf(logit - density_shift);
  const float d = fmaxf(density[i] * decay, sigma);
  density[i] = d;
  const unsigned long long m = __ballot(d > threshold);
  const int lane = lane_id();
  if (lane == 0) bits[i >> 5] = (uint32_t)m;
  if (lane == 32) bits[i >> 5] = (uint32_t)(m >> 32);
}

__global__ __launch_bounds__(F2N_BLOCK) void occ_lookup_kernel(
  const float * __restrict__ pts, int64_t n, const uint32_t * __restrict__ bits, int G,
  uint8_t * __restrict__ out)
{
  const int64_t i = (int64_t)blockIdx.x * F2N_BLOCK + threadIdx.x;
  if (i >= n) return;
  out[i] = occ_test_point(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], bits, G) ? 1 : 0;
}

}  // namespace

extern "C" int f2n_occ_update(
  const uint16_t * table_f16, const int32_t * primes, const float * bias, const float * mul,
  const float * w0, const float * b0, const float * probe_u, float * density, uint32_t * bits, int G,
  int L, int F, uint32_t T, int64_t level_stride, float density_shift, float threshold, float decay,
  void * stream)
{
  if (!f2n_occ_res_ok(G) || L > F2N_MAX_LEVELS) return F2N_E_INVALID_ARG;
  if (const int st = f2n_field_args_status(L, F, T, level_stride)) return st;
  if (!table_f16 || !primes || !bias || !mul || !w0 || !b0 || !density || !bits)
    return F2N_E_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(table_f16) % (2u * F)) return F2N_E_INVALID_ARG;
  if (!(decay >= 0.f) || threshold != threshold) return F2N_E_INVALID_ARG;
  int log2_g = 0;
  while ((1 << log2_g) < G) log2_g++;
  const int64_t cells = (int64_t)G * G * G;
  const dim3 grid((unsigned)(cells / F2N_BLOCK)), block(F2N_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  f2n_dispatch_field(F, T, [&](auto ff, auto p2) {
    hipLaunchKernelGGL(
      (occ_update_kernel<decltype(ff)::value, decltype(p2)::value>), grid, block, 0, s, table_f16,
      primes, bias, mul, w0, b0, probe_u, density, bits, G, log2_g, L, T, level_stride,
      density_shift, threshold, decay);
  });
  return f2n_launch_status();
}

extern "C" int f2n_occ_lookup(
  const float * pts, int64_t n, const uint32_t * bits, int G, uint8_t * out, void * stream)
{
  if (n < 0 || !f2n_occ_res_ok(G)) return F2N_E_INVALID_ARG;
  if (n == 0) return F2N_OK;
  if (!pts || !bits || !out) return F2N_E_INVALID_ARG;
  hipLaunchKernelGGL(
    occ_lookup_kernel, dim3(f2n_div_up(n, F2N_BLOCK)), dim3(F2N_BLOCK), 0, (hipStream_t)stream, pts,
    n, bits, G, out);
  return f2n_launch_status();
}
