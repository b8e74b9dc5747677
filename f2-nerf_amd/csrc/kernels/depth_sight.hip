// depth_sight.hip -- the per-ray line-of-sight losses of depth supervision (include/f2nerf_hip.h has
// the definition; Urban Radiance Fields, Rematas et al., CVPR 2022, section 4.2).  The reference has
// no such kernel: these stand beside WeightVar / WeightDist (segment_ops.hip) and follow their per-ray
// convention: one 64-lane wavefront per ray (ray_of_wave), lanes take 64 consecutive kept samples and
// walk the ray in strides of 64.  No atomics, no LDS, no scratch: the same bits on every run.
//
// EVALUATION ORDER (tests/depth_sight_model.py counts its bound from these lines; the library is
// built with -ffp-contract=off, so only the fmaf spelled out below are fused):
//   per ray      lo = z - eps, hi = z + eps                       one rounding each
//   per sample   m  = t - 0.5f * dt                               0.5f * dt is exact: one rounding
//                front = m < lo,  band = m >= lo && m <= hi       on those f32 values
//   per lane, strides in ascending order (sample s + lane, s + lane + 64, ...):
//                e = front ? fmaf(w, w, e) : e                    FMA: the product is not rounded
//                b = band  ? b + w         : b                    plain add
//                d = fmaf(w, m, d)                                FMA, every sample
//   after the strided loop has reconverged, all 64 lanes on (a lane that had no sample holds 0):
//                E = wave_sum(e), W = wave_sum(b), D = wave_sum(d)   (DPP scan tree of common.hiph)
//   forward      a = 1.f - W,  x = D - z,  out = (E, a * a, x * x)
//   backward     W, D, a, x exactly as the forward forms them (the same loop: the same bits), then
//                c0 = 2.f * g0 (exact),  c1 = g1 * (2.f * a),  c2 = g2 * (2.f * x)   one rounding each
//                base = front ? c0 * w : band ? -c1 : 0.f
//                dw   = fmaf(c2, m, base)                         FMA
// A ray is valid iff z is finite and > 0.  An invalid ray reads no sample: out = (0, 0, 0) and zeros
// over its own range of dw.  Nothing is written outside the ranges.
#include "common.hiph"

namespace
{

__device__ __forceinline__ int ray_of_wave()
{
  return (int)blockIdx.x * F2N_WAVES_PER_BLOCK + (int)(threadIdx.x >> 6);
}

__device__ __forceinline__ bool target_valid(float z) { return z > 0.f && z < __builtin_inff(); }

// The ray's three sums as every lane holds them after the reduction.
struct SightSums
{
  float E, W, D;
};

__device__ __forceinline__ SightSums sight_sums(
  const float * __restrict__ w, const float * __restrict__ t, const float * __restrict__ dt, int s,
  int e, int lane, float lo, float hi)
{
  float ef = 0.f, wb = 0.f, d = 0.f;
  for (int i = s + lane; i < e; i += F2N_WAVE) {
    const float wi = w[i];
    const float m = t[i] - 0.5f * dt[i];
    const bool front = m < lo;
    const bool band = m >= lo && m <= hi;
    ef = front ? fmaf(wi, wi, ef) : ef;
    wb = band ? wb + wi : wb;
    d = fmaf(wi, m, d);
  }
  // (the loop has reconverged: every lane takes part in the scans)
  SightSums r;
  r.E = wave_sum(ef);
  r.W = wave_sum(wb);
  r.D = wave_sum(d);
  return r;
}

__global__ __launch_bounds__(F2N_BLOCK) void depth_sight_fwd_kernel(
  const float * __restrict__ w, const float * __restrict__ t, const float * __restrict__ dt,
  const int32_t * __restrict__ idx, const float * __restrict__ z, float eps,
  float * __restrict__ out, int n_rays)
{
  const int r = ray_of_wave();
  if (r >= n_rays) return;
  const int lane = lane_id();
  const float zr = z[r];
  float * o = out + 3 * (int64_t)r;
  if (!target_valid(zr)) {
    if (lane < 3) o[lane] = 0.f;
    return;
  }
  const int s = idx[2 * r], e = idx[2 * r + 1];
  const SightSums sum = sight_sums(w, t, dt, s, e, lane, zr - eps, zr + eps);
  const float a = 1.f - sum.W, x = sum.D - zr;
  if (lane == 0) {
    o[0] = sum.E;
    o[1] = a * a;
    o[2] = x * x;
  }
}

__global__ __launch_bounds__(F2N_BLOCK) void depth_sight_bwd_kernel(
  const float * __restrict__ w, const float * __restrict__ t, const float * __restrict__ dt,
  const int32_t * __restrict__ idx, const float * __restrict__ z, float eps,
  const float * __restrict__ d_out, float * __restrict__ dw, int n_rays)
{
  const int r = ray_of_wave();
  if (r >= n_rays) return;
  const int lane = lane_id();
  const int s = idx[2 * r], e = idx[2 * r + 1];
  const float zr = z[r];
  if (!target_valid(zr)) {
    for (int i = s + lane; i < e; i += F2N_WAVE) dw[i] = 0.f;
    return;
  }
  const float lo = zr - eps, hi = zr + eps;
  const SightSums sum = sight_sums(w, t, dt, s, e, lane, lo, hi);
  const float a = 1.f - sum.W, x = sum.D - zr;
  const float * g = d_out + 3 * (int64_t)r;
  const float c0 = 2.f * g[0], c1 = g[1] * (2.f * a), c2 = g[2] * (2.f * x);
  for (int i = s + lane; i < e; i += F2N_WAVE) {
    const float wi = w[i];
    const float m = t[i] - 0.5f * dt[i];
    const bool front = m < lo;
    const bool band = m >= lo && m <= hi;
    const float base = front ? c0 * wi : band ? -c1 : 0.f;
    dw[i] = fmaf(c2, m, base);
  }
}

inline dim3 ray_grid(int n_rays) { return dim3(f2n_div_up(n_rays, F2N_WAVES_PER_BLOCK)); }

// finite and >= 0 (false for NaN)
inline bool eps_ok(float eps) { return eps >= 0.f && eps < __builtin_inff(); }

}  // namespace

extern "C" int f2n_depth_sight_fwd(
  const float * weights, const float * t, const float * dt, const int32_t * idx, const float * z,
  float eps, float * out, int n_rays, void * stream)
{
  if (!idx || !z || !out || n_rays < 0 || !eps_ok(eps)) return F2N_E_INVALID_ARG;
  if (n_rays == 0) return F2N_OK;
  hipLaunchKernelGGL(
    depth_sight_fwd_kernel, ray_grid(n_rays), dim3(F2N_BLOCK), 0, (hipStream_t)stream, weights, t,
    dt, idx, z, eps, out, n_rays);
  return f2n_launch_status();
}

extern "C" int f2n_depth_sight_bwd(
  const float * weights, const float * t, const float * dt, const int32_t * idx, const float * z,
  float eps, const float * d_out, float * dw, int n_rays, void * stream)
{
  if (!idx || !z || !d_out || !dw || n_rays < 0 || !eps_ok(eps)) return F2N_E_INVALID_ARG;
  if (n_rays == 0) return F2N_OK;
  hipLaunchKernelGGL(
    depth_sight_bwd_kernel, ray_grid(n_rays), dim3(F2N_BLOCK), 0, (hipStream_t)stream, weights, t,
    dt, idx, z, eps, d_out, dw, n_rays);
  return f2n_launch_status();
}
