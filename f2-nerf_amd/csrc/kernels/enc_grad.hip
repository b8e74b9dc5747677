// enc_grad.hip -- the hash encoding's true derivative with respect to position, as a vector-Jacobian
// product with the gradient of the encoding: what a camera fitted through the render needs of the
// field (density_grad.hiph holds the per-level arithmetic and its evaluation order).
//
// The function differentiated is the trilinear interpolant the forward computes (reference
// src/hash_3d_anchored.cu:25-93), enc[p, lF + k] = sum_d w_d(frac_l) f_{l,d,k}, so with g = d(loss)/d(enc)
//   G[p] = sum_l mul_l * sum_pairs (s_hi - s_lo) * w_pair,   s_d = sum_k g[p, lF + k] f_{l,d,k},
// all three axes' interpolation weights in place.  This is NOT quirk Q5 (src/hash_3d_anchored.cu:138-143,
// the corner features signed by the corner bit and rounded through f16), which f2n_hash_bwd's pts_grad
// and f2n_hash_rays_grad keep for parity; the entries here replace that form where a caller asks for
// the derivative itself.
//
//   f2n_hash_pts_grad_exact   one lane per point (f2n_density_grad's shape): pts_grad [n,3] at the
//                             CONTRACTED point, no contraction Jacobian.
//   f2n_hash_rays_grad_exact  one wavefront per ray (hash_rays_grad_kernel's shape): 64-sample strides
//                             over the ray's segment, the level loop in registers, the contraction's
//                             Jacobian as density_grad_point spells it, d o += dp, m = fmaf(t, dp, m),
//                             DPP wave sums, the lane-0 epilogue d d = (m - n (n.m)) / |d|.
//
// Both are density_grad_level<F, POW2> with the sample's own g[p, lF .. lF+F) -- unscaled f32, no f16
// rounding, no grad_scale -- where f2n_density_grad passes the uniform row w0[lF .. lF+F).  No
// atomics, no workspace, nothing read back: the same bits on every run.
#include "density_grad.hiph"

namespace
{

// sum over the levels, in level order, the first onto 0, of the level terms at the contracted point
// (x, y, z) with the weights g[(lF + k) * g_ld_chan]
template <int F, bool POW2>
__device__ __forceinline__ void enc_grad_levels(
  float x, float y, float z, const uint16_t * __restrict__ table,
  const int32_t * __restrict__ primes, const float * __restrict__ bias,
  const float * __restrict__ mul, const float * __restrict__ g, int64_t g_ld_chan, int L, uint32_t T,
  int64_t level_stride, float & gx, float & gy, float & gz)
{
  gx = gy = gz = 0.f;
#pragma unroll 1
  for (int l = 0; l < L; l++) {
    const LevelParams lp = load_level(primes, bias, mul, l);
    const float * gl = g + (int64_t)(l * F) * g_ld_chan;
    float gk[F];
#pragma unroll
    for (int k = 0; k < F; k++) gk[k] = gl[k * g_ld_chan];
    density_grad_level<F, POW2>(x, y, z, lp, T, table + level_stride * l, gk, gx, gy, gz);
  }
}

template <int F, bool POW2>
__global__ __launch_bounds__(F2N_BLOCK) void hash_pts_grad_exact_kernel(
  const float * __restrict__ pts, const uint16_t * __restrict__ table,
  const int32_t * __restrict__ primes, const float * __restrict__ bias,
  const float * __restrict__ mul, const float * __restrict__ grad_out, int64_t g_ld_point,
  int64_t g_ld_chan, float * __restrict__ pts_grad, int64_t n, int L, uint32_t T,
  int64_t level_stride)
{
  const int64_t i = (int64_t)blockIdx.x * F2N_BLOCK + threadIdx.x;
  if (i >= n) return;
  float gx, gy, gz;
  enc_grad_levels<F, POW2>(
    pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], table, primes, bias, mul,
    grad_out + i * g_ld_point, g_ld_chan, L, T, level_stride, gx, gy, gz);
  pts_grad[3 * i] = gx;
  pts_grad[3 * i + 1] = gy;
  pts_grad[3 * i + 2] = gz;
}

template <int F, bool POW2>
__global__ __launch_bounds__(F2N_BLOCK) void hash_rays_grad_exact_kernel(
  const float * __restrict__ pts, const float * __restrict__ t, const int32_t * __restrict__ bounds,
  const float * __restrict__ rays_d, const uint16_t * __restrict__ table,
  const int32_t * __restrict__ primes, const float * __restrict__ bias,
  const float * __restrict__ mul, const float * __restrict__ grad_out, int64_t g_ld_point,
  int64_t g_ld_chan, float * __restrict__ d_rays_o, float * __restrict__ d_rays_d, int n_rays,
  int L, uint32_t T, int64_t level_stride)
{
  const int r = (int)blockIdx.x * F2N_WAVES_PER_BLOCK + (int)(threadIdx.x >> 6);
  if (r >= n_rays) return;  // wave-uniform
  const int lane = lane_id();
  const int s = bounds[2 * r], e = bounds[2 * r + 1];
  float ox = 0.f, oy = 0.f, oz = 0.f;  // sum dp
  float mx = 0.f, my = 0.f, mz = 0.f;  // sum t * dp
  for (int c = s; c < e; c += F2N_WAVE) {
    const int64_t i = (int64_t)c + lane;
    if (i >= e) continue;
    const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    const float ti = t[i];
    float x = px, y = py, z = pz;
    contract_point(x, y, z);
    float gx, gy, gz;  // gradient at the contracted point
    enc_grad_levels<F, POW2>(
      x, y, z, table, primes, bias, mul, grad_out + i * g_ld_point, g_ld_chan, L, T, level_stride,
      gx, gy, gz);
    // the contraction's Jacobian, as density_grad_point spells it
    const float n2 = fmaf(pz, pz, fmaf(py, py, px * px));
    const float nrm = sqrtf(n2);
    float dx, dy, dz;
    if (nrm <= 1.f) {
      const float poison = (nrm == 0.f) ? __builtin_nanf("") : 0.f;
      dx = gx + poison;
      dy = gy + poison;
      dz = gz + poison;
    } else {
      const float inv = 1.f / nrm;
      const float ja = (2.f - inv) * inv;
      const float da_over_n = (2.f * inv - 2.f) * inv * inv * inv;
      const float pg = fmaf(pz, gz, fmaf(py, gy, px * gx));
      const float cc = da_over_n * pg;
      dx = fmaf(cc, px, ja * gx);
      dy = fmaf(cc, py, ja * gy);
      dz = fmaf(cc, pz, ja * gz);
    }
    // pts = o + n * t: d o += dp, d n += t dp
    ox += dx;
    oy += dy;
    oz += dz;
    mx = fmaf(ti, dx, mx);
    my = fmaf(ti, dy, my);
    mz = fmaf(ti, dz, mz);
  }
  ox = wave_sum(ox);
  oy = wave_sum(oy);
  oz = wave_sum(oz);
  mx = wave_sum(mx);
  my = wave_sum(my);
  mz = wave_sum(mz);
  if (lane == 0) {
    // n = d/|d| as the sampler forms it (sampler.hip load_ray); d d = (m - n (n.m)) / |d|
    const float qx = rays_d[3 * r], qy = rays_d[3 * r + 1], qz = rays_d[3 * r + 2];
    const float dn = sqrtf(fmaf(qz, qz, fmaf(qy, qy, qx * qx)));
    const float nx = qx / dn, ny = qy / dn, nz = qz / dn;
    const float nm = fmaf(nz, mz, fmaf(ny, my, nx * mx));
    d_rays_o[3 * r] = ox;
    d_rays_o[3 * r + 1] = oy;
    d_rays_o[3 * r + 2] = oz;
    d_rays_d[3 * r] = (mx - nx * nm) / dn;
    d_rays_d[3 * r + 1] = (my - ny * nm) / dn;
    d_rays_d[3 * r + 2] = (mz - nz * nm) / dn;
  }
}

}  // namespace

// Checks in f2n_hash_bwd's order: pointers, counts, F, the rest of the field, the table's alignment.
extern "C" int f2n_hash_pts_grad_exact(
  const float * pts, const uint16_t * table_f16, const int32_t * primes, const float * bias,
  const float * mul, const float * grad_out, int64_t g_ld_point, int64_t g_ld_chan,
  float * pts_grad, int64_t n, int L, int F, uint32_t T, int64_t level_stride, void * stream)
{
  if (!pts || !table_f16 || !primes || !bias || !mul || !grad_out || !pts_grad)
    return F2N_E_INVALID_ARG;
  if (n < 0 || g_ld_point < 0 || g_ld_chan < 0) return F2N_E_INVALID_ARG;
  if (F != 1 && F != 2 && F != 4 && F != 8) return F2N_E_UNSUPPORTED;
  if (!f2n_hash_args_ok(n, L, F, T, level_stride)) return F2N_E_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(table_f16) % (2u * F)) return F2N_E_INVALID_ARG;
  if (n > (int64_t)0x7fffffff * F2N_BLOCK) return F2N_E_INVALID_ARG;  // the grid's x extent
  if (n == 0) return F2N_OK;
  const dim3 grid(f2n_div_up(n, F2N_BLOCK)), block(F2N_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  f2n_dispatch_field(F, T, [&](auto ff, auto p2) {
    hipLaunchKernelGGL(
      (hash_pts_grad_exact_kernel<decltype(ff)::value, decltype(p2)::value>), grid, block, 0, s,
      pts, table_f16, primes, bias, mul, grad_out, g_ld_point, g_ld_chan, pts_grad, n, L, T,
      level_stride);
  });
  return f2n_launch_status();
}

// Checks in f2n_hash_rays_grad's order.
extern "C" int f2n_hash_rays_grad_exact(
  const float * pts, const float * t, const int32_t * bounds, const float * rays_d,
  const uint16_t * table_f16, const int32_t * primes, const float * bias, const float * mul,
  const float * grad_out, int64_t g_ld_point, int64_t g_ld_chan, float * d_rays_o,
  float * d_rays_d, int n_rays, int L, int F, uint32_t T, int64_t level_stride, void * stream)
{
  if (!pts || !t || !bounds || !rays_d || !table_f16 || !primes || !bias || !mul || !grad_out ||
      !d_rays_o || !d_rays_d)
    return F2N_E_INVALID_ARG;
  if (n_rays < 0 || g_ld_point < 0 || g_ld_chan < 0) return F2N_E_INVALID_ARG;
  if (F != 1 && F != 2 && F != 4 && F != 8) return F2N_E_UNSUPPORTED;
  if (!f2n_hash_args_ok(0, L, F, T, level_stride)) return F2N_E_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(table_f16) % (2u * F)) return F2N_E_INVALID_ARG;
  if (n_rays == 0) return F2N_OK;
  const dim3 grid(f2n_div_up(n_rays, F2N_WAVES_PER_BLOCK)), block(F2N_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  f2n_dispatch_field(F, T, [&](auto ff, auto p2) {
    hipLaunchKernelGGL(
      (hash_rays_grad_exact_kernel<decltype(ff)::value, decltype(p2)::value>), grid, block, 0, s,
      pts, t, bounds, rays_d, table_f16, primes, bias, mul, grad_out, g_ld_point, g_ld_chan,
      d_rays_o, d_rays_d, n_rays, L, T, level_stride);
  });
  return f2n_launch_status();
}
