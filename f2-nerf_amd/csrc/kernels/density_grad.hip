// density_grad.hip -- the density logit's true spatial gradient and the per-ray normals composited
// from it (density_grad.hiph holds the arithmetic and its evaluation order).
//
//   f2n_density_grad  one lane per point: grad [n,3] = d(logit)/d(p) at the raw points.
//   f2n_ray_normals   one wavefront per ray (the composite kernels' shape): lanes walk the ray's
//                     segment of kept samples in 64-sample strides, every lane runs the whole level
//                     loop of its sample in registers, forms n^ = -g/|g| and accumulates
//                     fmaf(w, n^, acc); one DPP wave sum per component at the end, after the strided
//                     loop has reconverged, so every cross-lane move runs with all lanes on.  No
//                     atomics, no [n,3] buffer in between, a fixed summation order.
//
// Neither is the reference's point gradient (src/hash_3d_anchored.cu:138-143, quirk Q5).
#include "density_grad.hiph"

namespace
{

template <int F, bool POW2>
__global__ __launch_bounds__(F2N_BLOCK) void density_grad_kernel(
  const float * __restrict__ pts, const uint16_t * __restrict__ table,
  const int32_t * __restrict__ primes, const float * __restrict__ bias,
  const float * __restrict__ mul, const float * __restrict__ w0, float * __restrict__ grad,
  int64_t n, int L, uint32_t T, int64_t level_stride)
{
  const int64_t i = (int64_t)blockIdx.x * F2N_BLOCK + threadIdx.x;
  if (i >= n) return;
  float dx, dy, dz;
  density_grad_point<F, POW2>(
    pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], table, primes, bias, mul, w0, L, T, level_stride,
    dx, dy, dz);
  grad[3 * i] = dx;
  grad[3 * i + 1] = dy;
  grad[3 * i + 2] = dz;
}

template <int F, bool POW2>
__global__ __launch_bounds__(F2N_BLOCK) void ray_normals_kernel(
  const float * __restrict__ pts, const int32_t * __restrict__ bounds,
  const float * __restrict__ weights, const uint16_t * __restrict__ table,
  const int32_t * __restrict__ primes, const float * __restrict__ bias,
  const float * __restrict__ mul, const float * __restrict__ w0, float * __restrict__ normals,
  int n_rays, int L, uint32_t T, int64_t level_stride)
{
  const int r = (int)blockIdx.x * F2N_WAVES_PER_BLOCK + (int)(threadIdx.x >> 6);
  if (r >= n_rays) return;  // wave-uniform
  const int lane = lane_id();
  const int s = bounds[2 * r], e = bounds[2 * r + 1];
  float ax = 0.f, ay = 0.f, az = 0.f;  // sum w n^ of this lane's samples
  for (int c = s; c < e; c += F2N_WAVE) {
    const int64_t i = (int64_t)c + lane;
    if (i >= e) continue;
    float gx, gy, gz;
    density_grad_point<F, POW2>(
      pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], table, primes, bias, mul, w0, L, T, level_stride,
      gx, gy, gz);
    density_normal(gx, gy, gz);
    const float w = weights[i];
    ax = fmaf(w, gx, ax);
    ay = fmaf(w, gy, ay);
    az = fmaf(w, gz, az);
  }
  ax = wave_sum(ax);
  ay = wave_sum(ay);
  az = wave_sum(az);
  if (lane == 0) {
    normals[3 * r] = ax;
    normals[3 * r + 1] = ay;
    normals[3 * r + 2] = az;
  }
}

// What both entries check of the field, in the order of the march: the field arguments
// (f2n_field_args_status), then the level count.
int grad_field_status(int L, int F, uint32_t T, int64_t level_stride)
{
  const int st = f2n_field_args_status(L, F, T, level_stride);
  if (st != F2N_OK) return st;
  if (L > F2N_MAX_LEVELS) return F2N_E_UNSUPPORTED;
  return F2N_OK;
}

}  // namespace

extern "C" int f2n_density_grad(
  const float * pts, const uint16_t * table_f16, const int32_t * primes, const float * bias,
  const float * mul, const float * w0, float * grad, int64_t n, int L, int F, uint32_t T,
  int64_t level_stride, void * stream)
{
  if (n < 0) return F2N_E_INVALID_ARG;
  const int st = grad_field_status(L, F, T, level_stride);
  if (st != F2N_OK) return st;
  if (n == 0) return F2N_OK;
  if (!pts || !table_f16 || !primes || !bias || !mul || !w0 || !grad) return F2N_E_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(table_f16) % (2u * F)) return F2N_E_INVALID_ARG;
  if (n > (int64_t)0x7fffffff * F2N_BLOCK) return F2N_E_INVALID_ARG;  // the grid's x extent
  const dim3 grid(f2n_div_up(n, F2N_BLOCK)), block(F2N_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  f2n_dispatch_field(F, T, [&](auto ff, auto p2) {
    hipLaunchKernelGGL(
      (density_grad_kernel<decltype(ff)::value, decltype(p2)::value>), grid, block, 0, s, pts,
      table_f16, primes, bias, mul, w0, grad, n, L, T, level_stride);
  });
  return f2n_launch_status();
}

extern "C" int f2n_ray_normals(
  const float * pts, const int32_t * bounds, const float * weights, const uint16_t * table_f16,
  const int32_t * primes, const float * bias, const float * mul, const float * w0,
  float * normals, int n_rays, int L, int F, uint32_t T, int64_t level_stride, void * stream)
{
  if (n_rays < 0) return F2N_E_INVALID_ARG;
  const int st = grad_field_status(L, F, T, level_stride);
  if (st != F2N_OK) return st;
  if (n_rays == 0) return F2N_OK;
  if (!pts || !bounds || !weights || !table_f16 || !primes || !bias || !mul || !w0 || !normals)
    return F2N_E_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(table_f16) % (2u * F)) return F2N_E_INVALID_ARG;
  const dim3 grid(f2n_div_up(n_rays, F2N_WAVES_PER_BLOCK)), block(F2N_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  f2n_dispatch_field(F, T, [&](auto ff, auto p2) {
    hipLaunchKernelGGL(
      (ray_normals_kernel<decltype(ff)::value, decltype(p2)::value>), grid, block, 0, s, pts, bounds,
      weights, table_f16, primes, bias, mul, w0, normals, n_rays, L, T, level_stride);
  });
  return f2n_launch_status();
}
