// pose_grad.hip -- the two backward kernels between a camera pose and the hash encoding of its
// samples: what autograd assembles in the reference when Localizer::optimize_pose_by_differential
// (reference src/localizer.cpp:142-167) differentiates Renderer::render_image with respect to the
// pose.
//
//   f2n_hash_rays_grad  d(enc) of the kept samples -> d(rays_o), d(rays_d).  Replaces, for rays that
//                       carry a gradient, the point-gradient half of Hash3DAnchoredBackwardKernel
//                       (src/hash_3d_anchored.cu:138-143, quirk Q5), the autograd chain of the scene
//                       contraction (src/hash_3d_anchored.cpp:79-82) and of the sampler's
//                       pts = o + d/|d| * t (src/points_sampler.cpp:24,44).
//   f2n_gen_rays_bwd    d(rays_o), d(rays_d) -> d(pose): the backward of get_rays_from_pose's
//                       matmul and expand (src/rays.cpp:7-28).
//
// Two gradients of the reference's chain are deliberately not formed, because they are zero or do
// not exist there:
//   * dt = |pts_k - pts_(k-1)| (quirk Q7) depends on rays_o not at all and on rays_d only through
//     |d/|d||; the normalisation's Jacobian (I - n n^T)/|d| annihilates that direction, so the path
//     is zero analytically (autograd forms it from roundings of the order of 1e-7 of the terms);
//   * the SH encoding of the directions has no backward in the reference (src/sh_shader.cu:105-115).
//
//   f2n_gen_rays_dist_bwd  the same for cameras with lens distortion: v_r is the undistorted
//                       direction of camera.hiph, which does not depend on the pose.
#include "camera.hiph"
#include "hash_grid.hiph"

namespace
{

__device__ __forceinline__ int ray_of_wave()
{
  return (int)blockIdx.x * F2N_WAVES_PER_BLOCK + (int)(threadIdx.x >> 6);
}

// ---- f2n_hash_rays_grad ---------------------------------------------------------------------------
//
// One wavefront per ray (the composite kernels' shape): lanes walk the ray's segment of kept samples
// in 64-sample strides, every lane runs the whole level loop of its sample in registers, and the
// per-ray sums are DPP wave sums at the end -- no float atomics, no [n,3] point-gradient buffer, and
// a fixed summation order (lane partials in stride order, then the fixed DPP tree).
//
// Per sample and level, the point gradient of quirk Q5 with the roundings of hash_bwd_kernel's
// WITH_PTS_GRAD branch (hash_grid.hip): gk = f16(grad_scale * g), then over the corners d and
// channels k, +-f16(feature * mul * gk) into the axis whose corner bit is set / clear; the level's
// sum is scaled by 1/grad_scale and the levels are added in order.  The result is the gradient at
// the CONTRACTED point; the contraction's Jacobian-vector product (contract_bwd_kernel's formula,
// NaN at |p| == 0 included) takes it to the raw point.
template <int F, bool POW2>
__global__ __launch_bounds__(F2N_BLOCK) void hash_rays_grad_kernel(
  const float * __restrict__ pts, const float * __restrict__ t, const int32_t * __restrict__ bounds,
  const float * __restrict__ rays_d, const uint16_t * __restrict__ table,
  const int32_t * __restrict__ primes, const float * __restrict__ bias,
  const float * __restrict__ mul, const float * __restrict__ grad_out, int64_t g_ld_point,
  int64_t g_ld_chan, float * __restrict__ d_rays_o, float * __restrict__ d_rays_d, int n_rays,
  int L, uint32_t T, int64_t level_stride, float grad_scale, float inv_scale)
{
  const int r = ray_of_wave();
  if (r >= n_rays) return;  // wave-uniform
  const int lane = lane_id();
  const int s = bounds[2 * r], e = bounds[2 * r + 1];
  using Row = typename RowBits<F>::type;
  float ox = 0.f, oy = 0.f, oz = 0.f;  // sum dp
  float mx = 0.f, my = 0.f, mz = 0.f;  // sum t * dp
  for (int c = s; c < e; c += F2N_WAVE) {
    const int64_t i = (int64_t)c + lane;
    if (i >= e) continue;
    const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    const float ti = t[i];
    float x = px, y = py, z = pz;
    contract_point(x, y, z);
    const float * gp = grad_out + i * g_ld_point;
    float gx = 0.f, gy = 0.f, gz = 0.f;  // gradient at the contracted point
    for (int l = 0; l < L; l++) {
      const LevelParams lp = load_level(primes, bias, mul, l);
      uint32_t row[8];
      float w[8];  // (unused: Q5 does not weight the corners)
      corner_rows_and_weights<POW2>(x, y, z, lp, T, row, w);
      const float * g = gp + (int64_t)(l * F) * g_ld_chan;
      float gk[F];
#pragma unroll
      for (int k = 0; k < F; k++) gk[k] = round_f16(g[k * g_ld_chan] * grad_scale);
      const Row * rows = reinterpret_cast<const Row *>(table + level_stride * l);
      Row rr[8];
#pragma unroll
      for (int d = 0; d < 8; d++) rr[d] = rows[row[d]];
      float lx = 0.f, ly = 0.f, lz = 0.f;
#pragma unroll
      for (int d = 0; d < 8; d++) {
        float f[F];
        unpack_row<F>(rr[d], f);
#pragma unroll
        for (int k = 0; k < F; k++) {
          const float nrm = f[k] * lp.mul * gk[k];
          const float pos = round_f16(nrm), neg = round_f16(-nrm);
          lx += (d & 4) ? pos : neg;
          ly += (d & 2) ? pos : neg;
          lz += (d & 1) ? pos : neg;
        }
      }
      gx += lx * inv_scale;
      gy += ly * inv_scale;
      gz += lz * inv_scale;
    }
    // contraction backward (contract_bwd_kernel)
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
      const float a = (2.f - inv) * inv;
      const float da_over_n = (2.f * inv - 2.f) * inv * inv * inv;
      const float pg = fmaf(pz, gz, fmaf(py, gy, px * gx));
      const float cc = da_over_n * pg;
      dx = fmaf(cc, px, a * gx);
      dy = fmaf(cc, py, a * gy);
      dz = fmaf(cc, pz, a * gz);
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

// ---- f2n_gen_rays_bwd -----------------------------------------------------------------------------
//
// rays_d = R v with v = ((col+.5-cx)/fx, -(row+.5-cy)/fy, -1), rays_o = t (rays.hip), so
//   d R[i][j] = sum_r d_d[r][i] v_r[j],   d t[i] = sum_r d_o[r][i].
// One pose per ray: one thread per ray writes its block.  One pose for all rays: a fixed partition
// of the rays into workgroups (pose_groups), DPP + LDS inside each, one partial per workgroup in the
// caller's workspace, and a single workgroup that adds the partials in index order -- the same bits
// on every run.

constexpr int kRaysPerGroup = 1024;  // 4 per thread
constexpr int kMaxGroups = 1024;

inline int64_t pose_groups(int64_t n)
{
  const int64_t g = (n + kRaysPerGroup - 1) / kRaysPerGroup;
  return g < 1 ? 1 : (g > kMaxGroups ? kMaxGroups : g);
}

// v_r with the float operations of gen_rays_kernel
__device__ __forceinline__ void camera_dir(
  const float * __restrict__ K, const int32_t * __restrict__ ij, int64_t first_pixel, int width,
  int64_t r, float & u, float & v)
{
  float row, col;
  if (ij) {
    row = (float)ij[2 * r];
    col = (float)ij[2 * r + 1];
  } else {
    const int64_t px = first_pixel + r;
    row = (float)(px / width);
    col = (float)(px % width);
  }
  u = ((col + .5f) - K[2]) / K[0];
  v = -(((row + .5f) - K[5]) / K[4]);
}

__global__ __launch_bounds__(F2N_BLOCK) void gen_rays_bwd_per_ray_kernel(
  const float * __restrict__ intrinsics, const int32_t * __restrict__ ij, int64_t first_pixel,
  int width, const float * __restrict__ d_o, const float * __restrict__ d_d,
  float * __restrict__ d_poses, int pose_ld, int64_t n)
{
  const int64_t r = (int64_t)blockIdx.x * F2N_BLOCK + threadIdx.x;
  if (r >= n) return;
  float u, v;
  camera_dir(intrinsics + r * 9, ij, first_pixel, width, r, u, v);
  const float w = -1.f;
  float * P = d_poses + r * pose_ld;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float g = d_d[3 * r + a];
    P[4 * a] = g * u;
    P[4 * a + 1] = g * v;
    P[4 * a + 2] = g * w;
    P[4 * a + 3] = d_o[3 * r + a];
  }
  if (pose_ld == 16) {
#pragma unroll
    for (int j = 12; j < 16; j++) P[j] = 0.f;
  }
}

// Sum of 12 per-thread values over the 256 threads of a workgroup, in a fixed order; valid in
// threads 0..11 (component = threadIdx.x).
__device__ __forceinline__ float block_sum12(const float (&acc)[12], float (*part)[12])
{
  const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int c = 0; c < 12; c++) {
    const float s = wave_sum(acc[c]);
    if (lane == 0) part[wave][c] = s;
  }
  __syncthreads();
  float out = 0.f;
  if (threadIdx.x < 12) {
#pragma unroll
    for (int w = 0; w < F2N_WAVES_PER_BLOCK; w++) out += part[w][threadIdx.x];
  }
  return out;
}

__global__ __launch_bounds__(F2N_BLOCK) void gen_rays_bwd_partial_kernel(
  const float * __restrict__ K, const int32_t * __restrict__ ij, int64_t first_pixel, int width,
  const float * __restrict__ d_o, const float * __restrict__ d_d, float * __restrict__ partial,
  int64_t n, int64_t per_group)
{
  __shared__ float part[F2N_WAVES_PER_BLOCK][12];
  const int64_t lo = (int64_t)blockIdx.x * per_group;
  const int64_t hi = (lo + per_group < n) ? lo + per_group : n;
  float acc[12];
#pragma unroll
  for (int c = 0; c < 12; c++) acc[c] = 0.f;
  for (int64_t r = lo + threadIdx.x; r < hi; r += F2N_BLOCK) {
    float u, v;
    camera_dir(K, ij, first_pixel, width, r, u, v);
    const float w = -1.f;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float g = d_d[3 * r + a];
      acc[4 * a] = fmaf(g, u, acc[4 * a]);
      acc[4 * a + 1] = fmaf(g, v, acc[4 * a + 1]);
      acc[4 * a + 2] = fmaf(g, w, acc[4 * a + 2]);
      acc[4 * a + 3] += d_o[3 * r + a];
    }
  }
  const float s = block_sum12(acc, part);
  if (threadIdx.x < 12) partial[12 * (int64_t)blockIdx.x + threadIdx.x] = s;
}

__global__ __launch_bounds__(F2N_BLOCK) void gen_rays_bwd_final_kernel(
  const float * __restrict__ partial, int groups, float * __restrict__ d_pose, int pose_ld)
{
  __shared__ float part[F2N_WAVES_PER_BLOCK][12];
  float acc[12];
#pragma unroll
  for (int c = 0; c < 12; c++) acc[c] = 0.f;
  for (int g = threadIdx.x; g < groups; g += F2N_BLOCK) {
#pragma unroll
    for (int c = 0; c < 12; c++) acc[c] += partial[12 * g + c];
  }
  const float s = block_sum12(acc, part);
  if (threadIdx.x < 12) d_pose[threadIdx.x] = s;
  if (pose_ld == 16 && threadIdx.x >= 12 && threadIdx.x < 16) d_pose[threadIdx.x] = 0.f;
}

// ---- f2n_gen_rays_dist_bwd ------------------------------------------------------------------------
//
// The per-ray and the partial kernel above with v_r from camera_pixel_to_dir (the function the
// forward calls): same partition, same order of the sums, the same final kernel.  A row of zeros in
// `dist` gives the bits of the kernels above.

__global__ __launch_bounds__(F2N_BLOCK) void lens_rays_bwd_per_ray_kernel(
  const float * __restrict__ intrinsics, const float * __restrict__ dist,
  const int32_t * __restrict__ ij, int64_t first_pixel, int width, const float * __restrict__ d_o,
  const float * __restrict__ d_d, float * __restrict__ d_poses, int pose_ld, int64_t n)
{
  const int64_t r = (int64_t)blockIdx.x * F2N_BLOCK + threadIdx.x;
  if (r >= n) return;
  float row, col, u, v;
  ray_pixel(ij, first_pixel, width, r, row, col);
  camera_pixel_to_dir(intrinsics + r * 9, load_lens(dist, r), row, col, u, v);
  const float w = -1.f;
  float * P = d_poses + r * pose_ld;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float g = d_d[3 * r + a];
    P[4 * a] = g * u;
    P[4 * a + 1] = g * v;
    P[4 * a + 2] = g * w;
    P[4 * a + 3] = d_o[3 * r + a];
  }
  if (pose_ld == 16) {
#pragma unroll
    for (int j = 12; j < 16; j++) P[j] = 0.f;
  }
}

__global__ __launch_bounds__(F2N_BLOCK) void lens_rays_bwd_partial_kernel(
  const float * __restrict__ K, const float * __restrict__ dist, const int32_t * __restrict__ ij,
  int64_t first_pixel, int width, const float * __restrict__ d_o, const float * __restrict__ d_d,
  float * __restrict__ partial, int64_t n, int64_t per_group)
{
  __shared__ float part[F2N_WAVES_PER_BLOCK][12];
  const int64_t lo = (int64_t)blockIdx.x * per_group;
  const int64_t hi = (lo + per_group < n) ? lo + per_group : n;
  const LensDist lens = load_lens(dist, 0);
  float acc[12];
#pragma unroll
  for (int c = 0; c < 12; c++) acc[c] = 0.f;
  for (int64_t r = lo + threadIdx.x; r < hi; r += F2N_BLOCK) {
    float row, col, u, v;
    ray_pixel(ij, first_pixel, width, r, row, col);
    camera_pixel_to_dir(K, lens, row, col, u, v);
    const float w = -1.f;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float g = d_d[3 * r + a];
      acc[4 * a] = fmaf(g, u, acc[4 * a]);
      acc[4 * a + 1] = fmaf(g, v, acc[4 * a + 1]);
      acc[4 * a + 2] = fmaf(g, w, acc[4 * a + 2]);
      acc[4 * a + 3] += d_o[3 * r + a];
    }
  }
  const float s = block_sum12(acc, part);
  if (threadIdx.x < 12) partial[12 * (int64_t)blockIdx.x + threadIdx.x] = s;
}

}  // namespace

extern "C" int f2n_hash_rays_grad(
  const float * pts, const float * t, const int32_t * bounds, const float * rays_d,
  const uint16_t * table_f16, const int32_t * primes, const float * bias, const float * mul,
  const float * grad_out, int64_t g_ld_point, int64_t g_ld_chan, float * d_rays_o,
  float * d_rays_d, int n_rays, int L, int F, uint32_t T, int64_t level_stride, float grad_scale,
  void * stream)
{
  if (!pts || !t || !bounds || !rays_d || !table_f16 || !primes || !bias || !mul || !grad_out ||
      !d_rays_o || !d_rays_d)
    return F2N_E_INVALID_ARG;
  if (n_rays < 0 || g_ld_point < 0 || g_ld_chan < 0) return F2N_E_INVALID_ARG;
  if (F != 1 && F != 2 && F != 4 && F != 8) return F2N_E_UNSUPPORTED;
  if (!f2n_hash_args_ok(0, L, F, T, level_stride)) return F2N_E_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(table_f16) % (2u * F)) return F2N_E_INVALID_ARG;
  int e = 0;
  const float m = frexpf(grad_scale, &e);
  if (!(grad_scale > 0.f) || m != 0.5f) return F2N_E_INVALID_ARG;  // power of two only
  if (n_rays == 0) return F2N_OK;
  const dim3 grid(f2n_div_up(n_rays, F2N_WAVES_PER_BLOCK)), block(F2N_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  const float inv = 1.f / grad_scale;
  f2n_dispatch_field(F, T, [&](auto ff, auto p2) {
    hipLaunchKernelGGL(
      (hash_rays_grad_kernel<decltype(ff)::value, decltype(p2)::value>), grid, block, 0, s, pts, t,
      bounds, rays_d, table_f16, primes, bias, mul, grad_out, g_ld_point, g_ld_chan, d_rays_o,
      d_rays_d, n_rays, L, T, level_stride, grad_scale, inv);
  });
  return f2n_launch_status();
}

extern "C" int64_t f2n_gen_rays_bwd_workspace_floats(int64_t n)
{
  return 12 * pose_groups(n < 0 ? 0 : n);
}

extern "C" int f2n_gen_rays_bwd(
  const float * intrinsics, int64_t n_cams, const int32_t * ij, int64_t first_pixel, int width,
  const float * d_rays_o, const float * d_rays_d, float * d_poses, int pose_ld, float * workspace,
  int64_t n, void * stream)
{
  if (!intrinsics || !d_rays_o || !d_rays_d || !d_poses || !workspace || n < 0 || n_cams < 1)
    return F2N_E_INVALID_ARG;
  if (pose_ld != 12 && pose_ld != 16) return F2N_E_INVALID_ARG;
  if (!ij && width <= 0) return F2N_E_INVALID_ARG;
  if (first_pixel < 0) return F2N_E_INVALID_ARG;
  if (n_cams != 1 && n_cams != n) return F2N_E_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (n_cams == 1) {
    const int64_t groups = pose_groups(n);
    const int64_t per = (n + groups - 1) / groups;
    hipLaunchKernelGGL(
      gen_rays_bwd_partial_kernel, dim3((unsigned)groups), dim3(F2N_BLOCK), 0, s, intrinsics, ij,
      first_pixel, width, d_rays_o, d_rays_d, workspace, n, per);
    if (hipGetLastError() != hipSuccess) return F2N_E_LAUNCH;
    hipLaunchKernelGGL(
      gen_rays_bwd_final_kernel, dim3(1), dim3(F2N_BLOCK), 0, s, workspace, (int)groups, d_poses,
      pose_ld);
    return f2n_launch_status();
  }
  hipLaunchKernelGGL(
    gen_rays_bwd_per_ray_kernel, dim3(f2n_div_up(n, F2N_BLOCK)), dim3(F2N_BLOCK), 0, s, intrinsics,
    ij, first_pixel, width, d_rays_o, d_rays_d, d_poses, pose_ld, n);
  return f2n_launch_status();
}

extern "C" int f2n_gen_rays_dist_bwd(
  const float * intrinsics, const float * dist, int64_t n_cams, const int32_t * ij,
  int64_t first_pixel, int width, const float * d_rays_o, const float * d_rays_d, float * d_poses,
  int pose_ld, float * workspace, int64_t n, void * stream)
{
  if (!intrinsics || !d_rays_o || !d_rays_d || !d_poses || !workspace || n < 0 || n_cams < 1)
    return F2N_E_INVALID_ARG;
  if (pose_ld != 12 && pose_ld != 16) return F2N_E_INVALID_ARG;
  if (!ij && width <= 0) return F2N_E_INVALID_ARG;
  if (first_pixel < 0) return F2N_E_INVALID_ARG;
  if (n_cams != 1 && n_cams != n) return F2N_E_INVALID_ARG;
  if (n == 0) return F2N_OK;
  if (!dist)  // pinhole: the existing kernels
    return f2n_gen_rays_bwd(
      intrinsics, n_cams, ij, first_pixel, width, d_rays_o, d_rays_d, d_poses, pose_ld, workspace, n,
      stream);
  hipStream_t s = (hipStream_t)stream;
  if (n_cams == 1) {
    const int64_t groups = pose_groups(n);
    const int64_t per = (n + groups - 1) / groups;
    hipLaunchKernelGGL(
      lens_rays_bwd_partial_kernel, dim3((unsigned)groups), dim3(F2N_BLOCK), 0, s, intrinsics, dist,
      ij, first_pixel, width, d_rays_o, d_rays_d, workspace, n, per);
    if (hipGetLastError() != hipSuccess) return F2N_E_LAUNCH;
    hipLaunchKernelGGL(
      gen_rays_bwd_final_kernel, dim3(1), dim3(F2N_BLOCK), 0, s, workspace, (int)groups, d_poses,
      pose_ld);
    return f2n_launch_status();
  }
  hipLaunchKernelGGL(
    lens_rays_bwd_per_ray_kernel, dim3(f2n_div_up(n, F2N_BLOCK)), dim3(F2N_BLOCK), 0, s, intrinsics,
    dist, ij, first_pixel, width, d_rays_o, d_rays_d, d_poses, pose_ld, n);
  return f2n_launch_status();
}
