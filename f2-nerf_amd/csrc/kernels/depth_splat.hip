// depth_splat.hip -- a point cloud to sparse per-camera depth maps (include/f2nerf_hip.h:
// f2n_depth_splat), the targets of the line-of-sight losses in depth_sight.hip.  The reference reads
// no range data: this stands beside the forward camera model f2n_project_points (rays.hip) and takes
// its pixel decisions from the same device function, camera_point_to_pixel (camera.hiph), after the
// same world -> camera-frame lines, so a point lands in the pixel that entry reports, bit for bit.
//
// One thread per point.  The value kept is the ray distance d = |p - t_cam| (what the samples' t
// measures along a unit direction), not the z-depth:
//     dx = p - t (three subtractions), d = sqrtf((dx*dx + dy*dy) + dz*dz)      no fused multiply-add
// The minimum per pixel is an unsigned 32-bit atomicMin on the float's bit pattern: positive floats
// order like their bits, and a minimum does not depend on the order of arrival, so two launches give
// the same bits.  The map is filled with +inf before the splat (an async 32-bit memset) and what is
// still +inf afterwards becomes 0 = "no return" (one launch): every element is written.
#include "camera.hiph"

namespace
{

constexpr uint32_t kInfBits = 0x7f800000u;

__global__ __launch_bounds__(F2N_BLOCK) void depth_splat_kernel(
  const float * __restrict__ points, const int32_t * __restrict__ cam_idx,
  const float * __restrict__ poses, int pose_ld, const float * __restrict__ intrinsics,
  const float * __restrict__ dist, int64_t n_cams, int h, int w, uint32_t * __restrict__ depth,
  int64_t n)
{
  const int64_t r = (int64_t)blockIdx.x * F2N_BLOCK + threadIdx.x;
  if (r >= n) return;
  const int64_t cam = cam_idx ? (int64_t)cam_idx[r] : (n_cams == n && n_cams > 1 ? r : 0);
  if (cam < 0 || cam >= n_cams) return;  // never an address
  // (the lines of project_points_kernel, rays.hip)
  const float * P = poses + cam * pose_ld;
  const float dx = points[3 * r] - P[3], dy = points[3 * r + 1] - P[7],
              dz = points[3 * r + 2] - P[11];
  const float cx = P[0] * dx + P[4] * dy + P[8] * dz;
  const float cy = P[1] * dx + P[5] * dy + P[9] * dz;
  const float cz = P[2] * dx + P[6] * dy + P[10] * dz;
  float prow = 0.f, pcol = 0.f;
  if (!camera_point_to_pixel(intrinsics + cam * 9, load_lens(dist, cam), cx, cy, cz, prow, pcol))
    return;
  const float fr = floorf(prow), fc = floorf(pcol);
  if (!(fr >= 0.f && fr < (float)h && fc >= 0.f && fc < (float)w)) return;  // (false for NaN)
  const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
  if (!(d < __builtin_inff())) return;  // overflow or NaN: no return
  const int64_t px = (cam * h + (int64_t)fr) * w + (int64_t)fc;
  atomicMin(depth + px, __float_as_uint(d));
}

__global__ __launch_bounds__(F2N_BLOCK) void depth_finish_kernel(uint32_t * __restrict__ depth, int64_t n)
{
  const int64_t i = (int64_t)blockIdx.x * F2N_BLOCK + threadIdx.x;
  if (i >= n) return;
  if (depth[i] == kInfBits) depth[i] = 0u;
}

}  // namespace

extern "C" int f2n_depth_splat(
  const float * points, const int32_t * cam_idx, const float * poses, int pose_ld,
  const float * intrinsics, const float * dist, int64_t n_cams, int h, int w, float * depth,
  int64_t n, void * stream)
{
  if (!poses || !intrinsics || !depth || n < 0 || n_cams < 1 || h < 1 || w < 1)
    return F2N_E_INVALID_ARG;
  if (n > 0 && !points) return F2N_E_INVALID_ARG;
  if (pose_ld != 12 && pose_ld != 16) return F2N_E_INVALID_ARG;
  if (!cam_idx && n_cams != 1 && n_cams != n) return F2N_E_INVALID_ARG;
  // (h, w < 2^31 each: the first product cannot overflow; the second is guarded before it is formed)
  const int64_t hw = (int64_t)h * w;
  if (n_cams >= ((int64_t)1 << 31) || hw >= ((int64_t)1 << 31) || hw * n_cams >= ((int64_t)1 << 31))
    return F2N_E_UNSUPPORTED;
  const int64_t total = hw * n_cams;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0)
    return hipMemsetAsync(depth, 0, total * sizeof(float), s) == hipSuccess ? F2N_OK : F2N_E_LAUNCH;
  if (hipMemsetD32Async((hipDeviceptr_t)depth, (int)kInfBits, (size_t)total, s) != hipSuccess)
    return F2N_E_LAUNCH;
  hipLaunchKernelGGL(
    depth_splat_kernel, dim3(f2n_div_up(n, F2N_BLOCK)), dim3(F2N_BLOCK), 0, s, points, cam_idx,
    poses, pose_ld, intrinsics, dist, n_cams, h, w, (uint32_t *)depth, n);
  hipLaunchKernelGGL(
    depth_finish_kernel, dim3(f2n_div_up(total, F2N_BLOCK)), dim3(F2N_BLOCK), 0, s,
    (uint32_t *)depth, total);
  return f2n_launch_status();
}
