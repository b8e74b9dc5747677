// localizer.hip -- the device side of the reference's particle localiser (src/localizer.cpp): the
// pose perturbation (:88-118), the scoring of rendered particles against the camera image
// (:236-248) and the pose average (:254-316).  The reference drives all three from the host around
// one render: per particle three Eigen rotations copied to the device and three mm launches; clip,
// index and the squared-error reduction as ATen launches on the image's device (the GPU when the
// caller passes the image there, as the ROS node does), then the P losses copied to the host for
// pow and the normalisation; and per particle a device-to-host copy of its rotation.
// Here each is one or two launches on data that never leaves the device.
//
// Sizes are tiny (P <= ~100 particles, K = 256 pixels), so the kernels are written for a fixed,
// reproducible order of every sum rather than for throughput: no atomics anywhere, f64 wherever the
// reference's own arithmetic is f64 or where f32 would overflow (the fifth power of the scores).
#include "common.hiph"

namespace
{

// ---- f2n_perturb_poses ---------------------------------------------------------------------------

// rows 1 and 2 of a 3x3 block (a = the first, b = the second) under [[c, s], [-s, c]]
__device__ __forceinline__ void rot_rows(float c, float s, float * a, float * b)
{
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const float x = a[j], y = b[j];
    a[j] = fmaf(s, y, c * x);
    b[j] = fmaf(c, y, -s * x);
  }
}

__global__ __launch_bounds__(F2N_BLOCK) void perturb_poses_kernel(
  const float * __restrict__ pose, const float * __restrict__ noise, float sx, float sy, float sz,
  float rx, float ry, float rz, float * __restrict__ poses, int P)
{
  const int p = blockIdx.x * F2N_BLOCK + threadIdx.x;
  if (p >= P) return;
  float r0[3], r1[3], r2[3], t[3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    r0[j] = pose[j];
    r1[j] = pose[4 + j];
    r2[j] = pose[8 + j];
    t[j] = pose[4 * j + 3];
  }
  if (p > 0) {
    const float * n = noise + 6 * (int64_t)p;
    t[0] += sx * n[0];
    t[1] += sy * n[1];
    t[2] += sz * n[2];
    // degrees -> radians as the reference spells it: float * M_PI / 180.0 in double, then to float
    const double rad = 3.14159265358979323846;
    const float tx = (float)((double)(rx * n[3]) * rad / 180.0);
    const float ty = (float)((double)(ry * n[4]) * rad / 180.0);
    const float tz = (float)((double)(rz * n[5]) * rad / 180.0);
    // R' = Mz My Mx R, every M the TRANSPOSE of the textbook rotation (see the header):
    //   Mx = [1 0 0; 0 c s; 0 -s c]   My = [c 0 -s; 0 1 0; s 0 c]   Mz = [c s 0; -s c 0; 0 0 1]
    rot_rows(cosf(tx), sinf(tx), r1, r2);
    rot_rows(cosf(ty), sinf(ty), r2, r0);
    rot_rows(cosf(tz), sinf(tz), r0, r1);
  }
  float * out = poses + 12 * (int64_t)p;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    out[j] = r0[j];
    out[4 + j] = r1[j];
    out[8 + j] = r2[j];
    out[4 * j + 3] = t[j];
  }
}

// ---- f2n_pose_scores -----------------------------------------------------------------------------

// Sum over the 64 lanes in a fixed butterfly order, the result in every lane.
__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, F2N_WAVE);
  return v;
}

// One wavefront per pose; the lanes walk the K pixels in strides of 64.
__global__ __launch_bounds__(F2N_BLOCK) void pose_loss_kernel(
  const float * __restrict__ colors, const float * __restrict__ image,
  const int32_t * __restrict__ ij, float * __restrict__ loss, double * __restrict__ score, int P,
  int K, int h, int w)
{
  const int p = blockIdx.x * F2N_WAVES_PER_BLOCK + (threadIdx.x / F2N_WAVE);
  if (p >= P) return;  // wave-uniform
  const int lane = threadIdx.x % F2N_WAVE;
  const float * c = colors + (int64_t)p * K * 3;
  double acc = 0.0;
  for (int k = lane; k < K; k += F2N_WAVE) {
    const int i = min(max(ij[2 * k], 0), h - 1);
    const int j = min(max(ij[2 * k + 1], 0), w - 1);
    const float * g = image + ((int64_t)i * w + j) * 3;
    const double d0 = (double)fminf(fmaxf(c[3 * k], 0.f), 1.f) - (double)g[0];
    const double d1 = (double)fminf(fmaxf(c[3 * k + 1], 0.f), 1.f) - (double)g[1];
    const double d2 = (double)fminf(fmaxf(c[3 * k + 2], 0.f), 1.f) - (double)g[2];
    acc += ((d0 * d0 + d1 * d1) + d2 * d2) / 3.0;
  }
  const double total = wave_sum_f64(acc);
  if (lane == 0) {
    const double x = (double)K / (total + 1e-6);
    const double x2 = x * x;
    loss[p] = (float)total;
    score[p] = x2 * x2 * x;
  }
}

// One workgroup: every thread forms the normaliser itself, over the P scores in index order (the
// loads are uniform), then the threads share the P divisions.
__global__ __launch_bounds__(F2N_BLOCK) void pose_weights_kernel(
  const double * __restrict__ score, float * __restrict__ weights, int P)
{
  double z = 0.0;
  for (int q = 0; q < P; q++) z += score[q];
  for (int p = threadIdx.x; p < P; p += F2N_BLOCK) weights[p] = (float)(score[p] / z);
}

// ---- f2n_average_pose ----------------------------------------------------------------------------

struct Quat
{
  double w, x, y, z;
};

// Rotation matrix (rows of a [3,4] pose) -> quaternion, by the branches of Eigen's
// Quaternion(Matrix3): trace > 0, else the largest diagonal element.
__device__ __forceinline__ Quat quat_from_pose(const float * __restrict__ m)
{
  const double m00 = m[0], m01 = m[1], m02 = m[2];
  const double m10 = m[4], m11 = m[5], m12 = m[6];
  const double m20 = m[8], m21 = m[9], m22 = m[10];
  Quat q;
  double t = m00 + m11 + m22;
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    q.w = 0.5 * t;
    t = 0.5 / t;
    q.x = (m21 - m12) * t;
    q.y = (m02 - m20) * t;
    q.z = (m10 - m01) * t;
  } else if (!(m11 > m00) && !(m22 > m00)) {  // i = 0, j = 1, k = 2
    t = sqrt(m00 - m11 - m22 + 1.0);
    q.x = 0.5 * t;
    t = 0.5 / t;
    q.w = (m21 - m12) * t;
    q.y = (m10 + m01) * t;
    q.z = (m20 + m02) * t;
  } else if (m11 > m00 && !(m22 > m11)) {  // i = 1, j = 2, k = 0
    t = sqrt(m11 - m22 - m00 + 1.0);
    q.y = 0.5 * t;
    t = 0.5 / t;
    q.w = (m02 - m20) * t;
    q.z = (m21 + m12) * t;
    q.x = (m01 + m10) * t;
  } else {  // i = 2, j = 0, k = 1
    t = sqrt(m22 - m00 - m11 + 1.0);
    q.z = 0.5 * t;
    t = 0.5 / t;
    q.w = (m10 - m01) * t;
    q.x = (m02 + m20) * t;
    q.y = (m12 + m21) * t;
  }
  return q;
}

// One workgroup.  Particles are taken in chunks of F2N_BLOCK: every thread puts its particle's
// (sign-aligned) quaternion and weighted position into LDS, then threads 0..6 each add one of the
// seven components over the chunk in index order.
__global__ __launch_bounds__(F2N_BLOCK) void average_pose_kernel(
  const float * __restrict__ poses, const float * __restrict__ weights, float * __restrict__ out,
  int P)
{
  __shared__ double part[7][F2N_BLOCK];
  __shared__ double total[7];
  const Quat front = quat_from_pose(poses);
  double acc = 0.0;
  for (int base = 0; base < P; base += F2N_BLOCK) {
    const int p = base + (int)threadIdx.x;
    if (p < P) {
      const float * m = poses + 12 * (int64_t)p;
      Quat q = quat_from_pose(m);
      const double dot = q.w * front.w + q.x * front.x + q.y * front.y + q.z * front.z;
      const double sgn = dot < 0.0 ? -1.0 : 1.0;
      const double wgt = (double)weights[p];
      part[0][threadIdx.x] = sgn * q.w;
      part[1][threadIdx.x] = sgn * q.x;
      part[2][threadIdx.x] = sgn * q.y;
      part[3][threadIdx.x] = sgn * q.z;
      part[4][threadIdx.x] = wgt * (double)m[3];
      part[5][threadIdx.x] = wgt * (double)m[7];
      part[6][threadIdx.x] = wgt * (double)m[11];
    }
    __syncthreads();
    if (threadIdx.x < 7) {
      const int cnt = min(F2N_BLOCK, P - base);
      for (int k = 0; k < cnt; k++) acc += part[threadIdx.x][k];
    }
    __syncthreads();
  }
  if (threadIdx.x < 7) total[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x != 0) return;
  // the UNWEIGHTED mean of the quaternions (src/localizer.cpp:274), normalised, as a matrix
  double w = total[0] / (double)P, x = total[1] / (double)P, y = total[2] / (double)P,
         z = total[3] / (double)P;
  const double norm = sqrt(w * w + x * x + y * y + z * z);
  w /= norm;
  x /= norm;
  y /= norm;
  z /= norm;
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  out[0] = (float)(1.0 - (tyy + tzz));
  out[1] = (float)(txy - twz);
  out[2] = (float)(txz + twy);
  out[3] = (float)total[4];
  out[4] = (float)(txy + twz);
  out[5] = (float)(1.0 - (txx + tzz));
  out[6] = (float)(tyz - twx);
  out[7] = (float)total[5];
  out[8] = (float)(txz - twy);
  out[9] = (float)(tyz + twx);
  out[10] = (float)(1.0 - (txx + tyy));
  out[11] = (float)total[6];
}

}  // namespace

extern "C" int f2n_perturb_poses(
  const float * pose, int pose_ld, const float * noise, float sigma_pos_x, float sigma_pos_y,
  float sigma_pos_z, float sigma_rot_x, float sigma_rot_y, float sigma_rot_z, float * poses, int P,
  void * stream)
{
  if (!pose || !noise || !poses || P < 0) return F2N_E_INVALID_ARG;
  if (pose_ld != 12 && pose_ld != 16) return F2N_E_INVALID_ARG;  // rows 0..2 of either are [R | t]
  if (P == 0) return F2N_OK;
  hipLaunchKernelGGL(
    perturb_poses_kernel, dim3(f2n_div_up(P, F2N_BLOCK)), dim3(F2N_BLOCK), 0, (hipStream_t)stream,
    pose, noise, sigma_pos_x, sigma_pos_y, sigma_pos_z, sigma_rot_x, sigma_rot_y, sigma_rot_z,
    poses, P);
  return f2n_launch_status();
}

extern "C" int f2n_pose_scores(
  const float * colors, const float * image, const int32_t * ij, float * loss, float * weights,
  double * workspace, int P, int K, int h, int w, void * stream)
{
  if (!colors || !image || !ij || !loss || !weights || !workspace) return F2N_E_INVALID_ARG;
  if (P < 0 || K < 1 || h < 1 || w < 1) return F2N_E_INVALID_ARG;
  if (P == 0) return F2N_OK;
  hipLaunchKernelGGL(
    pose_loss_kernel, dim3(f2n_div_up(P, F2N_WAVES_PER_BLOCK)), dim3(F2N_BLOCK), 0,
    (hipStream_t)stream, colors, image, ij, loss, workspace, P, K, h, w);
  if (f2n_launch_status() != F2N_OK) return F2N_E_LAUNCH;
  hipLaunchKernelGGL(
    pose_weights_kernel, dim3(1), dim3(F2N_BLOCK), 0, (hipStream_t)stream, workspace, weights, P);
  return f2n_launch_status();
}

extern "C" int f2n_average_pose(
  const float * poses, const float * weights, float * pose_out, int P, void * stream)
{
  if (!poses || !weights || !pose_out || P < 1) return F2N_E_INVALID_ARG;
  hipLaunchKernelGGL(
    average_pose_kernel, dim3(1), dim3(F2N_BLOCK), 0, (hipStream_t)stream, poses, weights, pose_out,
    P);
  return f2n_launch_status();
}
