// pose_refine.hip -- what joint refinement of the training poses needs beside the kernels of
// pose_grad.hip: the reduction of a random batch's ray gradients to one pose gradient per camera, and
// the rigid correction that a 6-vector applies to a pose.
//
//   f2n_cam_pose_grad     d(rays_o), d(rays_d) of a batch whose rays each name their own camera
//                         (Dataset::sample_random_rays, src/dataset.cpp:150-171) -> d(pose) per camera:
//                         the backward of get_rays_from_pose's matmul and expand (src/rays.cpp:7-28)
//                         followed by autograd's index_select backward, without its float atomics.
//   f2n_pose_compose      R' = Exp(omega) R, t' = t + tau: the parameterisation that stays on SO(3),
//   f2n_pose_compose_bwd  where Adam on the twelve raw entries of a pose (src/localizer.cpp:142-167)
//                         leaves it after one step.
#include "cam_pieces.hiph"

namespace
{

// ---- f2n_cam_pose_grad ----------------------------------------------------------------------------
//
// The per-camera sums of cam_pieces.hiph with the twelve terms of a pose: pieces of kPiece positions,
// one wavefront each, a camera that spans pieces finished by the second kernel in piece order.

struct PoseRays
{
  const float * __restrict__ intrinsics;
  const float * __restrict__ dist;
  const int32_t * __restrict__ ij;
  const float * __restrict__ d_o;
  const float * __restrict__ d_d;
  const int32_t * __restrict__ order;
  int n;

  struct Cam
  {
    const float * K;
    LensDist lens;
  };

  __device__ __forceinline__ Cam camera(int c) const
  {
    return {intrinsics + (int64_t)c * 9, load_lens(dist, c)};
  }

  // the twelve terms of the ray at position p, added to acc (row-major [3,4]: d_d[i] v[j] | d_o[i])
  __device__ __forceinline__ void add(float (&acc)[12], const Cam & cam, int p) const
  {
    const int64_t r = order ? order[p] : p;
    if (r < 0 || r >= n) return;  // a caller's order is not trusted with an address
    float u, v;
    camera_pixel_to_dir(cam.K, cam.lens, (float)ij[2 * r], (float)ij[2 * r + 1], u, v);
    const float w = -1.f;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float g = d_d[3 * r + a];
      acc[4 * a] += g * u;
      acc[4 * a + 1] += g * v;
      acc[4 * a + 2] += g * w;
      acc[4 * a + 3] += d_o[3 * r + a];
    }
  }
};

__global__ __launch_bounds__(F2N_BLOCK) void cam_pose_grad_piece_kernel(
  const float * __restrict__ intrinsics, const float * __restrict__ dist,
  const int32_t * __restrict__ ij, const float * __restrict__ d_o, const float * __restrict__ d_d,
  const int32_t * __restrict__ cam_start, const int32_t * __restrict__ order,
  float * __restrict__ d_poses, int pose_ld, float * __restrict__ ws, int n, int E, int G)
{
  const PoseRays rays = {intrinsics, dist, ij, d_o, d_d, order, n};
  cam_piece_sums<12>(rays, cam_start, d_poses, pose_ld, ws, n, E, G);
}

__global__ __launch_bounds__(F2N_BLOCK) void cam_pose_grad_final_kernel(
  const int32_t * __restrict__ cam_start, const float * __restrict__ ws,
  float * __restrict__ d_poses, int pose_ld, int n, int E, int G)
{
  cam_piece_finish<12>(cam_start, ws, d_poses, pose_ld, n, E, G);
}

// ---- f2n_pose_compose -----------------------------------------------------------------------------
//
// Exp(omega) = I + A K + B K^2 with K = hat(omega), th = |omega|, A = sin th / th,
// B = (1 - cos th) / th^2 = (sin(th/2) / (th/2))^2 / 2 (no cancellation), K^2 = omega omega^T - th^2 I.
// Everything in f64 (E threads: the rate does not matter), rounded once to f32.  Below kSeries the
// quotients are their Taylor polynomials, whose first neglected terms are under 1e-17 there.

constexpr double kSeries = 1e-2;

struct ExpCoef
{
  double A, B;    // as above
  double a1, b1;  // (dA/dth) / th and (dB/dth) / th
};

__device__ __forceinline__ ExpCoef exp_coef(double th2, bool with_derivatives)
{
  ExpCoef c;
  const double th = sqrt(th2);
  if (th < kSeries) {
    c.A = 1.0 - th2 / 6.0 * (1.0 - th2 / 20.0 * (1.0 - th2 / 42.0));
    c.B = 0.5 - th2 / 24.0 * (1.0 - th2 / 30.0 * (1.0 - th2 / 56.0));
    c.a1 = -1.0 / 3.0 + th2 / 30.0 * (1.0 - th2 / 28.0 * (1.0 - th2 / 54.0));
    c.b1 = -1.0 / 12.0 + th2 / 180.0 * (1.0 - th2 * (3.0 / 112.0) * (1.0 - th2 / 67.5));
    return c;
  }
  const double sn = sin(th), cs = cos(th);
  const double hs = sin(0.5 * th) / (0.5 * th);
  c.A = sn / th;
  c.B = 0.5 * hs * hs;
  c.a1 = c.b1 = 0.0;
  if (with_derivatives) {
    // dA/dth = (cos th - A) / th,  dB/dth = (A - 2 B) / th
    c.a1 = (cs - c.A) / th2;
    c.b1 = (c.A - 2.0 * c.B) / th2;
  }
  return c;
}

__global__ __launch_bounds__(F2N_BLOCK) void pose_compose_kernel(
  const float * __restrict__ base, int pose_ld, const float * __restrict__ delta,
  const int32_t * __restrict__ fixed, float * __restrict__ out, int E)
{
  const int c = (int)blockIdx.x * F2N_BLOCK + (int)threadIdx.x;
  if (c >= E) return;
  const float * P = base + (int64_t)c * pose_ld;
  const float * d = delta + (int64_t)c * 6;
  float * O = out + (int64_t)c * 12;
  const bool zero = d[0] == 0.f && d[1] == 0.f && d[2] == 0.f && d[3] == 0.f && d[4] == 0.f &&
                    d[5] == 0.f;
  if (zero || (fixed && fixed[c] != 0)) {
#pragma unroll
    for (int k = 0; k < 12; k++) O[k] = P[k];  // the base rows, bit for bit
    return;
  }
  const double wx = d[0], wy = d[1], wz = d[2];
  const double th2 = wx * wx + wy * wy + wz * wz;
  const ExpCoef e = exp_coef(th2, false);
  // rows of Exp(omega)
  const double E00 = 1.0 + e.B * (wx * wx - th2), E01 = -e.A * wz + e.B * wx * wy,
               E02 = e.A * wy + e.B * wx * wz;
  const double E10 = e.A * wz + e.B * wx * wy, E11 = 1.0 + e.B * (wy * wy - th2),
               E12 = -e.A * wx + e.B * wy * wz;
  const double E20 = -e.A * wy + e.B * wx * wz, E21 = e.A * wx + e.B * wy * wz,
               E22 = 1.0 + e.B * (wz * wz - th2);
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const double r0 = P[j], r1 = P[4 + j], r2 = P[8 + j];
    O[j] = (float)(E00 * r0 + E01 * r1 + E02 * r2);
    O[4 + j] = (float)(E10 * r0 + E11 * r1 + E12 * r2);
    O[8 + j] = (float)(E20 * r0 + E21 * r1 + E22 * r2);
  }
  O[3] = (float)((double)P[3] + (double)d[3]);
  O[7] = (float)((double)P[7] + (double)d[4]);
  O[11] = (float)((double)P[11] + (double)d[5]);
}

// With G = d_out[:, :3, :3] and M = G R^T:  dL/d omega_k = <M, dExp/d omega_k>, and
//   dExp/d omega_k = a1 omega_k K + A hat(e_k) + b1 omega_k K^2 + B (e_k omega^T + omega e_k^T - 2 omega_k I)
// so with m = (M21 - M12, M02 - M20, M10 - M01) (<M, hat(v)> = v . m):
//   dL/d omega = (a1 (omega . m) + b1 (omega^T M omega - th^2 tr M) - 2 B tr M) omega
//                + A m + B (M + M^T) omega.
// dL/d tau = d_out[:, :, 3].
__global__ __launch_bounds__(F2N_BLOCK) void pose_compose_bwd_kernel(
  const float * __restrict__ base, int pose_ld, const float * __restrict__ delta,
  const int32_t * __restrict__ fixed, const float * __restrict__ d_out,
  float * __restrict__ d_delta, int E)
{
  const int c = (int)blockIdx.x * F2N_BLOCK + (int)threadIdx.x;
  if (c >= E) return;
  float * D = d_delta + (int64_t)c * 6;
  if (fixed && fixed[c] != 0) {
#pragma unroll
    for (int k = 0; k < 6; k++) D[k] = 0.f;
    return;
  }
  const float * P = base + (int64_t)c * pose_ld;
  const float * d = delta + (int64_t)c * 6;
  const float * Gm = d_out + (int64_t)c * 12;
  double M[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int k = 0; k < 3; k++)
      M[i][k] = (double)Gm[4 * i] * (double)P[4 * k] + (double)Gm[4 * i + 1] * (double)P[4 * k + 1] +
                (double)Gm[4 * i + 2] * (double)P[4 * k + 2];
  }
  const double wx = d[0], wy = d[1], wz = d[2];
  const double th2 = wx * wx + wy * wy + wz * wz;
  const ExpCoef e = exp_coef(th2, true);
  const double mx = M[2][1] - M[1][2], my = M[0][2] - M[2][0], mz = M[1][0] - M[0][1];
  const double tr = M[0][0] + M[1][1] + M[2][2];
  // (M + M^T) omega and omega^T M omega
  const double sx = 2.0 * M[0][0] * wx + (M[0][1] + M[1][0]) * wy + (M[0][2] + M[2][0]) * wz;
  const double sy = (M[0][1] + M[1][0]) * wx + 2.0 * M[1][1] * wy + (M[1][2] + M[2][1]) * wz;
  const double sz = (M[0][2] + M[2][0]) * wx + (M[1][2] + M[2][1]) * wy + 2.0 * M[2][2] * wz;
  const double wMw = 0.5 * (wx * sx + wy * sy + wz * sz);
  const double along =
    e.a1 * (wx * mx + wy * my + wz * mz) + e.b1 * (wMw - th2 * tr) - 2.0 * e.B * tr;
  D[0] = (float)(along * wx + e.A * mx + e.B * sx);
  D[1] = (float)(along * wy + e.A * my + e.B * sy);
  D[2] = (float)(along * wz + e.A * mz + e.B * sz);
  D[3] = Gm[3];
  D[4] = Gm[7];
  D[5] = Gm[11];
}

}  // namespace

extern "C" int64_t f2n_cam_pose_grad_workspace_floats(int64_t n, int64_t n_cams)
{
  return 12 * (cam_pieces(n < 0 ? 0 : n) + (n_cams < 1 ? 1 : n_cams));
}

extern "C" int f2n_cam_pose_grad(
  const float * intrinsics, const float * dist, const int32_t * ij, const float * d_rays_o,
  const float * d_rays_d, const int32_t * cam_start, const int32_t * order, float * d_poses,
  int pose_ld, float * workspace, int64_t n, int64_t n_cams, void * stream)
{
  if (!intrinsics || !ij || !d_rays_o || !d_rays_d || !cam_start || !d_poses || !workspace)
    return F2N_E_INVALID_ARG;
  // positions and camera numbers are i32 (cam_start, order), and one thread per pose component
  if (n < 0 || n > INT32_MAX - kPiece || n_cams < 1 || n_cams > INT32_MAX / 16)
    return F2N_E_INVALID_ARG;
  if (pose_ld != 12 && pose_ld != 16) return F2N_E_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int G = (int)cam_pieces(n);
  if (G > 0) {
    hipLaunchKernelGGL(
      cam_pose_grad_piece_kernel, dim3(f2n_div_up(G, F2N_WAVES_PER_BLOCK)), dim3(F2N_BLOCK), 0, s,
      intrinsics, dist, ij, d_rays_o, d_rays_d, cam_start, order, d_poses, pose_ld, workspace, (int)n,
      (int)n_cams, G);
    if (hipGetLastError() != hipSuccess) return F2N_E_LAUNCH;
  }
  // (n == 0: every camera is empty, and this kernel reads n instead of trusting cam_start)
  hipLaunchKernelGGL(
    cam_pose_grad_final_kernel, dim3(f2n_div_up(n_cams * 12, F2N_BLOCK)), dim3(F2N_BLOCK), 0, s,
    cam_start, workspace, d_poses, pose_ld, (int)n, (int)n_cams, G);
  return f2n_launch_status();
}

extern "C" int f2n_pose_compose(
  const float * base, int pose_ld, const float * delta, const int32_t * fixed, float * out,
  int64_t n_cams, void * stream)
{
  if (!base || !delta || !out) return F2N_E_INVALID_ARG;
  if (n_cams < 0 || n_cams > INT32_MAX / 16) return F2N_E_INVALID_ARG;
  if (pose_ld != 12 && pose_ld != 16) return F2N_E_INVALID_ARG;
  if (n_cams == 0) return F2N_OK;
  hipLaunchKernelGGL(
    pose_compose_kernel, dim3(f2n_div_up(n_cams, F2N_BLOCK)), dim3(F2N_BLOCK), 0,
    (hipStream_t)stream, base, pose_ld, delta, fixed, out, (int)n_cams);
  return f2n_launch_status();
}

extern "C" int f2n_pose_compose_bwd(
  const float * base, int pose_ld, const float * delta, const int32_t * fixed, const float * d_out,
  float * d_delta, int64_t n_cams, void * stream)
{
  if (!base || !delta || !d_out || !d_delta) return F2N_E_INVALID_ARG;
  if (n_cams < 0 || n_cams > INT32_MAX / 16) return F2N_E_INVALID_ARG;
  if (pose_ld != 12 && pose_ld != 16) return F2N_E_INVALID_ARG;
  if (n_cams == 0) return F2N_OK;
  hipLaunchKernelGGL(
    pose_compose_bwd_kernel, dim3(f2n_div_up(n_cams, F2N_BLOCK)), dim3(F2N_BLOCK), 0,
    (hipStream_t)stream, base, pose_ld, delta, fixed, d_out, d_delta, (int)n_cams);
  return f2n_launch_status();
}
