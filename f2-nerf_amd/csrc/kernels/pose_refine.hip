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
#include "camera.hiph"

namespace
{

// ---- f2n_cam_pose_grad ----------------------------------------------------------------------------
//
// The camera-sorted ray list is cut into pieces of kPiece positions counted from the START OF THE LIST,
// one wavefront per piece.  A piece meets the cameras c_first .. c_last (two binary searches in
// cam_start); the wavefront takes them 64 at a time, one per lane:
//   * a run (camera intersected with piece) shorter than kLaneRun is summed by its lane alone, in
//     position order;
//   * a longer run is summed by the whole wavefront: 64-position strides from the run's start, twelve
//     lane accumulators, wave_sum in the fixed DPP tree.
// Where a run goes:
//   * the camera lies inside the piece          -> its d_poses block, finished;
//   * the camera begins here and goes on        -> workspace slot G + c;
//   * the camera came in from the piece before  -> workspace slot g (only one camera can).
// That is G + E slots of 12 floats and no scan of pieces per camera.  The second kernel, one thread per
// (camera, component), writes zeros for an empty camera and adds a spanning camera's slots in piece
// order.  The partition depends on cam_start alone and every order is fixed: the same bits on every
// run, no float atomics, no host read, two launches.  Work is O(n + E/64) per launch: one camera does
// not serialise through one wavefront, and empty cameras cost a lane each.

constexpr int kPiece = 1024;
constexpr int kLaneRun = 32;

__device__ __forceinline__ int clamp_int(int v, int lo, int hi)
{
  return v < lo ? lo : (v > hi ? hi : v);
}

// largest i in [0, E - 1] with cam_start[i] <= p: the camera that owns position p
__device__ __forceinline__ int camera_of(const int32_t * __restrict__ cam_start, int E, int p)
{
  int lo = 0, hi = E - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cam_start[mid] <= p)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// the twelve terms of the ray at position p, added to acc (row-major [3,4]: d_d[i] v[j] | d_o[i])
__device__ __forceinline__ void add_ray(
  float (&acc)[12], const float * __restrict__ K, const LensDist & lens,
  const int32_t * __restrict__ ij, const float * __restrict__ d_o, const float * __restrict__ d_d,
  const int32_t * __restrict__ order, int p, int n)
{
  const int64_t r = order ? order[p] : p;
  if (r < 0 || r >= n) return;  // a caller's order is not trusted with an address
  float u, v;
  camera_pixel_to_dir(K, lens, (float)ij[2 * r], (float)ij[2 * r + 1], u, v);
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

struct RunSpan
{
  int s_full, e_full;  // the camera's positions
  int s, e;            // ... inside the piece
};

__device__ __forceinline__ RunSpan run_span(
  const int32_t * __restrict__ cam_start, int c, int lo, int hi, int n)
{
  RunSpan r;
  r.s_full = clamp_int(cam_start[c], 0, n);
  r.e_full = clamp_int(cam_start[c + 1], r.s_full, n);
  r.s = r.s_full > lo ? r.s_full : lo;
  r.e = r.e_full < hi ? r.e_full : hi;
  if (r.e < r.s) r.e = r.s;
  return r;
}

__device__ __forceinline__ void store_run(
  const float (&acc)[12], const RunSpan & run, int c, int g, int G, int lo, int hi,
  float * __restrict__ d_poses, int pose_ld, float * __restrict__ ws)
{
  const bool whole = run.s_full >= lo && run.e_full <= hi;
  float * dst = whole ? d_poses + (int64_t)c * pose_ld
                      : ws + 12 * (run.s_full >= lo ? (int64_t)G + c : (int64_t)g);
#pragma unroll
  for (int k = 0; k < 12; k++) dst[k] = acc[k];
  if (whole && pose_ld == 16) {
#pragma unroll
    for (int k = 12; k < 16; k++) dst[k] = 0.f;
  }
}

__global__ __launch_bounds__(F2N_BLOCK) void cam_pose_grad_piece_kernel(
  const float * __restrict__ intrinsics, const float * __restrict__ dist,
  const int32_t * __restrict__ ij, const float * __restrict__ d_o, const float * __restrict__ d_d,
  const int32_t * __restrict__ cam_start, const int32_t * __restrict__ order,
  float * __restrict__ d_poses, int pose_ld, float * __restrict__ ws, int n, int E, int G)
{
  const int g = (int)blockIdx.x * F2N_WAVES_PER_BLOCK + (int)(threadIdx.x >> 6);
  if (g >= G) return;  // wave-uniform
  const int lane = lane_id();
  const int lo = g * kPiece;
  const int hi = (n - lo < kPiece) ? n : lo + kPiece;
  const int c_first = camera_of(cam_start, E, lo), c_last = camera_of(cam_start, E, hi - 1);
  for (int base = c_first; base <= c_last; base += F2N_WAVE) {
    const int c = base + lane;
    RunSpan run = {0, 0, 0, 0};
    if (c <= c_last) run = run_span(cam_start, c, lo, hi, n);
    const int len = run.e - run.s;
    if (len > 0 && len < kLaneRun) {
      float acc[12];
#pragma unroll
      for (int k = 0; k < 12; k++) acc[k] = 0.f;
      const float * K = intrinsics + (int64_t)c * 9;
      const LensDist lens = load_lens(dist, c);
      for (int p = run.s; p < run.e; p++) add_ray(acc, K, lens, ij, d_o, d_d, order, p, n);
      store_run(acc, run, c, g, G, lo, hi, d_poses, pose_ld, ws);
    }
    unsigned long long longs = __ballot(len >= kLaneRun);
    while (longs) {  // wave-uniform
      const int cc = base + (__ffsll(longs) - 1);
      longs &= longs - 1;
      const RunSpan wide = run_span(cam_start, cc, lo, hi, n);
      float acc[12];
#pragma unroll
      for (int k = 0; k < 12; k++) acc[k] = 0.f;
      const float * K = intrinsics + (int64_t)cc * 9;
      const LensDist lens = load_lens(dist, cc);
      for (int p0 = wide.s; p0 < wide.e; p0 += F2N_WAVE) {
        const int p = p0 + lane;
        if (p < wide.e) add_ray(acc, K, lens, ij, d_o, d_d, order, p, n);
      }
#pragma unroll
      for (int k = 0; k < 12; k++) acc[k] = wave_sum(acc[k]);
      if (lane == 0) store_run(acc, wide, cc, g, G, lo, hi, d_poses, pose_ld, ws);
    }
  }
}

__global__ __launch_bounds__(F2N_BLOCK) void cam_pose_grad_final_kernel(
  const int32_t * __restrict__ cam_start, const float * __restrict__ ws,
  float * __restrict__ d_poses, int pose_ld, int n, int E, int G)
{
  const int64_t t = (int64_t)blockIdx.x * F2N_BLOCK + threadIdx.x;
  if (t >= (int64_t)E * 12) return;
  const int c = (int)(t / 12), k = (int)(t % 12);
  const int s = clamp_int(cam_start[c], 0, n), e = clamp_int(cam_start[c + 1], s, n);
  float * P = d_poses + (int64_t)c * pose_ld;
  if (pose_ld == 16 && k < 4 && (s == e || ((e - 1) / kPiece != s / kPiece))) P[12 + k] = 0.f;
  if (s == e) {
    P[k] = 0.f;
    return;
  }
  const int g0 = s / kPiece, g1 = (e - 1) / kPiece;
  if (g0 == g1) return;  // written by the piece kernel
  float acc = ws[12 * ((int64_t)G + c) + k];
  for (int g = g0 + 1; g <= g1; g++) acc += ws[12 * (int64_t)g + k];
  P[k] = acc;
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

inline int64_t cam_pieces(int64_t n) { return (n + kPiece - 1) / kPiece; }

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
