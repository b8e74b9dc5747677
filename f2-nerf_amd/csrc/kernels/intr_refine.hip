// intr_refine.hip -- what refining the calibration while the field trains needs: the gradient of a
// batch's ray directions with respect to fx, fy, cx, cy, k1, k2, p1, p2 of each camera, and the
// shared correction that eight numbers per physical camera apply to the calibration of its images.
//
//   f2n_cam_intr_grad      d(rays_d) of a batch whose rays each name their own camera -> d(fx, fy, cx,
//                          cy, k1, k2, p1, p2) per camera: the backward of the pixel -> direction map of
//                          get_rays_from_pose (src/rays.cpp:7-28) in the calibration that
//                          cams_meta.tsv carries (src/dataset.cpp:59-63) and the reference treats as
//                          exact, summed per camera as f2n_cam_pose_grad sums (cam_pieces.hiph).
//   f2n_intr_compose       fx' = fx exp(g0), cx' = cx + g2 fx, k1' = k1 + g4, ...: one row of eight
//   f2n_intr_compose_bwd   dimensionless numbers per physical camera, shared by its images.
#include "cam_pieces.hiph"

namespace
{

// ---- f2n_cam_intr_grad ----------------------------------------------------------------------------
//
// The forward solves F(x, y; k) = (xd, yd) for the ideal point, xd = (col + .5 - cx) / fx,
// yd = (row + .5 - cy) / fy, and the ray is dir = R (x, -y, -1).  With g = dL/d(x, y) and J = dF/d(x, y)
// (symmetric) the implicit-function theorem at the point the forward returned gives, for a parameter
// q,  dL/dq = lambda . (d(xd, yd)/dq - dF/dq),  lambda = J^-1 g  -- not the derivative of the eight
// unrolled Newton steps.  A pinhole camera has F = identity, J = I, and the same formulas: its
// distortion coefficients receive a gradient too.

struct IntrRays
{
  const float * __restrict__ poses;
  int pose_ld;
  const float * __restrict__ intrinsics;
  const float * __restrict__ dist;
  const int32_t * __restrict__ ij;
  const float * __restrict__ d_d;
  const int32_t * __restrict__ order;
  int n;

  struct Cam
  {
    const float * K;
    LensDist lens;
    float r00, r10, r20;  // column 0 of R
    float r01, r11, r21;  // column 1 of R
  };

  __device__ __forceinline__ Cam camera(int c) const
  {
    const float * P = poses + (int64_t)c * pose_ld;
    return {intrinsics + (int64_t)c * 9, load_lens(dist, c), P[0], P[4], P[8], P[1], P[5], P[9]};
  }

  // the eight terms of the ray at position p, added to acc (fx, fy, cx, cy, k1, k2, p1, p2)
  __device__ __forceinline__ void add(float (&acc)[8], const Cam & cam, int p) const
  {
    const int64_t r = order ? order[p] : p;
    if (r < 0 || r >= n) return;  // a caller's order is not trusted with an address
    const float row = (float)ij[2 * r], col = (float)ij[2 * r + 1];
    float u, v;
    camera_pixel_to_dir(cam.K, cam.lens, row, col, u, v);  // the forward's bits
    const float x = u, y = -v;
    const float fx = cam.K[0], fy = cam.K[4];
    const float xd = ((col + .5f) - cam.K[2]) / fx;
    const float yd = ((row + .5f) - cam.K[5]) / fy;
    const float g0 = d_d[3 * r], g1 = d_d[3 * r + 1], g2 = d_d[3 * r + 2];
    const float gx = (g0 * cam.r00 + g1 * cam.r10) + g2 * cam.r20;
    const float gy = -((g0 * cam.r01 + g1 * cam.r11) + g2 * cam.r21);
    float a = 1.f, b = 0.f, d = 1.f;
    if (!lens_is_pinhole(cam.lens)) lens_jacobian(cam.lens, x, y, a, b, d);
    const float det = a * d - b * b;
    const float lx = (d * gx - b * gy) / det;
    const float ly = (a * gy - b * gx) / det;
    const bool ok = fabsf(det) > kLensMinDet && fabsf(lx) <= 3.4028234664e38f &&
                    fabsf(ly) <= 3.4028234664e38f;  // false for NaN as well
    if (!ok) return;  // exact zeros
    const float xx = x * x, yy = y * y, xy2 = 2.f * (x * y);
    const float r2 = xx + yy;
    const float s = lx * x + ly * y;
    acc[0] += -((lx * xd) / fx);
    acc[1] += -((ly * yd) / fy);
    acc[2] += -(lx / fx);
    acc[3] += -(ly / fy);
    acc[4] += -(r2 * s);
    acc[5] += -((r2 * r2) * s);
    acc[6] += -(xy2 * lx + (r2 + 2.f * yy) * ly);
    acc[7] += -((r2 + 2.f * xx) * lx + xy2 * ly);
  }
};

__global__ __launch_bounds__(F2N_BLOCK) void cam_intr_grad_piece_kernel(
  const float * __restrict__ poses, int pose_ld, const float * __restrict__ intrinsics,
  const float * __restrict__ dist, const int32_t * __restrict__ ij, const float * __restrict__ d_d,
  const int32_t * __restrict__ cam_start, const int32_t * __restrict__ order,
  float * __restrict__ d_intr, float * __restrict__ ws, int n, int E, int G)
{
  const IntrRays rays = {poses, pose_ld, intrinsics, dist, ij, d_d, order, n};
  cam_piece_sums<8>(rays, cam_start, d_intr, 8, ws, n, E, G);
}

__global__ __launch_bounds__(F2N_BLOCK) void cam_intr_grad_final_kernel(
  const int32_t * __restrict__ cam_start, const float * __restrict__ ws, float * __restrict__ d_intr,
  int n, int E, int G)
{
  cam_piece_finish<8>(cam_start, ws, d_intr, 8, n, E, G);
}

// ---- f2n_intr_compose -----------------------------------------------------------------------------
//
// Everything in f64 (E threads: the rate does not matter), each output rounded once to f32.  The
// centre moves in units of the BASE focal length, so the eight numbers are all dimensionless and of
// one scale, and one Adam learning rate fits them.

// the group of image e, or -1: fixed.  A group past the table is never used as an address.
__device__ __forceinline__ int group_of(const int32_t * __restrict__ group, int e, int G)
{
  const int g = group[e];
  return (g < 0 || g >= G) ? -1 : g;
}

__global__ __launch_bounds__(F2N_BLOCK) void intr_compose_kernel(
  const float * __restrict__ base_K, const float * __restrict__ base_dist,
  const float * __restrict__ gamma, const int32_t * __restrict__ group, float * __restrict__ out_K,
  float * __restrict__ out_dist, int E, int G)
{
  const int e = (int)blockIdx.x * F2N_BLOCK + (int)threadIdx.x;
  if (e >= E) return;
  const float * K = base_K + (int64_t)e * 9;
  float * O = out_K + (int64_t)e * 9;
  float * D = out_dist + (int64_t)e * 4;
  const LensDist L = load_lens(base_dist, e);
#pragma unroll
  for (int k = 0; k < 9; k++) O[k] = K[k];  // the base rows, bit for bit
  D[0] = L.k1;
  D[1] = L.k2;
  D[2] = L.p1;
  D[3] = L.p2;
  const int g = group_of(group, e, G);
  if (g < 0) return;
  const float * c = gamma + (int64_t)g * 8;
  const bool zero = c[0] == 0.f && c[1] == 0.f && c[2] == 0.f && c[3] == 0.f && c[4] == 0.f &&
                    c[5] == 0.f && c[6] == 0.f && c[7] == 0.f;
  if (zero) return;
  const double fx = K[0], fy = K[4];
  O[0] = (float)(fx * exp((double)c[0]));
  O[4] = (float)(fy * exp((double)c[1]));
  O[2] = (float)((double)K[2] + (double)c[2] * fx);
  O[5] = (float)((double)K[5] + (double)c[3] * fy);
  D[0] = (float)((double)L.k1 + (double)c[4]);
  D[1] = (float)((double)L.k2 + (double)c[5]);
  D[2] = (float)((double)L.p1 + (double)c[6]);
  D[3] = (float)((double)L.p2 + (double)c[7]);
}

// One thread per (group, column): the images in index order, an f64 sum, rounded once.  O(E) per
// thread and O(E G) in all -- G is the number of physical cameras, a handful.
__global__ __launch_bounds__(F2N_BLOCK) void intr_compose_bwd_kernel(
  const float * __restrict__ base_K, const float * __restrict__ gamma,
  const int32_t * __restrict__ group, const int32_t * __restrict__ learn,
  const float * __restrict__ d_K, const float * __restrict__ d_dist, float * __restrict__ d_gamma,
  int E, int G)
{
  const int t = (int)blockIdx.x * F2N_BLOCK + (int)threadIdx.x;
  if (t >= G * 8) return;
  const int g = t >> 3, k = t & 7;
  if (learn && learn[k] == 0) {
    d_gamma[t] = 0.f;
    return;
  }
  const float * src = k < 4 ? d_K : d_dist;
  if (!src) {  // no gradient came in for this half
    d_gamma[t] = 0.f;
    return;
  }
  // where image e keeps this column's incoming gradient and its base focal length
  const int at = k == 0 ? 0 : (k == 1 ? 4 : (k == 2 ? 2 : 5));
  const int focal = (k & 1) ? 4 : 0;
  const double grow = k < 2 ? exp((double)gamma[t]) : 1.0;
  double acc = 0.0;
  for (int e = 0; e < E; e++) {
    if (group_of(group, e, G) != g) continue;
    if (k < 4)
      acc += (double)src[(int64_t)e * 9 + at] * ((double)base_K[(int64_t)e * 9 + focal] * grow);
    else
      acc += (double)src[(int64_t)e * 4 + (k - 4)];
  }
  d_gamma[t] = (float)acc;
}

}  // namespace

extern "C" int64_t f2n_cam_intr_grad_workspace_floats(int64_t n, int64_t n_cams)
{
  return 8 * (cam_pieces(n < 0 ? 0 : n) + (n_cams < 1 ? 1 : n_cams));
}

extern "C" int f2n_cam_intr_grad(
  const float * poses, int pose_ld, const float * intrinsics, const float * dist, const int32_t * ij,
  const float * d_rays_d, const int32_t * cam_start, const int32_t * order, float * d_intr,
  float * workspace, int64_t n, int64_t n_cams, void * stream)
{
  if (!poses || !intrinsics || !ij || !d_rays_d || !cam_start || !d_intr || !workspace)
    return F2N_E_INVALID_ARG;
  // positions and camera numbers are i32 (cam_start, order), and one thread per component
  if (n < 0 || n > INT32_MAX - kPiece || n_cams < 1 || n_cams > INT32_MAX / 16)
    return F2N_E_INVALID_ARG;
  if (pose_ld != 12 && pose_ld != 16) return F2N_E_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int G = (int)cam_pieces(n);
  if (G > 0) {
    hipLaunchKernelGGL(
      cam_intr_grad_piece_kernel, dim3(f2n_div_up(G, F2N_WAVES_PER_BLOCK)), dim3(F2N_BLOCK), 0, s,
      poses, pose_ld, intrinsics, dist, ij, d_rays_d, cam_start, order, d_intr, workspace, (int)n,
      (int)n_cams, G);
    if (hipGetLastError() != hipSuccess) return F2N_E_LAUNCH;
  }
  // (n == 0: every camera is empty, and this kernel reads n instead of trusting cam_start)
  hipLaunchKernelGGL(
    cam_intr_grad_final_kernel, dim3(f2n_div_up(n_cams * 8, F2N_BLOCK)), dim3(F2N_BLOCK), 0, s,
    cam_start, workspace, d_intr, (int)n, (int)n_cams, G);
  return f2n_launch_status();
}

extern "C" int f2n_intr_compose(
  const float * base_K, const float * base_dist, const float * gamma, const int32_t * group,
  float * out_K, float * out_dist, int64_t n_images, int64_t n_groups, void * stream)
{
  if (!base_K || !gamma || !group || !out_K || !out_dist) return F2N_E_INVALID_ARG;
  if (n_images < 0 || n_images > INT32_MAX / 16 || n_groups < 1 || n_groups > INT32_MAX / 16)
    return F2N_E_INVALID_ARG;
  if (n_images == 0) return F2N_OK;
  hipLaunchKernelGGL(
    intr_compose_kernel, dim3(f2n_div_up(n_images, F2N_BLOCK)), dim3(F2N_BLOCK), 0,
    (hipStream_t)stream, base_K, base_dist, gamma, group, out_K, out_dist, (int)n_images,
    (int)n_groups);
  return f2n_launch_status();
}

extern "C" int f2n_intr_compose_bwd(
  const float * base_K, const float * base_dist, const float * gamma, const int32_t * group,
  const int32_t * learn, const float * d_K, const float * d_dist, float * d_gamma, int64_t n_images,
  int64_t n_groups, void * stream)
{
  (void)base_dist;  // k' = k + gamma: the derivative does not depend on the base coefficients
  if (!base_K || !gamma || !group || !d_gamma) return F2N_E_INVALID_ARG;
  if (n_images < 0 || n_images > INT32_MAX / 16 || n_groups < 1 || n_groups > INT32_MAX / 16)
    return F2N_E_INVALID_ARG;
  // (no images: every group is empty, and d_gamma is still overwritten)
  hipLaunchKernelGGL(
    intr_compose_bwd_kernel, dim3(f2n_div_up(n_groups * 8, F2N_BLOCK)), dim3(F2N_BLOCK), 0,
    (hipStream_t)stream, base_K, gamma, group, learn, d_K, d_dist, d_gamma, (int)n_images,
    (int)n_groups);
  return f2n_launch_status();
}
