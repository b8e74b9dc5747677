// envmap.hip -- a learned background: a cube map of colour logits looked up by ray direction
// (include/f2nerf_hip.h has the contracts).  The reference has no such model: its render blends a
// constant behind the field (src/renderer.cpp:103-110: rand in TRAIN, 0.5 otherwise).  Here
// tex [6, R, R, 3] f32 holds logits, 2 <= R <= 4096; a lookup uses the direction alone (any length),
// filters bilinearly inside one face and squashes with a sigmoid, so a texture of zeros is the
// render's own inference default, 0.5f, exactly.  Filtering clamps to the face's edge: there is no
// seamless filtering across faces.
//
// EVALUATION ORDER (tests/envmap_model.py follows these lines; the library is built with
// -ffp-contract=off, so only the fmaf spelled out below is fused).  All f32 unless said otherwise.
//   per ray, one lane each (256-lane workgroups), d = (x, y, z):
//     ax,ay,az = |x|,|y|,|z|
//     axis = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2)        a NaN compares false
//     m    = that |component|;  face = 2*axis + (component < 0)     (-0.0 is not < 0)
//     a ray whose m is not finite and positive (zero vector, NaN, inf) is DEGENERATE: bg = 0.5f in
//     all three channels, nothing else is read, and the backward skips it
//     (a,b) = axis 0: (y,z)   axis 1: (x,z)   axis 2: (x,y)         no sign flips
//     s = a / m;  t = b / m                                         IEEE division
//     u = fmaf(fmaf(s, 0.5f, 0.5f), (float)R, -0.5f)
//     u = u > 0.f ? u : 0.f;  u = u < (float)(R-1) ? u : (float)(R-1)     a NaN lands on 0
//     x0 = (int)floorf(u);  x1 = min(x0+1, R-1);  fx = u - (float)x0     exact
//     v, y0, y1, fy likewise from t
//     gx = 1.f - fx;  gy = 1.f - fy                                 one rounding each
//     w00 = gx*gy;  w10 = fx*gy;  w01 = gx*fy;  w11 = fx*fy         one rounding each
//   per channel c, Tjk = tex[face, y_k, x_j, c] = tex[((face*R + y_k)*R + x_j)*3 + c]:
//     logit = fmaf(w11, T11, fmaf(w01, T01, fmaf(w10, T10, w00*T00)))
//     bg    = 1.f / (1.f + expf(-logit))
//   backward, one lane per ray, the geometry recomputed exactly as above, bg the forward's output:
//     om = 1.f - bg;  ds = bg*om;  gl = d_bg*ds                     one rounding each
//     gl == 0: nothing.  gl not finite: bit 0 of flags, nothing added.  Otherwise for the corners
//     in the order 00, 10, 01, 11 with weight w:
//       p = (double)gl * (double)w                                  exact (24 x 24 bits)
//       v = ldexp(p, F2N_ENVMAP_SHIFT)                              exact
//       |v| > 2^62: v = copysign(2^62, v), bit 1 of flags
//       q = llrint(v)                                               round half to even
//       q != 0: acc[texel*3 + c] += q, a 64-bit integer atomicAdd in global memory
//     Integer sums do not depend on their order: the same bits on every run.  flags gets its bits
//     by atomicOr, and only from a lane that has one to set.
//   apply, one lane per element i of acc:
//     g = (float)ldexp((double)acc[i], -F2N_ENVMAP_SHIFT)           int64 -> f64 -> f32, both RNE
//     d_tex[i] = accumulate ? d_tex[i] + g : g;  acc[i] = 0
// No workgroup waits on another, no float atomics, no pre-combining inside a wavefront (most rays
// of a training batch are opaque, d_bg == 0, and issue no atomic at all).
#include "common.hiph"

namespace
{

constexpr int kEnvBlock = 256;
constexpr int kEnvMinR = 2, kEnvMaxR = 4096;

inline bool env_res_ok(int R) { return R >= kEnvMinR && R <= kEnvMaxR; }

struct EnvTap
{
  bool live;           // false: a degenerate ray
  int64_t t00, t10, t01, t11;  // texel indices (not yet times 3)
  float w00, w10, w01, w11;
};

__device__ __forceinline__ void env_axis(float s, int R, int & i0, int & i1, float & f)
{
  const float top = (float)(R - 1);
  float u = fmaf(fmaf(s, 0.5f, 0.5f), (float)R, -0.5f);
  u = u > 0.f ? u : 0.f;
  u = u < top ? u : top;
  i0 = (int)floorf(u);  // 0 .. R-1
  i1 = i0 + 1 < R ? i0 + 1 : R - 1;
  f = u - (float)i0;
}

__device__ __forceinline__ EnvTap env_tap(float x, float y, float z, int R)
{
  EnvTap tp;
  const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
  const int axis = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
  const float comp = axis == 0 ? x : (axis == 1 ? y : z);
  const float m = axis == 0 ? ax : (axis == 1 ? ay : az);
  tp.live = m > 0.f && m < __builtin_huge_valf();  // NaN fails both
  tp.t00 = tp.t10 = tp.t01 = tp.t11 = 0;
  tp.w00 = tp.w10 = tp.w01 = tp.w11 = 0.f;
  if (!tp.live) return tp;
  const int face = 2 * axis + (comp < 0.f ? 1 : 0);
  const float a = axis == 0 ? y : x;
  const float b = axis == 2 ? y : z;
  const float s = a / m, t = b / m;
  int x0, x1, y0, y1;
  float fx, fy;
  env_axis(s, R, x0, x1, fx);
  env_axis(t, R, y0, y1, fy);
  const float gx = 1.f - fx, gy = 1.f - fy;
  tp.w00 = gx * gy;
  tp.w10 = fx * gy;
  tp.w01 = gx * fy;
  tp.w11 = fx * fy;
  const int64_t row0 = ((int64_t)face * R + y0) * R, row1 = ((int64_t)face * R + y1) * R;
  tp.t00 = row0 + x0;
  tp.t10 = row0 + x1;
  tp.t01 = row1 + x0;
  tp.t11 = row1 + x1;  // all below 6*R*R
  return tp;
}

__global__ __launch_bounds__(kEnvBlock) void envmap_fwd_kernel(
  const float * __restrict__ dirs, const float * __restrict__ tex, int R, float * __restrict__ bg,
  int n_rays)
{
  const int r = blockIdx.x * kEnvBlock + threadIdx.x;
  if (r >= n_rays) return;
  const EnvTap tp = env_tap(dirs[3 * (int64_t)r], dirs[3 * (int64_t)r + 1], dirs[3 * (int64_t)r + 2], R);
  float * out = bg + 3 * (int64_t)r;
  if (!tp.live) {
    out[0] = out[1] = out[2] = 0.5f;
    return;
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float T00 = tex[3 * tp.t00 + c], T10 = tex[3 * tp.t10 + c], T01 = tex[3 * tp.t01 + c],
                T11 = tex[3 * tp.t11 + c];
    const float logit = fmaf(tp.w11, T11, fmaf(tp.w01, T01, fmaf(tp.w10, T10, tp.w00 * T00)));
    out[c] = 1.f / (1.f + expf(-logit));
  }
}

// bit 0: a gradient that is not finite was dropped; bit 1: a contribution was capped at 2^62
__device__ __forceinline__ int env_add(long long * acc, int64_t i, float gl, float w)
{
  const double p = (double)gl * (double)w;
  double v = ldexp(p, F2N_ENVMAP_SHIFT);
  int flag = 0;
  if (fabs(v) > 4611686018427387904.0) {
    v = copysign(4611686018427387904.0, v);
    flag = 2;
  }
  const long long q = llrint(v);
  if (q != 0) atomicAdd(reinterpret_cast<unsigned long long *>(acc + i), (unsigned long long)q);
  return flag;
}

__global__ __launch_bounds__(kEnvBlock) void envmap_bwd_kernel(
  const float * __restrict__ dirs, const float * __restrict__ bg, const float * __restrict__ d_bg,
  int R, long long * __restrict__ acc, int * __restrict__ flags, int n_rays)
{
  const int r = blockIdx.x * kEnvBlock + threadIdx.x;
  if (r >= n_rays) return;
  float gl[3];
  bool any = false;
  int flag = 0;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float b = bg[3 * (int64_t)r + c];
    const float om = 1.f - b;
    const float ds = b * om;
    gl[c] = d_bg[3 * (int64_t)r + c] * ds;
    any = any || gl[c] != 0.f;  // a NaN counts: it is flagged below, if the ray is live
  }
  if (!any) return;
  const EnvTap tp = env_tap(dirs[3 * (int64_t)r], dirs[3 * (int64_t)r + 1], dirs[3 * (int64_t)r + 2], R);
  if (!tp.live) return;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (gl[c] == 0.f) continue;
    if (!(fabsf(gl[c]) < __builtin_huge_valf())) {
      flag |= 1;
      continue;
    }
    flag |= env_add(acc, 3 * tp.t00 + c, gl[c], tp.w00);
    flag |= env_add(acc, 3 * tp.t10 + c, gl[c], tp.w10);
    flag |= env_add(acc, 3 * tp.t01 + c, gl[c], tp.w01);
    flag |= env_add(acc, 3 * tp.t11 + c, gl[c], tp.w11);
  }
  if (flag) atomicOr(flags, flag);
}

__global__ __launch_bounds__(kEnvBlock) void envmap_grad_apply_kernel(
  long long * __restrict__ acc, float * __restrict__ d_tex, int accumulate, int64_t n)
{
  const int64_t i = (int64_t)blockIdx.x * kEnvBlock + threadIdx.x;
  if (i >= n) return;
  const float g = (float)ldexp((double)acc[i], -F2N_ENVMAP_SHIFT);
  d_tex[i] = accumulate ? d_tex[i] + g : g;
  acc[i] = 0;
}

}  // namespace

extern "C" int64_t f2n_envmap_texels(int R) { return env_res_ok(R) ? 6 * (int64_t)R * R : 0; }

extern "C" int f2n_envmap_fwd(
  const float * dirs, const float * tex, int R, float * bg, int n_rays, void * stream)
{
  if (!dirs || !tex || !bg || n_rays < 0 || !env_res_ok(R)) return F2N_E_INVALID_ARG;
  if (n_rays == 0) return F2N_OK;
  hipLaunchKernelGGL(
    envmap_fwd_kernel, dim3(f2n_div_up(n_rays, kEnvBlock)), dim3(kEnvBlock), 0, (hipStream_t)stream,
    dirs, tex, R, bg, n_rays);
  return f2n_launch_status();
}

extern "C" int f2n_envmap_bwd(
  const float * dirs, const float * bg, const float * d_bg, int R, int64_t * acc, int32_t * flags,
  int n_rays, void * stream)
{
  if (!dirs || !bg || !d_bg || !acc || !flags || n_rays < 0 || !env_res_ok(R))
    return F2N_E_INVALID_ARG;
  if (n_rays == 0) return F2N_OK;
  hipLaunchKernelGGL(
    envmap_bwd_kernel, dim3(f2n_div_up(n_rays, kEnvBlock)), dim3(kEnvBlock), 0, (hipStream_t)stream,
    dirs, bg, d_bg, R, (long long *)acc, (int *)flags, n_rays);
  return f2n_launch_status();
}

extern "C" int f2n_envmap_grad_apply(
  int64_t * acc, int R, float * d_tex, int accumulate, void * stream)
{
  if (!acc || !d_tex || !env_res_ok(R) || (accumulate != 0 && accumulate != 1))
    return F2N_E_INVALID_ARG;
  const int64_t n = 18 * (int64_t)R * R;
  hipLaunchKernelGGL(
    envmap_grad_apply_kernel, dim3(f2n_div_up(n, kEnvBlock)), dim3(kEnvBlock), 0,
    (hipStream_t)stream, (long long *)acc, d_tex, accumulate, n);
  return f2n_launch_status();
}
