// loss_sup.hip -- the training loss with per-ray weights and alpha targets (include/f2nerf_hip.h has
// the definition).  It stands beside f2n_loss_fwd (loss.hip; reference src/main_functions/
// train_manager.cpp:78-96), which it leaves alone: the reference averages over every ray of the batch
// and knows neither a mask nor an alpha channel.  With m_r the ray weight (1 when absent), a_r the
// alpha target, O_r the rendered opacity, W = sum_r m_r (W = 1 when that sum is not positive):
//     gt'_rc = a_r gt_rc + (1 - a_r) bg_rc                       (alpha given; else gt' = gt)
//     colour = sum_r m_r sum_c sqrt((C_rc - gt'_rc)^2 + 1e-4) / (3 W)
//     var    = sum_r m_r sqrt(var_r + 1e-2) / W
//     opac   = sum_r m_r (O_r - a_r)^2 / W                       (alpha and opacity given; else 0)
//     loss   = colour + var_weight var + opacity_weight opac
//     out    = {loss, colour, var, opac, sum_r m_r sum_c (C - gt')^2, sum_r m_r}
// Three launches: one partial per workgroup, one single-workgroup tree that also writes out[6], and
// one pass that scales the gradients by 1 / W, which is only known after the sums.  No host read, no
// atomics: the same bits on every run.
//
// EVALUATION ORDER (tests/supervision_model.py counts its bound from these lines; the library is
// built with -ffp-contract=off, so only the fmaf spelled out below is fused).  All f32.
//   per ray, one lane each (256-lane workgroups):
//     m = ray_weight ? ray_weight[r] : 1.f
//     a ray with m == 0 reads nothing else: its terms are +0 and its gradients are written as +0
//     (a masked ray's colour may be anything, NaN included)
//   per channel c, alpha given:
//     om = 1.f - a                                  one rounding
//     tb = om * bg                                  one rounding
//     g  = fmaf(a, gt, tb)                          FMA: one rounding          (else g = gt, exact)
//   then
//     e  = C - g                                    one rounding
//     e2 = e * e                                    one rounding
//     rt = sqrtf(e2 + 1e-4f)                        two roundings (add, correctly rounded sqrt)
//     q  = e / rt                                   one rounding
//   per ray
//     s_col = m * ((rt_0 + rt_1) + rt_2)            two adds, one product
//     s_sq  = m * ((e2_0 + e2_1) + e2_2)            two adds, one product
//     u_col_c = m * q_c                             one rounding   (unscaled colour gradient)
//     rv = sqrtf(var + 1e-2f)                       two roundings
//     s_var = m * rv                                one rounding
//     u_var = (0.5f * var_weight) / rv * m          0.5f * var_weight exact; a division, a product
//     do = O - a                                    one rounding               (alpha and opacity given)
//     s_op = m * (do * do)                          two roundings
//     u_op = (2.f * opacity_weight) * do * m        2.f * opacity_weight exact; two products
//   the five sums (s_col, s_var, s_op, s_sq, m) per workgroup: wave_sum (the DPP scan tree of
//     common.hiph: 6 additions on a path), then the 4 wave totals added in order by thread 0;
//   the tree: thread t adds partials t, t + 256, ... in ascending order, then the same workgroup sum.
//     A term passes through at most 20 + ceil(n_blocks / 256) additions.
//   finish, thread 0:
//     W    = (sum_m > 0.f) ? sum_m : 1.f            (NaN counts as not positive)
//     colour = s_col / (3.f * W)                    one product, one division
//     var    = s_var / W,  opac = s_op / W          one division each
//     loss   = (colour + var * var_weight) + opac * opacity_weight      two products, two adds
//   scale, one lane per ray, W formed from out[5] exactly as above:
//     i3 = 1.f / (3.f * W),  i1 = 1.f / W           one product and one division; one division
//     d_colors = u_col * i3,  d_var = u_var * i1,  d_opacity = u_op * i1      one product each
#include "common.hiph"

namespace
{

constexpr int kSupBlock = 256;
constexpr int kSupSums = 5;

__device__ __forceinline__ float sup_block_sum(float v, float * smem)
{
  v = wave_sum(v);
  const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
  __syncthreads();
  if (lane == 0) smem[wave] = v;
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < kSupBlock / 64; i++) t += smem[i];
  }
  return t;  // valid in thread 0
}

__device__ __forceinline__ float sup_divisor(float sum_m) { return sum_m > 0.f ? sum_m : 1.f; }

__global__ __launch_bounds__(kSupBlock) void loss_sup_partial_kernel(
  const float * __restrict__ colors, const float * __restrict__ gt, const float * __restrict__ var,
  const float * __restrict__ ray_weight, const float * __restrict__ alpha,
  const float * __restrict__ opacity, const float * __restrict__ bg, float var_weight,
  float opacity_weight, float * __restrict__ d_colors, float * __restrict__ d_var,
  float * __restrict__ d_opacity, float * __restrict__ partial, int n_rays)
{
  __shared__ float smem[kSupBlock / 64];
  const int r = blockIdx.x * kSupBlock + threadIdx.x;
  const bool with_op = alpha && opacity;
  float s_col = 0.f, s_var = 0.f, s_op = 0.f, s_sq = 0.f, s_m = 0.f;
  if (r < n_rays) {
    const float m = ray_weight ? ray_weight[r] : 1.f;
    s_m = m;
    if (m == 0.f) {
      d_colors[3 * r] = d_colors[3 * r + 1] = d_colors[3 * r + 2] = 0.f;
      d_var[r] = 0.f;
      if (with_op) d_opacity[r] = 0.f;
    } else {
      const float a = alpha ? alpha[r] : 1.f;
      const float om = 1.f - a;
      float rt[3], e2[3];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        float g = gt[3 * r + c];
        if (alpha) g = fmaf(a, g, om * bg[3 * r + c]);
        const float e = colors[3 * r + c] - g;
        e2[c] = e * e;
        rt[c] = sqrtf(e2[c] + 1e-4f);
        d_colors[3 * r + c] = m * (e / rt[c]);
      }
      s_col = m * ((rt[0] + rt[1]) + rt[2]);
      s_sq = m * ((e2[0] + e2[1]) + e2[2]);
      const float rv = sqrtf(var[r] + 1e-2f);
      s_var = m * rv;
      d_var[r] = (0.5f * var_weight) / rv * m;
      if (with_op) {
        const float dop = opacity[r] - a;
        s_op = m * (dop * dop);
        d_opacity[r] = (2.f * opacity_weight) * dop * m;
      }
    }
  }
  const float t0 = sup_block_sum(s_col, smem), t1 = sup_block_sum(s_var, smem),
              t2 = sup_block_sum(s_op, smem), t3 = sup_block_sum(s_sq, smem),
              t4 = sup_block_sum(s_m, smem);
  if (threadIdx.x == 0) {
    float * p = partial + kSupSums * (int64_t)blockIdx.x;
    p[0] = t0;
    p[1] = t1;
    p[2] = t2;
    p[3] = t3;
    p[4] = t4;
  }
}

// out = {loss, colour, var, opac, sq_err_sum, sum_m}
__global__ __launch_bounds__(kSupBlock) void loss_sup_finish_kernel(
  const float * __restrict__ partial, int n_blocks, float var_weight, float opacity_weight,
  float * __restrict__ out)
{
  __shared__ float smem[kSupBlock / 64];
  float s[kSupSums] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < n_blocks; i += kSupBlock) {
#pragma unroll
    for (int k = 0; k < kSupSums; k++) s[k] += partial[kSupSums * (int64_t)i + k];
  }
#pragma unroll
  for (int k = 0; k < kSupSums; k++) s[k] = sup_block_sum(s[k], smem);
  if (threadIdx.x == 0) {
    const float W = sup_divisor(s[4]);
    const float colour = s[0] / (3.f * W), var = s[1] / W, opac = s[2] / W;
    out[0] = (colour + var * var_weight) + opac * opacity_weight;
    out[1] = colour;
    out[2] = var;
    out[3] = opac;
    out[4] = s[3];
    out[5] = s[4];
  }
}

__global__ __launch_bounds__(kSupBlock) void loss_sup_scale_kernel(
  const float * __restrict__ out, float * __restrict__ d_colors, float * __restrict__ d_var,
  float * __restrict__ d_opacity, int n_rays)
{
  const int r = blockIdx.x * kSupBlock + threadIdx.x;
  if (r >= n_rays) return;
  const float W = sup_divisor(out[5]);
  const float i3 = 1.f / (3.f * W), i1 = 1.f / W;
#pragma unroll
  for (int c = 0; c < 3; c++) d_colors[3 * r + c] = d_colors[3 * r + c] * i3;
  d_var[r] = d_var[r] * i1;
  if (d_opacity) d_opacity[r] = d_opacity[r] * i1;
}

}  // namespace

extern "C" int64_t f2n_loss_sup_workspace_floats(int n_rays)
{
  return kSupSums * (int64_t)f2n_div_up(n_rays > 0 ? n_rays : 1, kSupBlock);
}

extern "C" int f2n_loss_sup_fwd(
  const float * colors, const float * gt, const float * var, const float * ray_weight,
  const float * alpha, const float * opacity, const float * bg, int n_rays, float var_weight,
  float opacity_weight, float * d_colors, float * d_var, float * d_opacity, float * partial,
  float * out6, void * stream)
{
  if (!colors || !gt || !var || !d_colors || !d_var || !partial || !out6 || n_rays <= 0)
    return F2N_E_INVALID_ARG;
  if (alpha && !bg) return F2N_E_INVALID_ARG;
  if (alpha && opacity_weight != 0.f && !opacity) return F2N_E_INVALID_ARG;
  if (alpha && opacity && !d_opacity) return F2N_E_INVALID_ARG;
  const bool with_op = alpha && opacity;
  const int n_blocks = (int)f2n_div_up(n_rays, kSupBlock);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(
    loss_sup_partial_kernel, dim3(n_blocks), dim3(kSupBlock), 0, s, colors, gt, var, ray_weight,
    alpha, opacity, bg, var_weight, opacity_weight, d_colors, d_var, d_opacity, partial, n_rays);
  hipLaunchKernelGGL(
    loss_sup_finish_kernel, dim3(1), dim3(kSupBlock), 0, s, partial, n_blocks, var_weight,
    opacity_weight, out6);
  hipLaunchKernelGGL(
    loss_sup_scale_kernel, dim3(n_blocks), dim3(kSupBlock), 0, s, out6, d_colors, d_var,
    with_op ? d_opacity : nullptr, n_rays);
  return f2n_launch_status();
}
