// ray_walk_probe.hip -- f2n_ray_walk_probe: the ray walk of sampler.hiph made visible at every lane
// mapping.  A diagnostic entry: nothing in the host library calls it.
//
// The march and the one-pass render kernels run make_stride and keep_step with 64, 16 or 8 lanes to a
// ray, but only their counts and composited colours ever leave the device.  This kernel walks EVERY
// stride of every ray with the chosen RayLanes<W> and writes, per sample, what the walk holds in that
// lane: the sample (p, dt, t) and, with an optical depth per sample handed in, keep_step's exclusive
// depth and keep decision.  No field, no early break: live = the lane holds a sample.
#include "sampler.hiph"

namespace
{

template <int W>
__global__ __launch_bounds__(F2N_BLOCK) void ray_walk_probe_kernel(
  const float * __restrict__ rays_o, const float * __restrict__ rays_d,
  const float * __restrict__ noise, const float * __restrict__ sec_in, float * __restrict__ pts,
  float * __restrict__ dt, float * __restrict__ t, float * __restrict__ depth,
  uint8_t * __restrict__ keep, int n_rays, int S, float step, float t_thresh)
{
  using RL = RayLanes<W>;
  const int wave = (int)blockIdx.x * F2N_WAVES_PER_BLOCK + (int)(threadIdx.x >> 6);
  const int r0 = wave * RL::kRays;
  if (r0 >= n_rays) return;
  const int lane = lane_id();
  const int r_raw = r0 + RL::group(lane);
  const bool has_ray = r_raw < n_rays;
  const int r = has_ray ? r_raw : n_rays - 1;  // (the spare groups of the last wave redo the last ray)
  const RayFrame rf = load_ray(rays_o, rays_d, r);
  const int64_t base = (int64_t)r * S;
  const float * nrow = noise ? noise + base : nullptr;
  StrideState<W> carry = {};
  DepthState<W> ds = {};
  for (int k0 = 0; k0 < S; k0 += W) {
    const StrideSample sm = make_stride(rf, nrow, k0, S, step, carry, lane);
    const int64_t i = base + k0 + RL::sample(lane);
    const float sec = (sec_in && sm.valid) ? sec_in[i] : 0.f;
    const KeepStep ks = keep_step(sec, sm.valid, k0, S, t_thresh, ds, lane);
    if (has_ray && sm.valid) {
      pts[3 * i] = sm.px;
      pts[3 * i + 1] = sm.py;
      pts[3 * i + 2] = sm.pz;
      dt[i] = sm.dt;
      t[i] = sm.t;
      if (sec_in) {
        depth[i] = ks.depth;
        keep[i] = ks.keep ? 1 : 0;
      }
    }
  }
}

}  // namespace

extern "C" int f2n_ray_walk_probe(
  const float * rays_o, const float * rays_d, const float * noise, const float * sec_in, int width,
  float * pts, float * dt, float * t, float * depth, uint8_t * keep, int n_rays, int S, float step,
  float t_thresh, void * stream)
{
  if (n_rays < 0 || S < 1) return F2N_E_INVALID_ARG;
  if (width != 64 && width != 16 && width != 8) return F2N_E_INVALID_ARG;
  if ((int64_t)n_rays * S > INT32_MAX) return F2N_E_INVALID_ARG;
  if (n_rays == 0) return F2N_OK;
  if (!rays_o || !rays_d || !pts || !dt || !t) return F2N_E_INVALID_ARG;
  if (sec_in && (!depth || !keep)) return F2N_E_INVALID_ARG;
  const int rays_per_wave = 64 / width;
  const dim3 grid(f2n_div_up(n_rays, F2N_WAVES_PER_BLOCK * rays_per_wave)), block(F2N_BLOCK);
  hipStream_t s = (hipStream_t)stream;
#define F2N_PROBE(WW)                                                                              \
  hipLaunchKernelGGL(                                                                              \
    (ray_walk_probe_kernel<WW>), grid, block, 0, s, rays_o, rays_d, noise, sec_in, pts, dt, t,     \
    depth, keep, n_rays, S, step, t_thresh)
  switch (width) {
    case 64: F2N_PROBE(64); break;
    case 16: F2N_PROBE(16); break;
    default: F2N_PROBE(8); break;
  }
#undef F2N_PROBE
  return f2n_launch_status();
}
