// density_lattice_rows.hip -- the lane mapping f2n_density_lattice does NOT use, kept as a probe so
// that tools/microbench_mesh.py can measure it beside the one it does: a wavefront is 64 consecutive x
// of one lattice row (coalesced 256-byte stores, but 64 vertices strung along one axis touch more
// cells of a level than a 4 x 4 x 4 brick).  Same arithmetic and the same bits as
// f2-nerf_amd/csrc/kernels/density_lattice.hip; figures in NOTES.md section 29.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -shared \
//     -I include -I f2-nerf_amd/csrc/kernels -o tools/probes/libdensity_lattice_rows.so \
//     tools/probes/density_lattice_rows.hip          (tools/microbench_mesh.py does this itself)
#include "hash_grid.hiph"

namespace
{

template <int F, bool POW2>
__global__ __launch_bounds__(F2N_BLOCK) void density_lattice_rows_kernel(
  const uint16_t * __restrict__ table, const int32_t * __restrict__ primes,
  const float * __restrict__ bias, const float * __restrict__ mul, const float * __restrict__ w0,
  const float * __restrict__ b0, float * __restrict__ logit, float lo_x, float lo_y, float lo_z,
  float step_x, float step_y, float step_z, int nx, int ny, int nz, int chunks, int L, uint32_t T,
  int64_t level_stride, int first_pass)
{
  const uint32_t wave = blockIdx.x * (uint32_t)F2N_WAVES_PER_BLOCK + (threadIdx.x >> 6);
  const uint32_t cx = wave % (uint32_t)chunks, row = wave / (uint32_t)chunks;
  const int iy = (int)(row % (uint32_t)ny), iz = (int)(row / (uint32_t)ny);
  const int ix = (int)(64u * cx) + lane_id();
  if (ix >= nx || iz >= nz) return;
  float x = fmaf((float)ix, step_x, lo_x);
  float y = fmaf((float)iy, step_y, lo_y);
  float z = fmaf((float)iz, step_z, lo_z);
  contract_point(x, y, z);
  float * out = logit + ((int64_t)iz * ny + iy) * nx + ix;
  const float start = first_pass ? b0[0] : *out;
  *out = density_chain_in_order<F, POW2, true>(
    x, y, z, table, primes, bias, mul, w0, start, L, T, level_stride, [](int, __half) {});
}

constexpr int64_t kPassTableBytes = (int64_t)2 << 20;  // as density_lattice.hip

}  // namespace

extern "C" int f2n_density_lattice_rows(
  const uint16_t * table_f16, const int32_t * primes, const float * bias, const float * mul,
  const float * w0, const float * b0, float * logit, float lo_x, float lo_y, float lo_z,
  float step_x, float step_y, float step_z, int nx, int ny, int nz, int L, int F, uint32_t T,
  int64_t level_stride, void * stream)
{
  if (nx < 2 || ny < 2 || nz < 2) return F2N_E_INVALID_ARG;
  if ((int64_t)nx * ny >= ((int64_t)1 << 31) || (int64_t)nx * ny * nz >= ((int64_t)1 << 31))
    return F2N_E_INVALID_ARG;
  if (!(step_x > 0.f) || !(step_y > 0.f) || !(step_z > 0.f)) return F2N_E_INVALID_ARG;
  if (const int st = f2n_field_args_status(L, F, T, level_stride)) return st;
  if (L > F2N_MAX_LEVELS) return F2N_E_UNSUPPORTED;
  if (!table_f16 || !primes || !bias || !mul || !w0 || !b0 || !logit) return F2N_E_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(table_f16) % (2u * F)) return F2N_E_INVALID_ARG;
  const int chunks = (nx + 63) / 64;
  const int64_t waves = (int64_t)chunks * ny * nz;
  const dim3 grid(f2n_div_up(waves, F2N_WAVES_PER_BLOCK)), block(F2N_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  // the level passes of density_lattice.hip
  const int64_t level_bytes = 2 * (int64_t)T * F, stride_bytes = 2 * level_stride;
  int per_pass = 1;
  while (per_pass < L && per_pass * stride_bytes + level_bytes <= kPassTableBytes) per_pass++;
  f2n_dispatch_field(F, T, [&](auto ff, auto p2) {
    for (int l0 = 0; l0 < L; l0 += per_pass) {
      hipLaunchKernelGGL(
        (density_lattice_rows_kernel<decltype(ff)::value, decltype(p2)::value>), grid, block, 0, s,
        table_f16 + level_stride * l0, primes + 3 * l0, bias + 3 * l0, mul + l0, w0 + (int64_t)l0 * F,
        b0, logit, lo_x, lo_y, lo_z, step_x, step_y, step_z, nx, ny, nz, chunks,
        (L - l0 < per_pass) ? L - l0 : per_pass, T, level_stride, l0 == 0 ? 1 : 0);
    }
  });
  return f2n_launch_status();
}
