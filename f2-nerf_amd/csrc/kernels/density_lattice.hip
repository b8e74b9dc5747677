// density_lattice.hip -- the density logit on the vertices of an axis-aligned lattice in raw world
// space: no point array in, no encoding out, 4 bytes of memory traffic per vertex beside the gathers.
//
//   f2n_density_lattice  one lane per lattice vertex.  p = fmaf((float)i, step, lo) per axis, then the
//                        evaluation f2n_density_march and f2n_occ_update share: contract_point and
//                        density_chain_in_order (hash_grid.hiph) -- gather, per-channel f16 rounding,
//                        logit = fmaf(enc_c, w0[c], logit) in level order from b0.  density_shift is
//                        not subtracted.  A vertex at |p| == 0 yields NaN (quirk Q6) for itself only.
//
// Lane mapping.  The cost unit is the distinct 128-byte line per gather instruction (DESIGN.md
// section 5), so a wavefront should cover as few cells of a level as 64 vertices can: it is a
// 4 x 4 x 4 brick of vertices, lane = 16 bz + 4 by + bx.  Bricks are walked in Morton order inside
// super-bricks of 4 x 4 x 4 bricks (wave index bits: x0 y0 z0 x1 y1 z1), super-bricks x fastest: the
// four waves of a workgroup are a 2 x 2 x 1 block of bricks and consecutive workgroups stay inside one
// 16^3 block of vertices for sixteen workgroups.  Bricks that stick out of the lattice run with the
// lanes outside switched off; waves whose whole brick lies outside leave at once.  The corner rows
// are loaded in vertex-parity order (slot_rows_and_weights): neighbouring cells then ask for the
// vertex they share in the same load.
//
// Level passes.  A lane that walks all L levels at once gathers from the whole table (34 MiB at
// L = 16, F = 2, T = 2^19), which no L2 holds.  The entry therefore launches the kernel once per group
// of consecutive levels whose window of the table fits kPassTableBytes, in level order on the
// caller's stream: the first pass starts the chain from b0, every later one from the logit the pass
// before it stored, so the chain is the one chain, fmaf by fmaf, and the bits do not depend on the
// grouping.  A later pass costs 8 bytes per vertex of traffic; a small table takes one pass.
//
// The reference evaluates its field only on ray samples (src/renderer.cpp:61-62 through
// src/hash_3d_anchored.cpp:79-82); this entry has no counterpart there.
#include "hash_grid.hiph"

namespace
{

template <int F, bool POW2>
__global__ __launch_bounds__(F2N_BLOCK) void density_lattice_kernel(
  const uint16_t * __restrict__ table, const int32_t * __restrict__ primes,
  const float * __restrict__ bias, const float * __restrict__ mul, const float * __restrict__ w0,
  const float * __restrict__ b0, float * __restrict__ logit, float lo_x, float lo_y, float lo_z,
  float step_x, float step_y, float step_z, int nx, int ny, int nz, int sbx, int sby, int L,
  uint32_t T, int64_t level_stride, int first_pass)
{
  // (table, primes, bias, mul, w0 start at this pass's first level, L is its number of levels)
  // (wave-uniform up to the brick's origin)
  const uint32_t wave = blockIdx.x * (uint32_t)F2N_WAVES_PER_BLOCK + (threadIdx.x >> 6);
  const uint32_t m = wave & 63u, sb = wave >> 6;
  const uint32_t mx = (m & 1u) | ((m >> 2) & 2u), my = ((m >> 1) & 1u) | ((m >> 3) & 2u),
                 mz = ((m >> 2) & 1u) | ((m >> 4) & 2u);
  const uint32_t sx = sb % (uint32_t)sbx, sy = (sb / (uint32_t)sbx) % (uint32_t)sby,
                 sz = sb / ((uint32_t)sbx * (uint32_t)sby);
  const int lane = lane_id();
  const int ix = (int)(16u * sx + 4u * mx) + (lane & 3);
  const int iy = (int)(16u * sy + 4u * my) + ((lane >> 2) & 3);
  const int iz = (int)(16u * sz + 4u * mz) + (lane >> 4);
  if (ix >= nx || iy >= ny || iz >= nz) return;
  float x = fmaf((float)ix, step_x, lo_x);
  float y = fmaf((float)iy, step_y, lo_y);
  float z = fmaf((float)iz, step_z, lo_z);
  contract_point(x, y, z);
  float * out = logit + ((int64_t)iz * ny + iy) * nx + ix;
  const float start = first_pass ? b0[0] : *out;
  *out = density_chain_in_order<F, POW2, true>(
    x, y, z, table, primes, bias, mul, w0, start, L, T, level_stride, [](int, __half) {});
}

// The table bytes one pass may gather from: half of an XCD's 4 MiB L2, the other half left to the
// lattice's own traffic and to the pass before, which may still be draining.
constexpr int64_t kPassTableBytes = (int64_t)2 << 20;

}  // namespace

extern "C" int f2n_density_lattice(
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
  // super-bricks of 16^3 vertices, 64 waves = 16 workgroups each: fewer than 2^31 / 64 of them
  const int sbx = (nx + 15) / 16, sby = (ny + 15) / 16, sbz = (nz + 15) / 16;
  const dim3 grid((unsigned)((int64_t)sbx * sby * sbz * (64 / F2N_WAVES_PER_BLOCK))), block(F2N_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  // levels per pass: g levels reach over (g - 1) level_stride + T F elements of 2 bytes
  const int64_t level_bytes = 2 * (int64_t)T * F, stride_bytes = 2 * level_stride;
  int per_pass = 1;
  while (per_pass < L && per_pass * stride_bytes + level_bytes <= kPassTableBytes) per_pass++;
  f2n_dispatch_field(F, T, [&](auto ff, auto p2) {
    for (int l0 = 0; l0 < L; l0 += per_pass) {
      hipLaunchKernelGGL(
        (density_lattice_kernel<decltype(ff)::value, decltype(p2)::value>), grid, block, 0, s,
        table_f16 + level_stride * l0, primes + 3 * l0, bias + 3 * l0, mul + l0, w0 + (int64_t)l0 * F,
        b0, logit, lo_x, lo_y, lo_z, step_x, step_y, step_z, nx, ny, nz, sbx, sby,
        (L - l0 < per_pass) ? L - l0 : per_pass, T, level_stride, l0 == 0 ? 1 : 0);
    }
  });
  return f2n_launch_status();
}
