// occ_visibility.hip -- which cells of the occupancy bitfield (occupancy.hiph) the training cameras
// can sample: the marks of the cameras' rays, their dilation, per-cell view counts and the threshold.
//
// No reference counterpart (the reference fork has no occupancy grid, occupancy.hip).  A cell that no
// training ray samples has a density nothing supervises; f2n_occ_update keeps or drops it by chance,
// and a render from a pose off the training trajectory crosses it.  The set computed here is ANDed
// into an OccupancyGrid (host/occupancy_grid.hpp: set_allowed), so no route sees a bit outside it.
//
// The mark is the sampler's own walk without the field: the direction of gen_rays_dist_kernel
// (camera.hiph), load_ray and make_stride (sampler.hiph) with all-ones noise, contract_point
// (hash_grid.hiph), occ_axis_cell (occupancy.hiph) -- the shared device functions, so a VALIDATE
// sample of f2n_sample_rays and its mark fall into the same cell bit for bit.
#include "camera.hiph"
#include "occupancy.hiph"
#include "sampler.hiph"

namespace
{

// rows (or columns) walked at a pixel stride: min(a * s, n - 1) for a = 0 .. ceil((n - 1) / s)
static inline int walked_count(int n, int s) { return (n - 1 + s - 1) / s + 1; }

// One wavefront per ray in 64-sample strides, a persistent grid-stride loop over
// n_cams * n_rows * n_cols rays in camera-major, row-major order: the wavefronts of a workgroup walk
// neighbouring columns of one row of one camera, whose samples fall into the same words.
// A lane reads the word and issues the atomic only where its bit is still 0; of a run of lanes with
// the same cell only the first does.  Integer OR: the result does not depend on the order of arrival.
// (A stale read costs a redundant atomic, never a missing one.)
__global__ __launch_bounds__(F2N_BLOCK) void occ_mark_rays_kernel(
  const float * __restrict__ poses, int pose_ld, const float * __restrict__ intrinsics,
  const float * __restrict__ dist, int cam_first, int h, int w, int pixel_stride, int n_rows,
  int n_cols, const uint32_t * __restrict__ mask_bits, int n_steps, float step, uint32_t * bits,
  int G, int64_t n_rays)
{
  using RL = RayLanes<64>;
  const int lane = lane_id();
  const int64_t n_waves = (int64_t)gridDim.x * F2N_WAVES_PER_BLOCK;
  const int64_t per_cam = (int64_t)n_rows * n_cols;
  for (int64_t q = (int64_t)blockIdx.x * F2N_WAVES_PER_BLOCK + (threadIdx.x >> 6); q < n_rays;
       q += n_waves) {  // (wave-uniform)
    const int64_t cam = cam_first + q / per_cam;
    const int64_t rem = q % per_cam;
    const int row = (int)min((rem / n_cols) * pixel_stride, (int64_t)h - 1);
    const int col = (int)min((rem % n_cols) * pixel_stride, (int64_t)w - 1);
    if (mask_bits) {
      const int64_t g = (cam * h + row) * w + col;
      if (!((mask_bits[g >> 5] >> (uint32_t)(g & 31)) & 1u)) continue;
    }
    const float * P = poses + cam * pose_ld;  // rows of 4: [R | t]
    float u, v;
    camera_pixel_to_dir(intrinsics + cam * 9, load_lens(dist, cam), (float)row, (float)col, u, v);
    float o[3], d[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      d[a] = camera_dir_to_world(P, a, u, v);
      o[a] = P[4 * a + 3];
    }
    const RayFrame rf = load_ray(o, d, 0);
    StrideCarry carry = {};
    for (int k0 = 0; k0 < n_steps; k0 += F2N_WAVE) {
      const StrideSample sm = make_stride<64>(rf, nullptr, k0, n_steps, step, carry, lane);
      float x = sm.px, y = sm.py, z = sm.pz;
      contract_point(x, y, z);
      // a non-finite coordinate marks nothing and is never an address
      const bool ok = sm.valid && (fabsf(x) + fabsf(y) + fabsf(z) < __builtin_inff());
      int cell = -1;
      if (ok) {
        cell = (occ_axis_cell(z, G) * G + occ_axis_cell(y, G)) * G + occ_axis_cell(x, G);
      }
      // (the cell index moves through the DPP as bits; every lane takes part)
      const int before = __float_as_int(RL::prev(__int_as_float(cell), __int_as_float(-1), lane));
      if (cell >= 0 && cell != before) {
        const uint32_t bit = 1u << (uint32_t)(cell & 31);
        uint32_t * word = bits + (cell >> 5);
        if (!(*word & bit)) atomicOr(word, bit);
      }
    }
  }
}

// bits cx - 1 .. cx + 1 of one row of G bits ORed together; nothing beyond the row's ends
__device__ __forceinline__ uint32_t row_window(const uint32_t * __restrict__ row, int cx, int G)
{
  const int wi = cx >> 5, b = cx & 31;
  const uint32_t word = row[wi];
  uint32_t m = word >> b;
  if (b > 0)
    m |= word >> (b - 1);
  else if (wi > 0)
    m |= row[wi - 1] >> 31;
  if (b < 31)
    m |= word >> (b + 1);
  else if (wi < (G >> 5) - 1)
    m |= row[wi + 1];
  return m & 1u;
}

// One thread per cell, x fastest (occ_update_kernel's layout): the 64 lanes of a wavefront are two
// whole words, which lanes 0 and 32 write from one ballot.  No wrap-around: a neighbour outside
// [0, G)^3 does not exist.
__global__ __launch_bounds__(F2N_BLOCK) void occ_dilate_kernel(
  const uint32_t * __restrict__ in, uint32_t * __restrict__ out, int G, int log2_g)
{
  // (G^3 is a multiple of the block size: every thread owns a cell, no wave is partial)
  const uint32_t i = blockIdx.x * (uint32_t)F2N_BLOCK + threadIdx.x;
  const int cx = (int)(i & (uint32_t)(G - 1)), cy = (int)((i >> log2_g) & (uint32_t)(G - 1)),
            cz = (int)(i >> (2 * log2_g));
  const int row_words = G >> 5;
  uint32_t any = 0u;
  for (int dz = -1; dz <= 1; dz++) {
    const int z = cz + dz;
    if (z < 0 || z >= G) continue;
    for (int dy = -1; dy <= 1; dy++) {
      const int y = cy + dy;
      if (y < 0 || y >= G) continue;
      any |= row_window(in + ((int64_t)z * G + y) * row_words, cx, G);
    }
  }
  const unsigned long long m = __ballot(any != 0u);
  const int lane = lane_id();
  if (lane == 0) out[i >> 5] = (uint32_t)m;
  if (lane == 32) out[i >> 5] = (uint32_t)(m >> 32);
}

__global__ __launch_bounds__(F2N_BLOCK) void occ_count_add_kernel(
  const uint32_t * __restrict__ bits, uint8_t * __restrict__ count)
{
  const uint32_t i = blockIdx.x * (uint32_t)F2N_BLOCK + threadIdx.x;
  const uint32_t c = (uint32_t)count[i] + ((bits[i >> 5] >> (i & 31u)) & 1u);
  count[i] = (uint8_t)min(c, 255u);
}

__global__ __launch_bounds__(F2N_BLOCK) void occ_count_bits_kernel(
  const uint8_t * __restrict__ count, int min_count, uint32_t * __restrict__ bits)
{
  const uint32_t i = blockIdx.x * (uint32_t)F2N_BLOCK + threadIdx.x;
  const unsigned long long m = __ballot((int)count[i] >= min_count);
  const int lane = lane_id();
  if (lane == 0) bits[i >> 5] = (uint32_t)m;
  if (lane == 32) bits[i >> 5] = (uint32_t)(m >> 32);
}

static inline dim3 cell_grid(int G) { return dim3((unsigned)(((int64_t)G * G * G) / F2N_BLOCK)); }

}  // namespace

extern "C" int f2n_occ_mark_rays(
  const float * poses, int pose_ld, const float * intrinsics, const float * dist, int cam_first,
  int n_cams, int h, int w, int pixel_stride, const uint32_t * mask_bits, int n_steps, float step,
  uint32_t * bits, int G, void * stream)
{
  if (!poses || !intrinsics || !bits || !f2n_occ_res_ok(G)) return F2N_E_INVALID_ARG;
  if (pose_ld != 12 && pose_ld != 16) return F2N_E_INVALID_ARG;  // [3,4] or [4,4] row-major
  if (h < 1 || w < 1 || pixel_stride < 1 || n_steps < 1 || n_steps > 65536) return F2N_E_INVALID_ARG;
  if (cam_first < 0 || n_cams < 0) return F2N_E_INVALID_ARG;
  if (!(step > 0.f) || !(step < __builtin_inff())) return F2N_E_INVALID_ARG;  // false for NaN as well
  if (n_cams == 0) return F2N_OK;
  const int n_rows = walked_count(h, pixel_stride), n_cols = walked_count(w, pixel_stride);
  const int64_t n_rays = (int64_t)n_cams * n_rows * n_cols;
  // persistent: at most eight workgroups for each of the 256 compute units
  const int64_t blocks = (n_rays + F2N_WAVES_PER_BLOCK - 1) / F2N_WAVES_PER_BLOCK;
  const dim3 grid((unsigned)(blocks < 2048 ? blocks : 2048)), block(F2N_BLOCK);
  hipLaunchKernelGGL(
    occ_mark_rays_kernel, grid, block, 0, (hipStream_t)stream, poses, pose_ld, intrinsics, dist,
    cam_first, h, w, pixel_stride, n_rows, n_cols, mask_bits, n_steps, step, bits, G, n_rays);
  return f2n_launch_status();
}

extern "C" int f2n_occ_dilate(const uint32_t * in, uint32_t * out, int G, void * stream)
{
  if (!in || !out || in == out || !f2n_occ_res_ok(G)) return F2N_E_INVALID_ARG;
  int log2_g = 0;
  while ((1 << log2_g) < G) log2_g++;
  hipLaunchKernelGGL(
    occ_dilate_kernel, cell_grid(G), dim3(F2N_BLOCK), 0, (hipStream_t)stream, in, out, G, log2_g);
  return f2n_launch_status();
}

extern "C" int f2n_occ_count_add(const uint32_t * bits, uint8_t * count, int G, void * stream)
{
  if (!bits || !count || !f2n_occ_res_ok(G)) return F2N_E_INVALID_ARG;
  hipLaunchKernelGGL(
    occ_count_add_kernel, cell_grid(G), dim3(F2N_BLOCK), 0, (hipStream_t)stream, bits, count);
  return f2n_launch_status();
}

extern "C" int f2n_occ_count_bits(
  const uint8_t * count, int min_count, uint32_t * bits, int G, void * stream)
{
  if (!count || !bits || !f2n_occ_res_ok(G)) return F2N_E_INVALID_ARG;
  hipLaunchKernelGGL(
    occ_count_bits_kernel, cell_grid(G), dim3(F2N_BLOCK), 0, (hipStream_t)stream, count, min_count,
    bits);
  return f2n_launch_status();
}
