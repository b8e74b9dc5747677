// pixel_mask.hip -- per-pixel validity masks as bits, and a training-batch draw that only lands on
// valid pixels (include/f2nerf_hip.h has the contracts).  They stand beside the reference's
// Dataset::sample_random_rays (src/dataset.cpp:150-171), which draws (camera, row, col) with three
// randint calls over the whole image and knows no mask.
//
// PACK.  Global pixel g = (e*h + i)*w + j is bit (g & 31) of word (g >> 5); ceil(E*h*w / 32) words,
// unused bits of the last word zero.  One lane per pixel: the 64-lane ballot of "mask[g] != 0" is two
// words, written by lane 0 of the wavefront (the second only where it exists).  No atomics.  At most
// 2^20 workgroups are launched; beyond 2^28 pixels a workgroup walks on in strides of the grid, still
// one lane per pixel and one ballot per 64 of them.  The number of valid pixels: popcount of each
// ballot, one partial per workgroup (four wave counts added by thread 0), then a single-workgroup
// tree over the partials in int64 -- integer sums, the same on every run.
//
// DRAW.  One lane per ray.  Attempt a = 0 .. A-1 of ray r takes the four 32-bit words of
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011) with key
// (seed_lo, seed_hi) and counter (r, a, 0, 0).  The generator in full -- this is the specification,
// all arithmetic on uint32 with wrap-around, mulhi(a, b) = (a * b) >> 32 of the 64-bit product:
//     (c0, c1, c2, c3) = (r, a, 0, 0);  (k0, k1) = (seed_lo, seed_hi)
//     repeat 10 times, round n = 0 .. 9:
//         if n > 0:  k0 += 0x9E3779B9;  k1 += 0xBB67AE85          (Weyl sequence on the key)
//         hi0 = mulhi(0xD2511F53, c0);  lo0 = 0xD2511F53 * c0
//         hi1 = mulhi(0xCD9E8D57, c2);  lo1 = 0xCD9E8D57 * c2
//         (c0, c1, c2, c3) = (hi1 ^ c1 ^ k0,  lo1,  hi0 ^ c3 ^ k1,  lo0)
//     (x0, x1, x2, x3) = (c0, c1, c2, c3)
// Known answer: counter 0, key 0 gives 6627e8d5 e169c58d bc57ac4c 9b00dbd8.
// Then cam = mulhi(x0, E), i = mulhi(x1, h), j = mulhi(x2, w) (x3 is unused) and the attempt is kept
// iff bit g = (cam*h + i)*w + j is set.  The first kept attempt ends the ray: tries = a + 1.  When
// all A attempts miss, tries = 0 and (cam, i, j) hold the last attempt.  Redrawing the camera
// together with the pixel keeps the draw uniform over the valid pixels of the whole set; an all-ones
// mask takes one attempt per ray and is uniform over cameras and pixels, as src/dataset.cpp:150-171.
//
// DIVERGENCE.  A lane's number of attempts is geometric in the valid fraction f, and a wavefront
// runs as long as its unluckiest lane: the expected maximum of 64 such lanes, against the 1 / f a
// lane needs on average, is
//     f = 0.9    about 2.5 attempts per wavefront   (1.1 per lane)
//     f = 0.5    about 7.3                          (2 per lane)
//     f = 0.1    the cap: 0.9^32 = 3.4 % of the lanes miss all of A = 32 attempts, so 89 % of the
//                wavefronts run all 32 (10 per lane), and those 3.4 % of the rays come back with
//                tries = 0 (ray weight 0 in the host's batch).
// An attempt is ~40 integer instructions and one 4-byte load, so the draw stays small beside the
// render it feeds; flattening the divergence (per-image alias tables) is not attempted here.
#include "common.hiph"
#include "philox.hiph"

namespace
{

constexpr int kMaskBlock = 256;
constexpr int64_t kMaxPixels = (int64_t)1 << 36;
constexpr int64_t kMaxPackBlocks = (int64_t)1 << 20;

__global__ __launch_bounds__(kMaskBlock) void mask_pack_kernel(
  const uint8_t * __restrict__ mask, int64_t n_pixels, int64_t n_words, uint32_t * __restrict__ words,
  uint32_t * __restrict__ partial)
{
  __shared__ uint32_t wave_count[kMaskBlock / 64];
  const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
  const int64_t stride = (int64_t)gridDim.x * kMaskBlock;
  uint32_t count = 0;  // of this wavefront: at most 64 * 2^36 / 2^28
  // (the bound is the same for every lane of the workgroup: every lane takes part in every ballot)
  for (int64_t base = (int64_t)blockIdx.x * kMaskBlock; base < n_pixels; base += stride) {
    const int64_t g = base + threadIdx.x;
    const bool valid = g < n_pixels && mask[g] != 0;
    const uint64_t ballot = __ballot(valid);
    if (lane == 0) {
      const int64_t w0 = (g >> 6) * 2;  // g is the wavefront's first pixel here
      if (w0 < n_words) words[w0] = (uint32_t)ballot;
      if (w0 + 1 < n_words) words[w0 + 1] = (uint32_t)(ballot >> 32);
    }
    count += (uint32_t)__popcll(ballot);
  }
  if (lane == 0) wave_count[wave] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < kMaskBlock / 64; i++) c += wave_count[i];
    partial[blockIdx.x] = c;
  }
}

__global__ __launch_bounds__(kMaskBlock) void mask_count_kernel(
  const uint32_t * __restrict__ partial, int64_t n_blocks, int64_t * __restrict__ count)
{
  __shared__ int64_t tree[kMaskBlock];
  int64_t c = 0;
  for (int64_t i = threadIdx.x; i < n_blocks; i += kMaskBlock) c += partial[i];
  tree[threadIdx.x] = c;
  __syncthreads();
  for (int half = kMaskBlock / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) tree[threadIdx.x] += tree[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) count[0] = tree[0];
}

__global__ __launch_bounds__(kMaskBlock) void draw_pixels_masked_kernel(
  const uint32_t * __restrict__ bits, int E, int h, int w, uint32_t seed_lo, uint32_t seed_hi,
  int attempts, int32_t * __restrict__ cam, int32_t * __restrict__ ij, int32_t * __restrict__ tries,
  int n)
{
  const int r = blockIdx.x * kMaskBlock + threadIdx.x;
  if (r >= n) return;
  uint32_t c = 0, i = 0, j = 0;
  int used = 0;
  for (int a = 0; a < attempts; a++) {
    const Philox4 x = philox4x32_10((uint32_t)r, (uint32_t)a, 0u, 0u, seed_lo, seed_hi);
    c = __umulhi(x.x0, (uint32_t)E);  // < E
    i = __umulhi(x.x1, (uint32_t)h);  // < h
    j = __umulhi(x.x2, (uint32_t)w);  // < w: g < E*h*w, inside the words
    const int64_t g = ((int64_t)c * h + i) * w + j;
    if ((bits[g >> 5] >> (uint32_t)(g & 31)) & 1u) {
      used = a + 1;
      break;
    }
  }
  cam[r] = (int32_t)c;
  ij[2 * r] = (int32_t)i;
  ij[2 * r + 1] = (int32_t)j;
  tries[r] = used;
}

// E, h, w > 0 and E*h*w < 2^36, without overflow on the way
inline bool pixels_ok(int E, int h, int w)
{
  if (E <= 0 || h <= 0 || w <= 0) return false;
  const int64_t hw = (int64_t)h * w;  // < 2^62
  return hw < kMaxPixels && (int64_t)E <= (kMaxPixels - 1) / hw;
}

// workgroups of the pack: one per 256 pixels, 2^20 at the most
inline int64_t pack_blocks(int64_t n_pixels)
{
  const int64_t n_blocks = (n_pixels + kMaskBlock - 1) / kMaskBlock;
  return n_blocks < kMaxPackBlocks ? n_blocks : kMaxPackBlocks;
}

}  // namespace

extern "C" int64_t f2n_mask_words(int E, int h, int w)
{
  if (!pixels_ok(E, h, w)) return 0;
  return ((int64_t)E * h * w + 31) / 32;
}

extern "C" int64_t f2n_mask_pack_workspace_words(int E, int h, int w)
{
  if (!pixels_ok(E, h, w)) return 0;
  return pack_blocks((int64_t)E * h * w);
}

extern "C" int f2n_mask_pack(
  const uint8_t * mask, int E, int h, int w, uint32_t * words, int64_t * count, uint32_t * partial,
  void * stream)
{
  if (!mask || !words || !count || !partial || !pixels_ok(E, h, w)) return F2N_E_INVALID_ARG;
  const int64_t n_pixels = (int64_t)E * h * w;
  const int64_t n_words = (n_pixels + 31) / 32;
  const int64_t n_blocks = pack_blocks(n_pixels);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(
    mask_pack_kernel, dim3((unsigned)n_blocks), dim3(kMaskBlock), 0, s, mask, n_pixels, n_words,
    words, partial);
  hipLaunchKernelGGL(mask_count_kernel, dim3(1), dim3(kMaskBlock), 0, s, partial, n_blocks, count);
  return f2n_launch_status();
}

extern "C" int f2n_draw_pixels_masked(
  const uint32_t * bits, int E, int h, int w, uint32_t seed_lo, uint32_t seed_hi, int attempts,
  int32_t * cam, int32_t * ij, int32_t * tries, int n, void * stream)
{
  if (!bits || !cam || !ij || !tries || n < 0 || !pixels_ok(E, h, w) || attempts < 1 || attempts > 64)
    return F2N_E_INVALID_ARG;
  if (n == 0) return F2N_OK;
  hipLaunchKernelGGL(
    draw_pixels_masked_kernel, dim3(f2n_div_up(n, kMaskBlock)), dim3(kMaskBlock), 0,
    (hipStream_t)stream, bits, E, h, w, seed_lo, seed_hi, attempts, cam, ij, tries, n);
  return f2n_launch_status();
}
