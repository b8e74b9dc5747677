// ssim.hip -- structural similarity of image pairs, its gradient, and a patch draw (include/
// f2nerf_hip.h has the contracts).  The definition is the reference's rgb_ssim, scripts/eval.py:29-75
// (an 11-tap Gaussian, sigma 1.5, `valid` borders, k1 = 0.01, k2 = 0.03, max_val = 1), which runs on
// the host in scipy; here one kernel reads each image once.  pred, gt [B, h, w, 3] f32, interleaved.
//
// FILTER.  f[k] = exp(-0.5 ((k - 5) / 1.5)^2) / sum, k = 0 .. 10, in f64 on the host, rounded once to
// f32 (f2n_ssim_filter hands the eleven floats out); the kernels get them as launch arguments.
//
// TILES.  A workgroup of 256 lanes owns T x T = 16 x 16 map pixels (map = the (h-10) x (w-10) grid of
// `valid` window positions) of one image pair: grid (ceil(mw / T), ceil(mh / T), B), tile index
// ty * tiles_x + tx.  LDS: both images' (T+10)^2 pixels, rows of 78 words (2 x 8112 B), and the
// horizontal pass' five moments of the three channels, [3][5][26][16] words (24960 B), and 2048 B
// for the sums: 43232 B, three workgroups (twelve wavefronts) per CU.  Banks: a lane's word is
// 78 r + 3 j (+ channel) in the horizontal pass -- stride 3 inside a row and 78 = 14 (mod 64) between
// the rows a wavefront spans, and 3 (j - j') = 14 (mod 64) needs |j - j'| = 26 > 15: conflict-free;
// the vertical pass reads 64 consecutive words.
//
// EVALUATION ORDER of the forward (tests/ssim_model.py follows these lines; the library is built with
// -ffp-contract=off, so only the fmaf spelled out here is fused).  All f32 unless said otherwise.
//   staged pixel outside the image: 0 (only ever read for map pixels outside the map, never summed)
//   horizontal, staged row r, map column j, channel c, x = pred, y = gt; k ascending:
//     hx  = f[0] x[j]; hx = fmaf(f[k], x[j+k], hx)          likewise hy from y
//     hxx from p = x[j+k] * x[j+k] (one rounding), hyy from y * y, hxy from x * y, the same chain
//   vertical, map pixel (i, j): mux = f[0] hx[i][j]; mux = fmaf(f[k], hx[i+k][j], mux); likewise
//     muy, Exx, Eyy, Exy
//   mxx = mux mux; myy = muy muy; mxy = mux muy
//   sxx = Exx - mxx; syy = Eyy - myy; sxy = Exy - mxy
//   clip: sxx = sxx > 0 ? sxx : 0; syy likewise; lim = sqrtf(sxx syy) (correctly rounded);
//         a = |sxy| < lim ? |sxy| : lim; sxy = copysign(a, sxy)
//   N1 = 2 mxy + c1; N2 = 2 sxy + c2; D1 = (mxx + myy) + c1; D2 = (sxx + syy) + c2
//   P = D1 D2; S = (N1 N2) / P                               c1 = 1e-4f, c2 = 9e-4f, IEEE division
//   gmaps (clip = 0 only), nine floats per map pixel, index 3 c + {0, 1, 2}:
//     gmu = ((2 muy) (N2 - N1)) / P + (e / D2 - e / D1), e = (2 mux) S
//     gxx = -(S / D2);  gxy = (2 N1) / P
//   sums, f64: a lane adds its pixel's three S in channel order ((S0 + S1) + S2; 0 off the map), the
//     256 lanes are added by the tree t[i] += t[i + half], half = 128, 64 .. 1, and t[0] is the tile's
//     partial.  Second launch, one workgroup per image: lane l adds partials l, l + 256, .. in that
//     order, the same tree, ssim = (float)(t[0] / (double)(mh mw 3)).  (One lane adding 8040 partials
//     of a 1920 x 1080 pair one after the other would take as long as the first launch.)
//   No atomics anywhere: the same bits on every run.
//
// BACKWARD.  It reads the gmaps the forward wrote, and recomputes nothing: re-deriving them from the
// images needs a 20-pixel halo, (36 / 16)^2 = 5 times the forward's filtering per tile, where the
// maps cost nine floats per map pixel that a training step's forward has in registers anyway.
// A workgroup owns 16 x 16 INPUT pixels and gathers from the (16+10)^2 map pixels that reach them
// (map pixels off the map are staged as 0): d_pred is written once per element, no atomics, no
// memset.  LDS: [26][26 x 9] + [9][26][16] words = 39312 B.  With G one of the nine maps, input pixel
// (pi, pj), k ascending:
//     horizontal, map row q:  a = f[0] G[q][pj]; a = fmaf(f[k], G[q][pj - k], a)
//     vertical:               A = f[0] a[pi];    A = fmaf(f[k], a[pi - k], A)
//   A, Bq, C the filtered gmu, gxx, gxy of the channel:  v = (A + (2 x) Bq) + y C
//   d_pred = (float)((double)d_ssim_b / (double)(mh mw 3)) v;  d_ssim_b == 0: d_pred = +0, nothing read
//
// PATCH DRAW.  One wavefront per patch b.  Attempt a takes Philox4x32-10 (philox.hiph, specified in
// pixel_mask.hip) with key (seed_lo, seed_hi) and counter (b, a, 2, 0) -- word 2 of the counter is the
// draw's domain: 0 the masked draw, 1 the guided draw's in-cell pixel -- and cam = mulhi(x0, E),
// i0 = mulhi(x1, h - P + 1), j0 = mulhi(x2, w - P + 1).  With bits, lanes test the P^2 pixels 64 at a
// time and a ballot decides: the attempt is kept iff every pixel's bit is set; without bits the first
// attempt is kept.  tries = a + 1, patch_weight = 1; when every attempt missed tries = 0,
// patch_weight = 0 and the last attempt stays.  Pixel (u, v) of patch b is ray b P^2 + u P + v.
#include "common.hiph"
#include "philox.hiph"

namespace
{

constexpr int kT = F2N_SSIM_TILE;  // map pixels per tile side (forward), input pixels (backward)
constexpr int kTaps = 11;
constexpr int kHalo = kTaps - 1;
constexpr int kS = kT + kHalo;  // staged side: 26
constexpr int kBlock = 256;
constexpr float kC1 = 1e-4f, kC2 = 9e-4f;
static_assert(kT * kT == kBlock, "one lane per tile pixel");

struct SsimFilter
{
  float f[kTaps];
};

SsimFilter host_filter()
{
  double g[kTaps], sum = 0.0;
  for (int k = 0; k < kTaps; k++) {
    const double z = (double)(k - kTaps / 2) / 1.5;
    g[k] = exp(-0.5 * (z * z));
    sum += g[k];
  }
  SsimFilter out;
  for (int k = 0; k < kTaps; k++) out.f[k] = (float)(g[k] / sum);
  return out;
}

// t[0] = the 256 values added by the fixed tree; every lane of the workgroup calls it
__device__ __forceinline__ double block_tree_sum(double * t, double v)
{
  t[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int half = kBlock / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) t[threadIdx.x] += t[threadIdx.x + half];
    __syncthreads();
  }
  return t[0];
}

__global__ __launch_bounds__(kBlock) void ssim_fwd_kernel(
  const float * __restrict__ pred, const float * __restrict__ gt, int h, int w, int clip,
  SsimFilter flt, float * __restrict__ map, float * __restrict__ gmaps,
  double * __restrict__ partial)
{
  __shared__ float sx[kS * kS * 3], sy[kS * kS * 3];
  __shared__ float hbuf[3 * 5 * kS * kT];
  __shared__ double tree[kBlock];
  const int mh = h - kHalo, mw = w - kHalo;
  const int b = blockIdx.z, i0 = blockIdx.y * kT, j0 = blockIdx.x * kT;
  const int64_t img = (int64_t)b * h * w * 3;
  // stage (T+10)^2 pixels of both images; rows of 78 consecutive words
  for (int idx = threadIdx.x; idx < kS * kS * 3; idx += kBlock) {
    const int r = idx / (kS * 3), q = idx - r * (kS * 3);
    const int gi = i0 + r, gq = j0 * 3 + q;
    float vx = 0.f, vy = 0.f;
    if (gi < h && gq < w * 3) {
      const int64_t g = img + (int64_t)gi * w * 3 + gq;
      vx = pred[g];
      vy = gt[g];
    }
    sx[idx] = vx;
    sy[idx] = vy;
  }
  __syncthreads();
  // horizontal pass: item = (c, r, j), j fastest
  for (int item = threadIdx.x; item < 3 * kS * kT; item += kBlock) {
    const int c = item / (kS * kT), rj = item - c * (kS * kT);
    const int r = rj / kT, j = rj - r * kT;
    const float * px = sx + r * (kS * 3) + j * 3 + c;
    const float * py = sy + r * (kS * 3) + j * 3 + c;
    float x = px[0], y = py[0];
    float hx = flt.f[0] * x, hy = flt.f[0] * y;
    float hxx = flt.f[0] * (x * x), hyy = flt.f[0] * (y * y), hxy = flt.f[0] * (x * y);
#pragma unroll
    for (int k = 1; k < kTaps; k++) {
      x = px[3 * k];
      y = py[3 * k];
      hx = fmaf(flt.f[k], x, hx);
      hy = fmaf(flt.f[k], y, hy);
      hxx = fmaf(flt.f[k], x * x, hxx);
      hyy = fmaf(flt.f[k], y * y, hyy);
      hxy = fmaf(flt.f[k], x * y, hxy);
    }
    float * o = hbuf + c * (5 * kS * kT) + rj;
    o[0] = hx;
    o[kS * kT] = hy;
    o[2 * kS * kT] = hxx;
    o[3 * kS * kT] = hyy;
    o[4 * kS * kT] = hxy;
  }
  __syncthreads();
  // vertical pass and the index: one lane per map pixel
  const int ti = threadIdx.x / kT, tj = threadIdx.x - ti * kT;
  const int mi = i0 + ti, mj = j0 + tj;
  const bool live = mi < mh && mj < mw;
  double lane_sum = 0.0;
  if (live) {
    const int64_t mp = ((int64_t)b * mh + mi) * mw + mj;
    float S3[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      float m[5];
#pragma unroll
      for (int q = 0; q < 5; q++) {
        const float * p = hbuf + (c * 5 + q) * (kS * kT) + ti * kT + tj;
        float acc = flt.f[0] * p[0];
#pragma unroll
        for (int k = 1; k < kTaps; k++) acc = fmaf(flt.f[k], p[k * kT], acc);
        m[q] = acc;
      }
      const float mux = m[0], muy = m[1];
      const float mxx = mux * mux, myy = muy * muy, mxy = mux * muy;
      float sxx = m[2] - mxx, syy = m[3] - myy, sxy = m[4] - mxy;
      if (clip) {
        sxx = sxx > 0.f ? sxx : 0.f;
        syy = syy > 0.f ? syy : 0.f;
        const float lim = sqrtf(sxx * syy);
        const float a = fabsf(sxy) < lim ? fabsf(sxy) : lim;
        sxy = copysignf(a, sxy);
      }
      const float N1 = 2.f * mxy + kC1, N2 = 2.f * sxy + kC2;
      const float D1 = (mxx + myy) + kC1, D2 = (sxx + syy) + kC2;
      const float P = D1 * D2;
      const float S = (N1 * N2) / P;
      S3[c] = S;
      if (gmaps) {
        const float e = (2.f * mux) * S;
        const float gmu = ((2.f * muy) * (N2 - N1)) / P + (e / D2 - e / D1);
        float * g = gmaps + mp * 9 + c * 3;
        g[0] = gmu;
        g[1] = -(S / D2);
        g[2] = (2.f * N1) / P;
      }
    }
    if (map) {
      map[mp * 3] = S3[0];
      map[mp * 3 + 1] = S3[1];
      map[mp * 3 + 2] = S3[2];
    }
    lane_sum = ((double)S3[0] + (double)S3[1]) + (double)S3[2];
  }
  const double total = block_tree_sum(tree, lane_sum);
  if (threadIdx.x == 0)
    partial[(int64_t)b * gridDim.y * gridDim.x + (int64_t)blockIdx.y * gridDim.x + blockIdx.x] =
      total;
}

__global__ __launch_bounds__(kBlock) void ssim_reduce_kernel(
  const double * __restrict__ partial, int n_tiles, double n_values, float * __restrict__ ssim)
{
  __shared__ double tree[kBlock];
  const double * p = partial + (int64_t)blockIdx.x * n_tiles;
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_tiles; i += kBlock) acc += p[i];
  const double total = block_tree_sum(tree, acc);
  if (threadIdx.x == 0) ssim[blockIdx.x] = (float)(total / n_values);
}

__global__ __launch_bounds__(kBlock) void ssim_bwd_kernel(
  const float * __restrict__ pred, const float * __restrict__ gt, const float * __restrict__ gmaps,
  const float * __restrict__ d_ssim, int h, int w, SsimFilter flt, float * __restrict__ d_pred)
{
  __shared__ float sg[kS * kS * 9];
  __shared__ float hbuf[9 * kS * kT];
  const int mh = h - kHalo, mw = w - kHalo;
  const int b = blockIdx.z, i0 = blockIdx.y * kT, j0 = blockIdx.x * kT;
  const int ti = threadIdx.x / kT, tj = threadIdx.x - ti * kT;
  const int pi = i0 + ti, pj = j0 + tj;
  const bool live = pi < h && pj < w;
  const int64_t pix = (((int64_t)b * h + pi) * w + pj) * 3;
  const float ds = d_ssim[b];
  if (ds == 0.f) {  // (the same for every lane of the workgroup)
    if (live) d_pred[pix] = d_pred[pix + 1] = d_pred[pix + 2] = 0.f;
    return;
  }
  const float scale = (float)((double)ds / ((double)mh * (double)mw * 3.0));
  // stage the map pixels (i0 - 10 + r, j0 - 10 + s), r, s < 26; off the map: 0
  for (int idx = threadIdx.x; idx < kS * kS * 9; idx += kBlock) {
    const int r = idx / (kS * 9), q = idx - r * (kS * 9);
    const int s = q / 9, cm = q - s * 9;
    const int qi = i0 - kHalo + r, qj = j0 - kHalo + s;
    float v = 0.f;
    if (qi >= 0 && qi < mh && qj >= 0 && qj < mw)
      v = gmaps[(((int64_t)b * mh + qi) * mw + qj) * 9 + cm];
    sg[idx] = v;
  }
  __syncthreads();
  // horizontal: item = (cm, r, j), j fastest; input column j0 + j gathers staged columns j + 10 - k
  for (int item = threadIdx.x; item < 9 * kS * kT; item += kBlock) {
    const int cm = item / (kS * kT), rj = item - cm * (kS * kT);
    const int r = rj / kT, j = rj - r * kT;
    const float * p = sg + r * (kS * 9) + (j + kHalo) * 9 + cm;
    float acc = flt.f[0] * p[0];
#pragma unroll
    for (int k = 1; k < kTaps; k++) acc = fmaf(flt.f[k], p[-9 * k], acc);
    hbuf[item] = acc;
  }
  __syncthreads();
  if (!live) return;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float m[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
      // input row i0 + ti gathers staged rows ti + 10 - k
      const float * p = hbuf + (c * 3 + q) * (kS * kT) + (ti + kHalo) * kT + tj;
      float acc = flt.f[0] * p[0];
#pragma unroll
      for (int k = 1; k < kTaps; k++) acc = fmaf(flt.f[k], p[-k * kT], acc);
      m[q] = acc;
    }
    const float x = pred[pix + c], y = gt[pix + c];
    const float v = (m[0] + (2.f * x) * m[1]) + y * m[2];
    d_pred[pix + c] = scale * v;
  }
}

constexpr int kPatchWaves = kBlock / 64;

__global__ __launch_bounds__(kBlock) void draw_patches_kernel(
  const uint32_t * __restrict__ bits, int E, int h, int w, int P, uint32_t seed_lo, uint32_t seed_hi,
  int attempts, int32_t * __restrict__ cam, int32_t * __restrict__ ij, int32_t * __restrict__ tries,
  float * __restrict__ patch_weight, int n)
{
  const int lane = lane_id();
  const int b = blockIdx.x * kPatchWaves + (int)(threadIdx.x >> 6);
  if (b >= n) return;  // (a whole wavefront leaves)
  const int PP = P * P;
  uint32_t c = 0, i0 = 0, j0 = 0;
  int used = 0;
  for (int a = 0; a < attempts; a++) {
    const Philox4 x = philox4x32_10((uint32_t)b, (uint32_t)a, 2u, 0u, seed_lo, seed_hi);
    c = __umulhi(x.x0, (uint32_t)E);           // < E
    i0 = __umulhi(x.x1, (uint32_t)(h - P + 1));  // i0 + P <= h
    j0 = __umulhi(x.x2, (uint32_t)(w - P + 1));  // j0 + P <= w
    bool ok = true;
    if (bits) {
      for (int idx = lane; idx < PP; idx += 64) {
        const int u = idx / P, v = idx - u * P;
        const int64_t g = ((int64_t)c * h + (i0 + u)) * w + (j0 + v);  // < E*h*w
        ok = ok && ((bits[g >> 5] >> (uint32_t)(g & 31)) & 1u);
      }
    }
    if (__ballot(!ok) == 0) {  // (the same for every lane)
      used = a + 1;
      break;
    }
  }
  const int64_t base = (int64_t)b * PP;
  for (int idx = lane; idx < PP; idx += 64) {
    const int u = idx / P, v = idx - u * P;
    cam[base + idx] = (int32_t)c;
    ij[2 * (base + idx)] = (int32_t)i0 + u;
    ij[2 * (base + idx) + 1] = (int32_t)j0 + v;
  }
  if (lane == 0) {
    tries[b] = used;
    patch_weight[b] = used > 0 ? 1.f : 0.f;
  }
}

// B images of h x w: sides from 11, B within the grid's z extent, every index within int64
inline bool ssim_shape_ok(int B, int h, int w)
{
  return B >= 0 && B <= 65535 && h >= kTaps && w >= kTaps;
}

inline int64_t tiles_of(int n) { return (n + kT - 1) / kT; }

}  // namespace

extern "C" int f2n_ssim_filter(float * taps11)
{
  if (!taps11) return F2N_E_INVALID_ARG;
  const SsimFilter flt = host_filter();
  for (int k = 0; k < kTaps; k++) taps11[k] = flt.f[k];
  return F2N_OK;
}

extern "C" int64_t f2n_ssim_workspace_doubles(int B, int h, int w)
{
  if (!ssim_shape_ok(B, h, w)) return 0;
  return (int64_t)B * tiles_of(h - kHalo) * tiles_of(w - kHalo);
}

extern "C" int f2n_ssim_fwd(
  const float * pred, const float * gt, int B, int h, int w, int clip, float * ssim, float * map,
  float * gmaps, double * partial, void * stream)
{
  if (!pred || !gt || !ssim || !partial || !ssim_shape_ok(B, h, w) || (clip != 0 && clip != 1) ||
      (clip == 1 && gmaps))
    return F2N_E_INVALID_ARG;
  if (B == 0) return F2N_OK;
  const int mh = h - kHalo, mw = w - kHalo;
  const int64_t tx = tiles_of(mw), ty = tiles_of(mh);
  if (ty > 65535 || tx * ty > INT32_MAX) return F2N_E_INVALID_ARG;
  const SsimFilter flt = host_filter();
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(
    ssim_fwd_kernel, dim3((unsigned)tx, (unsigned)ty, (unsigned)B), dim3(kBlock), 0, s, pred, gt, h,
    w, clip, flt, map, gmaps, partial);
  hipLaunchKernelGGL(
    ssim_reduce_kernel, dim3((unsigned)B), dim3(kBlock), 0, s, (const double *)partial,
    (int)(tx * ty), (double)mh * (double)mw * 3.0, ssim);
  return f2n_launch_status();
}

extern "C" int f2n_ssim_bwd(
  const float * pred, const float * gt, const float * gmaps, const float * d_ssim, int B, int h,
  int w, float * d_pred, void * stream)
{
  if (!pred || !gt || !gmaps || !d_ssim || !d_pred || !ssim_shape_ok(B, h, w))
    return F2N_E_INVALID_ARG;
  if (B == 0) return F2N_OK;
  const int64_t tx = tiles_of(w), ty = tiles_of(h);
  if (ty > 65535) return F2N_E_INVALID_ARG;
  const SsimFilter flt = host_filter();
  hipLaunchKernelGGL(
    ssim_bwd_kernel, dim3((unsigned)tx, (unsigned)ty, (unsigned)B), dim3(kBlock), 0,
    (hipStream_t)stream, pred, gt, gmaps, d_ssim, h, w, flt, d_pred);
  return f2n_launch_status();
}

extern "C" int f2n_draw_patches(
  const uint32_t * bits, int E, int h, int w, int n_patches, int P, uint32_t seed_lo,
  uint32_t seed_hi, int attempts, int32_t * cam, int32_t * ij, int32_t * tries,
  float * patch_weight, void * stream)
{
  if (!cam || !ij || !tries || !patch_weight || n_patches < 0 || E <= 0 || h < kTaps || w < kTaps ||
      P < kTaps || P > (h < w ? h : w) || attempts < 1 || attempts > 64)
    return F2N_E_INVALID_ARG;
  // E*h*w < 2^36 as for the masks, and the rays' count within int32
  const int64_t hw = (int64_t)h * w;
  if (hw >= ((int64_t)1 << 36) || (int64_t)E > (((int64_t)1 << 36) - 1) / hw ||
      (int64_t)n_patches * P * P > INT32_MAX)
    return F2N_E_INVALID_ARG;
  if (n_patches == 0) return F2N_OK;
  hipLaunchKernelGGL(
    draw_patches_kernel, dim3(f2n_div_up(n_patches, kPatchWaves)), dim3(kBlock), 0,
    (hipStream_t)stream, bits, E, h, w, P, seed_lo, seed_hi, attempts, cam, ij, tries, patch_weight,
    n_patches);
  return f2n_launch_status();
}
