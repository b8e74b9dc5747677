// shade_mfma.hip -- backward of the per-sample network (see shade.hip for the network and its
// reference sites) on the f32 matrix cores: v_mfma_f32_16x16x4_f32, exact f32 (a k-ordered fmaf
// chain), so the parity bar of the VALU kernel carries over.
//
// Why: the VALU backward (shade.hip) reads its wave-uniform weights from LDS as broadcast
// ds_read_b128 -- 1 KiB of LDS bandwidth per 4 FMA instructions -- and measures 25 % of the f32 FMA
// rate; it is LDS-bound, not FMA-bound.  An MFMA takes both operands from VGPRs: one 256-byte weight
// read feeds 4 MFMAs = 4096 MACs, 64x less LDS traffic per MAC, and the weight-gradient products
// (sums over samples) become real GEMMs instead of broadcast loops.
//
// Layouts.  lane l = (q = l >> 4, m = l & 15).  One 16x16x4 MFMA: D[4q+r][m] += sum_k A[m][k] B[k][m]
// with lane (q, m) supplying a = A[row m][k = q], b = B[k = q][col m] and holding D rows 4q+r, r<4.
//   Q-layout (activations of a stride of 16 TS samples): lane (q, m) holds feature 4q+r (+16 per
//     M-tile) of samples 16T+m, T < TS.  An MFMA output IS in Q-layout (rows = features, cols = samples), and
//     is the next layer's B operand when that layer walks its k index in the order (M, r) with
//     k = 16M + 4q + r -- so the whole forward and the data-gradient chain need no lane movement.
//     The weight (A) operands are staged in LDS once per workgroup, pre-arranged per lane in
//     exactly that k order ("slots" of 64 floats, conflict-free ds_read_b32).
//   S-layout (for sums over samples: d w1, d w2, d w_h): operands need the SAMPLE on the k axis and
//     the feature on the lane, i.e. the transpose.  Each wave has an LDS tile [feature][kP]: Q-layout
//     registers are written with ds_write_b32 (lanes of a quarter = consecutive samples) and read back
//     as float4 = four consecutive k-steps (k-step t of quarter q = sample 16(t/4) + 4q + t%4).
//
// The 3-wide output layer is NOT on the matrix cores: as a 16-row MFMA operand 13 of its 16 rows are
// padding (round 2: 23-29 % of all issued products).  Each lane holds 16 hidden neurons of 4 samples
// in the Q-layout, so o[c][s] = sum_j w2[c][j] relu(pre[j][s]) is 48 vector FMAs per 16-neuron tile
// into per-quarter partial sums, and ONE product per (c, sample tile) with an all-ones A operand adds
// the four quarters (the MFMA's k axis) and hands the sum to every lane: 12 products instead of 64.
// Its two backward products (d w2, and d_hid = w2^T d_o) are vector FMAs on the same registers.
//
// Per 64 samples: 428 MFMAs + ~580 vector FMAs, ~130 KB of LDS traffic.  Accumulators of all
// parameter gradients stay in registers across the strides of a (persistent) wave; the waves of a
// workgroup meet in LDS at the end and send one set of atomics.
//
// Occupancy (round 5).  Strides of TS = 2 tiles (32 samples) at two waves per SIMD, one 8-wave
// workgroup per CU, are the default; TS = 4 (64 samples) at one wave per SIMD, the round-3 form, is
// F2N_OPT_SHADE_BWD_WAVES = 1.  At one wave every dependent chain was exposed (MFMA result -> vector
// op, LDS write -> transposed read): the matrix pipe was busy half the time.  Route taken: the
// issue's first one, not wave specialisation -- 32-sample strides halve every per-stride array; the
// hidden layer's weight operands are read from LDS when needed instead of pinned in 32 registers;
// the d w2 partials (48 registers replicated over a quarter's lanes) are reduce-scattered over the
// quarter every stride with three DPP steps, leaving 6; the next stride's inputs are no longer
// prefetched (the partner wave covers the wait); the end-of-kernel meet goes through the whole LDS
// in rounds.  With all of that every instantiation fits 256 registers without scratch; the WIDE
// kernels need the phase fences (V = 0) for it.  Launches of fewer than
// F2N_SHADE_BWD_TWO_WAVES_MIN_SAMPLES samples (few strides per wave) take the one-wave form, which
// is faster there.  The data-gradient chain per sample is unchanged:
// d_enc is bit-identical to the TS = 4 form, the parameter gradients differ in the order of sums.
//
// The per-ray constant.  On a dense [n_rays, S] grid the ray-uniform kernels (RAYS) form the SH half
// of the hidden layer, c = b1 + w1[:, 16:32] . SH16(dir), once per stride: 16 products whose 16
// columns are all the same vector, twice per ray forward and four times backward at S = 128.  Where
// the caller has one direction per ray, shade_ray_const_kernel forms c ONCE per ray -- a wave takes
// 16 rays as the 16 columns of those same products, so a row holds the bits the kernels form
// themselves -- into [n_rays, 80] (c[64], then SH16[16]), and shade_*_mfma_rays_kernel_const (the
// same bodies, RC = true) load it: 160 instead of 176 products per 64-sample stride forward, 154
// instead of 170 per 32-sample stride backward, no direction loads, no sh_basis.  The kernels that
// form c stay as they were, for per-sample directions and for callers of the older entries.
#include "shade_mfma.hiph"
#include "shade_fwd_mfma.hiph"

#include "sh_basis.hiph"

#include <cstdlib>

namespace
{

constexpr int kRayConst = F2N_SHADE_RAY_CONST_FLOATS;  // floats per ray of the per-ray constant: c[64], SH16[16]
// The forward loads c for the first kRcEarly neuron tiles with the stride's encoding, ahead of the
// head layer, and for the rest behind it, with the embedding row.  All four ahead is 16 live registers
// where the forming kernel holds a direction: 2 to 8 registers MORE than that kernel in six of the
// sixteen instantiations (C = 32 at four waves per SIMD: 98 against 96).  All four behind fits
// everywhere but leaves tile 0 waiting for memory: 0.412 against 0.395 ms per 8.4 M samples.  One
// ahead fits every instantiation with room (C = 32: 90), and tiles 1..3 have tile 0's 32 products
// to arrive in.
constexpr int kRcEarly = 1;

// TS = 16-sample column tiles per stride: 2 (the default, two waves per SIMD) or 4 (round 3, one).
template <int C, int TS>
struct MShape
{
  static_assert(C % 8 == 0 && C <= 64, "MFMA path: C must be 8, 16, 32 or 64");
  static_assert(TS == 2 || TS == 4, "16-sample tiles per stride: 2 or 4");
  static constexpr int kStride = 16 * TS;  // samples per stride
  static constexpr int kS1 = C / 4;    // k-steps of the head layer (quarter q owns channels q*kS1 ..)
  static constexpr int kM6 = (C + 15) / 16;  // 16-channel tiles of enc (C = 8: half a tile, zero padded)
  // weight operand slots (64 floats each, one per lane)
  static constexpr int oWA1 = 0;               // [t]        w_h[m][q*kS1 + t]
  static constexpr int oWA2 = oWA1 + kS1;      // [M*8 + t]  w1[16M+m][kappa2(t, q)]
  static constexpr int oWA5 = oWA2 + 32;       // [M*4 + r]  w1[16M+4q+r][m]
  static constexpr int oWA6 = oWA5 + 16;       // [M'*4 + r] w_h[4q+r][16M'+m]
  static constexpr int kSlots = oWA6 + kM6 * 4;
  static constexpr int oW2Q = kSlots * 64;     // [M][q][c] float4 over r: w2[c][16M+4q+r] (vector output layer)
  static constexpr int oBh = oW2Q + 4 * 4 * 3 * 4;  // b_h[16]
  static constexpr int oB1 = oBh + 16;         // b1[64]
  static constexpr int oB2 = oB1 + 64;         // b2[3], 0
  static constexpr int kWFloats = oB2 + 4;
  // per-wave S-layout tiles, rows of kStride samples.  Row pitch: 16-byte aligned rows, and the
  // float4 reads (row m, column 16u+4q) conflict-free in ds_read_b128's four 16-lane groups (banks
  // (a/4) mod 64, four per lane): the pitch must be 8 mod 16 so that the 16 rows m of a group start
  // on 16 distinct 4-bank slots.  40 and 72 are the smallest such pitches above 32 and 64 columns
  // (36 and 68 are 2-way).  C = 64 at two waves takes 36 -- 2-way on those reads -- because eight
  // 40-float tiles of 116 rows and the weights exceed the 160 KiB of a CU by 6 KiB.  (The b32 writes
  // of the Q-layout are 2-way at 40 and 72, which costs nothing extra on a ds_write_b32.)
  static constexpr int kP = (TS == 4) ? 72 : (C == 64) ? 36 : 40;
  static constexpr int oXS = 0;                // [32][kP]  X
  static constexpr int oES = oXS + 32 * kP;    // [C][kP]   enc
  static constexpr int oPS = oES + kM6 * 16 * kP;  // [16][kP]  one M-tile of relu(pre) / d_hid, then d_h
  static constexpr int oDS = oPS + 16 * kP;    // [4][kP]   d_o rows 0..2
  // d w2 partials per lane, [c][kW2M][kW2R]: TS = 4 all 48 (c, j) of the lane's quarter; TS = 2 an
  // eighth of them, the rest handed to partner lanes every stride (see the d w2 phase)
  static constexpr int kW2M = (TS == 4) ? 4 : 2, kW2R = (TS == 4) ? 4 : 1;
  static constexpr int kAccs = 41 + 3 * kW2M * kW2R + 4 * kM6;  // accumulator registers a wave hands to wave 0
  // TS = 4: a wave's tile also holds its accumulators at the end (the meet below)
  static constexpr int kWaveFloats =
    (TS == 4 && kAccs * 64 > oDS + 4 * kP) ? kAccs * 64 : oDS + 4 * kP;
  // TS = 2: two waves per SIMD, one 8-wave workgroup per CU.  The live state of a 32-sample stride
  // (32 pre-activations, ~100 accumulators, operands in flight) fits the 256 registers a wave gets
  // at two per SIMD without spilling, and the partner wave covers the chains one wave leaves exposed
  // (MFMA result -> vector op, LDS write -> transposed read, the weight operands read from LDS).
  // TS = 4, round 3: one wave per SIMD.  64 pre-activations and the accumulators do not fit 256
  // registers (hipcc parked the accumulators in scratch: 2.0-2.6 ms per 8.4 M samples), only 512.
  static constexpr int kWaves = (TS == 4) ? 4 : 8;
  static constexpr int kLdsFloats = kWFloats + kWaves * kWaveFloats;
  static_assert(kLdsFloats * 4 <= 160 * 1024, "LDS budget");
  // TS = 2, the end-of-kernel meet of the accumulators in wave 0: waves 1.. hand over kMeetRegs
  // registers per round through the whole LDS (one round since the d w2 partials take 6 registers)
  static constexpr int kMeetRegs = kLdsFloats / ((kWaves - 1) * 64);
  static constexpr int kMeetRounds = (kAccs + kMeetRegs - 1) / kMeetRegs;
};

// V & 1: the scheduler may mix the phases of a stride (the default of the one-wave form since the
// output layer moved to the vector pipe: 1.47 vs 1.54 ms per 8.4 M samples -- its vector phases then
// fill the gaps of the matrix phases around them; with every phase on the matrix cores, round 2, the
// fenced form was 5 % faster).  At two waves per SIMD the partner wave fills those gaps and the
// fenced form is the default (1.30 vs 1.33 ms).  F2N_OPT_SHADE_VARIANT = 1 puts the fences into the
// one-wave form, F2N_OPT_SHADE_BWD_WAVES = 3 takes them out of the two-wave form, for measurements.
template <int V>
__device__ __forceinline__ void phase_fence_v()
{
  if constexpr (!(V & 1)) __builtin_amdgcn_sched_barrier(0);
}

// row[byte_off / 4] with a wave-uniform row pointer: global_load_dword v, v_off, s[row:row+1]
// (Off = uint32_t: the saddr + 32-bit voffset form above; uint64_t, the WIDE kernels for C * n * 4 >=
// 2^32: a 64-bit add per access and the vaddr form -- ~6 % slower, against the 2-3x of falling back
// to the vector kernels)
template <typename T, typename Off>
__device__ __forceinline__ T ld_row(const T * row, Off byte_off)
{
  return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(row) + byte_off);
}
template <typename Off>
__device__ __forceinline__ void st_row(float * row, Off byte_off, float v)
{
  *reinterpret_cast<float *>(reinterpret_cast<char *>(row) + byte_off) = v;
}
template <bool WIDE>
struct RowOffset
{
  typedef uint32_t type;
};
template <>
struct RowOffset<true>
{
  typedef uint64_t type;
};

// another lane's v by DPP: 0x140 row_mirror, lane 15 - m within each 16-lane row; 0x141
// row_half_mirror, lane 7 - m within each 8; 0x4e quad_perm [2,3,0,1], lane m ^ 2
template <int kCtrl>
__device__ __forceinline__ float dpp_move(float v)
{
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), kCtrl, 0xf, 0xf, false));
}

// sum over the 16 lanes of a quarter (a DPP row), result in every lane of the quarter
__device__ __forceinline__ float quarter_sum(float v)
{
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 1);
  return v;
}

// The body of both backward kernels.  RAYS = false: the per-sample form, `sample_img` holds one image
// id per sample.  RAYS = true: the ray-uniform form for a dense [n_rays, S] grid of samples with
// S % 64 == 0 (n = n_rays * S), where every stride lies inside one ray: `sample_img` holds one image
// id per RAY, and the direction, SH16(dir), the embedding row and the SH half of the hidden layer
// c = b1 + w1[:, 16:32] . SH(dir) are wave-uniform inside a stride.  Per stride it then
//   - loads the direction and the image id once, through wave-uniform addresses, and evaluates
//     sh_basis once (no SH rows in the LDS tile, no per-sample dirs / image ids);
//   - forms c with 16 products for ONE sample tile -- every column of the result is the same --
//     and starts the accumulators of all TS sample tiles from it (16 TS products less);
//   - adds the SH half of d w1 as ONE product per neuron tile: d w1[j][16+i] = sh[i] sum_s d_pre[j][s],
//     and that sum is this stride's increment of acc_b1 (4 products instead of 16 TS).
// The head layer is untouched (logit and d_h are the per-sample form's terms in the same order); pre,
// d_enc and the parameter gradients are the same f32 terms added in another order (the SH part first
// instead of last, d w1[:, 16:] summed per stride before the product).
//
// RC (with RAYS; f2n_shade_bwd_rays_const): c and SH16(dir) were formed once per ray by
// shade_ray_const_kernel into `ray_const` [n_rays, 80].  load_inputs fetches the stride's c -- one
// 16-byte load per neuron tile, the address wave-uniform apart from q -- and its SH row m; the
// direction loads, sh_basis and the 16 products that formed c drop out, and the hidden layer's
// accumulators start from the loaded registers.  The buffer's c is a column of the same products, so
// every result keeps its bits.  `dirs` is not read.
template <int C, int V, bool WIDE, int TS, bool RAYS, bool RC = false>
__device__ __forceinline__ void shade_bwd_mfma_body(
  const float * __restrict__ enc, const float * __restrict__ dirs,
  const float * __restrict__ ray_const, const int32_t * __restrict__ sample_img,
  const float * __restrict__ p_w_h,
  const float * __restrict__ p_b_h, const float * __restrict__ p_w1,
  const float * __restrict__ p_b1, const float * __restrict__ p_w2,
  const float * __restrict__ p_b2, const float * __restrict__ p_emb,
  const float * __restrict__ d_logit, const float * __restrict__ d_rgb, float * __restrict__ d_enc,
  float * __restrict__ g_w_h, float * __restrict__ g_b_h, float * __restrict__ g_w1,
  float * __restrict__ g_b1, float * __restrict__ g_w2, float * __restrict__ g_b2,
  float * __restrict__ g_emb, int64_t n, int n_per_ray, int dir_per_ray)
{
  static_assert(RAYS || !RC, "the per-ray constant belongs to the ray-uniform form");
  using S = MShape<C, TS>;
  constexpr int kS1 = S::kS1, kM6 = S::kM6, kP = S::kP, kStride = S::kStride;
  __shared__ __attribute__((aligned(16))) float lds_all[S::kLdsFloats];
  float * lds_w = lds_all;

  // ---- stage the weight operands, pre-arranged per lane
  for (int i = threadIdx.x; i < S::kSlots * 64; i += S::kWaves * 64) {
    const int slot = i >> 6, l = i & 63, q = l >> 4, m = l & 15;
    float v;
    if (slot < S::oWA2) {
      const int t = slot - S::oWA1;
      v = p_w_h[m * C + q * kS1 + t];
    } else if (slot < S::oWA5) {
      const int M = (slot - S::oWA2) >> 3, t = (slot - S::oWA2) & 7;
      const int k = (t < 4) ? 4 * q + t : 16 + 4 * q + (t - 4);
      v = p_w1[(16 * M + m) * kIn2 + k];
    } else if (slot < S::oWA6) {
      const int M = (slot - S::oWA5) >> 2, r = (slot - S::oWA5) & 3;
      v = p_w1[(16 * M + 4 * q + r) * kIn2 + m];
    } else {
      const int M = (slot - S::oWA6) >> 2, r = (slot - S::oWA6) & 3;
      v = (16 * M + m < C) ? p_w_h[(4 * q + r) * C + 16 * M + m] : 0.f;
    }
    lds_w[i] = v;
  }
  if (threadIdx.x < 192) {  // output-layer weights of the vector path: [M][q][c][r] = w2[c][16M+4q+r]
    const int i = threadIdx.x, r = i & 3, c = (i >> 2) % 3, Mq = i / 12;
    lds_w[S::oW2Q + i] = p_w2[c * kHid + 16 * (Mq >> 2) + 4 * (Mq & 3) + r];
  }
  if (threadIdx.x < 16) lds_w[S::oBh + threadIdx.x] = p_b_h[threadIdx.x];
  if (threadIdx.x < 64) lds_w[S::oB1 + threadIdx.x] = p_b1[threadIdx.x];
  if (threadIdx.x < 4) lds_w[S::oB2 + threadIdx.x] = (threadIdx.x < 3) ? p_b2[threadIdx.x] : 0.f;

  const int lane = lane_id();
  // RAYS: the wave index in a scalar register, so that the stride's ray, its direction and its
  // image id are scalar loads
  const int wave = RAYS ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : (int)(threadIdx.x >> 6);
  const int q = lane >> 4, m = lane & 15;
  float * tile = lds_all + S::kWFloats + wave * S::kWaveFloats;
  float * XS = tile + S::oXS;
  float * ES = tile + S::oES;
  float * PS = tile + S::oPS;
  float * DS = tile + S::oDS;
  if constexpr (C % 16 != 0) {  // enc rows beyond C (read as zeros by the d w_h product)
    if (lane < kStride)
      for (int r = C; r < kM6 * 16; r++) ES[r * kP + lane] = 0.f;
  }
  __syncthreads();

  const float * wop = lds_w + lane;  // slot s of this lane: wop[s * 64]
  // One wave per SIMD, 512 registers: the hidden layer's weight operands stay in registers for the
  // whole kernel (C <= 32); read just in time from LDS they cost a full LDS latency every eight
  // products.  (The data-gradient operands of the last two phases are read when needed: the vector
  // phases of the output layer need their registers.)  At two waves per SIMD the 32 registers are
  // needed elsewhere and the partner wave covers the LDS latency.
  constexpr bool kWReg = TS == 4 && C <= 32;
  constexpr int kRegLo = S::oWA2, kRegHi = S::oWA5;  // the hidden layer's 32 slots
  float wreg[kWReg ? kRegHi - kRegLo : 1];
  if constexpr (kWReg) {
#pragma unroll
    for (int i = kRegLo; i < kRegHi; i++) wreg[i - kRegLo] = wop[i * 64];
  }
  auto W = [&](int slot) {
    const bool in_reg = kWReg && slot >= kRegLo && slot < kRegHi;
    return in_reg ? wreg[in_reg ? slot - kRegLo : 0] : wop[slot * 64];
  };
  // byte offsets of this quarter's first enc / d_enc row (quarter q owns channels q*kS1.., rows 4q..)
  using Off = typename RowOffset<WIDE>::type;
  const Off cE = (Off)((int64_t)(q * kS1) * n * 4), cD = (Off)((int64_t)(4 * q) * n * 4);
  const bool has_emb = (p_emb != nullptr) && (sample_img != nullptr);

  // per-lane accumulators that live across all strides of this wave
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc_w1[4][2];   // d w1[16M+4q+r][16N+m]
  constexpr int kW2M = S::kW2M, kW2R = S::kW2R;
  float acc_w2[3][kW2M][kW2R];  // d w2[c][16M+4q+r], partial over this lane's samples (vector FMAs);
                                // TS = 2: M = 2 M' + [m & 3 >= 2], r = m >> 2, over 8 lanes' samples
  float w2_even[3];             // TS = 2: the even M-tile's partials, combined with the odd one's
  f32x4 acc_wh[kM6];    // d w_h[4q+r][16N+m]
  float acc_b1[4];      // d b1[16M+m], partial over this quarter's k-steps (S-layout reads)
  f32x4 acc_bh = zero4; // d b_h[4q+r]
  float acc_b2 = 0.f;   // d b2[q]
  f32x4 acc_emb = zero4;  // d emb[emb_img][4q+r], partial over this lane's samples
  int emb_img = -1;
  auto flush_emb = [&]() {
    if (emb_img >= 0) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float t = quarter_sum(acc_emb[r]);
        if (m == 0) atomicAdd(g_emb + (int64_t)emb_img * kOut1 + 4 * q + r, t);
      }
    }
    acc_emb = zero4;
  };
#pragma unroll
  for (int M = 0; M < 4; M++) {
    acc_w1[M][0] = acc_w1[M][1] = zero4;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int r = 0; r < kW2R; r++)
        if (M < kW2M) acc_w2[c][M][r] = 0.f;
    acc_b1[M] = 0.f;
  }
#pragma unroll
  for (int N = 0; N < kM6; N++) acc_wh[N] = zero4;

  const int64_t n_strides = (n + kStride - 1) / kStride;
  const int64_t wave_global = (int64_t)blockIdx.x * S::kWaves + wave;
  const int64_t wave_count = (int64_t)gridDim.x * S::kWaves;
  // inputs of one stride that depend on nothing: issued together (one memory latency), and for
  // the NEXT stride while the current one is in its hidden layer
  float eB[kS1][TS];
  int img[TS];
#pragma unroll
  for (int T = 0; T < TS; T++) img[T] = 0;
  float dir[3];
  f32x4 cR[4];     // RC: the stride's c, rows 16M+4q+r
  float shR = 0.f; // RC: the stride's SH row m
  // SH: lane l evaluates sample s0 + l % kStride (at TS = 2 both halves of the wave the same 32)
  const int lS = lane % kStride;
  auto load_inputs = [&](int64_t st_, float (&eB_)[kS1][TS], int (&img_)[TS], float (&dir_)[3]) {
    const int64_t s0_ = st_ * kStride;  // may lie beyond the end: every index is clamped to a real sample
    if constexpr (RAYS) {  // every stride is whole (n % 64 == 0) and lies in one ray
      const uint32_t sc = (uint32_t)((s0_ < n) ? s0_ : n - kStride);
#pragma unroll
      for (int t = 0; t < kS1; t++)
#pragma unroll
        for (int T = 0; T < TS; T++) eB_[t][T] = ld_row(enc + (int64_t)t * n, (sc + 16 * T + m) * 4 + cE);
      // the stride's ray (a scalar): its image id, and its row of a per-ray `dirs`
      const uint32_t ray = (RC || has_emb || dir_per_ray) ? sc / (uint32_t)n_per_ray : 0u;
      if (has_emb) {
        const int id = sample_img[ray];
#pragma unroll
        for (int T = 0; T < TS; T++) img_[T] = id;
      }
      if constexpr (RC) {
        const float * rc = ray_const + (int64_t)ray * kRayConst;
#pragma unroll
        for (int M = 0; M < 4; M++) cR[M] = *reinterpret_cast<const f32x4 *>(rc + 16 * M + 4 * q);
        shR = rc[kHid + m];
        return;
      }
      const int64_t drow = dir_per_ray ? (int64_t)ray : (int64_t)sc;
#pragma unroll
      for (int k = 0; k < 3; k++) dir_[k] = dirs[drow * 3 + k];
      return;
    }
    uint32_t off_[TS];
#pragma unroll
    for (int T = 0; T < TS; T++) off_[T] = (uint32_t)(((s0_ + 16 * T + m < n) ? s0_ + 16 * T + m : n - 1) * 4);
#pragma unroll
    for (int t = 0; t < kS1; t++)
#pragma unroll
      for (int T = 0; T < TS; T++) eB_[t][T] = ld_row(enc + (int64_t)t * n, off_[T] + cE);
    if (has_emb) {
#pragma unroll
      for (int T = 0; T < TS; T++) img_[T] = ld_row(sample_img, off_[T]);
    }
    const uint32_t offL = (uint32_t)(((s0_ + lS < n) ? s0_ + lS : n - 1) * 12);
#pragma unroll
    for (int k = 0; k < 3; k++) dir_[k] = ld_row(dirs + k, offL);
  };
  if constexpr (TS == 4) {
    load_inputs(wave_global, eB, img, dir);
    issue_fence();
  }

  for (int64_t st = wave_global; st < n_strides; st += wave_count) {
    const int64_t s0 = st * kStride;
    // TS = 2: no prefetch of the next stride (its registers would spill); the partner wave on the
    // SIMD runs while this one waits
    if constexpr (TS == 2) load_inputs(st, eB, img, dir);
    // this lane's Q-layout samples 16T+m (clamped: invalid ones read a real sample and get zero
    // gradients).  Everything per sample is addressed as wave-uniform pointer + 32-bit byte offset
    // (the launcher guarantees C * n * 4 < 2^32): TS offset registers serve all rows.
    bool vT[TS];
    uint32_t offS[TS];
#pragma unroll
    for (int T = 0; T < TS; T++) {
      const int64_t s = s0 + 16 * T + m;
      vT[T] = RAYS || s < n;
      offS[T] = (uint32_t)((vT[T] ? s : n - 1) * 4);
    }

    // ---- head layer: h[4q+r][s] = w_h . enc + b_h
    f32x4 h[TS];
#pragma unroll
    for (int T = 0; T < TS; T++) h[T] = *reinterpret_cast<const f32x4 *>(lds_w + S::oBh + 4 * q);
#pragma unroll
    for (int t = 0; t < kS1; t++) {
      const float a = W(S::oWA1 + t);
#pragma unroll
      for (int T = 0; T < TS; T++) h[T] = mfma16(a, eB[t][T], h[T]);
    }
    // enc's S-layout image for d w_h at the end of the stride
#pragma unroll
    for (int t = 0; t < kS1; t++)
#pragma unroll
      for (int T = 0; T < TS; T++) ES[(q * kS1 + t) * kP + 16 * T + m] = eB[t][T];

    phase_fence_v<V>();
    // ---- shader input X: rows 0..15 = [1, h[1..15]] (+ embedding), rows 16..31 = SH16(dir)
    f32x4 Xh[TS];
    int img_cur[TS];
#pragma unroll
    for (int T = 0; T < TS; T++) img_cur[T] = img[T];
    float shq[4], shm = 0.f;  // RAYS: SH rows 4q+t' (the recompute's B operand) and row m (d w1's)
    {
      f32x4 e4[TS];
      if (has_emb) {
#pragma unroll
        for (int T = 0; T < TS; T++)
          if (!RAYS || T == 0)
            e4[T] = *reinterpret_cast<const f32x4 *>(p_emb + (int64_t)img_cur[T] * kOut1 + 4 * q);
      }
      // SH: lane l evaluates sample s0 + l % kStride and writes its column of the S-layout tile
      // directly (at TS = 2 the lower half of the wave rows 16..23, the upper half rows 24..31)
      // RAYS: one direction per stride, every lane evaluates it and keeps the rows it supplies
      float sh[16];
      if constexpr (!RC) sh_basis<4>(dir[0], dir[1], dir[2], sh);
      if constexpr (RC) {
        shm = shR;
      } else if constexpr (RAYS) {
#pragma unroll
        for (int t = 0; t < 4; t++)
          shq[t] = pick4(q, sh[t], sh[4 + t], sh[8 + t], sh[12 + t]);
        shm = pick4(
          m >> 2, pick4(m & 3, sh[0], sh[1], sh[2], sh[3]), pick4(m & 3, sh[4], sh[5], sh[6], sh[7]),
          pick4(m & 3, sh[8], sh[9], sh[10], sh[11]), pick4(m & 3, sh[12], sh[13], sh[14], sh[15]));
      } else if constexpr (TS == 4) {
#pragma unroll
        for (int k = 0; k < 16; k++) XS[(16 + k) * kP + lane] = sh[k];
      } else {
        const bool hi = lane >= 32;
#pragma unroll
        for (int k = 0; k < 8; k++) XS[(16 + (hi ? 8 : 0) + k) * kP + lS] = hi ? sh[8 + k] : sh[k];
      }
#pragma unroll
      for (int T = 0; T < TS; T++) {
        Xh[T] = h[T];
        if (q == 0) Xh[T][0] = 1.f;
        if (has_emb) Xh[T] += e4[RAYS ? 0 : T];
#pragma unroll
        for (int r = 0; r < 4; r++) XS[(4 * q + r) * kP + 16 * T + m] = Xh[T][r];
      }
    }
    if constexpr (!RAYS) wave_lds_sync();  // RAYS: XS is read in the d w1 phase only, behind two syncs

    phase_fence_v<V>();
    // ---- hidden layer: pre[16M+4q+r][s] = w1 . X + b1
    f32x4 pre[4][TS];
    if constexpr (RAYS) {
      // the SH half once for one sample tile (four independent chains), then the shading features
      if constexpr (RC) {
#pragma unroll
        for (int M = 0; M < 4; M++) pre[M][0] = cR[M];
      } else {
#pragma unroll
        for (int M = 0; M < 4; M++)
          pre[M][0] = *reinterpret_cast<const f32x4 *>(lds_w + S::oB1 + 16 * M + 4 * q);
#pragma unroll
        for (int t = 4; t < 8; t++)
#pragma unroll
          for (int M = 0; M < 4; M++) pre[M][0] = mfma16(W(S::oWA2 + M * 8 + t), shq[t - 4], pre[M][0]);
      }
#pragma unroll
      for (int M = 0; M < 4; M++) {
#pragma unroll
        for (int T = 1; T < TS; T++) pre[M][T] = pre[M][0];
#pragma unroll
        for (int t = 0; t < 4; t++) {
          const float a = W(S::oWA2 + M * 8 + t);
#pragma unroll
          for (int T = 0; T < TS; T++) pre[M][T] = mfma16(a, Xh[T][t], pre[M][T]);
        }
      }
    } else {
      float Xs[4][TS];  // SH rows 16+4q+t' of this lane's samples
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int T = 0; T < TS; T++) Xs[t][T] = XS[(16 + 4 * q + t) * kP + 16 * T + m];
#pragma unroll
      for (int M = 0; M < 4; M++) {
#pragma unroll
        for (int T = 0; T < TS; T++)
          pre[M][T] = *reinterpret_cast<const f32x4 *>(lds_w + S::oB1 + 16 * M + 4 * q);
#pragma unroll
        for (int t = 0; t < 8; t++) {
          const float a = W(S::oWA2 + M * 8 + t);
#pragma unroll
          for (int T = 0; T < TS; T++)
            pre[M][T] = mfma16(a, (t < 4) ? Xh[T][t] : Xs[t - 4][T], pre[M][T]);
        }
      }
    }

    phase_fence_v<V>();
    // ---- output layer on the vector pipe: per-quarter partial sums over this lane's 16 hidden
    // neurons (pre becomes relu(pre): its sign is all the ReLU's backward needs), the four quarters
    // summed by one all-ones product per (c, sample tile); then d_o for c = q
    float d_o[TS];
    {
      float g_rgb[TS];  // d_rgb[s][c = q]: in flight during the sums below
#pragma unroll
      for (int T = 0; T < TS; T++) g_rgb[T] = ld_row(d_rgb, 3 * offS[T] + ((q < 3) ? 4 * q : 8));
      issue_fence();
      float po[3][TS];
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int T = 0; T < TS; T++) po[c][T] = 0.f;
#pragma unroll
      for (int M = 0; M < 4; M++) {
        f32x4 wq[3];
#pragma unroll
        for (int c = 0; c < 3; c++)
          wq[c] = *reinterpret_cast<const f32x4 *>(lds_w + S::oW2Q + ((M * 4 + q) * 3 + c) * 4);
#pragma unroll
        for (int T = 0; T < TS; T++)
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const float p = relu(pre[M][T][r]);
            pre[M][T][r] = p;
#pragma unroll
            for (int c = 0; c < 3; c++) po[c][T] = __builtin_fmaf(wq[c][r], p, po[c][T]);
          }
      }
      const float b2q = lds_w[S::oB2 + q];
#pragma unroll
      for (int T = 0; T < TS; T++) {
        const float s0 = mfma16(1.f, po[0][T], zero4)[0];
        const float s1 = mfma16(1.f, po[1][T], zero4)[0];
        const float s2 = mfma16(1.f, po[2][T], zero4)[0];
        const float o = ((q == 0) ? s0 : (q == 1) ? s1 : s2) + b2q;
        const float sg = 1.f / (1.f + expf(-o));
        const float g = (vT[T] && q < 3) ? g_rgb[T] : 0.f;
        d_o[T] = g * (1.f + 2.f * kEps) * sg * (1.f - sg);
        acc_b2 += d_o[T];
        if (q < 3) DS[q * kP + 16 * T + m] = d_o[T];
      }
    }
    wave_lds_sync();

    phase_fence_v<V>();
    // ---- d w2[c][j] += sum_s d_o[c][s] relu(pre)[j][s] and d_hid[j][s] = [pre > 0] sum_c w2[c][j]
    // d_o[c][s], both on the registers that hold relu(pre): d_o of all three colours comes back from
    // the LDS tile (lane (q, m) computed colour q only); d_hid replaces pre
    {
      float doc[3][TS];
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int T = 0; T < TS; T++) doc[c][T] = DS[c * kP + 16 * T + m];
#pragma unroll
      for (int M = 0; M < 4; M++) {
        f32x4 wq[3];
#pragma unroll
        for (int c = 0; c < 3; c++)
          wq[c] = *reinterpret_cast<const f32x4 *>(lds_w + S::oW2Q + ((M * 4 + q) * 3 + c) * 4);
        auto d_hid = [&](int r) {
#pragma unroll
          for (int T = 0; T < TS; T++) {
            float dh = wq[0][r] * doc[0][T];
            dh = __builtin_fmaf(wq[1][r], doc[1][T], dh);
            dh = __builtin_fmaf(wq[2][r], doc[2][T], dh);
            pre[M][T][r] = (pre[M][T][r] > 0.f) ? dh : 0.f;
          }
        };
        if constexpr (kW2R == 4) {
#pragma unroll
          for (int r = 0; r < 4; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
              float t = doc[c][0] * pre[M][0][r];
#pragma unroll
              for (int T = 1; T < TS; T++) t = __builtin_fmaf(doc[c][T], pre[M][T][r], t);
              acc_w2[c][M][r] += t;
            }
            d_hid(r);
          }
        } else {
          float t4[3][4];
#pragma unroll
          for (int r = 0; r < 4; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
              float t = doc[c][0] * pre[M][0][r];
#pragma unroll
              for (int T = 1; T < TS; T++) t = __builtin_fmaf(doc[c][T], pre[M][T][r], t);
              t4[c][r] = t;
            }
          // three steps of a reduce-scatter over the quarter, 6 accumulators instead of 48: lane m
          // keeps rows r = 2 [m >= 8] + r' and adds them from lane 15 - m (DPP row_mirror), which
          // keeps the other two; then row r = m >> 2 from lane (m & 8) + 7 - (m & 7)
          // (row_half_mirror); then, over a pair of M-tiles, M = 2 M' + [m & 3 >= 2] from lane
          // m ^ 2 (quad_perm [2,3,0,1]).  The rest of the sum, over lanes m and m ^ 1, at the flush.
          const bool lo = m < 8, lo2 = (m & 7) < 4, lo3 = (m & 3) < 2;
#pragma unroll
          for (int c = 0; c < 3; c++) {
            float h2[2];
#pragma unroll
            for (int r = 0; r < 2; r++) {
              const float own = lo ? t4[c][r] : t4[c][r + 2];
              const float give = lo ? t4[c][r + 2] : t4[c][r];
              h2[r] = own + dpp_move<0x140>(give);
            }
            const float own = lo2 ? h2[0] : h2[1];
            const float give = lo2 ? h2[1] : h2[0];
            const float h1 = own + dpp_move<0x141>(give);
            if (M % 2 == 0) {
              w2_even[c] = h1;
            } else {
              const float own3 = lo3 ? w2_even[c] : h1;
              const float give3 = lo3 ? h1 : w2_even[c];
              acc_w2[c][M / 2][0] += own3 + dpp_move<0x4e>(give3);
            }
          }
#pragma unroll
          for (int r = 0; r < 4; r++) d_hid(r);
        }
      }
    }

    phase_fence_v<V>();
    // ---- d w1[j][i] += sum_s d_hid[j][s] X[i][s], the four neuron tiles streaming through the LDS
    // tile as above
    {
      auto put = [&](int M) {
#pragma unroll
        for (int T = 0; T < TS; T++)
#pragma unroll
          for (int r = 0; r < 4; r++) PS[(4 * q + r) * kP + 16 * T + m] = pre[M][T][r];
      };
      put(0);
      wave_lds_sync();
#pragma unroll
      for (int M = 0; M < 4; M++) {
        f32x4 a4[TS];
#pragma unroll
        for (int u = 0; u < TS; u++)
          a4[u] = *reinterpret_cast<const f32x4 *>(PS + m * kP + 16 * u + 4 * q);
        wave_lds_sync();
        if (M < 3) {
          put(M + 1);
          wave_lds_sync();
        }
        constexpr int kN = RAYS ? 1 : 2;  // RAYS: the SH half is one product per neuron tile, below
        float db = 0.f;                   // RAYS: this stride's increment of acc_b1[M]
#pragma unroll
        for (int u = 0; u < TS; u++) {
          const float su = (a4[u][0] + a4[u][1]) + (a4[u][2] + a4[u][3]);
          if constexpr (RAYS) db += su;
          else acc_b1[M] += su;
          f32x4 b4[kN];
#pragma unroll
          for (int N = 0; N < kN; N++)
            b4[N] = *reinterpret_cast<const f32x4 *>(XS + (16 * N + m) * kP + 16 * u + 4 * q);
#pragma unroll
          for (int k = 0; k < 4; k++)
#pragma unroll
            for (int N = 0; N < kN; N++) acc_w1[M][N] = mfma16(a4[u][k], b4[N][k], acc_w1[M][N]);
        }
        if constexpr (RAYS) {
          // lane (q, m): A[row m][k = q] = quarter q's part of d b1[16M+m], B[k = q][col m] = sh[m]
          acc_b1[M] += db;
          acc_w1[M][1] = mfma16(db, shm, acc_w1[M][1]);
        }
      }
    }

    // ---- the next stride's inputs (their registers are free since the head layer / the SH block;
    // issued behind the vector phases and the d w1 product, which leave no registers for them: the
    // 128 products of the last three phases, ~4 K cycles, cover the latency -- asking one phase
    // earlier, 260 products ahead, measured the same within noise, 1.45-1.50 ms, and spills the WIDE
    // instantiation)
    if constexpr (TS == 4) {
      load_inputs(st + wave_count, eB, img, dir);
      issue_fence();
    }

    phase_fence_v<V>();
    // ---- d_X rows 0..15 = w1[:, 0:16]^T . d_hid   (the SH inputs carry no gradient)
    float g_logit[TS];  // in flight during the products below
#pragma unroll
    for (int T = 0; T < TS; T++) g_logit[T] = ld_row(d_logit, offS[T]);
    issue_fence();
    f32x4 dX[TS];
#pragma unroll
    for (int T = 0; T < TS; T++) dX[T] = zero4;
#pragma unroll
    for (int M = 0; M < 4; M++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float a = W(S::oWA5 + M * 4 + r);
#pragma unroll
        for (int T = 0; T < TS; T++) dX[T] = mfma16(a, pre[M][T][r], dX[T]);
      }

    phase_fence_v<V>();
    // ---- appearance embedding: d emb[img][i] += d_X[i]  (row 0 included: X[0] = 1 + emb[0]).
    // A chunk of rays usually comes from ONE image: its row's gradient is accumulated in registers
    // and flushed when the image changes / at the end.  (One atomic per stride on the same 64 bytes,
    // from every wave of the chip, serialises in L2: 6.9 ms instead of 1.7 ms per launch.)
    if (has_emb) {
      const int img0 = __builtin_amdgcn_readfirstlane(img_cur[0]);
      bool one_img = true;
      if constexpr (!RAYS) {
#pragma unroll
        for (int T = 0; T < TS; T++) one_img = one_img && img_cur[T] == img0;
      }
      if (RAYS || __all(one_img)) {
        if (img0 != emb_img) {
          flush_emb();
          emb_img = img0;
        }
        if constexpr (TS == 4) acc_emb += (dX[0] + dX[1]) + (dX[2] + dX[3]);  // clamped samples carry zeros
        else acc_emb += dX[0] + dX[1];
      } else {
#pragma unroll
        for (int T = 0; T < TS; T++)
#pragma unroll
          for (int r = 0; r < 4; r++)
            if (vT[T]) atomicAdd(g_emb + (int64_t)img_cur[T] * kOut1 + 4 * q + r, dX[T][r]);
      }
    }

    // ---- d_h: the head outputs' gradient; row 0 is the density logit's
    f32x4 d_h[TS];
#pragma unroll
    for (int T = 0; T < TS; T++) {
      d_h[T] = dX[T];
      if (q == 0) d_h[T][0] = vT[T] ? g_logit[T] : 0.f;
      acc_bh += d_h[T];
#pragma unroll
      for (int r = 0; r < 4; r++) PS[(4 * q + r) * kP + 16 * T + m] = d_h[T][r];
    }

    phase_fence_v<V>();
    // ---- d_enc[c][s] = w_h^T . d_h
#pragma unroll
    for (int M = 0; M < kM6; M++) {
      f32x4 de[TS];
#pragma unroll
      for (int T = 0; T < TS; T++) de[T] = zero4;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float a = W(S::oWA6 + M * 4 + r);
#pragma unroll
        for (int T = 0; T < TS; T++) de[T] = mfma16(a, d_h[T][r], de[T]);
      }
#pragma unroll
      for (int T = 0; T < TS; T++)
        if (vT[T]) {
#pragma unroll
          for (int r = 0; r < 4; r++)
            if (C % 16 == 0 || 16 * M + 4 * q + r < C)
              st_row(d_enc + (int64_t)(16 * M + r) * n, offS[T] + cD, de[T][r]);
        }
    }

    phase_fence_v<V>();
    // ---- d w_h[i][c] += sum_s d_h[i][s] enc[c][s]
    wave_lds_sync();
#pragma unroll
    for (int u = 0; u < TS; u++) {
      const f32x4 a4 = *reinterpret_cast<const f32x4 *>(PS + m * kP + 16 * u + 4 * q);
#pragma unroll
      for (int N = 0; N < kM6; N++) {
        const f32x4 b4 = *reinterpret_cast<const f32x4 *>(ES + (16 * N + m) * kP + 16 * u + 4 * q);
#pragma unroll
        for (int k = 0; k < 4; k++) acc_wh[N] = mfma16(a4[k], b4[k], acc_wh[N]);
      }
    }
    wave_lds_sync();
  }

  // ---- flush the accumulators: the waves' sums meet in wave 0 first (the LDS is free now), so a
  // workgroup sends one set of atomics instead of one per wave -- with few strides per wave
  // (a 512-ray training batch: 8) the 4 160 atomics of every wave on the same 2 400 addresses were a
  // third of the kernel
  if (has_emb) flush_emb();
  {
    auto each_acc = [&](auto && fn) {
      int i = 0;
#pragma unroll
      for (int M = 0; M < 4; M++) {
#pragma unroll
        for (int N = 0; N < 2; N++)
#pragma unroll
          for (int r = 0; r < 4; r++) acc_w1[M][N][r] = fn(acc_w1[M][N][r], i++);
        acc_b1[M] = fn(acc_b1[M], i++);
      }
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int M = 0; M < kW2M; M++)
#pragma unroll
          for (int r = 0; r < kW2R; r++) acc_w2[c][M][r] = fn(acc_w2[c][M][r], i++);
#pragma unroll
      for (int N = 0; N < kM6; N++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc_wh[N][r] = fn(acc_wh[N][r], i++);
#pragma unroll
      for (int r = 0; r < 4; r++) acc_bh[r] = fn(acc_bh[r], i++);
      acc_b2 = fn(acc_b2, i++);
    };
    if constexpr (TS == 4) {  // one round through the waves' own tiles
      static_assert(S::kAccs * 64 <= S::kWaveFloats, "the accumulators fit a wave's tile region");
      wave_lds_sync();
      if (wave != 0) each_acc([&](float v, int i) { tile[i * 64 + lane] = v; return v; });
      __syncthreads();
      if (wave == 0) {
#pragma unroll
        for (int w = 1; w < S::kWaves; w++) {
          const float * other = lds_all + S::kWFloats + w * S::kWaveFloats;
          each_acc([&](float v, int i) { return v + other[i * 64 + lane]; });
        }
      }
    } else {
      // in rounds of kMeetRegs registers through the whole LDS (the weights are dead too); the sums
      // meet in the order wave 1, 2, .. as in one round
      constexpr int R = S::kMeetRegs;
#pragma unroll
      for (int rd = 0; rd < S::kMeetRounds; rd++) {
        const int lo = rd * R, hi = lo + R;
        __syncthreads();  // every wave is out of its loop / wave 0 has read the previous round
        if (wave != 0)
          each_acc([&](float v, int i) {
            if (i >= lo && i < hi) lds_all[((wave - 1) * R + i - lo) * 64 + lane] = v;
            return v;
          });
        __syncthreads();
        if (wave == 0) {
#pragma unroll
          for (int w = 1; w < S::kWaves; w++)
            each_acc([&](float v, int i) {
              return (i >= lo && i < hi) ? v + lds_all[((w - 1) * R + i - lo) * 64 + lane] : v;
            });
        }
      }
    }
    if (wave != 0) return;
  }
#pragma unroll
  for (int M = 0; M < 4; M++) {
#pragma unroll
    for (int N = 0; N < 2; N++)
#pragma unroll
      for (int r = 0; r < 4; r++)
        atomicAdd(g_w1 + (16 * M + 4 * q + r) * kIn2 + 16 * N + m, acc_w1[M][N][r]);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if constexpr (kW2R == 4) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const float t = quarter_sum(acc_w2[c][M][r]);  // over the quarter's 16 sample columns
          if (m == 0) atomicAdd(g_w2 + c * kHid + 16 * M + 4 * q + r, t);
        }
      } else if (M % 2 == 0) {  // lanes m and m ^ 1 hold M-tile M + [m & 3 >= 2], row m >> 2
        float t = acc_w2[c][M / 2][0];
        t += __shfl_xor(t, 1);
        if ((m & 1) == 0) atomicAdd(g_w2 + c * kHid + 16 * (M + ((m >> 1) & 1)) + 4 * q + (m >> 2), t);
      }
    }
    {
      float t = acc_b1[M];  // lane (q, m): neuron 16M+m, this quarter's samples
      t += __shfl_xor(t, 16);
      t += __shfl_xor(t, 32);
      if (q == 0) atomicAdd(g_b1 + 16 * M + m, t);
    }
  }
#pragma unroll
  for (int N = 0; N < kM6; N++)
#pragma unroll
    for (int r = 0; r < 4; r++)
      if (C % 16 == 0 || 16 * N + m < C) atomicAdd(g_w_h + (4 * q + r) * C + 16 * N + m, acc_wh[N][r]);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const float t = quarter_sum(acc_bh[r]);
    if (m == 0) atomicAdd(g_b_h + 4 * q + r, t);
  }
  {
    const float t = quarter_sum(acc_b2);
    if (m == 0 && q < 3) atomicAdd(g_b2 + q, t);
  }
}

#define F2N_SHADE_BWD_PARAMS(DIRS, IMG)                                                               \
  const float * __restrict__ enc, const float * __restrict__ DIRS, const int32_t * __restrict__ IMG,  \
    const float * __restrict__ p_w_h, const float * __restrict__ p_b_h,                               \
    const float * __restrict__ p_w1, const float * __restrict__ p_b1,                                 \
    const float * __restrict__ p_w2, const float * __restrict__ p_b2,                                 \
    const float * __restrict__ p_emb, const float * __restrict__ d_logit,                             \
    const float * __restrict__ d_rgb, float * __restrict__ d_enc, float * __restrict__ g_w_h,         \
    float * __restrict__ g_b_h, float * __restrict__ g_w1, float * __restrict__ g_b1,                 \
    float * __restrict__ g_w2, float * __restrict__ g_b2, float * __restrict__ g_emb
#define F2N_SHADE_BWD_ARGS(DIRS, RCONST, IMG)                                                         \
  enc, DIRS, RCONST, IMG, p_w_h, p_b_h, p_w1, p_b1, p_w2, p_b2, p_emb, d_logit, d_rgb, d_enc, g_w_h,   \
    g_b_h, g_w1, g_b1, g_w2, g_b2, g_emb

// per-sample form: any n, one image id per sample
template <int C, int V, bool WIDE, int TS>
__global__ __launch_bounds__((MShape<C, TS>::kWaves * 64)) void shade_bwd_mfma_kernel(
  F2N_SHADE_BWD_PARAMS(dirs, sample_img), int64_t n)
{
  shade_bwd_mfma_body<C, V, WIDE, TS, false>(F2N_SHADE_BWD_ARGS(dirs, nullptr, sample_img), n, 0, 0);
}

// ray-uniform form: n = n_rays * S samples in ray-major order, S % 64 == 0, one image id per ray;
// dir_per_ray: `dirs` is [n_rays, 3], one row per ray (0: [n, 3], the row of the stride's first sample)
template <int C, int V, bool WIDE, int TS>
__global__ __launch_bounds__((MShape<C, TS>::kWaves * 64)) void shade_bwd_mfma_rays_kernel(
  F2N_SHADE_BWD_PARAMS(dirs, ray_img), int64_t n, int S, int dir_per_ray)
{
  shade_bwd_mfma_body<C, V, WIDE, TS, true>(F2N_SHADE_BWD_ARGS(dirs, nullptr, ray_img), n, S, dir_per_ray);
}

// the ray-uniform form with the per-ray constant loaded: `ray_const` [n_rays, 80] from
// shade_ray_const_kernel in place of the directions
template <int C, int V, bool WIDE, int TS>
__global__ __launch_bounds__((MShape<C, TS>::kWaves * 64)) void shade_bwd_mfma_rays_kernel_const(
  F2N_SHADE_BWD_PARAMS(ray_const, ray_img), int64_t n, int S)
{
  shade_bwd_mfma_body<C, V, WIDE, TS, true, true>(
    F2N_SHADE_BWD_ARGS(nullptr, ray_const, ray_img), n, S, 1);
}
#undef F2N_SHADE_BWD_PARAMS
#undef F2N_SHADE_BWD_ARGS


// ---- forward on the matrix cores ------------------------------------------------------------------
// The forward third of the kernel above (head, hidden and output layer in the Q-layout, no lane
// movement), four waves per SIMD (three until the end of round 3; two, three, four: 0.584, 0.577,
// 0.551 ms per 8.4 M samples alone): no accumulators live across strides and the other waves hide one
// wave's loads.  The output layer STAYS on the matrix cores here (rows 0, 4, 8 of a 16-row operand):
// the vector form the backward uses was measured here too and lost, 0.58 against 0.55 ms per 8.2 M
// samples inside the bench -- 52 products fewer but 200 vector instructions more and, at 168
// registers, ten spilled; this kernel waits on latencies, not on the matrix pipe.  LDS: the three forward weight operands (56 slots at
// C = 32) + a 16-row tile per wave that moves SH16(dir) from lane = sample into the Q-layout.
//
// RAYS (see shade_bwd_mfma_body): `sample_img` holds one image id per ray, the direction and the id
// are loaded once per stride through wave-uniform addresses, sh_basis runs once, and the SH half of
// the hidden layer is formed for one sample tile (16 products) and starts all four: 176 products
// per stride instead of 224, no SH tile in LDS and none of its syncs.  No pre_out in that form.
//
// RC (with RAYS; f2n_shade_fwd_rays_const): c comes from `ray_const` [n_rays, 80], written once per
// ray by shade_ray_const_kernel -- one 16-byte load per neuron tile, the address wave-uniform apart
// from q: tile 0 issued with the stride's encoding, tiles 1..3 behind the head layer (kRcEarly).
// The direction loads, sh_basis and the 16 products drop out: 160 products per stride, the same
// bits.  `dirs` is not read.
template <int C, bool WIDE, int W, bool RAYS, bool RC = false>
__device__ __forceinline__ void shade_fwd_mfma_body(
  const float * __restrict__ enc, const float * __restrict__ dirs,
  const float * __restrict__ ray_const, const int32_t * __restrict__ sample_img,
  const float * __restrict__ p_w_h,
  const float * __restrict__ p_b_h, const float * __restrict__ p_w1,
  const float * __restrict__ p_b1, const float * __restrict__ p_w2,
  const float * __restrict__ p_b2, const float * __restrict__ p_emb, float * __restrict__ logit,
  float * __restrict__ rgb, float * __restrict__ pre_out, int64_t n, int n_per_ray, int dir_per_ray)
{
  static_assert(RAYS || !RC, "the per-ray constant belongs to the ray-uniform form");
  using S = FShape<C, W>;
  constexpr int kS1 = S::kS1, kP = S::kP;
  __shared__ __attribute__((aligned(16))) float lds_all[RAYS ? S::kWFloats : S::kLdsFloats];
  float * lds_w = lds_all;
  stage_fwd_weights<C, W>(lds_w, p_w_h, p_b_h, p_w1, p_b1, p_w2, p_b2);
  __syncthreads();

  const int lane = lane_id();
  const int wave = RAYS ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : (int)(threadIdx.x >> 6);
  const int q = lane >> 4, m = lane & 15;
  float * XS = lds_all + (RAYS ? 0 : S::kWFloats + wave * S::kWaveFloats);  // SH rows 0..15 of this wave
  const float * wop = lds_w + lane;
  using Off = typename RowOffset<WIDE>::type;
  const Off cE = (Off)((int64_t)(q * kS1) * n * 4), cP = (Off)((int64_t)(4 * q) * n * 4);
  const bool has_emb = (p_emb != nullptr) && (sample_img != nullptr);
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  const int64_t n_strides = (n + 63) / 64;
  const int64_t wave_count = (int64_t)gridDim.x * S::kWaves;
  for (int64_t st = (int64_t)blockIdx.x * S::kWaves + wave; st < n_strides; st += wave_count) {
    const int64_t s0 = st * 64;
    bool vT[4];
    uint32_t offS[4];
#pragma unroll
    for (int T = 0; T < 4; T++) {
      const int64_t s = s0 + 16 * T + m;
      vT[T] = RAYS || s < n;
      offS[T] = (uint32_t)((vT[T] ? s : n - 1) * 4);
    }
    float eB[kS1][4];
#pragma unroll
    for (int t = 0; t < kS1; t++)
#pragma unroll
      for (int T = 0; T < 4; T++) eB[t][T] = ld_row(enc + (int64_t)t * n, offS[T] + cE);
    int img[4] = {0, 0, 0, 0};
    float dir[3];
    f32x4 cR[4];  // RC: the stride's c, rows 16M+4q+r
    const float * rc = nullptr;
    if constexpr (RC) {
      const uint32_t ray = (uint32_t)s0 / (uint32_t)n_per_ray;
      if (has_emb) img[0] = sample_img[ray];
      rc = ray_const + (int64_t)ray * kRayConst;
#pragma unroll
      for (int M = 0; M < kRcEarly; M++) cR[M] = *reinterpret_cast<const f32x4 *>(rc + 16 * M + 4 * q);
    } else if constexpr (RAYS) {
      const uint32_t ray = (has_emb || dir_per_ray) ? (uint32_t)s0 / (uint32_t)n_per_ray : 0u;
      if (has_emb) img[0] = sample_img[ray];
      const int64_t drow = dir_per_ray ? (int64_t)ray : s0;
#pragma unroll
      for (int k = 0; k < 3; k++) dir[k] = dirs[drow * 3 + k];
    } else {
      if (has_emb) {
#pragma unroll
        for (int T = 0; T < 4; T++) img[T] = ld_row(sample_img, offS[T]);
      }
      const uint32_t offL = (uint32_t)(((s0 + lane < n) ? s0 + lane : n - 1) * 12);
#pragma unroll
      for (int k = 0; k < 3; k++) dir[k] = ld_row(dirs + k, offL);
    }
    issue_fence();

    // ---- head layer
    f32x4 h[4];
#pragma unroll
    for (int T = 0; T < 4; T++) h[T] = *reinterpret_cast<const f32x4 *>(lds_w + S::oBh + 4 * q);
#pragma unroll
    for (int t = 0; t < kS1; t++) {
      const float a = wop[(S::oWA1 + t) * 64];
#pragma unroll
      for (int T = 0; T < 4; T++) h[T] = mfma16(a, eB[t][T], h[T]);
    }
    if (q == 0) {
#pragma unroll
      for (int T = 0; T < 4; T++)
        if (vT[T]) st_row(logit, offS[T], h[T][0]);
    }

    // ---- shader input
    f32x4 Xh[4];
    float Xs[4][4];  // SH rows 4q+t of this lane's samples; RAYS: Xs[t][0] alone, the stride's
    {
      f32x4 e4[4];
      if (has_emb) {
#pragma unroll
        for (int T = 0; T < 4; T++)
          if (!RAYS || T == 0)
            e4[T] = *reinterpret_cast<const f32x4 *>(p_emb + (int64_t)img[T] * kOut1 + 4 * q);
      }
      float sh[16];
      if constexpr (!RC) sh_basis<4>(dir[0], dir[1], dir[2], sh);
      if constexpr (RC) {
#pragma unroll
        for (int M = kRcEarly; M < 4; M++) cR[M] = *reinterpret_cast<const f32x4 *>(rc + 16 * M + 4 * q);
      } else if constexpr (RAYS) {
#pragma unroll
        for (int t = 0; t < 4; t++)
          Xs[t][0] = pick4(q, sh[t], sh[4 + t], sh[8 + t], sh[12 + t]);
      } else {
#pragma unroll
        for (int k = 0; k < 16; k++) XS[k * kP + lane] = sh[k];
      }
#pragma unroll
      for (int T = 0; T < 4; T++) {
        Xh[T] = h[T];
        if (q == 0) Xh[T][0] = 1.f;
        if (has_emb) Xh[T] += e4[RAYS ? 0 : T];
      }
    }
    if constexpr (!RAYS) {
      wave_lds_sync();
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int T = 0; T < 4; T++) Xs[t][T] = XS[(4 * q + t) * kP + 16 * T + m];
      wave_lds_sync();
    }

    // ---- hidden layer, then the output layer on rows 0, 4, 8
    f32x4 o[4];
#pragma unroll
    for (int T = 0; T < 4; T++) {
      o[T] = zero4;
      o[T][0] = lds_w[S::oB2 + q];
    }
#pragma unroll
    for (int M = 0; M < 4; M++) {
      f32x4 pre[4];
      if constexpr (RAYS) {
        // c = b1 + w1[:, 16:32] . SH(dir) for one sample tile: the same in every column
        f32x4 c;
        if constexpr (RC) {
          c = cR[M];
        } else {
          c = *reinterpret_cast<const f32x4 *>(lds_w + S::oB1 + 16 * M + 4 * q);
#pragma unroll
          for (int t = 4; t < 8; t++) c = mfma16(wop[(S::oWA2 + M * 8 + t) * 64], Xs[t - 4][0], c);
        }
#pragma unroll
        for (int T = 0; T < 4; T++) pre[T] = c;
#pragma unroll
        for (int t = 0; t < 4; t++) {
          const float a = wop[(S::oWA2 + M * 8 + t) * 64];
#pragma unroll
          for (int T = 0; T < 4; T++) pre[T] = mfma16(a, Xh[T][t], pre[T]);
        }
      } else {
#pragma unroll
        for (int T = 0; T < 4; T++)
          pre[T] = *reinterpret_cast<const f32x4 *>(lds_w + S::oB1 + 16 * M + 4 * q);
#pragma unroll
        for (int t = 0; t < 8; t++) {
          const float a = wop[(S::oWA2 + M * 8 + t) * 64];
#pragma unroll
          for (int T = 0; T < 4; T++)
            pre[T] = mfma16(a, (t < 4) ? Xh[T][t] : Xs[t - 4][T], pre[T]);
        }
      }
      if (!RAYS && pre_out) {
#pragma unroll
        for (int T = 0; T < 4; T++)
          if (vT[T]) {
#pragma unroll
            for (int r = 0; r < 4; r++)
              st_row(pre_out + (int64_t)(16 * M + r) * n, offS[T] + cP, pre[T][r]);
          }
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float a = wop[(S::oWA3 + M * 4 + r) * 64];
#pragma unroll
        for (int T = 0; T < 4; T++) o[T] = mfma16(a, relu(pre[T][r]), o[T]);
      }
    }
    if (q < 3) {
#pragma unroll
      for (int T = 0; T < 4; T++)
        if (vT[T])
          st_row(rgb + q, 3 * offS[T], (1.f + 2.f * kEps) / (1.f + expf(-o[T][0])) - kEps);
    }
  }
}

#define F2N_SHADE_FWD_PARAMS(DIRS, IMG)                                                               \
  const float * __restrict__ enc, const float * __restrict__ DIRS, const int32_t * __restrict__ IMG,  \
    const float * __restrict__ p_w_h, const float * __restrict__ p_b_h,                               \
    const float * __restrict__ p_w1, const float * __restrict__ p_b1,                                 \
    const float * __restrict__ p_w2, const float * __restrict__ p_b2,                                 \
    const float * __restrict__ p_emb, float * __restrict__ logit, float * __restrict__ rgb

template <int C, bool WIDE, int W>
__global__ __launch_bounds__(W * 64) void shade_fwd_mfma_kernel(
  F2N_SHADE_FWD_PARAMS(dirs, sample_img), float * __restrict__ pre_out, int64_t n)
{
  shade_fwd_mfma_body<C, WIDE, W, false>(
    enc, dirs, nullptr, sample_img, p_w_h, p_b_h, p_w1, p_b1, p_w2, p_b2, p_emb, logit, rgb, pre_out, n,
    0, 0);
}

// ray-uniform form: n = n_rays * S samples in ray-major order, S % 64 == 0, one image id per ray;
// dir_per_ray as in shade_bwd_mfma_rays_kernel
template <int C, bool WIDE, int W>
__global__ __launch_bounds__(W * 64) void shade_fwd_mfma_rays_kernel(
  F2N_SHADE_FWD_PARAMS(dirs, ray_img), int64_t n, int S, int dir_per_ray)
{
  shade_fwd_mfma_body<C, WIDE, W, true>(
    enc, dirs, nullptr, ray_img, p_w_h, p_b_h, p_w1, p_b1, p_w2, p_b2, p_emb, logit, rgb, nullptr, n,
    S, dir_per_ray);
}

// the ray-uniform form with the per-ray constant loaded: `ray_const` [n_rays, 80] in place of the
// directions
template <int C, bool WIDE, int W>
__global__ __launch_bounds__(W * 64) void shade_fwd_mfma_rays_kernel_const(
  F2N_SHADE_FWD_PARAMS(ray_const, ray_img), int64_t n, int S)
{
  shade_fwd_mfma_body<C, WIDE, W, true, true>(
    enc, nullptr, ray_const, ray_img, p_w_h, p_b_h, p_w1, p_b1, p_w2, p_b2, p_emb, logit, rgb,
    nullptr, n, S, 1);
}

// The per-ray constant: out[ray] = { c[64] = b1 + w1[:, 16:32] . SH16(dir), SH16(dir)[16] }.  One wave
// takes 16 rays as the 16 columns of the products the network kernels issue for one: lane (q, m)
// supplies b = SH row 4q + t' of ray m against the same a = w1[16M+m][16 + 4q + t'], k-steps t = 4..7
// in that order from b1[16M+4q+r].  A column of a product does not depend on its neighbours, so row
// `ray` holds the bits the in-kernel form gives every sample of the ray.  Lane (q, m) ends up with
// c[16M+4q+r] of ray m -- the 16 bytes lane (q, .) of a consumer loads per M -- and writes the four SH
// rows it supplied behind them.
__global__ __launch_bounds__(256) void shade_ray_const_kernel(
  const float * __restrict__ dirs, const float * __restrict__ p_w1, const float * __restrict__ p_b1,
  float * __restrict__ out, int n_rays)
{
  const int lane = lane_id(), q = lane >> 4, m = lane & 15;
  const int64_t ray = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16 + m;
  const int64_t rd = (ray < n_rays) ? ray : n_rays - 1;  // a partial tile reads a real ray
  float sh[16];
  sh_basis<4>(dirs[rd * 3], dirs[rd * 3 + 1], dirs[rd * 3 + 2], sh);
  f32x4 b;
#pragma unroll
  for (int t = 0; t < 4; t++) b[t] = pick4(q, sh[t], sh[4 + t], sh[8 + t], sh[12 + t]);
  float * row = out + ray * kRayConst;
#pragma unroll
  for (int M = 0; M < 4; M++) {
    f32x4 c;
#pragma unroll
    for (int r = 0; r < 4; r++) c[r] = p_b1[16 * M + 4 * q + r];
#pragma unroll
    for (int t = 4; t < 8; t++) c = mfma16(p_w1[(16 * M + m) * kIn2 + 16 + 4 * q + (t - 4)], b[t - 4], c);
    if (ray < n_rays) *reinterpret_cast<f32x4 *>(row + 16 * M + 4 * q) = c;
  }
  if (ray < n_rays) *reinterpret_cast<f32x4 *>(row + kHid + 4 * q) = b;
}
#undef F2N_SHADE_FWD_PARAMS

}  // namespace

namespace f2n_detail
{

// Below this many samples per launch the one-wave form is faster (few strides per wave; measured
// in NOTES.md section 6)
constexpr int64_t kShadeBwdTwoWavesMinSamples = F2N_SHADE_BWD_TWO_WAVES_MIN_SAMPLES;

bool shade_bwd_mfma_supports(int C, int64_t n)
{
  // (per-sample offsets such as 12 s for d_rgb stay 32-bit: n < 2^28; the row offsets C n 4 are
  // 32-bit below 2^30 elements and 64-bit, the WIDE kernels, above)
  return (C == 8 || C == 16 || C == 32 || C == 64) && n < ((int64_t)1 << 28);
}

// S = 0: the per-sample kernels (img = one id per sample); S > 0: the ray-uniform kernels
// (img = one id per ray, n = n_rays * S; dir_per_ray: dirs [n_rays, 3] instead of [n, 3]).  The same
// choice of form (TS, fences, WIDE) for both.  ray_const (with S > 0): the ray-uniform kernels that
// load the per-ray constant, instantiation for instantiation the set of the ones that form it.
static int launch_shade_bwd_mfma_any(
  const float * enc_cm, int C, const float * dirs, const float * ray_const, const int32_t * img,
  const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, const float * d_logit, const float * d_rgb, float * d_enc_cm,
  float * g_w_h, float * g_b_h, float * g_w1, float * g_b1, float * g_w2, float * g_b2,
  float * g_app_emb, int64_t n, int S, int dir_per_ray, hipStream_t stream)
{
  // the embedding rows are read as float4
  if (app_emb && (reinterpret_cast<uintptr_t>(app_emb) & 15u)) return F2N_E_INVALID_ARG;
  if (n >= ((int64_t)1 << 28)) return F2N_E_UNSUPPORTED;  // 32-bit per-sample offsets
  const bool wide = (int64_t)C * n >= ((int64_t)1 << 30);   // row offsets beyond 32 bits
  // form: 0 by size, 1 one wave per SIMD, 2 / 3 two waves (phase-fenced / phases mixed)
  const int waves = f2n_get_option(F2N_OPT_SHADE_BWD_WAVES);
  // (the ray-uniform form at C = 64 with 64-bit row offsets, 2^24 samples and more, spills four
  // registers at two waves per SIMD: those launches take its one-wave form, which does not)
  const bool rays_one_wave = S > 0 && wide && C == 64;
  const int ts =
    (waves == 1 || (waves == 0 && n < kShadeBwdTwoWavesMinSamples) || rays_one_wave) ? 4 : 2;
  // scheduling (V & 1: phases may mix).  One wave: mixed unless F2N_OPT_SHADE_VARIANT = 1, as in
  // round 3.  Two waves: fenced (1.30 against 1.33 ms per 8.2 M samples) unless SHADE_BWD_WAVES = 3;
  // the WIDE kernels are always fenced there (mixed, they spill).
  const bool mixed = (ts == 4) ? f2n_get_option(F2N_OPT_SHADE_VARIANT) != 1 : waves == 3;
#define F2N_LAUNCH_MFMA_V(CC, VV, WW, TT)                                                            \
  {                                                                                                  \
    using MS = MShape<CC, TT>;                                                                       \
    const int64_t n_strides = (n + MS::kStride - 1) / MS::kStride;                                   \
    const unsigned grid = (unsigned)std::min<int64_t>(256, (n_strides + MS::kWaves - 1) / MS::kWaves); \
    if (S > 0 && ray_const) {                                                                        \
      if constexpr (!(CC == 64 && WW && TT == 2)) /* rays_one_wave */                                \
        hipLaunchKernelGGL(                                                                          \
          (shade_bwd_mfma_rays_kernel_const<CC, VV, WW, TT>), dim3(grid), dim3(MS::kWaves * 64), 0,  \
          stream, enc_cm, ray_const, img, w_h, b_h, w1, b1, w2, b2, app_emb, d_logit, d_rgb,         \
          d_enc_cm, g_w_h, g_b_h, g_w1, g_b1, g_w2, g_b2, g_app_emb, n, S);                          \
    } else if (S > 0) {                                                                              \
      if constexpr (!(CC == 64 && WW && TT == 2)) /* rays_one_wave */                                \
        hipLaunchKernelGGL(                                                                          \
          (shade_bwd_mfma_rays_kernel<CC, VV, WW, TT>), dim3(grid), dim3(MS::kWaves * 64), 0,        \
          stream, enc_cm, dirs, img, w_h, b_h, w1, b1, w2, b2, app_emb, d_logit, d_rgb, d_enc_cm,    \
          g_w_h, g_b_h, g_w1, g_b1, g_w2, g_b2, g_app_emb, n, S, dir_per_ray);                       \
    } else                                                                                           \
      hipLaunchKernelGGL(                                                                            \
        (shade_bwd_mfma_kernel<CC, VV, WW, TT>), dim3(grid), dim3(MS::kWaves * 64), 0, stream,       \
        enc_cm, dirs, img, w_h, b_h, w1, b1, w2, b2, app_emb, d_logit, d_rgb, d_enc_cm, g_w_h,       \
        g_b_h, g_w1, g_b1, g_w2, g_b2, g_app_emb, n);                                                \
  }
#define F2N_LAUNCH_MFMA_T(CC, TT)                            \
  if (wide) F2N_LAUNCH_MFMA_V(CC, (TT == 2 ? 0 : 1), true, TT) \
  else if (mixed) F2N_LAUNCH_MFMA_V(CC, 1, false, TT)        \
  else F2N_LAUNCH_MFMA_V(CC, 0, false, TT)
#define F2N_LAUNCH_MFMA(CC)                                \
  if (ts == 2) { F2N_LAUNCH_MFMA_T(CC, 2) }                \
  else { F2N_LAUNCH_MFMA_T(CC, 4) }
  switch (C) {
    case 8: F2N_LAUNCH_MFMA(8) break;
    case 16: F2N_LAUNCH_MFMA(16) break;
    case 32: F2N_LAUNCH_MFMA(32) break;
    case 64: F2N_LAUNCH_MFMA(64) break;
    default: return F2N_E_UNSUPPORTED;
  }
#undef F2N_LAUNCH_MFMA
#undef F2N_LAUNCH_MFMA_T
#undef F2N_LAUNCH_MFMA_V
  return f2n_launch_status();
}

int launch_shade_bwd_mfma(
  const float * enc_cm, int C, const float * dirs, const int32_t * sample_img, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, const float * d_logit, const float * d_rgb, float * d_enc_cm,
  float * g_w_h, float * g_b_h, float * g_w1, float * g_b1, float * g_w2, float * g_b2,
  float * g_app_emb, int64_t n, hipStream_t stream)
{
  return launch_shade_bwd_mfma_any(
    enc_cm, C, dirs, nullptr, sample_img, w_h, b_h, w1, b1, w2, b2, app_emb, d_logit, d_rgb, d_enc_cm,
    g_w_h, g_b_h, g_w1, g_b1, g_w2, g_b2, g_app_emb, n, 0, 0, stream);
}

int launch_shade_bwd_mfma_rays(
  const float * enc_cm, int C, const float * dirs, const int32_t * ray_img, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, const float * d_logit, const float * d_rgb, float * d_enc_cm,
  float * g_w_h, float * g_b_h, float * g_w1, float * g_b1, float * g_w2, float * g_b2,
  float * g_app_emb, int n_rays, int S, bool dir_per_ray, hipStream_t stream)
{
  if (S <= 0 || S % 64 != 0 || n_rays <= 0) return F2N_E_INVALID_ARG;
  return launch_shade_bwd_mfma_any(
    enc_cm, C, dirs, nullptr, ray_img, w_h, b_h, w1, b1, w2, b2, app_emb, d_logit, d_rgb, d_enc_cm,
    g_w_h, g_b_h, g_w1, g_b1, g_w2, g_b2, g_app_emb, (int64_t)n_rays * S, S, dir_per_ray ? 1 : 0,
    stream);
}

int launch_shade_bwd_mfma_rays_const(
  const float * enc_cm, int C, const float * ray_const, const int32_t * ray_img, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, const float * d_logit, const float * d_rgb, float * d_enc_cm,
  float * g_w_h, float * g_b_h, float * g_w1, float * g_b1, float * g_w2, float * g_b2,
  float * g_app_emb, int n_rays, int S, hipStream_t stream)
{
  if (S <= 0 || S % 64 != 0 || n_rays <= 0 || !ray_const) return F2N_E_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(ray_const) & 15u) return F2N_E_INVALID_ARG;  // read as float4
  return launch_shade_bwd_mfma_any(
    enc_cm, C, nullptr, ray_const, ray_img, w_h, b_h, w1, b1, w2, b2, app_emb, d_logit, d_rgb,
    d_enc_cm, g_w_h, g_b_h, g_w1, g_b1, g_w2, g_b2, g_app_emb, (int64_t)n_rays * S, S, 1, stream);
}


// S = 0: the per-sample kernels; S > 0: the ray-uniform kernels (img per ray, no pre_cm)
static int launch_shade_fwd_mfma_any(
  const float * enc_cm, int C, const float * dirs, const float * ray_const, const int32_t * img,
  const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, float * logit, float * rgb, float * pre_cm, int64_t n, int S,
  int dir_per_ray, hipStream_t stream)
{
  const int64_t n_strides = (n + 63) / 64;
  if (app_emb && (reinterpret_cast<uintptr_t>(app_emb) & 15u)) return F2N_E_INVALID_ARG;
  if (n >= ((int64_t)1 << 28)) return F2N_E_UNSUPPORTED;  // 32-bit per-sample offsets
  const bool wide = (int64_t)(pre_cm ? 64 : C) * n >= ((int64_t)1 << 30);  // row offsets beyond 32 bits
  const bool two_per_simd = f2n_get_option(F2N_OPT_SHADE_VARIANT) == 2;
#define F2N_LAUNCH_FWD_W(CC, WW, KW)                                                               \
  {                                                                                                \
    constexpr int kW = KW;                                                                         \
    const unsigned grid = (unsigned)std::min<int64_t>(256, (n_strides + kW - 1) / kW);             \
    if (S > 0 && ray_const)                                                                        \
      hipLaunchKernelGGL(                                                                          \
        (shade_fwd_mfma_rays_kernel_const<CC, WW, KW>), dim3(grid), dim3(kW * 64), 0, stream,      \
        enc_cm, ray_const, img, w_h, b_h, w1, b1, w2, b2, app_emb, logit, rgb, n, S);              \
    else if (S > 0)                                                                                \
      hipLaunchKernelGGL(                                                                          \
        (shade_fwd_mfma_rays_kernel<CC, WW, KW>), dim3(grid), dim3(kW * 64), 0, stream, enc_cm,    \
        dirs, img, w_h, b_h, w1, b1, w2, b2, app_emb, logit, rgb, n, S, dir_per_ray);              \
    else                                                                                           \
      hipLaunchKernelGGL(                                                                          \
        (shade_fwd_mfma_kernel<CC, WW, KW>), dim3(grid), dim3(kW * 64), 0, stream, enc_cm, dirs,   \
        img, w_h, b_h, w1, b1, w2, b2, app_emb, logit, rgb, pre_cm, n);                            \
  }
#define F2N_LAUNCH_FWD(CC)                                                   \
  if (wide) F2N_LAUNCH_FWD_W(CC, true, 12)                                   \
  else if (two_per_simd) F2N_LAUNCH_FWD_W(CC, false, 8)                      \
  else if (f2n_get_option(F2N_OPT_SHADE_VARIANT) == 3) F2N_LAUNCH_FWD_W(CC, false, 12) \
  else F2N_LAUNCH_FWD_W(CC, false, 16)
  switch (C) {
    case 8: F2N_LAUNCH_FWD(8) break;
    case 16: F2N_LAUNCH_FWD(16) break;
    case 32: F2N_LAUNCH_FWD(32) break;
    case 64: F2N_LAUNCH_FWD(64) break;
    default: return F2N_E_UNSUPPORTED;
  }
#undef F2N_LAUNCH_FWD
#undef F2N_LAUNCH_FWD_W
  return f2n_launch_status();
}

int launch_shade_fwd_mfma(
  const float * enc_cm, int C, const float * dirs, const int32_t * sample_img, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, float * logit, float * rgb, float * pre_cm, int64_t n, hipStream_t stream)
{
  return launch_shade_fwd_mfma_any(
    enc_cm, C, dirs, nullptr, sample_img, w_h, b_h, w1, b1, w2, b2, app_emb, logit, rgb, pre_cm, n, 0,
    0, stream);
}

int launch_shade_fwd_mfma_rays(
  const float * enc_cm, int C, const float * dirs, const int32_t * ray_img, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, float * logit, float * rgb, int n_rays, int S, bool dir_per_ray,
  hipStream_t stream)
{
  if (S <= 0 || S % 64 != 0 || n_rays <= 0) return F2N_E_INVALID_ARG;
  return launch_shade_fwd_mfma_any(
    enc_cm, C, dirs, nullptr, ray_img, w_h, b_h, w1, b1, w2, b2, app_emb, logit, rgb, nullptr,
    (int64_t)n_rays * S, S, dir_per_ray ? 1 : 0, stream);
}

int launch_shade_fwd_mfma_rays_const(
  const float * enc_cm, int C, const float * ray_const, const int32_t * ray_img, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, float * logit, float * rgb, int n_rays, int S, hipStream_t stream)
{
  if (S <= 0 || S % 64 != 0 || n_rays <= 0 || !ray_const) return F2N_E_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(ray_const) & 15u) return F2N_E_INVALID_ARG;  // read as float4
  return launch_shade_fwd_mfma_any(
    enc_cm, C, nullptr, ray_const, ray_img, w_h, b_h, w1, b1, w2, b2, app_emb, logit, rgb, nullptr,
    (int64_t)n_rays * S, S, 1, stream);
}

int launch_shade_ray_const(
  const float * ray_dirs, const float * w1, const float * b1, float * ray_const, int n_rays,
  hipStream_t stream)
{
  if (n_rays <= 0 || !ray_dirs || !w1 || !b1 || !ray_const) return F2N_E_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(ray_const) & 15u) return F2N_E_INVALID_ARG;  // written as float4
  const unsigned grid = (unsigned)(((int64_t)n_rays + 63) / 64);  // 4 waves of 16 rays per workgroup
  hipLaunchKernelGGL(
    shade_ray_const_kernel, dim3(grid), dim3(256), 0, stream, ray_dirs, w1, b1, ray_const, n_rays);
  return f2n_launch_status();
}

}  // namespace f2n_detail
