/*
 * f2nerf_hip.h -- C ABI of libf2nerf_hip.so: the MI355X (gfx950) kernels behind the F2-NeRF
 * rendering hot path (hash-grid encode, ray sampling / early termination, SH encode, ragged per-ray
 * compositing; forward and backward).
 *
 * This is the drop-in boundary.  Every entry point replaces one CUDA kernel launch site (or one
 * run of ATen launches) of SakodaShintaro/f2-nerf; the reference interface each one stands in for
 * is cited as file:line (relative to the reference checkout).  INTEGRATION.md shows the LibTorch
 * wrappers that bind them.
 *
 * Conventions (inherited from the reference's launch sites):
 *   - all pointers are DEVICE pointers to contiguous, caller-owned, caller-allocated buffers;
 *   - no entry point allocates, frees, synchronises or keeps state between calls (calls arrive
 *     from the forward thread and from the autograd engine's device thread); the one exception is
 *     the explicit, process-wide kernel-route table of f2n_set_option below (atomics; defaults =
 *     the production routes; nothing is read from the environment);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *   - return value: F2N_OK (0) or a negative F2N_E_* code; nothing throws;
 *   - counts are elements, never bytes; `idx`/`bounds` are [n_rays, 2] int32 {start, end}.
 */
#ifndef F2NERF_HIP_H_
#define F2NERF_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: f2n_set_option / f2n_get_option (explicit process-wide route table; nothing is read from the
 *    environment any more), f2n_density_margin, f2n_hash_bwd_set_overflow_counter; f2n_hash_bwd_binned
 *    returns F2N_E_UNSUPPORTED for a workspace that cannot hold one tile and applies to n >= 65536. */
#define F2N_ABI_VERSION 2

#define F2N_OK 0
#define F2N_E_INVALID_ARG (-1) /* null pointer, negative count, unsupported L/F/degree ...     */
#define F2N_E_LAUNCH (-2)      /* hipGetLastError() != hipSuccess right after the launch        */
#define F2N_E_UNSUPPORTED (-3) /* valid request the build does not cover (e.g. F not in 1,2,4,8) */

#define F2N_MAX_LEVELS 32

int f2n_abi_version(void);
const char * f2n_status_string(int status);

/* Kernel-route switches for A/B measurements and for tests that must cover every route.  They
 * select between implementations of the SAME operation (results agree within the documented bars);
 * value 0 is always the production default.  Process-wide, lock-free (relaxed atomics): safe to
 * call while other threads launch, takes effect for launches issued afterwards.
 * f2n_set_option returns the previous value, or F2N_E_INVALID_ARG for an unknown key / value. */
#define F2N_OPT_SHADE_FWD 0     /* 0 matrix-core forward, 1 one-sample-per-lane vector kernel       */
#define F2N_OPT_SHADE_BWD 1     /* 0 matrix-core backward, 1 vector (VALU + LDS) backward           */
#define F2N_OPT_SHADE_VARIANT 2 /* matrix-core backward at one wave per SIMD: 0 phases may overlap, 1
                                  phase-fenced (the two-wave form: F2N_OPT_SHADE_BWD_WAVES); the
                                  matrix-core FORWARD: 0 four waves per SIMD, 3 three, 2 two          */
#define F2N_OPT_RAYTILE 3       /* f2n_hash_fwd_raytile: 0 a workgroup takes its ray tile (32 samples,
                                  16 unless S % 32 == 0) through a group of levels
                                  (f2n_hash_raytile_default_groups); 16, 32: one level per
                                  workgroup, tiles of that many samples; same bits                */
#define F2N_OPT_HASH_BWD 4      /* f2n_hash_bwd route: 0 auto, 1 global atomics, 2 LDS-sliced       */
#define F2N_OPT_BWD_COMBINE 5   /* binned backward: 0 combine coarse levels per tile, 1 never       */
#define F2N_OPT_RAYTILE_WALK 6  /* lanes of f2n_hash_fwd_raytile: 0 chosen per tile, 1 across rays at one
                                   sample index, 2 along a ray, 3 across rays in depth order        */
#define F2N_OPT_MARCH 7         /* f2n_density_march: 0 eight rays per wavefront in strides of 8 samples,
                                  1 one ray per wavefront in strides of 64 (round 2), 2 four rays in
                                  strides of 16; same counts                                          */
#define F2N_OPT_BWD_PHASES 8    /* binned backward, overlapping level windows (level_stride < T*F): 0 the
                                  slices of levels that share elements add with float atomics, 1 the
                                  reduce pass runs in ceil(T*F / level_stride) launches of levels that
                                  do not overlap: bit-reproducible also when accumulating into an
                                  existing gradient, 4-25 % slower                                   */
#define F2N_OPT_RAY_ORDER 9     /* Renderer dense first pass: 0 rays bucketed into pixel-compact bundles
                                  (f2n_ray_keys) and results handed back in caller order, 1 rays
                                  rendered in the caller's order; same results bit for bit          */
#define F2N_OPT_SHADE_BWD_WAVES 10 /* matrix-core backward: 0 chosen by size (two waves per SIMD in
                                  32-sample strides from F2N_SHADE_BWD_TWO_WAVES_MIN_SAMPLES samples
                                  per launch, one below), 1 one wave per SIMD in 64-sample strides
                                  (round 3), 2 two waves per SIMD, 3 two waves with the phases of a
                                  stride mixed (not fenced; WIDE kernels stay fenced); same d_enc bit
                                  for bit, parameter gradients within the order of float sums       */
#define F2N_SHADE_BWD_TWO_WAVES_MIN_SAMPLES (3 << 19)
#define F2N_OPT_SHADE_RAYS 11   /* Renderer, fused per-sample network on a dense [n_rays, S] grid of
                                  samples with S % 64 == 0: 0 the ray-uniform kernels
                                  (f2n_shade_fwd_rays / f2n_shade_bwd_rays), 1 always the per-sample
                                  kernels; same logit bit for bit, everything else within rounding    */
#define F2N_OPT_DENSE_LEAN 12   /* Renderer, dense first pass with the ray-uniform network kernels and
                                  no gradient into rays or bg_color: 0 one sampler kernel writes the
                                  contracted positions and one direction per ray (f2n_sample_dense,
                                  f2n_shade_*_raydirs; no world positions, no per-sample directions,
                                  the noise read raw and in place), train_step takes the weight
                                  variance in bucketed order and undefined gradients are not
                                  materialised as zeros; 1 f2n_sample_rays + f2n_contract_fwd and the
                                  per-sample arrays; same results bit for bit (network parameter
                                  gradients: within the order of their float atomics)               */
#define F2N_OPT_COUNT 13
/* Keys 0 .. F2N_OPT_COUNT - 1 are the first table, closed with ABI 2: key 13 stays rejected.  Options
 * added since are numbered from F2N_OPT2_FIRST, F2N_OPT2_COUNT of them; same calls, same rules. */
#define F2N_OPT2_FIRST 64
#define F2N_OPT_GATHER_PAIRED (F2N_OPT2_FIRST + 0)
                                /* the order of a sample's 8 corner loads in f2n_hash_fwd_raytile and in
                                  the density chain of the march and the one-pass render (f2n_density_march,
                                  _march_occ, f2n_render_rays, _head, _tail): 0 by vertex parity (load j
                                  fetches the vertex of the lane's cell whose coordinate parities are j,
                                  so lanes in neighbouring cells ask for a shared vertex in the same
                                  load), 1 by corner (load d fetches corner d of the lane's own cell);
                                  the same rows, the same sum, the same bits                         */
#define F2N_OPT2_COUNT 1
int f2n_set_option(int key, int value);
int f2n_get_option(int key);

/* ------------------------------------------------------------------ hash grid (rows A1, A2) --- */

/* feat_pool.to(torch::kFloat16) -- src/hash_3d_anchored.cu:169,198.  RNE cast of n elements. */
int f2n_table_to_f16(const float * table_f32, uint16_t * table_f16, int64_t n, void * stream);

/* Hash3DAnchoredForwardKernel<__half><<<(ceil(n/512), L), 512>>> + out.to(kFloat32)
 * -- src/hash_3d_anchored.cu:60-93,164-178.
 *   pts        [n,3] f32, already contracted
 *   table_f16  f16 pool; level l starts at element level_stride*l (reference: level_stride = T,
 *              quirk Q2), rows of F channels, row index = hash % T
 *   primes     [L,3] i32; bias [L,3] f32; mul [L] f32 (host table, see f2n_level_mul in the host lib)
 *   out        f32 holding the f16-rounded feature; element (p, c) at out[p*out_ld_point + c*out_ld_chan],
 *              c = l*F + k.  Reference layout: out_ld_point = L*F, out_ld_chan = 1.
 *   idx_out    optional [n, L, 8] u32 hash rows (parity tests); NULL in production. */
int f2n_hash_fwd(
  const float * pts, const uint16_t * table_f16, const int32_t * primes, const float * bias,
  const float * mul, float * out, int64_t out_ld_point, int64_t out_ld_chan, uint32_t * idx_out,
  int64_t n, int L, int F, uint32_t T, int64_t level_stride, void * stream);

/* f2n_hash_fwd for a DENSE sample grid: pts [n_rays, S, 3] ray-major as f2n_sample_rays writes it
 * (the input of the first field evaluation, src/renderer.cpp:61), out_cm channel-major
 * [L*F, n_rays*S] (element (p, c) at out_cm[c*n + p], 16-byte aligned).  Same arithmetic, same
 * results; the lanes of a wavefront walk neighbouring RAYS at one sample index instead of
 * consecutive samples of one ray, so image-ordered ray batches (src/renderer.cpp render of a whole
 * view, src/main_functions/train_manager.cpp:170-190) share gathered table lines.
 * F2N_E_UNSUPPORTED unless S is a multiple of 16: call f2n_hash_fwd instead. */
int f2n_hash_fwd_raytile(
  const float * pts, const uint16_t * table_f16, const int32_t * primes, const float * bias,
  const float * mul, float * out_cm, int n_rays, int S, int L, int F, uint32_t T,
  int64_t level_stride, void * stream);

/* f2n_hash_fwd_raytile with the schedule of its levels spelled out (Hash3DAnchoredForwardKernel,
 * src/hash_3d_anchored.cu:60-93, evaluates one level per block; so does F2N_OPT_RAYTILE = 16 | 32).
 * One workgroup takes a tile of 64 rays x 32 samples (16 unless S is a multiple of 32) through a
 * GROUP of consecutive levels: the tile's points, its walk and its depth order are set up once per
 * group.
 * Bit l of group_starts set: level l opens a group; bit 0 is implied.  Same arguments, same results
 * bit for bit under every mask.  A bit at or above L: F2N_E_INVALID_ARG; L > 32: F2N_E_UNSUPPORTED;
 * both, and every check of f2n_hash_fwd_raytile, before any HIP work. */
int f2n_hash_fwd_raytile_groups(
  const float * pts, const uint16_t * table_f16, const int32_t * primes, const float * bias,
  const float * mul, float * out_cm, int n_rays, int S, int L, int F, uint32_t T,
  int64_t level_stride, uint32_t group_starts, void * stream);

/* The group_starts that f2n_hash_fwd_raytile uses under F2N_OPT_RAYTILE = 0 for L levels and a grid
 * of `tiles` tiles (ceil(n_rays / 64) * S / 32, or S / 16 unless S is a multiple of 32).  No
 * counterpart in the reference, whose Hash3DAnchoredForwardKernel (src/hash_3d_anchored.cu:60-93)
 * has one level per block and nothing to schedule; exported so that a caller, a measurement or a
 * test can name the default without a GPU.  From a level's position l / (L - 1):
 *   tiles >= 1024  the levels below 2/3 form one group, the levels from 2/3 on go two to a group,
 *                  counted from the first of them (L = 16: 0-9, 10-11, 12-13, 14-15 = 0x5401);
 *   tiles < 1024   the levels below 2/5 form one group, those from 2/5 to below 2/3 a second, every
 *                  level from 2/3 on its own (L = 16: 0-5, 6-9, 10, 11, ... 15 = 0xfc41).
 * L = 1: 1; L = 2: 3.  Host arithmetic, no HIP work.  Returns the mask, a value in [1, 2^32), or a
 * negative status: F2N_E_INVALID_ARG for L < 1 or tiles < 0, F2N_E_UNSUPPORTED for L > 32. */
int64_t f2n_hash_raytile_default_groups(int L, int64_t tiles);

/* Hash3DAnchoredBackwardKernel<__half> + the /grad_scale epilogue
 * -- src/hash_3d_anchored.cu:95-145,190-215.
 *   grad_out    element (p, c) at grad_out[p*g_ld_point + c*g_ld_chan], f32
 *   table_grad  f32, same element indexing as table_f16, ACCUMULATED INTO (caller zeroes it):
 *               += f16(f16(grad_scale*g) * w_d) / grad_scale per corner.  The reference accumulates
 *               with order-dependent f16 atomics; here the sum is kept in f32 (documented in
 *               DESIGN.md).  grad_scale must be a power of two (reference: 128).
 *   pts_grad    [n,3] f32 or NULL (NULL = points need no gradient: the training case).  Overwritten. */
int f2n_hash_bwd(
  const float * pts, const uint16_t * table_f16, const int32_t * primes, const float * bias,
  const float * mul, const float * grad_out, int64_t g_ld_point, int64_t g_ld_chan,
  float * table_grad, float * pts_grad, int64_t n, int L, int F, uint32_t T, int64_t level_stride,
  float grad_scale, void * stream);

/* Same operation as f2n_hash_bwd without the point gradient, for large batches: contributions are
 * binned by table slice into a caller-provided workspace and summed EXACTLY (64-bit fixed point) in
 * LDS, so the scattered f16/f32 atomics of Hash3DAnchoredBackwardKernel
 * (src/hash_3d_anchored.cu:129-137) disappear and the result does not depend on summation order --
 * with one condition: a record that finds an LDS queue, a workspace region or a run full, or that
 * holds a non-finite half, is applied directly with a global float atomic, and where two such
 * records meet on one element the last bits depend on their order (as the reference's own atomics
 * do everywhere).  f2n_hash_bwd_set_overflow_counter() makes the passes count those records.
 * Tables with more than 64 LDS-sized slices per level (T*F > 2^20, e.g. T = 2^22, F = 8) take a
 * second binning pass; coarse levels whose cells are shared by the points of a tile are combined
 * before they are binned (F2N_OPT_BWD_COMBINE).
 * f2n_hash_bwd_workspace_bytes returns the recommended workspace size (at most 64 GiB), or 0 when
 * the binned path does not apply to (n, L, F, T): n < 65536 or T*F > 2^26 -- use f2n_hash_bwd then.
 * workspace: device memory, 256-byte aligned, contents undefined on entry and exit.  A smaller
 * workspace makes the passes run in several rounds over the points (same results);
 * F2N_E_UNSUPPORTED when it cannot hold one 1024-point tile. */
int64_t f2n_hash_bwd_workspace_bytes(int64_t n, int L, int F, uint32_t T);
/* Overflow accounting of f2n_hash_bwd_binned (process-wide, like f2n_set_option): a caller-owned
 * device word (8-byte aligned) that every later call increments once per record it applied with a
 * global float atomic instead of the exact sum (a full queue / region / run, a combined sum beyond
 * the f16 range) -- 0 afterwards means the result is independent of summation order, bit for bit.
 * NULL (the default) switches the counting off.  The reference's kernel has no such distinction:
 * every one of its adds is an order-dependent atomic (src/hash_3d_anchored.cu:129-137). */
int f2n_hash_bwd_set_overflow_counter(uint64_t * device_counter);
int f2n_hash_bwd_binned(
  const float * pts, const int32_t * primes, const float * bias, const float * mul,
  const float * grad_out, int64_t g_ld_point, int64_t g_ld_chan, float * table_grad, int64_t n,
  int L, int F, uint32_t T, int64_t level_stride, float grad_scale, void * workspace,
  int64_t workspace_bytes, void * stream);

/* Scene contraction of Hash3DAnchored::query -- src/hash_3d_anchored.cpp:79-82 (8 ATen launches):
 *   x = p if |p| <= 1 else (2 - 1/|p|) * p/|p|, evaluated as the reference's mask expression
 *   (|p| == 0 gives NaN, quirk Q6).  The backward is the Jacobian-vector product autograd builds. */
int f2n_contract_fwd(const float * pts, float * x, int64_t n, void * stream);
int f2n_contract_bwd(const float * pts, const float * dx, float * dpts, int64_t n, void * stream);

/* Gradient of the rays from the gradient of their samples' encoding, for rays that carry one (pose
 * optimisation, src/localizer.cpp:142-167): the point gradient of Hash3DAnchoredBackwardKernel
 * (quirk Q5, src/hash_3d_anchored.cu:138-143, same per-term f16 roundings as f2n_hash_bwd), the
 * contraction's backward (f2n_contract_bwd) and the backward of pts = o + t d/|d|
 * (src/points_sampler.cpp:24,44), summed per ray -- one launch, no table gradient, no atomics, the
 * same bits on every run.
 *   pts        [n,3] f32 RAW (uncontracted) positions of the kept samples, t [n] their depths
 *   bounds     [n_rays, 2] segment of each ray in pts / t / grad_out
 *   rays_d     [n_rays, 3] the ray directions as given to the sampler (not normalised)
 *   table_f16 .. level_stride, grad_scale: as f2n_hash_bwd; grad_out element (p, c) at
 *              grad_out[p*g_ld_point + c*g_ld_chan]
 *   d_rays_o, d_rays_d [n_rays, 3] overwritten; a ray with an empty segment gets zeros.
 * Not formed, as in the reference: the path through dt = |pts_k - pts_k-1| (quirk Q7; it depends on
 * d only through |d/|d||, which the normalisation's Jacobian annihilates) and a gradient through the
 * SH directions (src/sh_shader.cu:105-115 has no backward for them). */
int f2n_hash_rays_grad(
  const float * pts, const float * t, const int32_t * bounds, const float * rays_d,
  const uint16_t * table_f16, const int32_t * primes, const float * bias, const float * mul,
  const float * grad_out, int64_t g_ld_point, int64_t g_ld_chan, float * d_rays_o,
  float * d_rays_d, int n_rays, int L, int F, uint32_t T, int64_t level_stride, float grad_scale,
  void * stream);

/* The encoding's true derivative with respect to position, as a vector-Jacobian product with the
 * gradient of the encoding: the trilinear interpolant of Hash3DAnchoredForwardKernel
 * (src/hash_3d_anchored.cu:25-93), enc[p, lF+k] = sum_d w_d(frac_l) f_{l,d,k}, differentiated in f32
 * with all three axes' interpolation weights,
 *   pts_grad[p] = sum_l mul_l sum_pairs (s_hi - s_lo) w_pair,  s_d = sum_k g[p, lF+k] f_{l,d,k},
 * in the evaluation order of f2n_density_grad (the same device function, with the sample's own
 * g[p, lF .. lF+F) where that entry takes w0; g is read as unscaled f32: no f16 rounding, no
 * grad_scale).  This is NOT quirk Q5: it replaces the form of src/hash_3d_anchored.cu:138-143 (the
 * corner features signed by the corner bit, the other two axes' weights missing, every term rounded
 * to f16), which f2n_hash_bwd's pts_grad keeps, for callers that ask for the derivative itself.  The
 * magnitude differs: Q5 is about 4 times the derivative taken at the centre of the other two axes.
 *   pts        [n,3] f32, ALREADY CONTRACTED, as f2n_hash_bwd takes it
 *   table_f16 .. level_stride: as f2n_hash_bwd; grad_out element (p, c) at
 *              grad_out[p*g_ld_point + c*g_ld_chan], f32
 *   pts_grad   [n,3] f32, overwritten: the levels' terms in level order, the first onto 0.  No
 *              contraction Jacobian: f2n_contract_bwd follows, as it follows f2n_hash_bwd.
 * One lane per point, no atomics, no workspace, the same bits on every run; n == 0 is F2N_OK without
 * a launch. */
int f2n_hash_pts_grad_exact(
  const float * pts, const uint16_t * table_f16, const int32_t * primes, const float * bias,
  const float * mul, const float * grad_out, int64_t g_ld_point, int64_t g_ld_chan,
  float * pts_grad, int64_t n, int L, int F, uint32_t T, int64_t level_stride, void * stream);

/* f2n_hash_rays_grad with the encoding's true derivative: per kept sample the vector
 * f2n_hash_pts_grad_exact forms (the interpolant of src/hash_3d_anchored.cu:25-93 differentiated with
 * all three axes' weights, f2n_density_grad's evaluation order, g unscaled f32), then, exactly as in
 * f2n_hash_rays_grad, the contraction's Jacobian at the raw point (NaN at |p| == 0), d o += dp,
 * m = fmaf(t, dp, m), the wave sums and d d = (m - n (n.m)) / |d|.  This is NOT quirk Q5: it
 * replaces the form of src/hash_3d_anchored.cu:138-143 that f2n_hash_rays_grad keeps.  Arguments as
 * f2n_hash_rays_grad, without grad_scale (pts RAW).  d_rays_o, d_rays_d [n_rays, 3] overwritten; a
 * ray with an empty segment gets zeros, a non-finite sample poisons its own ray only.  Still not
 * formed: the path through dt (quirk Q7), a gradient through the SH directions
 * (src/sh_shader.cu:105-115) and a gradient to t.
 * One wavefront per ray, one launch, no atomics, no workspace, the same bits on every run;
 * n_rays == 0 is F2N_OK without a launch. */
int f2n_hash_rays_grad_exact(
  const float * pts, const float * t, const int32_t * bounds, const float * rays_d,
  const uint16_t * table_f16, const int32_t * primes, const float * bias, const float * mul,
  const float * grad_out, int64_t g_ld_point, int64_t g_ld_chan, float * d_rays_o,
  float * d_rays_d, int n_rays, int L, int F, uint32_t T, int64_t level_stride, void * stream);

/* The density logit's spatial gradient: d(logit)/d(p) of the trilinear interpolant the forward
 * computes (src/hash_3d_anchored.cu:25-93 behind the contraction of src/hash_3d_anchored.cpp:79-82)
 * followed by row 0 of the field head,
 *   logit(p) = b0 + sum_l sum_k w0[l F + k] sum_d w_d(frac_l) f_{l,d,k},
 * the march's density chain without the per-channel f16 rounding of the blend, differentiated in f32
 * per level with all three axes' interpolation weights and taken through the contraction's Jacobian
 * to the raw point.  It is NOT what src/hash_3d_anchored.cu:138-143 computes (quirk Q5: the corner
 * features signed by the corner bit, without the other two axes' weights), which f2n_hash_bwd's
 * pts_grad and f2n_hash_rays_grad reproduce.
 *   pts        [n,3] f32 RAW (uncontracted) positions; |p| == 0 yields NaN for that point only
 *   table_f16 .. level_stride: as f2n_hash_fwd; L <= F2N_MAX_LEVELS (F2N_E_UNSUPPORTED above)
 *   w0         [L*F] f32, row 0 of the field head; its bias does not enter
 *   grad       [n,3] f32, overwritten
 * One lane per point, no atomics; n == 0 is F2N_OK without a launch. */
int f2n_density_grad(
  const float * pts, const uint16_t * table_f16, const int32_t * primes, const float * bias,
  const float * mul, const float * w0, float * grad, int64_t n, int L, int F, uint32_t T,
  int64_t level_stride, void * stream);

/* Per-ray normals N_r = sum_k w_k n^_k over the ray's kept samples, n^ = -g/|g| with g the
 * gradient f2n_density_grad forms (same device function: the interpolant of
 * src/hash_3d_anchored.cu:25-93 behind src/hash_3d_anchored.cpp:79-82, NOT the Q5 vector of
 * src/hash_3d_anchored.cu:138-143); n^ = 0 where g is zero in all three components.  Not
 * renormalised: |N_r| is at most the ray's opacity and the background contributes nothing.
 *   pts        [n,3] f32 RAW positions of the kept samples, weights [n] their compositing weights
 *   bounds     [n_rays, 2] segment of each ray in pts / weights
 *   table_f16 .. level_stride, w0: as f2n_density_grad
 *   normals    [n_rays, 3] f32, every element written; a ray with an empty segment gets zeros, a
 *              non-finite sample poisons its own ray only.
 * One wavefront per ray, one launch, no atomics, the same bits on every run. */
int f2n_ray_normals(
  const float * pts, const int32_t * bounds, const float * weights, const uint16_t * table_f16,
  const int32_t * primes, const float * bias, const float * mul, const float * w0,
  float * normals, int n_rays, int L, int F, uint32_t T, int64_t level_stride, void * stream);

/* The density logit on the vertices of an axis-aligned lattice in RAW world space, no point array in
 * and no encoding out: the evaluation the early-stop pass applies to its samples
 * (src/renderer.cpp:61-62 through the contraction of src/hash_3d_anchored.cpp:79-82), which the
 * reference itself never runs off a ray.  Vertex (ix, iy, iz) sits at p = fmaf((float)i, step, lo) per
 * axis; its value is f2n_density_march's logit bit for bit: the contraction of f2n_contract_fwd, the
 * gather and per-channel f16 rounding of f2n_hash_fwd, logit = fmaf(enc_c, w0[c], logit) in level
 * order from b0.  density_shift is NOT subtracted (a caller folds it into its level).
 *   table_f16 .. level_stride: as f2n_hash_fwd; L <= F2N_MAX_LEVELS (F2N_E_UNSUPPORTED above)
 *   w0 [L*F], b0 [1]: as f2n_density_march
 *   lo, step   f32 per axis, every step > 0
 *   nx, ny, nz each >= 2, nx*ny*nz < 2^31
 *   logit      [nz, ny, nx] f32, x fastest, every element written; a vertex at |p| == 0 yields NaN
 *              (quirk Q6) for itself only.
 * One lane per vertex, a wavefront is a 4x4x4 brick of vertices; one launch per group of consecutive
 * levels whose part of the table fits half an L2 (one launch for a small table), each continuing the
 * chain from the logit the one before it stored: the same chain and the same bits however the levels
 * are grouped.  No atomics. */
int f2n_density_lattice(
  const uint16_t * table_f16, const int32_t * primes, const float * bias, const float * mul,
  const float * w0, const float * b0, float * logit, float lo_x, float lo_y, float lo_z,
  float step_x, float step_y, float step_z, int nx, int ny, int nz, int L, int F, uint32_t T,
  int64_t level_stride, void * stream);

/* ------------------------------------------------------------------ mesh extraction ----------- */

/* Marching tetrahedra on a scalar lattice.  The reference has no mesher: its geometry is per ray
 * (src/renderer.cpp:58-90); these two entries are independent of the field and are applied to
 * f2n_density_lattice's logits of the density of src/hash_3d_anchored.cpp:79-86.
 *   values     [nz, ny, nx] f32, x fastest; vertex (x, y, z) has lattice index (z ny + y) nx + x and
 *              is inside iff value > level (NaN is outside); nx, ny, nz >= 2, nx*ny*nz < 2^31
 * Every cell is six Kuhn tetrahedra around its body diagonal, so every tetrahedron edge runs from a
 * vertex a to a + d, d = dx + 2 dy + 4 dz in 1..7, and a owns it.  An owned edge whose ends differ
 * carries one mesh vertex.  The orders (vertices by (owner, d), triangles by (cell, tetrahedron,
 * triangle)), the tetrahedra, the triangles of each case and their winding -- (b - a) x (c - a)
 * points from the inside corners to the outside ones -- are stated in mesh.hip's header comment.
 * f2n_mesh_count writes, per lattice vertex,
 *   mask   [n] u8  bit d - 1: the owned edge d crosses
 *   vcount [n] u8  popcount(mask), tcount [n] u8  triangles of the cell at this vertex (at most 12). */
int f2n_mesh_count(
  const float * values, uint8_t * mask, uint8_t * vcount, uint8_t * tcount, int nx, int ny, int nz,
  float level, void * stream);

/* f2n_mesh_emit writes the mesh, given f2n_mesh_count's mask of the same values and level (no
 * reference counterpart either; the field is that of src/hash_3d_anchored.cpp:79-86):
 *   voff, toff [n] i64  EXCLUSIVE prefix sums of vcount and tcount
 *   n_vertices, n_triangles  their totals; at or above 2^31 (3 n_triangles for the latter):
 *              F2N_E_UNSUPPORTED; both 0: F2N_OK without a launch; one of them 0: F2N_E_INVALID_ARG
 *   vertices   [n_vertices, 3] f32: on the edge a -> b = a + d, t = (level - s_a) / (s_b - s_a),
 *              t = 0.5 if !(t >= 0 && t <= 1), p = fmaf(t, p_b - p_a, p_a) per axis with
 *              p = fmaf((float)i, step, lo)
 *   triangles  [n_triangles, 3] i32 indices into vertices
 * Every store is checked against the totals: inputs that do not belong together skip stores and never
 * write outside the two arrays.  No atomics, the same bits on every run. */
int f2n_mesh_emit(
  const float * values, const uint8_t * mask, const int64_t * voff, const int64_t * toff,
  float * vertices, int32_t * triangles, int64_t n_vertices, int64_t n_triangles, float lo_x,
  float lo_y, float lo_z, float step_x, float step_y, float step_z, float level, int nx, int ny,
  int nz, void * stream);

/* ------------------------------------------------------------------ SH encode (row A6) -------- */

/* SHKernel<<<ceil(n/512), 512>>> -- src/sh_shader.cu:11-115.  dirs [n,3] -> out [n, degree^2],
 * degree 1..8 (F2N_E_UNSUPPORTED above); out 16-byte aligned. */
int f2n_sh_encode(const float * dirs, float * out, int64_t n, int degree, void * stream);

/* ------------------------------------------------------------------ ragged per-ray ops (A7) --- */

/* FlexSumForwardKernel / BackwardKernel -- src/CustomOps/FlexOps.cu:6-27,98-153 */
int f2n_seg_sum_fwd(const float * val, const int32_t * idx, float * sum, int n_rays, void * stream);
int f2n_seg_sum_bwd(const float * dsum, const int32_t * idx, float * dval, int n_rays, void * stream);
/* FlexSumVecForwardKernel / BackwardKernel -- src/CustomOps/FlexOps.cu:29-54 */
int f2n_seg_sum_vec_fwd(
  const float * val, const int32_t * idx, float * sum, int n_rays, int vec, void * stream);
int f2n_seg_sum_vec_bwd(
  const float * dsum, const int32_t * idx, float * dval, int n_rays, int vec, void * stream);
/* FlexAccumulateSumForwardKernel / BackwardKernel -- src/CustomOps/FlexOps.cu:56-94,155-199 */
int f2n_seg_scan_fwd(
  const float * val, const int32_t * idx, float * sum, int n_rays, int include_this, void * stream);
int f2n_seg_scan_bwd(
  const float * dsum, const int32_t * idx, float * dval, int n_rays, int include_this,
  void * stream);

/* WeightVarLossForwardKernel / BackwardKernel -- src/CustomOps/CustomOps.cu:13-67 (row A10) */
int f2n_weight_var_fwd(
  const float * weights, const int32_t * idx, float * out_vars, int n_rays, void * stream);
int f2n_weight_var_bwd(
  const float * weights, const int32_t * idx, const float * dvars, float * dw, int n_rays,
  void * stream);

/* The interval distortion loss of mip-NeRF 360 (eq. 15) per ray.  The reference has NO such kernel:
 * these stand beside its one weight regulariser, WeightVarLoss*Kernel (src/CustomOps/CustomOps.cu:13-67),
 * and are used where it is used (src/main_functions/train_manager.cpp:80-93).  WeightVar measures the
 * spread of the weights in sample INDEX (x_i = i/16); with an occupancy grid or jittered steps list
 * neighbours are no longer equally far apart, and this term works on the samples' real positions.
 *   weights, t, dt [n] f32: compositing weight, interval END (the raw t, without compositing's
 *   t_shift) and interval width of every kept sample; midpoint m_k = t_k - dt_k / 2.
 * For ray r with kept samples [s, e) = idx[r]:
 *     D_r       = sum_i sum_j w_i w_j |m_i - m_j|  +  1/3 sum_i w_i^2 dt_i       (i, j in [s, e))
 *     dD_r/dw_i = 2 sum_j w_j |m_i - m_j|  +  2/3 w_i dt_i
 * PRECONDITION: m is non-decreasing along a ray (the sampler guarantees it, thinned by a grid or
 * not).  Under it the double sum is evaluated in O(n) by prefix sums over positions taken relative to
 * the ray's FIRST midpoint (x_i = m_i - m_s, one f32 subtraction each), so a ray that starts far from
 * the origin pays no cancellation for its offset.  One wavefront per ray, no atomics and no LDS: the
 * same bits on every run.
 *   f2n_weight_dist_fwd: out[r] = D_r; an empty ray gives 0.
 *   f2n_weight_dist_bwd: dw[k] = d_out[r] * dD_r/dw_k for k in ray r's range, nothing is written
 *     outside the ranges (the caller zeroes dw if it needs zeros there).  Recomputed from the inputs;
 *     no state is saved by the forward.
 * t and dt receive no gradient: sample positions are data on every training route.
 * A null idx or output, or n_rays < 0: F2N_E_INVALID_ARG before any HIP work; n_rays == 0: F2N_OK. */
int f2n_weight_dist_fwd(
  const float * weights, const float * t, const float * dt, const int32_t * idx, float * out,
  int n_rays, void * stream);
int f2n_weight_dist_bwd(
  const float * weights, const float * t, const float * dt, const int32_t * idx,
  const float * d_out, float * dw, int n_rays, void * stream);

/* The line-of-sight losses of depth supervision per ray (Urban Radiance Fields, Rematas et al., CVPR
 * 2022, section 4.2: empty space, near surface, expected depth).  The reference has NO such kernel and
 * reads no range data: these stand beside WeightVarLoss*Kernel (src/CustomOps/CustomOps.cu:13-67) and
 * f2n_weight_dist_* above, on the same arrays, and are used where those are used
 * (src/main_functions/train_manager.cpp:80-93).
 *   weights, t, dt [n] f32 and idx [n_rays, 2] as for f2n_weight_dist_*: t is the interval END, the
 *   midpoint is m_k = t_k - 0.5f * dt_k in f32 (one rounding).
 *   z   [n_rays] f32: the ray's target distance, in the units of t (Euclidean distance along the unit
 *       ray direction).  A ray is VALID iff z is finite and > 0.
 *   eps f32 >= 0: half-width of the surface band; the caller schedules it.
 * For a valid ray, lo = z - eps and hi = z + eps in f32 (one rounding each); sample k is FRONT if
 * m_k < lo, BAND if m_k >= lo and m_k <= hi, BEHIND otherwise -- comparisons of f32 values, which are
 * the definition.  Then
 *     E_r = sum_front w_k^2                                (free space before the return)
 *     W_r = sum_band  w_k,      N_r = (1 - W_r)^2          (the weight belongs in the band)
 *     d_r = sum_all   w_k m_k,  X_r = (d_r - z_r)^2        (expected depth, not normalised by opacity)
 *   f2n_depth_sight_fwd: out [n_rays, 3] = (E_r, N_r, X_r).  An invalid ray gives (0, 0, 0); a valid
 *     ray with an empty range gives (0, 1, z^2).
 *   f2n_depth_sight_bwd: with (g0, g1, g2) = d_out[r],
 *         dw_k = g0 2 w_k [front]  -  g1 2 (1 - W_r) [band]  +  g2 2 (d_r - z_r) m_k
 *     for k in ray r's range; an invalid ray WRITES ZEROS over its own range.  Every element inside
 *     some range is written, nothing outside (the caller zeroes dw if it needs zeros there).
 *     Recomputed from the inputs; no state is saved by the forward.
 * t, dt and z receive no gradient.  A non-finite weight poisons its own ray only.  One wavefront per
 * ray, no atomics, no LDS, no scratch: the same bits on every run; the evaluation order is fixed in
 * the header comment of depth_sight.hip (the per-ray convention of the kernels that replace
 * src/CustomOps/CustomOps.cu:13-67).  Not here: URF's Gaussian near-surface kernel (the band with a
 * shrinking eps is its limit).
 * A null idx, z or output, n_rays < 0, or an eps that is negative or not finite: F2N_E_INVALID_ARG
 * before any HIP work; n_rays == 0: F2N_OK. */
int f2n_depth_sight_fwd(
  const float * weights, const float * t, const float * dt, const int32_t * idx, const float * z,
  float eps, float * out, int n_rays, void * stream);
int f2n_depth_sight_bwd(
  const float * weights, const float * t, const float * dt, const int32_t * idx, const float * z,
  float eps, const float * d_out, float * dw, int n_rays, void * stream);

/* ------------------------------------------------------------------ scatter (row A9) ---------- */

/* ScatterIdxKernal -- src/CustomOps/Scatter.cu:111-132 */
int f2n_scatter_idx(
  const int32_t * idx, const int32_t * emb_idx, int32_t * all_emb_idx, int n_rays, void * stream);
/* ScatterAddFuncForward (+ the clone at :63) -- src/CustomOps/Scatter.cu:11-19,45-70.
 * sum[p,c] = to_add[p,c] + emb[scatter_idx[p], c]; sum may alias to_add. */
int f2n_scatter_add_fwd(
  const float * emb, const int32_t * scatter_idx, const float * to_add, float * sum, int64_t n_all,
  int C, void * stream);
/* ScatterAddFuncBackwardBlock + torch::sum(dim 1) -- src/CustomOps/Scatter.cu:21-41,72-101.
 * demb [n_emb, C] is overwritten (zeroed, then accumulated) on `stream`. */
int f2n_scatter_add_bwd(
  const int32_t * scatter_idx, const float * dsum, float * demb, int64_t n_all, int n_emb, int C,
  void * stream);

/* ------------------------------------------------------------------ sampler (rows A4, A5) ----- */

/* get_rays_from_pose -- src/rays.cpp:7-28, for both callers: a view's pixel grid
 * (src/renderer.cpp:153-172, src/dataset.cpp:128-146) and the random training batch with one camera
 * per ray (src/dataset.cpp:150-171, without its index_select of poses and intrinsics).
 *   poses      [n_cams] blocks of pose_ld floats: a row-major [3,4] (pose_ld = 12) or [4,4] (16)
 *   intrinsics [n_cams, 3, 3]
 *   cam_idx    [n] i32 camera of each ray; NULL: camera 0 when n_cams == 1, camera r when n_cams == n
 *   ij         [n, 2] i32 (row, col); NULL: ray r is pixel first_pixel + r of a `width`-wide image
 *   rays_o, rays_d [n, 3]: origin = t, dir = R . ((col+.5-cx)/fx, -(row+.5-cy)/fy, -1), not normalised */
int f2n_gen_rays(
  const float * poses, int pose_ld, const float * intrinsics, int64_t n_cams,
  const int32_t * cam_idx, const int32_t * ij, int64_t first_pixel, int width, float * rays_o,
  float * rays_d, int64_t n, void * stream);

/* Backward of f2n_gen_rays with respect to the poses (the matmul and expand of src/rays.cpp:7-28,
 * differentiated by autograd in the reference's pose optimisation, src/localizer.cpp:142-167), for
 * constant intrinsics.  Addressing as f2n_gen_rays (no cam_idx: n_cams is 1 or n):
 *   d_poses [n_cams] blocks of pose_ld floats, overwritten:
 *     d_pose[i][3] = sum_r d_rays_o[r][i],  d_pose[i][j] = sum_r d_rays_d[r][i] * v_r[j] (j < 3),
 *     v_r the camera-frame direction of ray r as f2n_gen_rays forms it; row 3 of a [4,4] block = 0.
 *   n_cams == 1: a sum over all n rays in a fixed partition and order (the same bits on every run);
 *   n_cams == n: one pose per ray, no sum.
 *   workspace: f2n_gen_rays_bwd_workspace_floats(n) floats of device memory, contents undefined. */
int64_t f2n_gen_rays_bwd_workspace_floats(int64_t n);
int f2n_gen_rays_bwd(
  const float * intrinsics, int64_t n_cams, const int32_t * ij, int64_t first_pixel, int width,
  const float * d_rays_o, const float * d_rays_d, float * d_poses, int pose_ld, float * workspace,
  int64_t n, void * stream);

/* f2n_gen_rays for cameras with lens distortion: the k1, k2, p1, p2 that cams_meta.tsv carries per
 * image (src/dataset.cpp:59-63 reads them; get_rays_from_pose, src/rays.cpp:7-28, ignores them and
 * treats every camera as a pinhole).  The OpenCV / COLMAP "OPENCV" model on the normalised image
 * point, y down: with r2 = x^2 + y^2 and rad = 1 + r2 (k1 + k2 r2),
 *     xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2),   yd = y rad + p1 (r2 + 2 y^2) + 2 p2 x y.
 * Pixel (row, col) is the DISTORTED point xd = (col+.5-cx)/fx, yd = (row+.5-cy)/fy; the ray is
 * dir = R . (x, -y, -1) with (x, y) the solution of the model: exactly 8 Newton steps from (xd, yd),
 * f32, analytic Jacobian, no data-dependent exit (the same bits on every run); a step whose
 * determinant is not above 1e-8 in magnitude, or that would leave the finite numbers, is skipped, so
 * finite arguments give finite rays.
 *   dist  [n_cams, 4] (k1, k2, p1, p2), addressed like intrinsics: each ray uses its camera's row.
 *         NULL, or a row of four exact zeros: that camera is a pinhole and its rays are the bits of
 *         f2n_gen_rays (no iteration).
 * Everything else as f2n_gen_rays.  Not modelled: fisheye and other camera models, k3 and beyond. */
int f2n_gen_rays_dist(
  const float * poses, int pose_ld, const float * intrinsics, const float * dist, int64_t n_cams,
  const int32_t * cam_idx, const int32_t * ij, int64_t first_pixel, int width, float * rays_o,
  float * rays_d, int64_t n, void * stream);

/* f2n_gen_rays_bwd for f2n_gen_rays_dist (src/rays.cpp:7-28 under autograd, src/localizer.cpp:142-167;
 * coefficients of src/dataset.cpp:59-63): v_r is the undistorted direction (x, -y, -1), formed by the
 * device function the forward calls; it does not depend on the pose, so the formulas of
 * f2n_gen_rays_bwd stand as they are.  dist [n_cams, 4] or NULL, n_cams is 1 or n.  The workspace is
 * f2n_gen_rays_bwd_workspace_floats(n) floats; n_cams == 1 sums in the same fixed partition and
 * order (the same bits on every run; with zero coefficients the bits of f2n_gen_rays_bwd).  Neither
 * the intrinsics nor the coefficients receive a gradient here (f2n_cam_intr_grad forms theirs).
 * n == 0 returns F2N_OK and writes nothing. */
int f2n_gen_rays_dist_bwd(
  const float * intrinsics, const float * dist, int64_t n_cams, const int32_t * ij,
  int64_t first_pixel, int width, const float * d_rays_o, const float * d_rays_d, float * d_poses,
  int pose_ld, float * workspace, int64_t n, void * stream);

/* The backward of f2n_gen_rays / f2n_gen_rays_dist for a batch in which every ray names its own
 * camera: the random training batch of Dataset::sample_random_rays (src/dataset.cpp:150-171), whose
 * rays src/rays.cpp:7-28 forms from index_select'ed poses.  It is what joint refinement of the
 * training poses needs and what f2n_gen_rays_bwd (n_cams 1 or n) cannot give: one pose gradient per
 * camera, summed over that camera's rays.
 *   intrinsics [n_cams, 3, 3];  dist [n_cams, 4] or NULL (pinhole; a row of zeros gives its bits)
 *   ij         [n, 2] i32 (row, col), required
 *   d_rays_o, d_rays_d [n, 3]
 *   cam_start  [n_cams + 1] i32, non-decreasing from 0 to n: camera c owns positions
 *              cam_start[c] .. cam_start[c+1] of the camera-sorted ray list
 *   order      [n] i32: position p of that list is caller ray order[p]; NULL: the identity (the
 *              caller's rays are already sorted by camera)
 *   d_poses    [n_cams] blocks of pose_ld floats (12 or 16), every element overwritten:
 *                d_pose_c[i][3] = sum d_rays_o[r][i],  d_pose_c[i][j] = sum d_rays_d[r][i] * v_r[j]
 *              over the rays of camera c, v_r as the forward forms it; a camera without rays gets
 *              exact zeros; row 3 of a [4,4] block is zero.
 *   workspace  f2n_cam_pose_grad_workspace_floats(n, n_cams) floats, contents undefined on entry.
 * The list is cut into pieces of 1024 positions, one wavefront each; a camera inside one piece is
 * finished there, one that spans pieces has its partials added in piece order by a second kernel.
 * No float atomics, a partition and an order that depend on cam_start alone (the same bits on every
 * run), no host read, two launches.  n == 0 returns F2N_OK and zero-fills d_poses.  Values of
 * cam_start and order outside 0..n are clamped or skipped, never used as an address. */
int64_t f2n_cam_pose_grad_workspace_floats(int64_t n, int64_t n_cams);
int f2n_cam_pose_grad(
  const float * intrinsics, const float * dist, const int32_t * ij, const float * d_rays_o,
  const float * d_rays_d, const int32_t * cam_start, const int32_t * order, float * d_poses,
  int pose_ld, float * workspace, int64_t n, int64_t n_cams, void * stream);

/* A rigid correction of each camera pose by a 6-vector, the parameterisation of a camera optimiser.
 * The reference's only pose optimisation runs Adam on the twelve raw entries of a [3,4] matrix
 * (src/localizer.cpp:142-167), which leaves SO(3) after the first step; this stays on it.
 *   base   [n_cams] blocks of pose_ld floats (12 or 16; rows 0..2 are [R | t])
 *   delta  [n_cams, 6] = (omega_x, omega_y, omega_z, tau_x, tau_y, tau_z)
 *   fixed  [n_cams] i32 or NULL: a camera with a non-zero entry is not corrected (the gauge)
 *   out    [n_cams, 3, 4]:  R' = Exp(omega) R,  t' = t + tau -- left multiplication in the NeRF
 *          frame, the frame f2n_perturb_poses perturbs in (src/localizer.cpp:88-118).
 * Exp is Rodrigues' formula with its Taylor polynomial below |omega| = 1e-2, f64 inside, rounded once
 * to f32.  A camera whose six numbers are all zero, and every fixed camera, gets its base rows bit
 * for bit.  One thread per camera. */
int f2n_pose_compose(
  const float * base, int pose_ld, const float * delta, const int32_t * fixed, float * out,
  int64_t n_cams, void * stream);

/* Backward of f2n_pose_compose with respect to delta (what autograd would assemble from a Rodrigues
 * chain of ATen ops under src/localizer.cpp:142-167's Adam loop): d_out [n_cams, 3, 4] ->
 * d_delta [n_cams, 6], the analytic derivative of Exp at the given omega (not only at zero), f64
 * inside.  d tau = d_out[:, :, 3].  A fixed camera gets exact zeros.  The base poses receive no
 * gradient. */
int f2n_pose_compose_bwd(
  const float * base, int pose_ld, const float * delta, const int32_t * fixed, const float * d_out,
  float * d_delta, int64_t n_cams, void * stream);

/* The gradient of a batch's ray directions with respect to the calibration of each camera: the
 * fx, fy, cx, cy of its intrinsic and the k1, k2, p1, p2 of f2n_gen_rays_dist, which cams_meta.tsv
 * carries (src/dataset.cpp:59-63) and src/rays.cpp:7-28 treats as exact.  The batch, its addressing,
 * cam_start, order, the clamping of values outside 0..n and n == 0 (zero-fills d_intr) are those of
 * f2n_cam_pose_grad; rays_o does not depend on the calibration, so there is no d_rays_o.
 *   poses      [n_cams] blocks of pose_ld floats (12 or 16): R of each camera
 *   d_intr     [n_cams, 8] = d(fx, fy, cx, cy, k1, k2, p1, p2), every element overwritten
 *   workspace  f2n_cam_intr_grad_workspace_floats(n, n_cams) floats, contents undefined on entry.
 * For a ray of camera c with (x, y) the ideal point the forward returned (the same device function,
 * the same bits), xd = (col+.5-cx)/fx, yd = (row+.5-cy)/fy, r2 = x^2 + y^2:
 *     gx =  sum_i d_rays_d[r][i] R_c[i][0],   gy = -sum_i d_rays_d[r][i] R_c[i][1]
 *     J = [[a, b], [b, d]] the Jacobian of the distortion model at (x, y),  det = a d - b b
 *     lx = (d gx - b gy) / det,   ly = (a gy - b gx) / det
 *     d_intr[c] += ( -lx xd / fx, -ly yd / fy, -lx / fx, -ly / fy,
 *                    -r2 (lx x + ly y), -r2^2 (lx x + ly y),
 *                    -(2 x y lx + (r2 + 2 y^2) ly), -((r2 + 2 x^2) lx + 2 x y ly) )
 * the implicit-function gradient at the forward's point, not the derivative of its Newton steps.  A
 * camera whose four coefficients are zero (or a NULL dist) takes J = I and still receives the gradient
 * to its coefficients.  A ray with |det| <= 1e-8 or a non-finite lx, ly contributes exact zeros.  The
 * sums per camera are f2n_cam_pose_grad's: pieces of 1024 positions, no float atomics, the same bits
 * on every run, no host read, two launches. */
int64_t f2n_cam_intr_grad_workspace_floats(int64_t n, int64_t n_cams);
int f2n_cam_intr_grad(
  const float * poses, int pose_ld, const float * intrinsics, const float * dist,
  const int32_t * ij, const float * d_rays_d, const int32_t * cam_start, const int32_t * order,
  float * d_intr, float * workspace, int64_t n, int64_t n_cams, void * stream);

/* A shared correction of the calibration per physical camera, the parameterisation of
 * self-calibration (the reference reads fx, fy, cx, cy and k1, k2, p1, p2 per image from
 * cams_meta.tsv, src/dataset.cpp:59-63, and never changes them).  Image e belongs to group
 * g = group[e]; a negative group marks a fixed image.  With c = gamma[g]:
 *     fx' = fx exp(c0)    fy' = fy exp(c1)    cx' = cx + c2 fx    cy' = cy + c3 fy   (base fx, fy)
 *     k1' = k1 + c4       k2' = k2 + c5       p1' = p1 + c6       p2' = p2 + c7
 * eight dimensionless numbers of one scale.
 *   base_K     [n_images, 3, 3];  base_dist [n_images, 4] or NULL (zeros)
 *   gamma      [n_groups, 8];     group [n_images] i32
 *   out_K      [n_images, 3, 3], the other entries of K copied;  out_dist [n_images, 4]
 * f64 inside, each output rounded once.  An image whose eight numbers all compare equal to zero, or
 * whose group is negative, gets its base rows bit for bit.  A group >= n_groups is the caller's error:
 * the kernel treats it as fixed and never uses it as an address.  One thread per image. */
int f2n_intr_compose(
  const float * base_K, const float * base_dist, const float * gamma, const int32_t * group,
  float * out_K, float * out_dist, int64_t n_images, int64_t n_groups, void * stream);

/* Backward of f2n_intr_compose with respect to gamma: d_K [n_images, 3, 3] or NULL (zeros; only
 * [0][0], [1][1], [0][2], [1][2] are read), d_dist [n_images, 4] or NULL (zeros) ->
 *     d_gamma[g] = sum over the images of group g of
 *                  (dfx' fx', dfy' fy', dcx' fx, dcy' fy, dk1', dk2', dp1', dp2'),
 * every element of d_gamma [n_groups, 8] overwritten.  The sum is taken in f64 in image-index order
 * and rounded once: the same bits on every run, no float atomics.  learn [8] i32 or NULL: a column
 * whose flag is 0 gets exact zeros.  A group without images gets exact zeros. */
int f2n_intr_compose_bwd(
  const float * base_K, const float * base_dist, const float * gamma, const int32_t * group,
  const int32_t * learn, const float * d_K, const float * d_dist, float * d_gamma,
  int64_t n_images, int64_t n_groups, void * stream);

/* The forward model of the same camera, the inverse of f2n_gen_rays_dist (the projection that
 * src/rays.cpp:7-28 inverts, with the coefficients of src/dataset.cpp:59-63): world point -> pixel.
 *   points  [n, 3]; poses, pose_ld, intrinsics, dist (NULL = pinhole), n_cams, cam_idx: addressed as
 *           in f2n_gen_rays_dist, each point under its camera
 *   pix     [n, 2] f32 continuous (row, col), pixel (i, j) centred at (i + .5, j + .5):
 *           c = R^T (p - t), x = c_x / -c_z, y = -c_y / -c_z, distorted as above,
 *           row = yd fy + cy, col = xd fx + cx
 *   valid   [n] i32: 1 iff the point lies strictly in front of the camera (c_z < 0); pix of a point
 *           that does not is (0, 0).  No test against the image bounds: the caller knows its h, w. */
int f2n_project_points(
  const float * points, const float * poses, int pose_ld, const float * intrinsics,
  const float * dist, int64_t n_cams, const int32_t * cam_idx, float * pix, int32_t * valid,
  int64_t n, void * stream);

/* A point cloud to sparse per-camera depth maps: the targets of f2n_depth_sight_*.  The reference
 * reads no range data; the camera is the one f2n_project_points models (the projection that
 * src/rays.cpp:7-28 inverts, with the coefficients of src/dataset.cpp:59-63), and every point is
 * projected by the device function that entry calls, so its pixel decisions agree bit for bit.
 *   points  [n, 3] in the frame of the poses;  cam_idx [n] i32: point i is seen by camera cam_idx[i]
 *           (NULL: addressed as in f2n_project_points); a value outside [0, n_cams) skips the point,
 *           it is never used as an address
 *   poses, pose_ld, intrinsics, dist (NULL = pinhole), n_cams: as in f2n_project_points
 *   depth   [n_cams, h, w] f32, every element written; 0 = no return
 * A point is skipped unless it lies strictly in front of its camera (c_z < 0) and
 * (floor(row), floor(col)) falls inside [0, h) x [0, w).  Otherwise d = |p - t_cam|, the distance
 * ALONG THE RAY (what the samples' t measures), not the z-depth, and each pixel keeps the minimum:
 * an unsigned 32-bit atomicMin on the float's bit pattern (positive floats order like their bits).
 * A minimum does not depend on the order of arrival: two launches give the same bits.  The entry
 * fills the map with +inf, splats, and turns what is still +inf into 0 -- an async memset and two
 * launches on `stream`; no allocation, no sync, no host read.  No occlusion reasoning beyond that
 * per-pixel minimum.
 * Null poses, intrinsics or depth (or points with n > 0), n < 0, n_cams, h or w < 1, a pose_ld other
 * than 12 or 16: F2N_E_INVALID_ARG; h * w * n_cams >= 2^31: F2N_E_UNSUPPORTED; both before any HIP
 * work.  n == 0: all zeros and F2N_OK. */
int f2n_depth_splat(
  const float * points, const int32_t * cam_idx, const float * poses, int pose_ld,
  const float * intrinsics, const float * dist, int64_t n_cams, int h, int w, float * depth,
  int64_t n, void * stream);

/* PtsSampler::get_samples (about 20 ATen launches) -- src/points_sampler.cpp:20-64.
 *   noise   [n_rays, S] f32 step multipliers (TRAIN: U[0.5,1.5)), or NULL for all-ones (VALIDATE)
 *   outputs pts [n_rays*S, 3], dirs [n_rays*S, 3], dt [n_rays*S], t [n_rays*S], bounds [n_rays,2]
 *   S = MAX_SAMPLE_PER_RAY (1024), step = SAMPLE_L (1/256) in the reference (src/points_sampler.hpp:15,39) */
int f2n_sample_rays(
  const float * rays_o, const float * rays_d, const float * noise, float * pts, float * dirs,
  float * dt, float * t, int32_t * bounds, int n_rays, int S, float step, void * stream);

/* f2n_sample_rays followed by f2n_contract_fwd for a dense grid that goes straight to the hash
 * encode and the ray-uniform network kernels -- src/points_sampler.cpp:20-64 and the contraction of
 * src/hash_3d_anchored.cpp:79-82 -- without the arrays only those two steps exchange:
 *   noise      [n_rays, S] f32 or NULL (all ones), as f2n_sample_rays
 *   noise_row  [n_rays] i32 or NULL: ray r reads row noise_row[r] of `noise` (rays reordered after
 *              the noise was drawn; an entry outside [0, n_rays) is clamped); NULL = row r
 *   noise_affine 1: `noise` holds the uniform draw u in [0, 1) and the step multiplier is
 *              (u - .5f) + 1.f, rounded twice as the two ATen passes of src/points_sampler.cpp:35
 *              round it; 0: `noise` holds the multiplier
 *   outputs    x [n_rays*S, 3] CONTRACTED positions (f2n_contract_fwd of f2n_sample_rays' pts, bit for
 *              bit), dt, t [n_rays*S] and bounds [n_rays, 2] as f2n_sample_rays, ray_dirs [n_rays, 3]
 *              the unit direction of each ray (every row of f2n_sample_rays' dirs for that ray)
 * No world positions and no per-sample directions are written. */
int f2n_sample_dense(
  const float * rays_o, const float * rays_d, const float * noise, const int32_t * noise_row,
  int noise_affine, float * x, float * dt, float * t, int32_t * bounds, float * ray_dirs,
  int n_rays, int S, float step, void * stream);

/* Early-stop pass of Renderer::render fused into one march -- src/renderer.cpp:58-90 together with
 * src/points_sampler.cpp:20-64, src/hash_3d_anchored.cpp:79-86 (contraction, hash encode, row 0 of the
 * Linear) and src/CustomOps/CustomOps.cpp:10-14 (TruncExp fwd).  One wavefront walks one ray in 64-sample
 * strides and stops at the first stride whose transmittance exp(-sum sigma*dt) falls to
 * <= t_thresh; kept[r] = number of leading samples with T > t_thresh (the mask of :68 is a prefix).
 *   w0 [L*F] = mlp.weight[0, :], b0 = mlp.bias[0]; density = exp(w0.enc + b0 - density_shift) */
int f2n_density_march(
  const float * rays_o, const float * rays_d, const float * noise, const uint16_t * table_f16,
  const int32_t * primes, const float * bias, const float * mul, const float * w0, const float * b0,
  int32_t * kept, int n_rays, int S, float step, int L, int F, uint32_t T, int64_t level_stride,
  float t_thresh, float density_shift, void * stream);

/* The same keep-prefix as f2n_density_march (src/renderer.cpp:61-68 semantics), computed from an
 * encoding that already exists for ALL n_rays*S samples: enc_cm channel-major [C, n_rays*S] as
 * f2n_hash_fwd writes it, dt [n_rays*S] as f2n_sample_rays writes it.  Identical FMA chain, scan and
 * threshold test, hence identical counts.  The host picks this route when most samples survive, so
 * that the field is evaluated once (level-major, L2-friendly) and reused by the shading pass --
 * the reference evaluates it twice (src/renderer.cpp:61 and :92). */
int f2n_density_scan(
  const float * enc_cm, int C, const float * dt, const float * w0, const float * b0, int32_t * kept,
  int n_rays, int S, float t_thresh, float density_shift, void * stream);

/* A cheap sufficient test for "f2n_density_scan would keep every sample of every ray": logit
 * [n_rays*S] are density logits of the dense grid (any evaluation of the field head, e.g. the fused
 * per-sample network's), dt as above.  flag[0] (int32, zeroed by the caller) is set when some ray's
 * total optical depth sum_k exp(logit_k - density_shift) dt_k is not below depth_limit; choose
 * depth_limit = -ln(t_thresh) - margin with a margin far above the rounding differences between two
 * evaluations of the logit (the host uses 0.5).  Part of the same block src/renderer.cpp:61-68. */
int f2n_density_margin(
  const float * logit, const float * dt, int32_t * flag, int n_rays, int S, float density_shift,
  float depth_limit, void * stream);

/* Channel-major companion of the four index() gathers at src/renderer.cpp:71-74 for [C, n] tensors:
 * dst[c, bounds[r].start + k] = src[c, r*S + k] for k < bounds[r].end - bounds[r].start. */
int f2n_compact_rows_cm(
  const float * src, int64_t n_src, float * dst, int64_t n_dst, int C, const int32_t * bounds,
  int n_rays, int S, void * stream);

/* cumsum of the per-ray counts -> bounds (src/renderer.cpp:76-83).  total[0] = sum(kept).
 * Single-workgroup scan; n_rays <= 2^24. */
int f2n_bounds_from_counts(
  const int32_t * kept, int32_t * bounds, int32_t * total, int n_rays, void * stream);

/* where(mask) + the four index() gathers (src/renderer.cpp:69-74) without materialising the dense
 * sample arrays: re-derives the first (end-start) samples of each ray straight into the compacted
 * outputs pts/dirs [n_kept,3], dt/t [n_kept]. */
int f2n_sample_compact(
  const float * rays_o, const float * rays_d, const float * noise, const int32_t * bounds,
  float * pts, float * dirs, float * dt, float * t, int n_rays, int S, float step, void * stream);

/* Diagnostic: the ray walk behind every sampler, march and one-pass render kernel -- the samples of
 * src/points_sampler.cpp:20-64 and the early stop of src/renderer.cpp:58-90 -- written out sample by
 * sample at one of its three lane mappings.  The march and the render kernels give a ray 64, 16 or 8
 * lanes and let only counts and colours leave the device; this entry walks EVERY stride of every ray
 * (no early break; a lane is live when it holds a sample) at the mapping asked for and writes what
 * each lane holds.  Nothing in the host library calls it.
 *   noise    [n_rays, S] f32 step multipliers or NULL (all ones), as f2n_sample_rays
 *   sec_in   [n_rays, S] f32 optical depth sigma * dt of every sample, or NULL (none)
 *   width    64, 16 or 8: lanes to a ray
 *   outputs  pts [n_rays*S, 3], dt, t [n_rays*S]: f2n_sample_rays' values bit for bit at every width;
 *            with sec_in, depth [n_rays*S] f32 = the exclusive sum of sec_in in front of the sample as
 *            the early stop forms it, and keep [n_rays*S] u8 = expf(-depth) > t_thresh.  Without
 *            sec_in, depth and keep may be NULL and are not written.
 * A width other than the three, a null among rays_o, rays_d, pts, dt, t (or depth, keep with sec_in),
 * n_rays < 0, S < 1 or n_rays * S > INT32_MAX: F2N_E_INVALID_ARG before any HIP work; n_rays == 0:
 * F2N_OK. */
int f2n_ray_walk_probe(
  const float * rays_o, const float * rays_d, const float * noise, const float * sec_in, int width,
  float * pts, float * dt, float * t, float * depth, uint8_t * keep, int n_rays, int S, float step,
  float t_thresh, void * stream);

/* ------------------------------------------------------------------ occupancy bitfield -------- */

/* Empty-space skipping for the early-stop march.  The reference fork stripped upstream's occupancy
 * grid and kept only its trace (src/main_functions/train_manager.cpp:102, "output colors have no
 * grad due to the occupancy grid"), so its first pass (src/renderer.cpp:58-90) evaluates the field on
 * every sample in front of the first surface.  The grid: G x G x G bits over the contracted space
 * [-2, 2)^3 (src/hash_3d_anchored.cpp:79-82), G a power of two in 32..256; per axis
 *   c = (int)floorf((x + 2.f) * (0.25f * (float)G)) clamped to [0, G-1],
 * bit i = (cz*G + cy)*G + cx in bit (i & 31) of uint32 word (i >> 5); bits is [G^3 / 32] words.  A
 * point with a non-finite contracted coordinate (|p| = 0, quirk Q6) reads as occupied.
 * Rendering with a grid is the reference's render with the density of every sample in an unoccupied
 * cell set to exactly zero and those samples dropped; with an all-ones grid it is today's render. */

/* One maintenance pass over all G^3 cells, one thread per cell, no atomics (the same bits on every
 * run).  Per cell the density sigma = exp(w0 . f16(enc(x)) + b0 - density_shift) at ONE probe point
 * x = ((float)c + u) * (4.f / G) - 2.f per axis -- a contracted-space point, so no contraction --
 * with the gather, f16 rounding and level-ordered FMA chain of f2n_density_march (the field
 * evaluation of src/renderer.cpp:61-62); then
 *   density[i] = max(density[i] * decay, sigma),  bit i = density[i] > threshold.
 *   probe_u    [G^3, 3] f32 in [0,1), cell i's offsets (x, y, z), or NULL for the cell centre (0.5)
 *   density    [G^3] f32, read and written; bits [G^3/32] overwritten
 * A sample whose density equals the threshold carries at most threshold * 1.5 * step of optical depth
 * under TRAIN jitter (src/points_sampler.cpp:31-36).  A probe is one point, not a bound on its cell:
 * hence the decay (a cell seen dense stays on for a while) and the caller-supplied jitter u. */
int f2n_occ_update(
  const uint16_t * table_f16, const int32_t * primes, const float * bias, const float * mul,
  const float * w0, const float * b0, const float * probe_u, float * density, uint32_t * bits, int G,
  int L, int F, uint32_t T, int64_t level_stride, float density_shift, float threshold, float decay,
  void * stream);

/* The lookup every kernel below uses, on its own: raw (uncontracted) points [n,3] in, out[i] = 1 if
 * the cell of contract(pts[i]) (src/hash_3d_anchored.cpp:79-82) is occupied, else 0. */
int f2n_occ_lookup(
  const float * pts, int64_t n, const uint32_t * bits, int G, uint8_t * out, void * stream);

/* f2n_density_march (src/renderer.cpp:58-90 with src/points_sampler.cpp:20-64) with a grid: the
 * sampler is unchanged (sample k keeps the t, p, dt of the full sequence),
 *   sec_k = occupied(p_k) ? sigma_k * dt_k : 0,  T_k = exp(-exclusive_scan(sec)),
 *   len[r]  = number of leading samples with T_k > t_thresh (a prefix, as at :68),
 *   kept[r] = number of occupied samples among them: the ray's sample list is
 *             {k < len[r] : occupied(p_k)} in order of k.
 * One wavefront per ray in 64-sample strides; a stride without an occupied sample is not encoded.
 * The scan adds what f2n_density_march's adds: with an all-ones grid kept = len = its kept. */
int f2n_density_march_occ(
  const float * rays_o, const float * rays_d, const float * noise, const uint16_t * table_f16,
  const int32_t * primes, const float * bias, const float * mul, const float * w0, const float * b0,
  const uint32_t * bits, int G, int32_t * kept, int32_t * len, int n_rays, int S, float step, int L,
  int F, uint32_t T, int64_t level_stride, float t_thresh, float density_shift, void * stream);

/* f2n_sample_compact (src/renderer.cpp:69-74) for that list: bounds from f2n_bounds_from_counts on
 * kept, len from f2n_density_march_occ with the same grid; sample k of the list is written at
 * bounds[r].start + (number of occupied samples before k).  Outputs as f2n_sample_compact. */
int f2n_sample_compact_occ(
  const float * rays_o, const float * rays_d, const float * noise, const int32_t * bounds,
  const int32_t * len, const uint32_t * bits, int G, float * pts, float * dirs, float * dt,
  float * t, int n_rays, int S, float step, void * stream);

/* The cells the training cameras can sample (no reference counterpart).  "Camera c marks cell i":
 * there is a walked pixel (row, col) of c and a k in [0, n_steps) such that VALIDATE sample k of that
 * pixel's ray -- the direction of f2n_gen_rays_dist (src/rays.cpp:7-28: pixel centre at +0.5; the
 * Newton steps when the camera's row of dist is non-zero, the pinhole expression when it is zero or
 * dist is NULL), origin = the pose's translation, f2n_sample_rays' walk (src/points_sampler.cpp:31-48)
 * with all-ones noise, S = n_steps and the given step -- contracts (src/hash_3d_anchored.cpp:79-82)
 * into cell i (the cell expression above).  The kernel calls the device functions
 * those entries call: the same bits.  A sample with a non-finite contracted coordinate marks nothing.
 * Walked pixels at pixel_stride s >= 1: rows min(a*s, h-1) for a = 0 .. ceil((h-1)/s), columns
 * likewise, so the last row and the last column are always walked; with mask_bits (f2n_mask_pack's
 * layout: global pixel g = (cam*h + row)*w + col, cam the camera's ABSOLUTE row in the tables) a
 * pixel whose bit is 0 is skipped.
 *   poses [*, pose_ld] (pose_ld 12 or 16), intrinsics [*, 9], dist [*, 4] or NULL: the tables of
 *   f2n_gen_rays_dist; cameras cam_first .. cam_first + n_cams - 1 are walked
 *   bits [G^3/32]: ORed into, never cleared
 * One wavefront per ray in 64-sample strides (f2n_density_march_occ without the field), a
 * persistent grid-stride loop over the rays; integer atomic OR only, issued where the bit read as 0
 * and by the first lane of a run of equal cells: the result does not depend on the order of arrival.
 * A null table or bits, a G the grid does not accept, pose_ld not 12 or 16, h, w, pixel_stride or
 * n_steps < 1, n_steps > 65536, cam_first < 0, n_cams < 0, step not positive and finite:
 * F2N_E_INVALID_ARG before any HIP work; then n_cams == 0: F2N_OK, nothing written.  No allocation,
 * no synchronisation, no host read: capturable in a graph, like the three entries below. */
int f2n_occ_mark_rays(
  const float * poses, int pose_ld, const float * intrinsics, const float * dist, int cam_first,
  int n_cams, int h, int w, int pixel_stride, const uint32_t * mask_bits, int n_steps, float step,
  uint32_t * bits, int G, void * stream);

/* out bit (x, y, z) = OR of in over |dx|, |dy|, |dz| <= 1 inside [0, G)^3: no wrap-around.  A TRAIN
 * sample (src/points_sampler.cpp:31-36: jitter in [0.5, 1.5) steps) lies within half a step of a
 * VALIDATE sample of its ray; while that is at most a cell, one pass covers it.  One thread per cell,
 * no atomics.  in == out, a null or a bad G: F2N_E_INVALID_ARG. */
int f2n_occ_dilate(const uint32_t * in, uint32_t * out, int G, void * stream);

/* Views per cell: count [G^3] u8, count[i] = min(255, count[i] + bit i), called once per camera with
 * that camera's (dilated) marks. */
int f2n_occ_count_add(const uint32_t * bits, uint8_t * count, int G, void * stream);

/* bit i = count[i] >= min_count; bits [G^3/32] overwritten: the grid the march reads
 * (src/renderer.cpp:58-90 with f2n_density_march_occ) once ANDed into an occupancy bitfield. */
int f2n_occ_count_bits(
  const uint8_t * count, int min_count, uint32_t * bits, int G, void * stream);

/* ------------------------------------------------------------------ ray order --------------- */

/* Bucketing of a ray batch for the gather locality of f2n_hash_fwd_raytile (no reference
 * counterpart: Renderer::render, src/renderer.cpp:33-123, renders rays in the order it is given
 * them; its RenderResult, :122, is what the gathers below restore).  keys [n] int32 (>= 0) from
 * the direction alone (cube-face projection, 14 bits per face axis, Hilbert order): sorted stably,
 * 64 consecutive rays of one view become a compact pixel blob.  A zero direction, or one with an
 * infinite or NaN component, has key 0. */
int f2n_ray_keys(const float * rays_d, int32_t * keys, int n, void * stream);

/* Inputs of ray j of the sorted order from caller ray order[j] (order: the int64 indices of a
 * stable sort of the keys): rays_o / rays_d / bg [n,3], emb_idx [n], noise [n, S] (emb_idx, bg,
 * noise may be NULL together with their outputs); perm[j] = order[j] as int32, inv[perm[j]] = j. */
int f2n_ray_permute(
  const int64_t * order, int n, int S, const float * rays_o, const float * rays_d,
  const int32_t * emb_idx, const float * bg, const float * noise, int32_t * perm, float * rays_o_p,
  float * rays_d_p, int32_t * emb_idx_p, float * bg_p, float * noise_p, int32_t * inv,
  void * stream);

/* dst row i = src row map[i], rows of row_floats floats (a permutation's gather; with the inverse
 * map it is also the scatter). */
int f2n_gather_rows(
  const float * src, float * dst, const int32_t * map, int n, int row_floats, void * stream);

/* Ragged counterpart: dst[dst_bounds[i].start + k] = src[src_bounds[map[i]].start + k] for
 * k < dst_bounds[i].end - dst_bounds[i].start (the two segments have equal lengths). */
int f2n_gather_segments(
  const float * src, const int32_t * src_bounds, float * dst, const int32_t * dst_bounds,
  const int32_t * map, int n_rays, void * stream);

/* counts[i] = bounds[map[i]].end - bounds[map[i]].start (f2n_bounds_from_counts turns them into
 * the bounds of the caller's order). */
int f2n_counts_through(
  const int32_t * bounds, const int32_t * map, int32_t * counts, int n_rays, void * stream);

/* ------------------------------------------------------------------ compositing (rows A7, A8) - */

/* src/renderer.cpp:93,107-118 as one pass per ray:
 *   sigma = exp(logit - density_shift); s = sigma*dt; alpha = 1-exp(-s); T = exp(-excl_scan(s));
 *   w = T*alpha; T_last = exp(-sum s); C = sum w*rgb + T_last*bg; D = sum w*(t+t_shift)/(1-T_last+1e-4)
 *   logit element i at logit[i*logit_ld] (column 0 of the [n,16] field output: logit_ld = 16)
 *   outputs colors [n_rays,3], depths [n_rays], weights [n], last_trans [n_rays] (saved for bwd) */
int f2n_composite_fwd(
  const float * logit, int64_t logit_ld, const float * rgb, const float * dt, const float * t,
  const int32_t * bounds, const float * bg, float * colors, float * depths, float * weights,
  float * last_trans, int n_rays, float density_shift, float t_shift, void * stream);

/* Backward of the above = FlexSum/FlexSumVec/FlexAccumulateSum backward kernels plus the ATen
 * element-wise backward and TruncExp::backward (src/CustomOps/CustomOps.cpp:16-20: exp(clamp(x,-100,5))).
 *   in : d_colors [n_rays,3], d_depths [n_rays], d_weights [n] (NULL = zeros)
 *   out: d_logit [n] (dense), d_rgb [n,3] */
int f2n_composite_bwd(
  const float * logit, int64_t logit_ld, const float * rgb, const float * dt, const float * t,
  const int32_t * bounds, const float * bg, const float * weights, const float * last_trans,
  const float * d_colors, const float * d_depths, const float * d_weights, float * d_logit,
  float * d_rgb, int n_rays, float density_shift, float t_shift, void * stream);

/* ------------------------------------------------------------------ fused per-sample network -- */

/* Everything between the hash encode and the compositing, one kernel per direction:
 *   h = mlp(enc)                       Linear(C->16) of Hash3DAnchored::query -- src/hash_3d_anchored.cpp:86
 *   logit = h[0]                       density logit                          -- src/renderer.cpp:93
 *   X = cat(1, h[1:16]) (+ app_emb[sample_img]) ++ SH16(dirs)                 -- src/renderer.cpp:95-104,
 *                                                                                src/sh_shader.cpp:24-25
 *   rgb = (1+2e)*sigmoid(mlp2(relu(mlp1(X)))) - e, e = 1e-3                   -- src/sh_shader.cpp:26-28
 * i.e. the three nn::Linear GEMMs, torch::cat x2, ScatterAdd (src/CustomOps/Scatter.cu:11-19),
 * SHKernel (src/sh_shader.cu:11-103) and the element-wise tail.  enc_cm / d_enc_cm are
 * channel-major [C, n] (C = L*F in {8,16,32,64}); w_h [16,C], w1 [64,32], w2 [3,64] row-major as
 * nn::Linear stores them; sample_img [n] image id per sample or NULL (no appearance embedding).
 * pre_cm: optional [64, n] output of the hidden layer's pre-activations (what autograd would have
 * saved for the ReLU); give it to f2n_shade_bwd and that kernel loads them instead of recomputing. */
int f2n_shade_fwd(
  const float * enc_cm, int C, const float * dirs, const int32_t * sample_img, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, float * logit, float * rgb, float * pre_cm, int64_t n, void * stream);

/* Backward of the above (recomputes the forward per sample).  d_enc_cm is overwritten; the seven
 * parameter gradients are ACCUMULATED INTO (caller zeroes them); g_app_emb may be NULL when
 * app_emb / sample_img are; pre_cm = the forward's optional output or NULL (recompute).  Replaces the
 * autograd chain of the ops listed above, including
 * ScatterAddFuncBackwardBlock -- src/CustomOps/Scatter.cu:21-41,72-101. */
int f2n_shade_bwd(
  const float * enc_cm, int C, const float * dirs, const int32_t * sample_img, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, const float * d_logit, const float * d_rgb, float * d_enc_cm,
  float * g_w_h, float * g_b_h, float * g_w1, float * g_b1, float * g_w2, float * g_b2,
  float * g_app_emb, const float * pre_cm, int64_t n, void * stream);

/* The same network on a dense grid of samples: n = n_rays * S samples in ray-major order (the
 * sampler's [n_rays, S] grid before compaction), S a multiple of 64, so that every 64-sample stride
 * of the kernels lies inside one ray.  The reference lines are those of f2n_shade_fwd --
 * src/hash_3d_anchored.cpp:86, src/renderer.cpp:93-104, src/sh_shader.cpp:24-28, src/sh_shader.cu:11-103.
 * What is the same for every sample of a ray is done once per stride: the direction (read from
 * dirs[3 * s0] of the stride's first sample: `dirs` stays the per-sample [n, 3] array and must hold
 * the ray's direction in every sample of the ray), SH16(dir), the embedding row of ray_img[ray]
 * ([n_rays] image id per ray, or NULL: no appearance embedding -- it replaces sample_img and the
 * ScatterIdx launch, src/CustomOps/Scatter.cu:43-70) and the SH half of the hidden layer,
 * b1 + w1[:, 16:32] . SH(dir).  Matrix-core kernels only: F2N_E_UNSUPPORTED for a C other than 8, 16,
 * 32, 64 and for 2^28 samples or more; F2N_E_INVALID_ARG for S % 64 != 0 or a null pointer.
 * Numerics: logit is bit-identical to f2n_shade_fwd's (the head layer is untouched); rgb agrees to
 * rounding, not to the bit (the same f32 terms, the SH part of the hidden layer added first instead
 * of last). */
int f2n_shade_fwd_rays(
  const float * enc_cm, int C, const float * dirs, const int32_t * ray_img, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, float * logit, float * rgb, int n_rays, int S, void * stream);

/* Backward of the above, with the contract of f2n_shade_bwd (d_enc_cm overwritten, the seven
 * parameter gradients accumulated into) -- the autograd chain of the same reference lines and
 * ScatterAddFuncBackwardBlock, src/CustomOps/Scatter.cu:21-41,72-101.  F2N_OPT_SHADE_BWD_WAVES and
 * F2N_OPT_SHADE_VARIANT choose its form as they do for f2n_shade_bwd.  d_enc and the parameter
 * gradients agree with f2n_shade_bwd's to rounding, not to the bit: the same f32 terms in another
 * order (d w1[:, 16:32] is summed over the samples of a stride before it is multiplied by SH(dir)). */
int f2n_shade_bwd_rays(
  const float * enc_cm, int C, const float * dirs, const int32_t * ray_img, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, const float * d_logit, const float * d_rgb, float * d_enc_cm,
  float * g_w_h, float * g_b_h, float * g_w1, float * g_b1, float * g_w2, float * g_b2,
  float * g_app_emb, int n_rays, int S, void * stream);

/* f2n_shade_fwd_rays / f2n_shade_bwd_rays with ONE direction row per ray: ray_dirs [n_rays, 3] (what
 * f2n_sample_dense writes) in place of the per-sample [n, 3] array, addressed per stride as ray_img
 * is.  Same kernels (a scalar argument selects the row), same arguments otherwise, same status codes,
 * and for equal directions the same bits as those entries. */
int f2n_shade_fwd_raydirs(
  const float * enc_cm, int C, const float * ray_dirs, const int32_t * ray_img, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, float * logit, float * rgb, int n_rays, int S, void * stream);

int f2n_shade_bwd_raydirs(
  const float * enc_cm, int C, const float * ray_dirs, const int32_t * ray_img, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, const float * d_logit, const float * d_rgb, float * d_enc_cm,
  float * g_w_h, float * g_b_h, float * g_w1, float * g_b1, float * g_w2, float * g_b2,
  float * g_app_emb, int n_rays, int S, void * stream);

/* The per-ray half of the hidden layer formed ONCE per ray instead of once per stride of the two
 * entries above (which form it twice per ray forward and four times backward at S = 128) -- the SH
 * input of src/sh_shader.cpp:24-28 (src/sh_shader.cu:11-103) through the first Linear of the colour MLP.
 *   ray_const [n_rays, F2N_SHADE_RAY_CONST_FLOATS], 16-byte aligned; row of a ray:
 *     [0, 64)   c[j] = b1[j] + sum_i w1[j][16 + i] SH16(dir)[i], the f32 chain the ray-uniform kernels
 *               run: from b1[j], fmaf over i = 0, 4, 8, 12, 1, 5, 9, 13, 2, ... (k-step by k-step of the
 *               matrix product, the four quarters of a k-step in order)
 *     [64, 80)  SH16(dir), as f2n_sh_encode evaluates it
 * f2n_shade_ray_const writes it from ray_dirs [n_rays, 3], w1 [64, 32] and b1 [64] in one small launch
 * (a wavefront takes 16 rays as the 16 columns of the products the network kernels issue for one, so
 * a row holds the bits those kernels form themselves).  n_rays = 0 is F2N_OK; n_rays < 0, a null or a
 * misaligned ray_const F2N_E_INVALID_ARG. */
#define F2N_SHADE_RAY_CONST_FLOATS 80
int f2n_shade_ray_const(
  const float * ray_dirs, const float * w1, const float * b1, float * ray_const, int n_rays,
  void * stream);

/* f2n_shade_fwd_raydirs / f2n_shade_bwd_raydirs loading that row instead of forming it: kernels of
 * their own (shade_*_mfma_rays_kernel_const), 16 matrix products per stride fewer, no direction loads
 * and no SH evaluation; the same reference lines as f2n_shade_fwd_rays, src/renderer.cpp:93-104.
 * ray_const must have been written from the w1 and b1 passed here and from the rays' directions.
 * Same status codes and the same choice of form as those entries; logit, rgb and d_enc are theirs bit
 * for bit, the parameter gradients the same f32 terms in the same per-wave order.  The forward takes
 * no directions; the backward takes ray_dirs [n_rays, 3] in the place f2n_shade_bwd_raydirs does
 * (required, and not read while every form of the loading kernel fits its registers: all do). */
int f2n_shade_fwd_rays_const(
  const float * enc_cm, int C, const float * ray_const, const int32_t * ray_img, const float * w_h,
  const float * b_h, const float * w1, const float * b1, const float * w2, const float * b2,
  const float * app_emb, float * logit, float * rgb, int n_rays, int S, void * stream);

int f2n_shade_bwd_rays_const(
  const float * enc_cm, int C, const float * ray_dirs, const float * ray_const,
  const int32_t * ray_img, const float * w_h, const float * b_h, const float * w1, const float * b1,
  const float * w2, const float * b2, const float * app_emb, const float * d_logit,
  const float * d_rgb, float * d_enc_cm, float * g_w_h, float * g_b_h, float * g_w1, float * g_b1,
  float * g_w2, float * g_b2, float * g_app_emb, int n_rays, int S, void * stream);

/* ------------------------------------------------------------------ one-pass inference render - */

/* Renderer::render without gradients as ONE kernel, rays in and colours out -- src/renderer.cpp:33-123
 * as used by render_all_rays (src/renderer.cpp:125-151), render_image (src/renderer.cpp:153-172) and
 * Localizer::evaluate_poses (src/localizer.cpp:172): the sampler (src/points_sampler.cpp:20-64), the
 * early-stop first pass (:58-90), the second field query, the shader (:92-105) and the compositing
 * sums (:107-118).  One wavefront per ray in 64-sample strides; per stride the field is evaluated
 * ONCE: its f16-rounded encoding feeds
 *   the chain  logit_c = fma(enc_c, w_h[0][c], .) from b_h[0], in f2n_density_march's order -- it
 *              decides which samples exist: kept (and len) are f2n_density_march's, or with a grid
 *              f2n_density_march_occ's, bit for bit;
 *   the network of f2n_shade_fwd_rays on the matrix cores (head Linear(C->16), embedding row of
 *              ray_img[ray], SH16(dir), Linear(32->64), ReLU, Linear(64->3), sigmoid tail), whose
 *              h[0] is the density logit that weights the kept samples, as in f2n_composite_fwd.
 * Nothing per-sample is written: no compaction, no survivor count, O(n_rays) memory, no workspace, no
 * atomics (two launches give the same bits); capturable in a hipGraph.
 *   w_h [16,C], b_h [16], w1 [64,32], b1 [64], w2 [3,64], b2 [3]  row-major, as f2n_shade_fwd
 *   app_emb [*,16] (16-byte aligned) with ray_img [n_rays], or both NULL: no appearance embedding
 *   occ_bits [G^3/32] with G a power of two in 32..256, or NULL: no grid (G is then ignored); an
 *            all-ones grid gives the bits of no grid
 *   bg [n_rays,3];  outputs colors [n_rays,3], depths [n_rays], last_trans [n_rays] (1 - opacity),
 *   kept [n_rays] (samples composited), len [n_rays] or NULL (the prefix length kept was thinned from)
 * C = L*F in {8,16,32,64} with F in {1,2,4,8} and L <= 32, else F2N_E_UNSUPPORTED; any S >= 1 (the
 * last stride is partial when S % 64 != 0).  No per-sample weights and no gradients: training and
 * pose optimisation keep the routes above. */
int f2n_render_rays(
  const float * rays_o, const float * rays_d, const float * noise /* [n_rays,S] or NULL */,
  const uint16_t * table, const int32_t * primes, const float * bias, const float * mul,
  const float * w_h, const float * b_h, const float * w1, const float * b1,
  const float * w2, const float * b2,
  const float * app_emb, const int32_t * ray_img /* both NULL: no appearance embedding */,
  const uint32_t * occ_bits /* NULL: no grid */, int G,
  const float * bg, float * colors, float * depths, float * last_trans,
  int32_t * kept, int32_t * len /* may be NULL */,
  int n_rays, int S, float step, int L, int F, uint32_t T, int64_t level_stride,
  float t_thresh, float density_shift, float t_shift, void * stream);

/* f2n_render_rays where rays are short, in two launches that still read nothing back.  Replaces the
 * same sites: src/renderer.cpp:33-123 as used by src/renderer.cpp:125-151 and src/localizer.cpp:172.
 *
 * f2n_render_rays_head renders the first n_head samples of every ray EIGHT rays to a wavefront (a ray
 * owns 8 lanes, strides of 8 samples, f2n_density_march's default mapping): a ray that stops after
 * three samples costs an eighth of a wavefront's stride, not a whole one.  kept and len are still
 * f2n_density_march's / f2n_density_march_occ's bit for bit; colours, depths and last_trans agree
 * with f2n_render_rays to rounding (the same terms; the sums inside a stride in another order).  A
 * ray that ends inside the head gets its outputs; a ray still alive at sample n_head gets none yet:
 * its state goes to `state` and it is marked pending.
 * f2n_render_rays_tail resumes the pending rays at sample n_head in f2n_render_rays's one-ray form
 * and writes their outputs; the others are skipped.  Same arguments as the head, after it on the
 * same stream.
 *   n_head  a multiple of 64 (the block boundary of the 64-lane scan, where both forms' carries are
 *           the same bits), or any value >= S: the whole ray in the short form, no state written,
 *           state may be NULL and the tail is a no-op.  Anything else: F2N_E_INVALID_ARG.
 *   state   f2n_render_rays_state_bytes(n_rays) bytes, 16-byte aligned: 64 bytes per ray,
 *           16 words: [0] int32 pending, [1] cumulative noise, [2..4] last sample point, [5] the
 *           march's optical depth, [6] the compositing optical depth, [7..10] partial r, g, b, depth,
 *           [11] int32 kept, [12] int32 len, [13..15] unused.  NULL with n_head < S:
 *           F2N_E_INVALID_ARG.  Written by the head in full before the tail reads it: no need to
 *           clear it.
 * Everything else as f2n_render_rays.  No atomics, no other workspace: two runs give the same bits. */
int64_t f2n_render_rays_state_bytes(int n_rays);
int f2n_render_rays_head(
  const float * rays_o, const float * rays_d, const float * noise /* [n_rays,S] or NULL */,
  const uint16_t * table, const int32_t * primes, const float * bias, const float * mul,
  const float * w_h, const float * b_h, const float * w1, const float * b1,
  const float * w2, const float * b2,
  const float * app_emb, const int32_t * ray_img /* both NULL: no appearance embedding */,
  const uint32_t * occ_bits /* NULL: no grid */, int G,
  const float * bg, float * colors, float * depths, float * last_trans,
  int32_t * kept, int32_t * len /* may be NULL */,
  int n_rays, int S, float step, int L, int F, uint32_t T, int64_t level_stride,
  float t_thresh, float density_shift, float t_shift, int n_head, void * state, void * stream);
/* The second launch (see above): the rest of src/renderer.cpp:33-123 for the rays that are still alive
 * after n_head samples, as src/renderer.cpp:125-151 and src/localizer.cpp:172 use it. */
int f2n_render_rays_tail(
  const float * rays_o, const float * rays_d, const float * noise /* [n_rays,S] or NULL */,
  const uint16_t * table, const int32_t * primes, const float * bias, const float * mul,
  const float * w_h, const float * b_h, const float * w1, const float * b1,
  const float * w2, const float * b2,
  const float * app_emb, const int32_t * ray_img /* both NULL: no appearance embedding */,
  const uint32_t * occ_bits /* NULL: no grid */, int G,
  const float * bg, float * colors, float * depths, float * last_trans,
  int32_t * kept, int32_t * len /* may be NULL */,
  int n_rays, int S, float step, int L, int F, uint32_t T, int64_t level_stride,
  float t_thresh, float density_shift, float t_shift, int n_head, const void * state,
  void * stream);

/* ------------------------------------------------------------------ level weights -------------- */

/* Coarse-to-fine weights of the encoding's L levels from a progress alpha in [1, L] (the schedule of
 * bundle-adjusting fields), for level l = 0 .. L-1:
 *   w_l = 0                               for alpha - l <= 0
 *   w_l = (1 - cos(pi (alpha - l))) / 2   for 0 < alpha - l < 1
 *   w_l = 1                               otherwise
 * evaluated in double and rounded to f32.  No counterpart in the reference, whose
 * Hash3DAnchored::Query (src/hash_3d_anchored.cpp:79-87) hands every level to the head at full
 * weight; a caller applies the weights by scaling the head's columns (W_h[:, lF..lF+F) by w_l), which
 * every kernel that takes w_h then honours with no change of its own.
 *   w_host    [L] floats, HOST memory
 *   l_active  1 + the index of the last non-zero weight (>= 1): the levels a level-of-detail entry
 *             below has to walk
 * Host arithmetic, no HIP work.  F2N_E_INVALID_ARG for L < 1, L > F2N_MAX_LEVELS, alpha < 1, a
 * non-finite alpha or a NULL pointer; alpha > L is taken as L. */
int f2n_level_weights(double alpha, int L, float * w_host, int * l_active);

/* The three one-pass entries above with a level of detail: the field is walked over its first
 * L_active levels only, and the network sees zeros for the others -- what a head whose columns from
 * L_active * F on are zero computes, without gathering what it would multiply by zero.
 * No counterpart in the reference, whose Renderer::Render (src/renderer.cpp:33-123) always queries
 * every level.  Each wavefront clears rows [L_active * F, C) of its f16 tile once, before its first stride;
 * table, primes, bias, mul, w_h and level_stride stay those of the full L.
 *   L_active  1 <= L_active <= L, else F2N_E_INVALID_ARG (after every check of the entry without it,
 *             before any HIP work).  L_active == L: the entry without it, launch for launch and bit
 *             for bit -- which is how those entries are implemented.
 * Everything else as the entry of the same name without the suffix. */
int f2n_render_rays_lod(
  const float * rays_o, const float * rays_d, const float * noise /* [n_rays,S] or NULL */,
  const uint16_t * table, const int32_t * primes, const float * bias, const float * mul,
  const float * w_h, const float * b_h, const float * w1, const float * b1,
  const float * w2, const float * b2,
  const float * app_emb, const int32_t * ray_img /* both NULL: no appearance embedding */,
  const uint32_t * occ_bits /* NULL: no grid */, int G,
  const float * bg, float * colors, float * depths, float * last_trans,
  int32_t * kept, int32_t * len /* may be NULL */,
  int n_rays, int S, float step, int L, int L_active, int F, uint32_t T, int64_t level_stride,
  float t_thresh, float density_shift, float t_shift, void * stream);
/* f2n_render_rays_head over L_active levels (see f2n_render_rays_lod; src/renderer.cpp:33-123). */
int f2n_render_rays_head_lod(
  const float * rays_o, const float * rays_d, const float * noise /* [n_rays,S] or NULL */,
  const uint16_t * table, const int32_t * primes, const float * bias, const float * mul,
  const float * w_h, const float * b_h, const float * w1, const float * b1,
  const float * w2, const float * b2,
  const float * app_emb, const int32_t * ray_img /* both NULL: no appearance embedding */,
  const uint32_t * occ_bits /* NULL: no grid */, int G,
  const float * bg, float * colors, float * depths, float * last_trans,
  int32_t * kept, int32_t * len /* may be NULL */,
  int n_rays, int S, float step, int L, int L_active, int F, uint32_t T, int64_t level_stride,
  float t_thresh, float density_shift, float t_shift, int n_head, void * state, void * stream);
/* f2n_render_rays_tail over L_active levels (see f2n_render_rays_lod; src/renderer.cpp:33-123):
 * the same L_active as the head before it. */
int f2n_render_rays_tail_lod(
  const float * rays_o, const float * rays_d, const float * noise /* [n_rays,S] or NULL */,
  const uint16_t * table, const int32_t * primes, const float * bias, const float * mul,
  const float * w_h, const float * b_h, const float * w1, const float * b1,
  const float * w2, const float * b2,
  const float * app_emb, const int32_t * ray_img /* both NULL: no appearance embedding */,
  const uint32_t * occ_bits /* NULL: no grid */, int G,
  const float * bg, float * colors, float * depths, float * last_trans,
  int32_t * kept, int32_t * len /* may be NULL */,
  int n_rays, int S, float step, int L, int L_active, int F, uint32_t T, int64_t level_stride,
  float t_thresh, float density_shift, float t_shift, int n_head, const void * state,
  void * stream);

/* ------------------------------------------------------------------ optimiser (section 8f) ----- */

/* One fused pass of torch::optim::Adam::step() over one f32 parameter tensor -- the call at
 * src/main_functions/train_manager.cpp:106 with the options of src/hash_3d_anchored.cpp:90-114
 * (betas 0.9/0.99, eps 1e-15, weight decay 0 for the table, 1e-6 elsewhere) -- that also writes the
 * RNE f16 copy of the updated parameter when shadow_f16 != NULL (the feat_pool.to(kFloat16) of
 * src/hash_3d_anchored.cu:169,198, done once here instead of three times per iteration).
 * `step` is the 1-based step count (bias corrections 1 - beta^step are formed on the host). */
int f2n_adam_step(
  float * param, const float * grad, float * exp_avg, float * exp_avg_sq, uint16_t * shadow_f16,
  int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
  void * stream);

/* The loss of the training iteration -- src/main_functions/train_manager.cpp:78-96:
 *   color_loss = mean sqrt((colors - gt)^2 + 1e-4), var_loss = mean sqrt(var + 1e-2),
 *   loss = color_loss + var_weight * var_loss, sq_err_sum = sum (colors - gt)^2 (PSNR, :95-96).
 * colors, gt [n_rays, 3]; var [n_rays] (CustomOps::WeightVar).  Writes out4 = {loss, color_loss,
 * var_loss, sq_err_sum} and the gradients of loss w.r.t. colors / var (closed forms; multiply by the
 * upstream gradient).  partial: scratch of f2n_loss_workspace_floats(n_rays) floats.  Deterministic. */
int64_t f2n_loss_workspace_floats(int n_rays);
int f2n_loss_fwd(
  const float * colors, const float * gt, const float * var, int n_rays, float var_weight,
  float * d_colors, float * d_var, float * partial, float * out4, void * stream);

/* The same loss with per-ray weights and alpha targets (masked training; the sky / segmentation loss
 * of Urban Radiance Fields, Rematas et al., CVPR 2022, section 4.3, as a squared error).  The
 * reference has NO such loss: src/main_functions/train_manager.cpp:78-96 averages over every ray of
 * the batch.  This entry stands beside f2n_loss_fwd, which does not change.  Per-ray inputs, each
 * nullable:
 *   ray_weight [n_rays] m_r      null: 1 everywhere
 *   alpha      [n_rays] a_r      null: no alpha handling
 *   opacity    [n_rays] O_r      the rendered sum of weights; required when alpha is given and
 *                                opacity_weight != 0
 *   bg         [n_rays, 3]       the background the render blended in; required with alpha
 * With W = sum_r m_r, and W = 1 when that sum is not positive:
 *   gt'    = a gt + (1 - a) bg                                  (alpha given; else gt' = gt)
 *   colour = sum_r m_r sum_c sqrt((C - gt')^2 + 1e-4) / (3 W)
 *   var    = sum_r m_r sqrt(var_r + 1e-2) / W
 *   opac   = sum_r m_r (O_r - a_r)^2 / W                        (alpha and opacity given; else 0)
 *   loss   = colour + var_weight var + opacity_weight opac
 *   out6   = {loss, colour, var, opac, sum_r m_r sum_c (C - gt')^2, sum_r m_r}
 * out6[5] is the sum as it came out (0 when every ray is masked), not the divisor W.  An a_r = 0 ray
 * (sky) has the background itself as its colour target, so the colour term does not fight the
 * opacity term, which pulls O_r to 0; the squared error stays bounded where O reaches 0 or 1.
 * Writes the gradients of loss w.r.t. colors [n_rays, 3], var [n_rays] and, when alpha and opacity
 * are given, opacity [n_rays] (d_opacity is required then, ignored otherwise); gt, alpha, bg and
 * ray_weight get none.  A ray with m_r == 0 is not read beyond its weight: its terms and gradients
 * are exactly +0 whatever its colour holds.  partial: scratch of f2n_loss_sup_workspace_floats(n_rays)
 * floats.  Three launches (partials, tree, the 1 / W scaling of the gradients), no host read, no
 * atomics: deterministic.  The evaluation order is fixed in the header comment of loss_sup.hip.
 * A null among colors, gt, var, d_colors, d_var, partial, out6, a missing bg / opacity / d_opacity as
 * above, or n_rays <= 0: F2N_E_INVALID_ARG before any HIP work. */
int64_t f2n_loss_sup_workspace_floats(int n_rays);
int f2n_loss_sup_fwd(
  const float * colors, const float * gt, const float * var, const float * ray_weight,
  const float * alpha, const float * opacity, const float * bg, int n_rays, float var_weight,
  float opacity_weight, float * d_colors, float * d_var, float * d_opacity, float * partial,
  float * out6, void * stream);

/* ------------------------------------------------------------------ pixel masks --------------- */

/* Per-pixel validity masks of a set of E images of h x w pixels, as bits, and the training-batch
 * draw that only lands on valid pixels.  The reference has neither: Dataset::sample_random_rays --
 * src/dataset.cpp:150-171 -- draws (camera, row, col) with three randint calls over the whole image.
 *   f2n_mask_pack: mask [E, h, w] u8 (non-zero = valid) -> words [f2n_mask_words(E, h, w)] u32.
 *     Global pixel g = (e*h + i)*w + j is bit (g & 31) of word (g >> 5); unused bits of the last word
 *     are zero.  count: one int64 on the device, the number of valid pixels.  partial: scratch of
 *     f2n_mask_pack_workspace_words(E, h, w) u32.  One lane per pixel, a 64-lane ballot is two words;
 *     integer sums in a fixed tree; no atomics.
 *   f2n_draw_pixels_masked: n rays, one lane each.  Attempt a = 0 .. attempts-1 of ray r takes the
 *     four words (x0, x1, x2, x3) of Philox4x32-10 with key (seed_lo, seed_hi) and counter (r, a, 0, 0)
 *     (written out in full in the header comment of pixel_mask.hip), cam = mulhi(x0, E),
 *     i = mulhi(x1, h), j = mulhi(x2, w); the first attempt whose bit is set is kept.
 *       cam [n] i32, ij [n, 2] i32 (row, col), tries [n] i32: the attempts used, 1 .. attempts, or 0
 *       when every attempt missed -- cam and ij then hold the last attempt.
 *     Uniform over the valid pixels of the whole set (the camera is redrawn with the pixel); with an
 *     all-ones mask uniform over cameras and pixels, as src/dataset.cpp:150-171.
 * E, h, w <= 0 or E*h*w >= 2^36: the two size queries answer 0.  A null pointer, such sizes, n < 0 or
 * attempts outside 1 .. 64: F2N_E_INVALID_ARG before any HIP work; n == 0: F2N_OK. */
int64_t f2n_mask_words(int E, int h, int w);
int64_t f2n_mask_pack_workspace_words(int E, int h, int w);
int f2n_mask_pack(
  const uint8_t * mask, int E, int h, int w, uint32_t * words, int64_t * count, uint32_t * partial,
  void * stream);
int f2n_draw_pixels_masked(
  const uint32_t * bits, int E, int h, int w, uint32_t seed_lo, uint32_t seed_hi, int attempts,
  int32_t * cam, int32_t * ij, int32_t * tries, int n, void * stream);

/* ------------------------------------------------------------------ error map ----------------- */

/* Error-guided ray sampling: a per-image grid of running colour errors, its CDF, and a batch draw
 * that spends rays where the error is (the error map of instant-ngp, Mueller et al., SIGGRAPH 2022).
 * The reference has none of it: Dataset::sample_random_rays -- src/dataset.cpp:150-171 -- draws
 * uniformly over pixels.  Geometry, all integers: E images of h x w pixels, gh x gw cells per image,
 * 1 <= gh <= h, 1 <= gw <= w; pixel (e, i, j) lies in cell c = (e*gh + (i*gh)/h)*gw + (j*gw)/w, and
 * cell row a covers pixel rows ceil(a*h/gh) .. ceil((a+1)*h/gh) - 1 (columns alike).  Limits:
 * n_cells = E*gh*gw < 2^24, h*w < 2^31, E*h*w < 2^36.  Every entry below answers F2N_E_INVALID_ARG
 * before any HIP work for a null among its required pointers or sizes outside these limits; n == 0 is
 * F2N_OK where there is an n, and excuses no bad argument.  The evaluation orders are fixed in the
 * header comment of error_map.hip.
 *
 * Valid pixels per cell, beside src/dataset.cpp:150-171: counts [n_cells] i32 from the packed bits of
 * f2n_mask_pack; bits null = no mask, the closed form rows x cols.  One wavefront per cell, no
 * atomics. */
int f2n_mask_cell_counts(
  const uint32_t * bits, int E, int h, int w, int gh, int gw, int32_t * counts, void * stream);

/* The errors of one rendered batch into the accumulators, beside src/dataset.cpp:150-171.  Per ray,
 * in f64 on the f32 inputs: e_r = sum_c (C - gt')^2 with gt' = a gt + (1 - a) bg when alpha is given
 * (bg is then required), as in f2n_loss_sup_fwd.  A ray is skipped when ray_weight is given and its
 * m_r == 0, when e_r is not finite, and when cam / ij lie outside the set (no out-of-bounds access
 * whatever they hold).  Otherwise llrint(min(e_r, 4) 2^20) is added to acc_sum [n_cells] u64 and 1 to
 * acc_cnt [n_cells] u32 of the ray's cell: integer atomics, so the sums do not depend on order.  The
 * raw error is recorded, never the error times an importance weight.
 *   colors, gt [n, 3]; alpha, ray_weight [n] nullable; bg [n, 3]; cam [n] i32; ij [n, 2] i32 */
int f2n_error_map_accum(
  const float * colors, const float * gt, const float * alpha, const float * bg,
  const float * ray_weight, const int32_t * cam, const int32_t * ij, int n, int E, int h, int w,
  int gh, int gw, uint64_t * acc_sum, uint32_t * acc_cnt, void * stream);

/* Fold the accumulators into the map, beside src/dataset.cpp:150-171.  Per cell with cnt > 0:
 * value = f32(decay value + (1 - decay) sum / (2^20 cnt)) in f64; a cell no ray hit keeps its value;
 * every accumulator is left at zero.  decay in [0, 1] (NaN is invalid); 1 <= n_cells < 2^24. */
int f2n_error_map_apply(
  float * value, uint64_t * acc_sum, uint32_t * acc_cnt, int n_cells, float decay, void * stream);

/* The map's CDF, beside src/dataset.cpp:150-171.  mass[c] = clamp(llrint(value[c] 2^16), 1, 2^24)
 * counts[c] as u64 (a non-finite value counts as the floor 1; a negative count as 0); cdf [n_cells]
 * u64 is the inclusive prefix sum, below 2^60.  partial: scratch of
 * f2n_error_cdf_workspace_words(n_cells) u64 words (0 for n_cells outside 1 .. 2^24 - 1).  Three
 * launches -- tile sums, one workgroup over them, add-back -- and no workgroup waits on another. */
int64_t f2n_error_cdf_workspace_words(int n_cells);
int f2n_error_cdf(
  const float * value, const int32_t * counts, int n_cells, uint64_t * cdf, uint64_t * partial,
  void * stream);

/* The batch draw that follows the map, beside src/dataset.cpp:150-171 and f2n_draw_pixels_masked.
 * One lane per ray r; T = llrint(uniform_fraction 2^32), u = T / 2^32, uniform_fraction in [0, 1];
 * (x0 .. x3) = Philox4x32-10 with key (seed_lo, seed_hi) and counter (r, 0, 0, 0);
 * total = cdf[n_cells - 1].
 *   x3 < T (as u64) or total == 0: the masked draw exactly, attempts a with counter (r, a, 0, 0).
 *   else: t = mulhi64((x0 << 32) | x1, total), the cell is the first c with cdf[c] > t, and attempt a
 *     with counter (r, a, 1, 0) takes i = i0 + mulhi(y0, rows), j = j0 + mulhi(y1, cols) in that cell.
 *   The first attempt whose bit is set is kept; bits null = every pixel valid.
 *   cam, ij, tries as f2n_draw_pixels_masked (tries 0: every attempt missed, the last one stays).
 *   ray_weight [n] f32 = 1 / ((1 - u) q_c N / total + u) in f64, rounded once; q_c the quantised
 *     value of the kept pixel's cell, N = n_valid[0]; 0 where tries == 0.  The uniform pdf over the
 *     pdf used: expectation 1 under the draw, never above 1 / u, exactly 1 at u = 1 -- where cam, ij
 *     and tries equal f2n_draw_pixels_masked's bit for bit.
 * n_valid: one int64 on the device (PixelMask's count, or E*h*w without a mask); never read on the
 * host.  counts and value are those the cdf was made from.  attempts in 1 .. 64. */
int f2n_draw_pixels_guided(
  const uint32_t * bits, const int32_t * counts, const float * value, const uint64_t * cdf,
  const int64_t * n_valid, int E, int h, int w, int gh, int gw, uint32_t seed_lo, uint32_t seed_hi,
  int attempts, float uniform_fraction, int32_t * cam, int32_t * ij, int32_t * tries,
  float * ray_weight, int n, void * stream);

/* ------------------------------------------------------------------ learned background -------- */

/* A cube map of colour logits looked up by ray direction: the background a render blends behind the
 * field, learned from the images.  The reference has none: src/renderer.cpp:103-110 blends a
 * constant (rand in TRAIN, 0.5 otherwise).
 *   tex   [6, R, R, 3] f32 logits, 2 <= R <= 4096; face = 2*axis + (component < 0) of the largest
 *         |component| (ties: x before y before z), in-face coordinates the other two components
 *         divided by it, in axis order and without sign flips; bilinear, clamped to the face's edge
 *         (no filtering across faces); bg = sigmoid(logit).  A texture of zeros gives 0.5f exactly.
 *   dirs  [n_rays, 3], any length.  A ray whose largest |component| is not finite and positive
 *         (zero vector, NaN, inf) gets bg = 0.5 and contributes no gradient.
 *   bg    [n_rays, 3]
 * The evaluation order is fixed in the header comment of envmap.hip.  Every entry of this section
 * answers F2N_E_INVALID_ARG before any HIP work for a null pointer, R outside 2 .. 4096 or
 * n_rays < 0; n_rays == 0 is F2N_OK without a launch, and excuses no bad argument.  Directions
 * receive no gradient (pose optimisation through the sky is not covered).
 *   f2n_envmap_texels: 6*R*R, or 0 when R is out of range.
 *   f2n_envmap_fwd: one lane per ray, one launch. */
#define F2N_ENVMAP_SHIFT 48 /* the fixed point of the texture gradient: units of 2^-48 */
int64_t f2n_envmap_texels(int R);
int f2n_envmap_fwd(
  const float * dirs, const float * tex, int R, float * bg, int n_rays, void * stream);

/* The texture's gradient, beside src/renderer.cpp:103-110.  bg is f2n_envmap_fwd's saved output, the
 * geometry is recomputed.  Per ray and channel gl = d_bg * (bg * (1 - bg)) in f32; gl == 0 adds
 * nothing (an opaque ray issues no atomic); gl not finite adds nothing and sets bit 0 of flags [1]
 * i32; otherwise each of the four corners gets llrint(gl * w * 2^F2N_ENVMAP_SHIFT), the product
 * exact in f64, |.| capped at 2^62 (bit 1 of flags), added to acc [6*R*R*3] i64 by a 64-bit integer
 * atomicAdd when it is not 0.  Integer sums do not depend on their order: the gradient has the same
 * bits on every run.  The quantum is 2^-48 = 3.6e-15, the range of a texel's sum +-2^14.  acc must
 * hold zeros before the first call; flags is only ever or-ed into.  The host reads neither. */
int f2n_envmap_bwd(
  const float * dirs, const float * bg, const float * d_bg, int R, int64_t * acc, int32_t * flags,
  int n_rays, void * stream);

/* The sums as a gradient, beside src/renderer.cpp:103-110:
 * d_tex[i] (+)= (float)ldexp((double)acc[i], -F2N_ENVMAP_SHIFT) over the 6*R*R*3 elements, and
 * acc[i] = 0: ready for the next step without a memset, so a whole step stays capturable in a
 * hipGraph.  accumulate is 0 or 1 (anything else: F2N_E_INVALID_ARG). */
int f2n_envmap_grad_apply(int64_t * acc, int R, float * d_tex, int accumulate, void * stream);

/* ------------------------------------------------------------------ SSIM ---------------------- */

/* Structural similarity of B image pairs and its gradient, beside the reference's rgb_ssim --
 * scripts/eval.py:29-75, which runs in scipy on the host (its C++ scores a view by squared error
 * alone, src/main_functions/test.cpp:38-40): an 11-tap Gaussian (sigma 1.5, centred, normalised),
 * `valid` borders, k1 = 0.01, k2 = 0.03, max_val = 1, so c1 = 1e-4 and c2 = 9e-4.
 *   pred, gt [B, h, w, 3] f32, interleaved and contiguous; h, w >= 11; B <= 65535.
 *   Per channel, with mux, muy, Exx, Eyy, Exy the separable `valid` correlations of x, y, x^2, y^2, xy:
 *     sxx = Exx - mux^2, syy = Eyy - muy^2, sxy = Exy - mux muy
 *     S = (2 mux muy + c1)(2 sxy + c2) / ((mux^2 + muy^2 + c1)(sxx + syy + c2))
 *   ssim [B] = the mean of S over the (h-10)(w-10) 3 values of the map.
 *   clip = 1: the reference's clamps before S -- sxx, syy >= 0, |sxy| <= sqrt(sxx syy), sign kept: the
 *     metric.  clip = 0: the plain expression: the differentiable form.  The clamps act on rounding
 *     error only.
 *   map [B, h-10, w-10, 3] or null: S itself.
 *   gmaps [B, h-10, w-10, 9] or null, clip = 0 only: per channel c the partials of S by mux, Exx and
 *     Exy at index 3 c + {0, 1, 2}; what f2n_ssim_bwd reads.
 *   partial: scratch of f2n_ssim_workspace_doubles(B, h, w) doubles (one per tile; 0 for bad sizes).
 * A tile of F2N_SSIM_TILE^2 map pixels per workgroup, staged in LDS with its 10-pixel halo; each tile
 * writes one f64 partial and a second launch adds an image's partials in a fixed order in f64,
 * divides and rounds once.  No atomics: the same bits on every run.  The evaluation order is fixed in
 * the header comment of ssim.hip.  f2n_ssim_filter writes the eleven f32 taps (host only).
 * A null among pred, gt, ssim, partial, sizes outside the above, clip not 0 or 1, or gmaps with
 * clip = 1: F2N_E_INVALID_ARG before any HIP work; B == 0: F2N_OK without a launch. */
#define F2N_SSIM_TILE 16
int f2n_ssim_filter(float * taps11);
int64_t f2n_ssim_workspace_doubles(int B, int h, int w);
int f2n_ssim_fwd(
  const float * pred, const float * gt, int B, int h, int w, int clip, float * ssim, float * map,
  float * gmaps, double * partial, void * stream);

/* The gradient of the clip = 0 form by pred, beside scripts/eval.py:29-75 (which has none; the
 * reference's loss, src/main_functions/train_manager.cpp:78-96, has no structural term):
 *   d_pred(p) = d_ssim_b / n_b [ (f * gmu)(p) + 2 x(p) (f * gxx)(p) + y(p) (f * gxy)(p) ]
 * with * the `full` separable convolution over the map, n_b = (h-10)(w-10) 3, and gmaps those the
 * forward wrote for the same pred and gt.  A workgroup owns 16 x 16 input pixels and gathers: every
 * element of d_pred [B, h, w, 3] is written exactly once, no atomics, no memset; an image whose
 * d_ssim is 0 gets exact zeros.  gt receives no gradient.  Any null pointer or sizes as above:
 * F2N_E_INVALID_ARG; B == 0: F2N_OK. */
int f2n_ssim_bwd(
  const float * pred, const float * gt, const float * gmaps, const float * d_ssim, int B, int h,
  int w, float * d_pred, void * stream);

/* A training batch of n_patches patches of P x P pixels from E images of h x w, beside
 * src/dataset.cpp:150-171 and f2n_draw_pixels_masked.  One wavefront per patch b; attempt a takes
 * Philox4x32-10 with key (seed_lo, seed_hi) and counter (b, a, 2, 0), cam = mulhi(x0, E),
 * i0 = mulhi(x1, h - P + 1), j0 = mulhi(x2, w - P + 1).  bits (the words of f2n_mask_pack) or null:
 * with bits an attempt is kept only if all P^2 pixels are valid (lanes test pixels, a ballot
 * decides); without, the first attempt is kept.
 *   cam [n P^2] i32, ij [n P^2, 2] i32 (row, col): patch-major, row-major inside a patch -- pixel
 *   (u, v) of patch b is ray b P^2 + u P + v.  tries [n] i32: attempts used, or 0 when every attempt
 *   missed (the last one stays); patch_weight [n] f32: 1, or 0 where tries is 0.
 * Integers decide everything and nothing is read on the host.  A null among the outputs, n_patches
 * < 0, E < 1, h or w below 11, P outside 11 .. min(h, w), attempts outside 1 .. 64, E*h*w >= 2^36 or
 * n_patches P^2 >= 2^31: F2N_E_INVALID_ARG before any HIP work; n_patches == 0: F2N_OK. */
int f2n_draw_patches(
  const uint32_t * bits, int E, int h, int w, int n_patches, int P, uint32_t seed_lo,
  uint32_t seed_hi, int attempts, int32_t * cam, int32_t * ij, int32_t * tries,
  float * patch_weight, void * stream);

/* ------------------------------------------------------------------ robust loss --------------- */

/* Per-ray weights of a trimmed colour loss with patch-smoothed inlier masks (RobustNeRF, Sabour et
 * al., CVPR 2023, section 3.2), beside f2n_loss_sup_fwd, whose ray_weight they become.  The reference
 * has no such loss: src/main_functions/train_manager.cpp:78-96 averages over every ray of the batch.
 *   colors, target [n_rays, 3] f32; ray_weight [n_rays] m_r, null = 1.
 *   A ray is considered iff m_r != 0; one that is not gets weight +0 and omega 0, takes no part in any
 *   count and its colours are not read.  eps_r = (d0 d0 + d1 d1) + d2 d2 in f32 with d = colors -
 *   target, a non-finite eps becoming +inf.  N_c considered rays,
 *     k = min(N_c, max(1, (int64)ceil((double)quantile N_c))),
 *   T the k-th smallest eps among them, found exactly by radix selection on its bits (LDS histograms
 *   of integer atomics).  w0_r = isfinite(eps_r) && eps_r <= T: every tie at T is an inlier.
 *   P > 0: the rays are n_rays / P^2 patches of P x P pixels in the layout of f2n_draw_patches.
 *     W_r: over the considered pixels of the 3 x 3 window clipped to the patch, cnt of them and s with
 *       w0 = 1, W = cnt > 0 && (float)s >= box_thresh (float)cnt;
 *     R_block: the patch tiled from its top-left corner into nbhd x nbhd blocks (edge blocks are what
 *       is left), cnt considered pixels and s of them with W = 1, R = cnt > 0 && (float)s >=
 *       nbhd_thresh (float)cnt;
 *     omega_r = w0_r | W_r | R_block(r) for a considered ray.
 *   P = 0: scattered rays, omega = w0.
 *   weight_out [n_rays] = m_r where omega_r is set, else +0; omega_out [n_rays] u8 or null: omega
 *   itself; stats4 = {T, N_c, sum w0, sum omega}, the counts integer sums converted at the end.
 *   N_c == 0: T = 0 and every output is zero.
 *   workspace: f2n_robust_workspace_words(n_rays) u32 words (0 for an invalid n_rays).
 * One launch for P = 0, three for P > 0 (select, one workgroup per patch, the patches' counts); no
 * workgroup waits on another, nothing is read on the host, no float atomics: the same bits on every
 * run, and capturable in a hipGraph.  The arithmetic and its order are fixed in the header comment of
 * robust_mask.hip.  Valid: 1 <= n_rays < 2^24; P == 0, or 3 <= P <= 64 with n_rays % P^2 == 0 and
 * 1 <= nbhd <= P; quantile in (0, 1]; both thresholds in [0, 1] (NaN is invalid); colors, target,
 * weight_out, stats4 and workspace not null.  Anything else: F2N_E_INVALID_ARG before any HIP work. */
int64_t f2n_robust_workspace_words(int n_rays);
int f2n_robust_weights(
  const float * colors, const float * target, const float * ray_weight, int n_rays, int P, int nbhd,
  float quantile, float box_thresh, float nbhd_thresh, float * weight_out, uint8_t * omega_out,
  float * stats4, uint32_t * workspace, void * stream);

/* ------------------------------------------------------------------ localiser ----------------- */

/* The particle loop of Localizer::optimize_pose_by_random_search -- src/localizer.cpp:88-118 (per
 * particle a clone, three Eigen rotations copied to the device and three mm launches).
 *   pose    one pose, pose_ld floats (12 or 16, as f2n_gen_rays: rows 0..2 are [R | t])
 *   noise   [P,6] f32 standard normals: positions x, y, z then rotations x, y, z (row 0 is unused)
 *   sigma_pos_*  standard deviations of the position noise in the NeRF frame
 *   sigma_rot_*  standard deviations of the rotation noise about the NeRF axes, in DEGREES
 *   poses   [P,3,4]: particle 0 is the input pose unchanged; particle p > 0 has
 *           t += sigma_pos * n and R' = Mz My Mx R with theta = sigma_rot * n * pi/180.
 * As coded, not as intended: the reference builds each axis rotation as a column-major Eigen matrix
 * and reads its storage with from_blob as row-major (:104-113), so every M is the TRANSPOSE of the
 * textbook rotation, i.e. a rotation by -theta.  The noise is symmetric, so the distribution is the
 * same; this entry keeps the transposes so that a given noise tensor reproduces the reference's
 * poses.  One thread per particle. */
int f2n_perturb_poses(
  const float * pose, int pose_ld, const float * noise, float sigma_pos_x, float sigma_pos_y,
  float sigma_pos_z, float sigma_rot_x, float sigma_rot_y, float sigma_rot_z, float * poses, int P,
  void * stream);

/* The scoring tail of Localizer::evaluate_poses -- src/localizer.cpp:236-248 (clip, index and the
 * squared-error reduction as ATen launches on the image's device -- the GPU when the caller passes
 * the image there, as the ROS node does -- then a copy of the P losses to the host, where pow and
 * the normalisation run in f32).
 *   colors  [P,K,3] as rendered (not yet clipped), pose-major
 *   image   [h,w,3]; ij [K,2] i32 (row, col), clamped to the image
 *   loss    [P]: loss_p = sum_k mean_ch (clip(colors, 0, 1) - image[i_k, j_k])^2
 *   weights [P]: s_p = (K / (loss_p + 1e-6))^5, w_p = s_p / sum_q s_q
 *   workspace  P doubles of device memory, 8-byte aligned, contents undefined on entry and exit
 * One wavefront per pose walks the pixels in strides of 64 and reduces in a fixed order; the
 * normaliser is the sum of the P scores in index order.  No atomics: the same bits on every run.
 * Different from the reference: loss, s and the normaliser are accumulated in f64 and rounded once
 * to f32, so the result is the exact formula to a rounding, and it stays finite where the
 * reference's f32 pow overflows (loss below about 3e-6 gives s > 3e38, then inf / inf = NaN
 * weights). */
int f2n_pose_scores(
  const float * colors, const float * image, const int32_t * ij, float * loss, float * weights,
  double * workspace, int P, int K, int h, int w, void * stream);

/* Localizer::calc_average_pose with compute_rotation_average -- src/localizer.cpp:254-316 (per
 * particle a device-to-host copy of its rotation, Eigen on the host, a copy back).
 *   poses [P,3,4], weights [P] -> pose_out [3,4]; P >= 1 (there is no mean of nothing: P == 0 is
 *   F2N_E_INVALID_ARG here, where the two entries above accept it and do nothing)
 * position = sum_p w_p t_p.  Rotation, as coded in the reference: every matrix to a quaternion by
 * Eigen's branches (trace > 0, else the largest diagonal element); a quaternion whose dot product
 * with particle 0's is negative is flipped; the mean is UNWEIGHTED (cumulative /= size; the weights
 * vector is filled and never used, :288-304); the mean is normalised and turned back into a matrix.
 * The reference's memcpy into a column-major Eigen matrix and from_blob out of one transpose twice
 * (conjugate quaternions in, conjugate out), which cancels: this is the plain computation.
 * f64 inside, as the reference; one workgroup, every sum in index order. */
int f2n_average_pose(
  const float * poses, const float * weights, float * pose_out, int P, void * stream);

#ifdef __cplusplus
}
#endif

#endif /* F2NERF_HIP_H_ */
