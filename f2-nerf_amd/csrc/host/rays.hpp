// rays.hpp -- pixel -> world-space ray generation (reference src/rays.hpp:7-13, src/rays.cpp:7-28)
// and the two callers that feed the renderer: a view's pixel grid (src/dataset.cpp:128-146,
// src/renderer.cpp:153-172) and the random training batch (src/dataset.cpp:150-171).
#pragma once

#include <torch/torch.h>

#include <tuple>

struct alignas(32) Rays
{
  torch::Tensor origins;
  torch::Tensor dirs;
};

// Gradients: get_rays_from_pose and get_view_rays are differentiable in the pose when grad mode is on
// and pose.requires_grad() (the reference's Localizer optimises a [3,4] pose through render_image,
// src/localizer.cpp:142-167): the backward (f2n_gen_rays_bwd) returns d(pose) in the pose's own shape
// ([B,3,4] / [B,4,4], or [3,4] / [4,4] through get_view_rays), row 3 of a [4,4] pose zero, the sum
// over the rays in a fixed order.  The intrinsics are constants there: only
// get_rays_from_calibrated_cameras hands them a gradient.
//
// Lens distortion: every function takes an optional `dist` holding (k1, k2, p1, p2) per camera, the
// columns CamsMeta::dist_params reads from cams_meta.tsv (src/dataset.cpp:59-63; the reference's
// src/rays.cpp:7-28 ignores them).  Defined: the pixel is undistorted in the kernel
// (f2n_gen_rays_dist, 8 Newton steps) and the backward is f2n_gen_rays_dist_bwd.  Undefined: the
// pinhole entry points, as before.  A camera whose four numbers are zero gives the pinhole bits
// either way.  Like the intrinsics, `dist` receives a gradient from
// get_rays_from_calibrated_cameras alone; every other function detaches it.

// pose [B,3,4] (or [B,4,4]), intrinsic [B,3,3], ij [N,2] = (row, col), float or integer; B == 1 or
// B == N.  Pixel centres (+0.5), camera looks down -z, y up.  One kernel (f2n_gen_rays).
// dist: [B,4].
Rays get_rays_from_pose(
  const torch::Tensor & pose, const torch::Tensor & intrinsic, const torch::Tensor & ij,
  const torch::Tensor & dist = {});

// The same K pixels under each of P poses that share one camera, pose-major (ray p*K + k is pixel k
// under pose p): what the reference's Localizer::evaluate_poses builds with one get_rays_from_pose
// per pose and two cats (src/localizer.cpp:218-231), as one f2n_gen_rays launch with a per-ray
// camera index.  poses [P,3,4] (or [P,4,4]), intrinsic [3,3], ij [K,2] int32.  Not differentiated.
// dist: [4], the one camera's.
Rays get_rays_from_poses(
  const torch::Tensor & poses, const torch::Tensor & intrinsic, const torch::Tensor & ij,
  const torch::Tensor & dist = {});

// All h*w pixels of one view in row-major order, without materialising the pixel grid
// (Dataset::get_rays_from_pose(idx) / Renderer::render_image of the reference).
// dist: [4] or [1,4].
Rays get_view_rays(
  const torch::Tensor & pose, const torch::Tensor & intrinsic, int h, int w,
  const torch::Tensor & dist = {});

// Dataset::sample_random_rays (src/dataset.cpp:150-171) with everything on the device: camera and
// pixel indices are drawn there, each ray reads its own camera from the pose / intrinsic tables
// (no index_select, no host randint + copy).  images: optional [E, h, w, 3] for the ground truth.
// Not differentiated: the rays carry no gradient to `poses` (training samples are data).
// dist: [E,4], one row per image.
// Returns {rays, gt_colors [n,3] (undefined without images), cam_indices [n] i32}.
std::tuple<Rays, torch::Tensor, torch::Tensor> sample_random_rays(
  const torch::Tensor & poses, const torch::Tensor & intrinsics, int h, int w, int64_t batch_size,
  const torch::Tensor & images = {}, const torch::Tensor & dist = {});

// The rays of a batch in which ray r comes from camera cam_idx[r] and pixel ij[r]: the launch that
// sample_random_rays makes (the same bits), and differentiable in the poses when grad mode is on and
// poses.requires_grad().  poses [E,3,4] (or [E,4,4]), intrinsics [E,3,3], cam_idx [n] i32 in 0..E-1,
// ij [n,2] i32, dist [E,4].  The backward is f2n_cam_pose_grad: d(poses) in the poses' shape, one sum
// per camera in a fixed order, without float atomics and without a host read (a training step that
// refines its poses stays capturable).  A cam_idx that is not known to be sorted gets its order from a
// stable sort; pass sorted = true when it is non-decreasing, and no permutation is made at all.
// Undefined gradients of the origins or the directions count as zeros.
Rays get_rays_from_cameras(
  const torch::Tensor & poses, const torch::Tensor & intrinsics, const torch::Tensor & cam_idx,
  const torch::Tensor & ij, const torch::Tensor & dist = {}, bool sorted = false);

// get_rays_from_cameras with the calibration as a variable: the one function here whose intrinsics
// and `dist` receive a gradient (self-calibration, intrinsics_refiner.hpp).  The rays are the bits of
// get_rays_from_cameras.  Under grad mode the backward forms, each only if its input requires it,
//   d(poses)       f2n_cam_pose_grad, the bits of get_rays_from_cameras' backward
//   d(intrinsics)  [E,3,3], zero outside [0][0], [1][1], [0][2], [1][2]   } f2n_cam_intr_grad, one
//   d(dist)        in dist's shape; an undefined dist (pinhole) has none   } launch for both
// over one sort and one cam_start.  Without a calibration that requires a gradient it is
// get_rays_from_cameras.
Rays get_rays_from_calibrated_cameras(
  const torch::Tensor & poses, const torch::Tensor & intrinsics, const torch::Tensor & dist,
  const torch::Tensor & cam_idx, const torch::Tensor & ij, bool sorted = false);

// The camera and pixel draw that the refiners' sample_random_rays share: cameras drawn on the device
// and SORTED before the pixels are drawn, so the per-camera sums of the backward need no permutation.
// cam_idx [n] i32 and ij [n,2] i32, when defined, replace the draws; a given cam_idx need not be
// sorted (sorted = false then).
struct CameraBatch
{
  torch::Tensor cam;  // [n] i32
  torch::Tensor ij;   // [n,2] i32
  bool sorted;
};
CameraBatch draw_camera_batch(
  int64_t n_cameras, int h, int w, int64_t batch_size, const torch::Tensor & cam_idx,
  const torch::Tensor & ij, const torch::Device & device);
// images [E,h,w,3] at the batch's pixels -> [n,3] on the batch's device; undefined without images
torch::Tensor gather_colors(const torch::Tensor & images, const CameraBatch & b, int h, int w);

// The forward model, world point -> pixel (f2n_project_points): points [N,3]; pose [B,3,4] (or
// [B,4,4], or one [3,4] / [4,4]), intrinsic [B,3,3] (or [3,3]), dist [B,4] (or [4]; undefined =
// pinhole); B == 1 or B == N.  Returns {pix [N,2] f32 continuous (row, col) with pixel (i, j) centred
// at (i + .5, j + .5), valid [N] i32: 1 iff the point lies strictly in front of its camera}.  No
// image-bounds test.  Not differentiated.
std::tuple<torch::Tensor, torch::Tensor> project_points(
  const torch::Tensor & points, const torch::Tensor & pose, const torch::Tensor & intrinsic,
  const torch::Tensor & dist = {});
