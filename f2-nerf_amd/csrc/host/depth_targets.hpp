// depth_targets.hpp -- depth targets for the line-of-sight losses (CustomOps::DepthSight): a point
// cloud splatted once into sparse per-camera depth maps, and the per-batch lookup of a ray's target.
//
// The reference reads no range data (its dataset holds images, poses and intrinsics only,
// src/dataset.cpp:59-63); the lookup is the index arithmetic its Dataset::sample_random_rays applies
// to colours (src/dataset.cpp:150-171), applied to depth.
#pragma once

#include "common.hpp"

namespace f2n
{

// f2n_depth_splat: points [n,3] in the frame of the poses, cam_idx [n] i32 (point i is seen by camera
// cam_idx[i]; out-of-range values are skipped), poses [E,3,4] or [E,4,4], intrinsics [E,3,3], dist
// [E,4] (k1, k2, p1, p2) or undefined (pinhole) -> depth [E,h,w] f32: per pixel the smallest distance
// |p - t_cam| ALONG THE RAY of the points that fall into it, 0 where none does.  The same bits on
// every run; no sync.  Distances are in the units of the poses: feed normalised poses and points.
Tensor splat_depth(
  const Tensor & points, const Tensor & cam_idx, const Tensor & poses, const Tensor & intrinsics,
  const Tensor & dist, int h, int w);

// depth_maps [E,h,w], cam_idx [n], ij [n,2] (row, col) -> [n]: depth_maps[cam, i, j] of every ray, the
// flat index (cam * h + i) * w + j of src/dataset.cpp:150-171.  A ray whose camera, row or column lies
// outside [0,E) x [0,h) x [0,w) gets 0 = no return (checked per component, on the device: an index that
// is out of range in one component is never read as another pixel or camera).  ATen only.
Tensor gather_depth(const Tensor & depth_maps, const Tensor & cam_idx, const Tensor & ij);

}  // namespace f2n
