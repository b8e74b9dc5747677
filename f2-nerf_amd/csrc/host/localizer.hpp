// localizer.hpp -- Localizer: camera pose from one image and a trained field, by scoring perturbed
// poses against the image (particles) or by Adam on the pose through the render.
//
// Public surface of reference src/localizer.hpp:9-64 (Particle, LocalizerParam, Localizer with
// render_image / optimize_pose_by_random_search / optimize_pose_by_differential / world2camera /
// camera2world / calc_average_pose / radius / infer_height / infer_width).  The reference surrounds
// one render of P*K rays with host-driven work: a get_rays_from_pose per pose, half a dozen ATen
// launches to score the colours and a copy of the P losses to the host for pow and normalisation,
// per particle three rotations copied up and one copied down (src/localizer.cpp:64-128,176-316).  Here the particles stay on the device from the noise to the
// averaged pose: f2n_perturb_poses, one f2n_gen_rays launch, the fused render, f2n_pose_scores,
// f2n_average_pose.  The forms that return tensors read nothing back; the forms with the
// reference's signatures (std::vector<Particle>) read the P weights once.
#pragma once

#include <array>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "renderer.hpp"

struct Particle
{
  torch::Tensor pose;  // (3, 4)
  float weight;
};

struct LocalizerParam
{
  std::string train_result_dir;
  int32_t render_pixel_num = 256;
  float noise_position_x = 0.025f;
  float noise_position_y = 0.025f;
  float noise_position_z = 0.025f;
  float noise_rotation_x = 2.5f;
  float noise_rotation_y = 2.5f;
  float noise_rotation_z = 2.5f;
  int32_t resize_factor = 1;
  // render particles and images with the one-kernel inference path (RendererOptions::one_pass); not
  // part of inference_params.yaml
  bool one_pass = false;
  // with one_pass: RendererOptions::one_pass_head (0 = one ray per wavefront, -1 = whole rays eight
  // to a wavefront, a positive multiple of 64 = head then tail)
  int one_pass_head = 0;
  // lens distortion (k1, k2, p1, p2) of the camera whose images are localised, the columns of
  // cams_meta.tsv (src/dataset.cpp:59-63): pose_rays and render_image undistort their pixels in the
  // ray kernel, so the image handed in is the raw one.  They act on normalised coordinates:
  // resize_factor leaves them alone.  Zeros = pinhole.  Not part of inference_params.yaml either.
  std::array<float, 4> dist_params = {0.f, 0.f, 0.f, 0.f};
  // optimize_pose_by_differential receives the encoding's true derivative instead of the reference's
  // point gradient (Hash3DAnchoredOptions::exact_point_grad, set on the renderer's field in init).
  // The gradient is about a quarter the size: a learning rate tuned without it does not carry over.
  // Not part of inference_params.yaml either.
  bool exact_ray_grad = false;
  // Level of detail of every render the Localizer makes: the coarse-to-fine progress alpha in
  // [1, n_levels] handed to Renderer::set_coarse_to_fine in init (a wide, smooth basin for the
  // particles and the pose optimiser, and fewer levels to gather).  < 0: off, the renderer's weights
  // are left as they are.  Not part of inference_params.yaml either.
  double level_alpha = -1.;
};

namespace f2n
{

// Thin wrappers of the three C-ABI entries (allocation of the outputs, the current stream).
// pose [3,4] or [4,4], noise [P,6], sigmas = {pos x, y, z (NeRF frame), rot x, y, z (degrees)}
// -> poses [P,3,4]
Tensor perturb_poses(const Tensor & pose, const Tensor & noise, const std::array<float, 6> & sigmas);
// colors [P,K,3] (or [P*K,3] with K taken from ij), image [h,w,3], ij [K,2] i32 -> {loss, weights} [P]
std::pair<Tensor, Tensor> pose_scores(const Tensor & colors, const Tensor & image, const Tensor & ij);
// poses [P,3,4], weights [P] -> [3,4]
Tensor average_pose(const Tensor & poses, const Tensor & weights);

}  // namespace f2n

class Localizer
{
  using Tensor = torch::Tensor;

public:
  // What evaluate_poses_full returns: everything on the device.
  struct PoseScores
  {
    Tensor weights;  // [P]
    Tensor loss;     // [P]
    Tensor colors;   // [P,K,3] as rendered (not clipped)
    Tensor ij;       // [K,2] int32, the pixels that were rendered
  };

  Localizer() = default;
  // inference_params.yaml and checkpoints/latest/renderer.pt of param.train_result_dir
  // (src/localizer.cpp:13-62)
  explicit Localizer(const LocalizerParam & param);
  // An existing renderer and the values the file would give: intrinsic [3,3], the training image
  // size, the normalising centre [3] and radius.  resize_factor applies to both forms.
  Localizer(
    const LocalizerParam & param, std::shared_ptr<Renderer> renderer, const Tensor & intrinsic,
    int height, int width, const Tensor & center, float radius);

  Tensor render_image(const Tensor & pose);

  // initial_pose [3,4] (or [4,4]), image [infer_height, infer_width, 3].  noise: [particle_num, 6]
  // standard normals, undefined = drawn on the device.
  std::vector<Particle> optimize_pose_by_random_search(
    Tensor initial_pose, Tensor image_tensor, int64_t particle_num, float noise_coeff,
    const Tensor & noise = {});
  // the same without a host read: {poses [P,3,4], weights [P]}
  std::pair<Tensor, Tensor> random_search(
    const Tensor & initial_pose, const Tensor & image_tensor, int64_t particle_num,
    float noise_coeff, const Tensor & noise = {});

  std::vector<Tensor> optimize_pose_by_differential(
    Tensor initial_pose, Tensor image_tensor, int64_t iteration_num);

  Tensor world2camera(const Tensor & pose_in_world);
  Tensor camera2world(const Tensor & pose_in_camera);

  static Tensor calc_average_pose(const std::vector<Particle> & particles);
  static Tensor calc_average_pose(const Tensor & poses, const Tensor & weights);

  // poses [P,3,4] (or [P,4,4]); ij [K,2] int32 (row, col), undefined = render_pixel_num pixels drawn
  // without replacement on the device.  Returns the weights [P] on the device.
  Tensor evaluate_poses(const Tensor & poses, const Tensor & image, const Tensor & ij = {});
  PoseScores evaluate_poses_full(const Tensor & poses, const Tensor & image, const Tensor & ij = {});
  // the rays evaluate_poses renders: pixel k under pose p is ray p*K + k
  Rays pose_rays(const Tensor & poses, const Tensor & ij);

  // {pos x, y, z, rot x, y, z} in the NeRF frame for f2n_perturb_poses (src/localizer.cpp:74-79)
  std::array<float, 6> noise_sigmas(float noise_coeff) const;

  // LocalizerParam::level_alpha for a Localizer that exists already; < 0 clears the renderer's weights
  void set_level_alpha(double alpha);

  float radius() const { return radius_; }
  int infer_height() const { return infer_height_; }
  int infer_width() const { return infer_width_; }
  std::shared_ptr<Renderer> renderer() const { return renderer_; }
  const Tensor & intrinsic() const { return intrinsic_; }

private:
  void init(const Tensor & intrinsic, int height, int width, const Tensor & center, float radius);

  LocalizerParam param_;

  std::shared_ptr<Renderer> renderer_;

  Tensor axes_;  // [3,3]: the NeRF axes in the world frame

  int infer_height_ = 0, infer_width_ = 0;
  Tensor intrinsic_;
  Tensor dist_;  // [4] on the device; undefined when param_.dist_params is all zeros
  Tensor center_;
  float radius_ = 1.f;
};
