// bindings.cpp -- pybind11 view of the C++/LibTorch operator surface, for bench.py and tests/.
// Nothing here computes: every function forwards to the classes in this directory, which in turn
// call the C ABI of libf2nerf_hip.so.
#include <torch/extension.h>

#include "depth_targets.hpp"
#include "env_map.hpp"
#include "error_map.hpp"
#include "fused_adam.hpp"
#include "hash_3d_anchored.hpp"
#include "intrinsics_refiner.hpp"
#include "kernel_timer.hpp"
#include "localizer.hpp"
#include "mesh.hpp"
#include "occupancy_grid.hpp"
#include "pixel_mask.hpp"
#include "points_sampler.hpp"
#include "pose_refiner.hpp"
#include "ragged_ops.hpp"
#include "rays.hpp"
#include "scene_files.hpp"
#include "renderer.hpp"
#include "sh_shader.hpp"
#include "ssim.hpp"

namespace py = pybind11;
using torch::Tensor;

namespace
{

torch::Device parse_device(const std::string & s)
{
  return s.empty() ? f2n::default_device() : torch::Device(s);
}

Hash3DAnchoredOptions field_options(
  int64_t n_levels, int64_t n_channels, int64_t log2_table, int64_t level_stride,
  const std::string & device)
{
  Hash3DAnchoredOptions o;
  o.n_levels = n_levels;
  o.n_channels = n_channels;
  o.log2_table = log2_table;
  o.level_stride = level_stride;
  o.device = parse_device(device);
  return o;
}

py::dict named_params(torch::nn::Module & m)
{
  py::dict d;
  for (auto & kv : m.named_parameters()) d[py::str(kv.key())] = kv.value();
  return d;
}

c10::optional<Tensor> grad_or_none(const Tensor & t)
{
  return t.grad().defined() ? c10::optional<Tensor>(t.grad()) : c10::nullopt;
}

Tensor opt_tensor(const c10::optional<Tensor> & t) { return t.has_value() ? *t : Tensor(); }

RunningMode parse_mode(const std::string & m)
{
  if (m == "train" || m == "TRAIN") return RunningMode::TRAIN;
  if (m == "validate" || m == "VALIDATE") return RunningMode::VALIDATE;
  throw std::invalid_argument("mode must be 'train' or 'validate'");
}

py::tuple result_tuple(const RenderResult & r)
{
  return py::make_tuple(r.colors, r.depths, r.weights, r.idx_start_end);
}

c10::optional<Tensor> tensor_or_none(const Tensor & t)
{
  return t.defined() ? c10::optional<Tensor>(t) : c10::nullopt;
}

// What every Renderer.train_step* entry does with its arguments: one f2n::train_step, the GIL
// released (loss.backward() runs the autograd engine, which must not be entered holding it).
f2n::TrainStepResult run_train_step(
  Renderer & r, const Tensor & o, const Tensor & d, const Tensor & emb_idx, const Tensor & gt,
  float var_loss_weight, const c10::optional<Tensor> & noise, const c10::optional<Tensor> & bg,
  bool backward, float dist_loss_weight, const c10::optional<Tensor> & depth_target,
  const f2n::DepthLossOptions & depth_loss, const f2n::RaySupervision & sup = {},
  const f2n::PatchLoss & patch = {}, const f2n::RobustLoss & robust = {})
{
  const f2n::LossTerms terms{
    var_loss_weight, dist_loss_weight, opt_tensor(depth_target), depth_loss, sup, patch, robust};
  py::gil_scoped_release no_gil;
  return f2n::train_step(r, o, d, emb_idx, gt, terms, opt_tensor(noise), opt_tensor(bg), backward);
}

struct AdamHandle
{
  std::shared_ptr<torch::optim::Optimizer> opt;
};

py::list particle_list(const std::vector<Particle> & particles)
{
  py::list l;
  for (const Particle & p : particles) l.append(py::make_tuple(p.pose, p.weight));
  return l;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
  m.doc() = "F2-NeRF rendering hot path: LibTorch C++ operator surface over libf2nerf_hip.so";
  m.attr("MAX_SAMPLE_PER_RAY") = MAX_SAMPLE_PER_RAY;

  // ---- free operators (FlexOps / CustomOps / TruncExp) ------------------------------------------
  m.def("flex_sum", &FlexOps::Sum, "FlexOps::Sum(val, idx_start_end)");
  m.def("flex_accumulate_sum", &FlexOps::AccumulateSum, "FlexOps::AccumulateSum");
  m.def("weight_var", &CustomOps::WeightVar, "CustomOps::WeightVar");
  m.def("weight_dist", &CustomOps::WeightDist, "CustomOps::WeightDist(weights, t, dt, idx_start_end)");
  m.def(
    "depth_sight", &CustomOps::DepthSight, py::arg("weights"), py::arg("t"), py::arg("dt"),
    py::arg("idx_start_end"), py::arg("z"), py::arg("eps"),
    "CustomOps::DepthSight -> [n_rays, 3] (empty space, near surface, expected depth)");
  m.def(
    "splat_depth",
    [](const Tensor & points, const Tensor & cam_idx, const Tensor & poses, const Tensor & intr,
       const c10::optional<Tensor> & dist, int h, int w) {
      return f2n::splat_depth(points, cam_idx, poses, intr, opt_tensor(dist), h, w);
    },
    py::arg("points"), py::arg("cam_idx"), py::arg("poses"), py::arg("intrinsics"),
    py::arg("dist") = py::none(), py::arg("h"), py::arg("w"),
    "f2n_depth_splat -> depth [E,h,w]: per pixel the smallest ray distance |p - t_cam|, 0 = no return");
  m.def(
    "gather_depth", &f2n::gather_depth, py::arg("depth_maps"), py::arg("cam_idx"), py::arg("ij"),
    "depth_maps[cam_idx, ij[:,0], ij[:,1]] -> [n]: a batch's depth targets");
  m.def("scatter_add", &CustomOps::ScatterAdd, "CustomOps::ScatterAdd(emb, idx, to_add)");
  m.def("scatter_idx", &CustomOps::ScatterIdx, "CustomOps::ScatterIdx(n_all, idx_start_end, emb_idx)");
  m.def("trunc_exp", [](const Tensor & x) { return torch::autograd::TruncExp::apply(x)[0]; });
  m.def(
    "composite",
    [](const Tensor & field_out, const Tensor & rgb, const Tensor & dt, const Tensor & t,
       const Tensor & idx, const Tensor & bg) {
      auto o = f2n::composite(field_out, rgb, dt, t, idx, bg);
      return py::make_tuple(o.colors, o.depths, o.weights);
    });
  // dist: optional (k1, k2, p1, p2) per camera, see rays.hpp; None = pinhole
  m.def(
    "get_rays_from_pose",
    [](const Tensor & pose, const Tensor & intr, const Tensor & ij,
       const c10::optional<Tensor> & dist) {
      Rays r = get_rays_from_pose(pose, intr, ij, opt_tensor(dist));
      return py::make_tuple(r.origins, r.dirs);
    },
    py::arg("pose"), py::arg("intrinsic"), py::arg("ij"), py::arg("dist") = py::none());
  m.def(
    "get_rays_from_poses",
    [](const Tensor & poses, const Tensor & intr, const Tensor & ij,
       const c10::optional<Tensor> & dist) {
      Rays r = get_rays_from_poses(poses, intr, ij, opt_tensor(dist));
      return py::make_tuple(r.origins, r.dirs);
    },
    py::arg("poses"), py::arg("intrinsic"), py::arg("ij"), py::arg("dist") = py::none());
  m.def(
    "get_view_rays",
    [](const Tensor & pose, const Tensor & intr, int h, int w, const c10::optional<Tensor> & dist) {
      Rays r = get_view_rays(pose, intr, h, w, opt_tensor(dist));
      return py::make_tuple(r.origins, r.dirs);
    },
    py::arg("pose"), py::arg("intrinsic"), py::arg("h"), py::arg("w"),
    py::arg("dist") = py::none());
  m.def(
    "sample_random_rays",
    [](const Tensor & poses, const Tensor & intr, int h, int w, int64_t n,
       const c10::optional<Tensor> & images, const c10::optional<Tensor> & dist) {
      auto [r, gt, cam] =
        sample_random_rays(poses, intr, h, w, n, opt_tensor(images), opt_tensor(dist));
      return py::make_tuple(r.origins, r.dirs, gt, cam);
    },
    py::arg("poses"), py::arg("intrinsics"), py::arg("h"), py::arg("w"), py::arg("batch_size"),
    py::arg("images") = py::none(), py::arg("dist") = py::none());
  m.def(
    "get_rays_from_cameras",
    [](const Tensor & poses, const Tensor & intr, const Tensor & cam_idx, const Tensor & ij,
       const c10::optional<Tensor> & dist, bool sorted) {
      Rays r = get_rays_from_cameras(poses, intr, cam_idx, ij, opt_tensor(dist), sorted);
      return py::make_tuple(r.origins, r.dirs);
    },
    py::arg("poses"), py::arg("intrinsics"), py::arg("cam_idx"), py::arg("ij"),
    py::arg("dist") = py::none(), py::arg("sorted") = false,
    "rays of a batch with one camera per ray, differentiable in the poses (f2n_cam_pose_grad)");
  m.def(
    "pose_compose",
    [](const Tensor & base, const Tensor & delta, const c10::optional<Tensor> & fixed) {
      return pose_compose(base, delta, opt_tensor(fixed));
    },
    py::arg("base"), py::arg("delta"), py::arg("fixed") = py::none(),
    "f2n_pose_compose: R' = Exp(omega) R, t' = t + tau -> [E,3,4], differentiable in delta");
  m.def(
    "pose_compose_bwd",
    [](const Tensor & base, const Tensor & delta, const c10::optional<Tensor> & fixed,
       const Tensor & d_out) { return pose_compose_bwd(base, delta, opt_tensor(fixed), d_out); },
    py::arg("base"), py::arg("delta"), py::arg("fixed"), py::arg("d_out"),
    "f2n_pose_compose_bwd: d_out [E,3,4] -> d_delta [E,6]");
  m.def(
    "get_rays_from_calibrated_cameras",
    [](const Tensor & poses, const Tensor & intr, const c10::optional<Tensor> & dist,
       const Tensor & cam_idx, const Tensor & ij, bool sorted) {
      Rays r = get_rays_from_calibrated_cameras(poses, intr, opt_tensor(dist), cam_idx, ij, sorted);
      return py::make_tuple(r.origins, r.dirs);
    },
    py::arg("poses"), py::arg("intrinsics"), py::arg("dist"), py::arg("cam_idx"), py::arg("ij"),
    py::arg("sorted") = false,
    "get_rays_from_cameras, differentiable in the poses (f2n_cam_pose_grad) and in the intrinsics "
    "and dist (f2n_cam_intr_grad)");
  m.def(
    "intr_compose",
    [](const Tensor & base_K, const c10::optional<Tensor> & base_dist, const Tensor & gamma,
       const Tensor & group, const c10::optional<Tensor> & learn) {
      auto [K, dist] = intr_compose(base_K, opt_tensor(base_dist), gamma, group, opt_tensor(learn));
      return py::make_tuple(K, dist);
    },
    py::arg("base_K"), py::arg("base_dist"), py::arg("gamma"), py::arg("group"),
    py::arg("learn") = py::none(),
    "f2n_intr_compose: a shared calibration correction per camera group -> (K' [E,3,3], "
    "dist' [E,4]), differentiable in gamma");
  m.def(
    "intr_compose_bwd",
    [](const Tensor & base_K, const c10::optional<Tensor> & base_dist, const Tensor & gamma,
       const Tensor & group, const c10::optional<Tensor> & learn, const c10::optional<Tensor> & d_K,
       const c10::optional<Tensor> & d_dist) {
      return intr_compose_bwd(
        base_K, opt_tensor(base_dist), gamma, group, opt_tensor(learn), opt_tensor(d_K),
        opt_tensor(d_dist));
    },
    py::arg("base_K"), py::arg("base_dist"), py::arg("gamma"), py::arg("group"), py::arg("learn"),
    py::arg("d_K"), py::arg("d_dist"),
    "f2n_intr_compose_bwd: d_K [E,3,3], d_dist [E,4] -> d_gamma [G,8]");
  m.def(
    "envmap_query", &f2n::envmap_query, py::arg("dirs"), py::arg("texture"),
    "f2n_envmap_fwd: dirs [n,3], texture [6,R,R,3] logits -> bg [n,3]; no autograd");
  m.def(
    "envmap_bwd", &f2n::envmap_bwd, py::arg("dirs"), py::arg("bg"), py::arg("d_bg"), py::arg("R"),
    py::arg("acc"), py::arg("flags"),
    "f2n_envmap_bwd: adds d_bg's fixed-point contributions to acc (int64 [6*R*R*3]), ors into "
    "flags (int32 [1])");
  m.def(
    "envmap_grad_apply", &f2n::envmap_grad_apply, py::arg("acc"), py::arg("R"), py::arg("d_tex"),
    py::arg("accumulate") = false,
    "f2n_envmap_grad_apply: d_tex (+)= acc * 2^-48, acc = 0");
  m.def(
    "project_points",
    [](const Tensor & points, const Tensor & pose, const Tensor & intr,
       const c10::optional<Tensor> & dist) {
      return project_points(points, pose, intr, opt_tensor(dist));
    },
    py::arg("points"), py::arg("pose"), py::arg("intrinsic"), py::arg("dist") = py::none(),
    "f2n_project_points -> (pix [N,2] (row, col), valid [N] i32)");
  m.def("train_loss", &f2n::train_loss, py::arg("colors"), py::arg("gt_colors"), py::arg("var"),
        py::arg("var_loss_weight"));
  m.def(
    "train_loss_sup",
    [](const Tensor & colors, const Tensor & gt, const Tensor & var,
       const c10::optional<Tensor> & opacity, const c10::optional<Tensor> & ray_weight,
       const c10::optional<Tensor> & alpha, const c10::optional<Tensor> & bg, float var_loss_weight,
       float opacity_weight) {
      return f2n::train_loss_sup(
        colors, gt, var, opt_tensor(opacity), opt_tensor(ray_weight), opt_tensor(alpha),
        opt_tensor(bg), var_loss_weight, opacity_weight);
    },
    py::arg("colors"), py::arg("gt_colors"), py::arg("var"), py::arg("opacity") = py::none(),
    py::arg("ray_weight") = py::none(), py::arg("alpha") = py::none(),
    py::arg("bg_color") = py::none(), py::arg("var_loss_weight") = 0.f,
    py::arg("opacity_weight") = 0.f,
    "f2n_loss_sup_fwd as one autograd node -> [6] = (loss, colour, var, opacity term, weighted "
    "squared error, sum of the ray weights); see f2n::train_loss_sup");
  py::class_<f2n::PixelMask>(m, "PixelMask")
    .def_static("from_mask", &f2n::PixelMask::from_mask, py::arg("mask"),
                "mask [E,h,w] (or [h,w]) uint8 / bool on the GPU, non-zero = valid (f2n_mask_pack)")
    .def_readonly("bits", &f2n::PixelMask::bits, "[ceil(E*h*w / 32)] int32 holding the uint32 words")
    .def_readonly("count", &f2n::PixelMask::count, "[1] int64 on the device: valid pixels")
    .def_readonly("E", &f2n::PixelMask::E)
    .def_readonly("h", &f2n::PixelMask::h)
    .def_readonly("w", &f2n::PixelMask::w);
  m.def(
    "draw_pixels_masked",
    [](const f2n::PixelMask & mask, int64_t n, uint64_t seed, int attempts) {
      auto [cam, ij, tries] = f2n::draw_pixels_masked(mask, n, seed, attempts);
      return py::make_tuple(cam, ij, tries);
    },
    py::arg("mask"), py::arg("n"), py::arg("seed"), py::arg("attempts") = 32,
    "f2n_draw_pixels_masked -> (cam [n] i32, ij [n,2] i32, tries [n] i32; 0 = every attempt missed)");
  m.def(
    "sample_masked_rays",
    [](const Tensor & poses, const Tensor & intr, const f2n::PixelMask & mask, int64_t n,
       uint64_t seed, const c10::optional<Tensor> & images, const c10::optional<Tensor> & dist,
       int attempts) {
      f2n::MaskedBatch b = f2n::sample_masked_rays(
        poses, intr, mask, n, seed, opt_tensor(images), opt_tensor(dist), attempts);
      py::dict d;
      d["rays_o"] = b.rays.origins;
      d["rays_d"] = b.rays.dirs;
      d["gt"] = tensor_or_none(b.gt);
      d["alpha"] = tensor_or_none(b.alpha);
      d["cam"] = b.cam;
      d["ray_weight"] = b.ray_weight;
      d["ij"] = b.ij;
      d["tries"] = b.tries;
      return d;
    },
    py::arg("poses"), py::arg("intrinsics"), py::arg("mask"), py::arg("batch_size"),
    py::arg("seed"), py::arg("images") = py::none(), py::arg("dist") = py::none(),
    py::arg("attempts") = 32,
    "sample_random_rays restricted to the mask's valid pixels: dict of rays_o, rays_d, gt | None, "
    "alpha | None (images with four channels), cam, ray_weight (0 where every attempt missed), ij, "
    "tries; see f2n::sample_masked_rays");
  py::class_<f2n::ErrorMapOptions>(m, "ErrorMapOptions")
    .def(
      py::init([](int gh, int gw, float decay, float uniform_fraction, int attempts,
                  float init_value) {
        return f2n::ErrorMapOptions{gh, gw, decay, uniform_fraction, attempts, init_value};
      }),
      py::arg("gh") = 32, py::arg("gw") = 32, py::arg("decay") = 0.95f,
      py::arg("uniform_fraction") = 0.1f, py::arg("attempts") = 32, py::arg("init_value") = 1.f,
      "cells per image, the weight of the old value in update(), the share of uniformly drawn "
      "rays, attempts per ray and the value every cell starts at")
    .def_readwrite("gh", &f2n::ErrorMapOptions::gh)
    .def_readwrite("gw", &f2n::ErrorMapOptions::gw)
    .def_readwrite("decay", &f2n::ErrorMapOptions::decay)
    .def_readwrite("uniform_fraction", &f2n::ErrorMapOptions::uniform_fraction)
    .def_readwrite("attempts", &f2n::ErrorMapOptions::attempts)
    .def_readwrite("init_value", &f2n::ErrorMapOptions::init_value);
  py::class_<f2n::ErrorMap>(m, "ErrorMap")
    .def(
      py::init([](int64_t E, int64_t h, int64_t w, const f2n::ErrorMapOptions & options,
                  const f2n::PixelMask * mask) {
        if (mask) {
          TORCH_CHECK(
            mask->E == E && mask->h == h && mask->w == w, "the mask and E, h, w disagree");
          return f2n::ErrorMap(*mask, options);
        }
        return f2n::ErrorMap(E, h, w, options, torch::Device(torch::kCUDA));
      }),
      py::arg("E"), py::arg("h"), py::arg("w"), py::arg("options") = f2n::ErrorMapOptions(),
      py::arg("mask") = py::none(),
      "per-image error map of E images of h x w pixels, on the GPU; mask: a PixelMask or None")
    .def(
      "accumulate",
      [](f2n::ErrorMap & map, const Tensor & colors, const Tensor & gt, const Tensor & cam,
         const Tensor & ij, const c10::optional<Tensor> & ray_weight,
         const c10::optional<Tensor> & alpha, const c10::optional<Tensor> & bg) {
        map.accumulate(colors, gt, cam, ij, opt_tensor(ray_weight), opt_tensor(alpha), opt_tensor(bg));
      },
      py::arg("colors"), py::arg("gt"), py::arg("cam"), py::arg("ij"),
      py::arg("ray_weight") = py::none(), py::arg("alpha") = py::none(), py::arg("bg") = py::none(),
      "f2n_error_map_accum: the raw errors of one rendered batch into the accumulators")
    .def("update", &f2n::ErrorMap::update, "f2n_error_map_apply, then f2n_error_cdf")
    .def(
      "draw",
      [](const f2n::ErrorMap & map, int64_t n, uint64_t seed) {
        f2n::GuidedDraw d = map.draw(n, seed);
        return py::make_tuple(d.cam, d.ij, d.tries, d.ray_weight);
      },
      py::arg("n"), py::arg("seed"),
      "f2n_draw_pixels_guided -> (cam [n] i32, ij [n,2] i32, tries [n] i32, ray_weight [n] f32)")
    .def_readwrite("options", &f2n::ErrorMap::options)
    .def_readonly("E", &f2n::ErrorMap::E)
    .def_readonly("h", &f2n::ErrorMap::h)
    .def_readonly("w", &f2n::ErrorMap::w)
    .def_readonly("n_cells", &f2n::ErrorMap::n_cells)
    .def_readonly("value", &f2n::ErrorMap::value, "[n_cells] f32")
    .def_readonly("counts", &f2n::ErrorMap::counts, "[n_cells] i32: valid pixels per cell")
    .def_readonly("cdf", &f2n::ErrorMap::cdf, "[n_cells] int64 holding the uint64 prefix sums")
    .def_readonly("acc_sum", &f2n::ErrorMap::acc_sum, "[n_cells] int64 holding the uint64 sums")
    .def_readonly("acc_cnt", &f2n::ErrorMap::acc_cnt, "[n_cells] int32 holding the uint32 counts")
    .def_readonly("n_valid", &f2n::ErrorMap::n_valid, "[1] int64 on the device");
  m.def(
    "sample_guided_rays",
    [](const Tensor & poses, const Tensor & intr, const f2n::ErrorMap & map, int64_t n, uint64_t seed,
       const c10::optional<Tensor> & images, const c10::optional<Tensor> & dist) {
      f2n::MaskedBatch b =
        f2n::sample_guided_rays(poses, intr, map, n, seed, opt_tensor(images), opt_tensor(dist));
      py::dict d;
      d["rays_o"] = b.rays.origins;
      d["rays_d"] = b.rays.dirs;
      d["gt"] = tensor_or_none(b.gt);
      d["alpha"] = tensor_or_none(b.alpha);
      d["cam"] = b.cam;
      d["ray_weight"] = b.ray_weight;
      d["ij"] = b.ij;
      d["tries"] = b.tries;
      return d;
    },
    py::arg("poses"), py::arg("intrinsics"), py::arg("map"), py::arg("batch_size"), py::arg("seed"),
    py::arg("images") = py::none(), py::arg("dist") = py::none(),
    "sample_masked_rays with the guided draw of an ErrorMap: the same dict, ray_weight being the "
    "importance weight (0 where every attempt missed); see f2n::sample_guided_rays");
  m.def(
    "ssim",
    [](const Tensor & pred, const Tensor & gt, bool clip, bool want_map) {
      f2n::SsimOut o = f2n::ssim(pred, gt, clip, want_map);
      return py::make_tuple(o.ssim, tensor_or_none(o.map));
    },
    py::arg("pred"), py::arg("gt"), py::arg("clip") = true, py::arg("want_map") = false,
    "f2n_ssim_fwd: pred, gt [B,h,w,3] or [h,w,3] -> (ssim [B], map [B,h-10,w-10,3] | None); clip: "
    "the reference's clamps (the metric form).  Not differentiated");
  m.def("ssim_loss", &CustomOps::Ssim, py::arg("pred"), py::arg("gt"),
        "CustomOps::Ssim(pred, gt) -> [B]: the unclamped form, differentiable in pred only");
  m.def(
    "image_scores",
    [](const Tensor & pred, const Tensor & gt) {
      f2n::ImageScores sc = f2n::image_scores(pred, gt);
      py::dict d;
      d["mse"] = sc.mse;
      d["psnr"] = sc.psnr;
      d["ssim"] = sc.ssim;
      d["score"] = sc.score;
      return d;
    },
    py::arg("pred"), py::arg("gt"),
    "per-view mse, psnr, ssim (clipped, inputs clamped to [0,1]) and the Localizer's score, device "
    "tensors [B]; see f2n::image_scores");
  m.def(
    "draw_patches",
    [](int64_t E, int64_t h, int64_t w, int64_t n_patches, int64_t P, uint64_t seed,
       const f2n::PixelMask * mask, int attempts) {
      f2n::PatchDraw d = f2n::draw_patches(
        E, h, w, n_patches, P, seed, mask ? *mask : f2n::PixelMask(), attempts);
      return py::make_tuple(d.cam, d.ij, d.tries, d.patch_weight);
    },
    py::arg("E"), py::arg("h"), py::arg("w"), py::arg("n_patches"), py::arg("P"), py::arg("seed"),
    py::arg("mask") = py::none(), py::arg("attempts") = 32,
    "f2n_draw_patches -> (cam [n P^2] i32, ij [n P^2,2] i32, tries [n] i32, patch_weight [n] f32)");
  m.def(
    "sample_patch_rays",
    [](const Tensor & poses, const Tensor & intr, int64_t h, int64_t w, int64_t n_patches, int64_t P,
       uint64_t seed, const c10::optional<Tensor> & images, const f2n::PixelMask * mask,
       const c10::optional<Tensor> & dist, int attempts) {
      f2n::PatchBatch pb = f2n::sample_patch_rays(
        poses, intr, h, w, n_patches, P, seed, opt_tensor(images),
        mask ? *mask : f2n::PixelMask(), opt_tensor(dist), attempts);
      const f2n::MaskedBatch & b = pb.batch;
      py::dict d;
      d["rays_o"] = b.rays.origins;
      d["rays_d"] = b.rays.dirs;
      d["gt"] = tensor_or_none(b.gt);
      d["alpha"] = tensor_or_none(b.alpha);
      d["cam"] = b.cam;
      d["ray_weight"] = b.ray_weight;
      d["ij"] = b.ij;
      d["tries"] = b.tries;
      d["patch_weight"] = pb.patch_weight;
      return d;
    },
    py::arg("poses"), py::arg("intrinsics"), py::arg("h"), py::arg("w"), py::arg("n_patches"),
    py::arg("P"), py::arg("seed"), py::arg("images") = py::none(), py::arg("mask") = py::none(),
    py::arg("dist") = py::none(), py::arg("attempts") = 32,
    "a batch of n_patches P x P patches: sample_masked_rays' dict (tries and patch_weight per "
    "patch, ray_weight the patch's weight on its rays); see f2n::sample_patch_rays");
  m.def(
    "level_weights",
    [](double alpha, int64_t L) {
      auto [w, la] = f2n::level_weights(alpha, L);
      return py::make_tuple(w, la);
    },
    py::arg("alpha"), py::arg("n_levels"), "f2n_level_weights -> (weights [L] on the CPU, l_active)");
  py::class_<f2n::CoarseToFine>(m, "CoarseToFine")
    .def(py::init([](double start, double end, double base) {
           return f2n::CoarseToFine{start, end, base};
         }),
         py::arg("start") = 0., py::arg("end") = 1., py::arg("base") = 1.)
    .def_readwrite("start", &f2n::CoarseToFine::start)
    .def_readwrite("end", &f2n::CoarseToFine::end)
    .def_readwrite("base", &f2n::CoarseToFine::base)
    .def("alpha_at", &f2n::CoarseToFine::alpha_at, py::arg("it"), py::arg("n_levels"),
         "base + (L - base) * clamp((it - start) / (end - start), 0, 1)");
  m.def("ray_order", &f2n::ray_order, "caller indices of rays_d sorted into pixel-compact bundles");
  m.def("manual_seed", [](uint64_t s) { torch::manual_seed(s); });
  m.def("kernel_timer_enable", &f2n::kernel_timer_enable);
  m.def("kernel_timer_collect", []() {
    py::dict d;
    for (auto & t : f2n::kernel_timer_collect())
      d[py::str(t.name)] = py::make_tuple(t.launches, t.total_ms, t.units);
    return d;
  });

  // ---- Hash3DAnchored ----------------------------------------------------------------------------
  py::class_<Hash3DAnchored, std::shared_ptr<Hash3DAnchored>>(m, "Hash3DAnchored")
    .def(
      py::init([](int64_t L, int64_t F, int64_t log2_T, int64_t stride, const std::string & dev) {
        return std::make_shared<Hash3DAnchored>(field_options(L, F, log2_T, stride, dev));
      }),
      py::arg("n_levels") = 16, py::arg("n_channels") = 2, py::arg("log2_table") = 19,
      py::arg("level_stride") = 0, py::arg("device") = "")
    .def("query", &Hash3DAnchored::query)
    .def("table_f16", &Hash3DAnchored::table_f16)
    .def("density_grad", &Hash3DAnchored::density_grad, py::call_guard<py::gil_scoped_release>(),
         py::arg("points"),
         "d(density logit)/d(position) [n,3] at raw points: the interpolant's true gradient, detached")
    .def("density_head", &Hash3DAnchored::density_head, "(row 0 of the field head [L*F], its bias [1])")
    .def("named_parameters", [](Hash3DAnchored & s) { return named_params(s); })
    .def(
      "encode",
      [](Hash3DAnchored & s, const Tensor & x) {
        auto info = torch::make_intrusive<Hash3DAnchoredInfo>();
        info->hash3d_ = &s;
        return torch::autograd::Hash3DAnchoredFunction::apply(x, s.feat_pool_, torch::IValue(info))[0];
      },
      "Hash3DAnchoredFunction::apply(points, feat_pool, info)[0] on already-contracted points")
    .def(
      "set_accumulate_in_place", [](Hash3DAnchored & s, bool on) { s.options_.accumulate_in_place = on; },
      "Hash3DAnchoredOptions::accumulate_in_place: add into feat_pool.grad directly once it exists")
    .def("set_exact_point_grad", &Hash3DAnchored::set_exact_point_grad,
         "Hash3DAnchoredOptions::exact_point_grad: points and rays that require a gradient receive the "
         "encoding's true derivative instead of the reference's point gradient (quirk Q5)")
    .def("set_level_weights", &Hash3DAnchored::set_level_weights, py::arg("weights"),
         "per-level weights [L] >= 0 (CPU or device), folded into the field head; copied in place "
         "into one persistent device tensor: see Hash3DAnchored::set_level_weights")
    .def("clear_level_weights", &Hash3DAnchored::clear_level_weights)
    .def("level_weights", [](const Hash3DAnchored & s) { return tensor_or_none(s.level_weights()); },
         "the host copy [L] of the weights, or None when none are set")
    .def("active_levels", &Hash3DAnchored::active_levels,
         "1 + the index of the last non-zero weight; n_levels when none are set")
    .def("head_weight", &Hash3DAnchored::head_weight,
         "mlp.weight itself without level weights, else mlp.weight * (lw (x) 1_F) (carries autograd)")
    .def("set_skip_masked_levels",
         [](Hash3DAnchored & s, bool on) { s.options_.skip_masked_levels = on; },
         "Hash3DAnchoredOptions::skip_masked_levels: walk active_levels() levels only (default on)")
    .def_property_readonly(
      "skip_masked_levels", [](const Hash3DAnchored & s) { return s.options_.skip_masked_levels; })
    .def_readonly("pool_size", &Hash3DAnchored::pool_size_)
    .def_readonly("local_size", &Hash3DAnchored::local_size_)
    .def_readonly("level_stride", &Hash3DAnchored::level_stride_)
    .def_readonly("feat_pool", &Hash3DAnchored::feat_pool_)
    .def_readonly("prim_pool", &Hash3DAnchored::prim_pool_)
    .def_readonly("bias_pool", &Hash3DAnchored::bias_pool_)
    .def_readonly("level_mul", &Hash3DAnchored::level_mul_);

  // ---- PtsSampler --------------------------------------------------------------------------------
  py::class_<PtsSampler, std::shared_ptr<PtsSampler>>(m, "PtsSampler")
    .def(
      py::init([](int max_samples, float step) {
        PtsSamplerOptions o;
        o.max_samples = max_samples;
        o.step = step;
        return std::make_shared<PtsSampler>(o);
      }),
      py::arg("max_samples") = MAX_SAMPLE_PER_RAY, py::arg("step") = 1.0f / 256)
    .def(
      "get_samples",
      [](PtsSampler & s, const Tensor & o, const Tensor & d, const std::string & mode,
         const c10::optional<Tensor> & noise) {
        SampleResultFlex r = noise.has_value() ? s.get_samples(o, d, *noise)
                                               : s.get_samples(o, d, parse_mode(mode));
        return py::make_tuple(r.pts, r.dirs, r.dt, r.t, r.pts_idx_bounds);
      },
      py::arg("rays_o"), py::arg("rays_d"), py::arg("mode") = "validate",
      py::arg("noise") = py::none())
    .def(
      "get_samples_aten",
      [](PtsSampler & s, const Tensor & o, const Tensor & d, const c10::optional<Tensor> & noise) {
        SampleResultFlex r = s.get_samples_aten(o, d, opt_tensor(noise));
        return py::make_tuple(r.pts, r.dirs, r.dt, r.t, r.pts_idx_bounds);
      },
      py::arg("rays_o"), py::arg("rays_d"), py::arg("noise") = py::none());

  // ---- SHShader ----------------------------------------------------------------------------------
  py::class_<SHShader, std::shared_ptr<SHShader>>(m, "SHShader")
    .def(
      py::init([](const std::string & dev) { return std::make_shared<SHShader>(parse_device(dev)); }),
      py::arg("device") = "")
    .def("query", &SHShader::query)
    .def("encode", &SHShader::encode)
    .def("named_parameters", [](SHShader & s) { return named_params(s); });

  // ---- camera visibility (occ_visibility.hpp) ------------------------------------------------------
  py::class_<f2n::VisibilityOptions>(m, "VisibilityOptions")
    .def(
      py::init([](int64_t resolution, int pixel_stride, int n_steps, float step, int min_views,
                  int dilate) {
        f2n::VisibilityOptions o;
        o.resolution = resolution;
        o.pixel_stride = pixel_stride;
        o.n_steps = n_steps;
        o.step = step;
        o.min_views = min_views;
        o.dilate = dilate;
        return o;
      }),
      py::arg("resolution") = 128, py::arg("pixel_stride") = 1, py::arg("n_steps") = -1,
      py::arg("step") = 1.0f / 256, py::arg("min_views") = 1, py::arg("dilate") = 1)
    .def_readwrite("resolution", &f2n::VisibilityOptions::resolution)
    .def_readwrite("pixel_stride", &f2n::VisibilityOptions::pixel_stride)
    .def_readwrite("n_steps", &f2n::VisibilityOptions::n_steps)
    .def_readwrite("step", &f2n::VisibilityOptions::step)
    .def_readwrite("min_views", &f2n::VisibilityOptions::min_views)
    .def_readwrite("dilate", &f2n::VisibilityOptions::dilate);
  m.def(
    "camera_view_counts",
    [](const Tensor & poses, const Tensor & intr, int64_t h, int64_t w,
       const f2n::VisibilityOptions & opts, const c10::optional<Tensor> & dist,
       const f2n::PixelMask * mask) {
      return f2n::camera_view_counts(poses, intr, h, w, opts, opt_tensor(dist), mask);
    },
    py::arg("poses"), py::arg("intrinsics"), py::arg("h"), py::arg("w"),
    py::arg("opts") = f2n::VisibilityOptions(), py::arg("dist") = py::none(),
    py::arg("mask") = py::none(),
    "uint8 [G,G,G]: how many cameras see each cell (saturating at 255); poses are the normalised ones");
  m.def(
    "camera_visibility",
    [](const Tensor & poses, const Tensor & intr, int64_t h, int64_t w,
       const f2n::VisibilityOptions & opts, const c10::optional<Tensor> & dist,
       const f2n::PixelMask * mask) {
      return f2n::camera_visibility(poses, intr, h, w, opts, opt_tensor(dist), mask);
    },
    py::arg("poses"), py::arg("intrinsics"), py::arg("h"), py::arg("w"),
    py::arg("opts") = f2n::VisibilityOptions(), py::arg("dist") = py::none(),
    py::arg("mask") = py::none(),
    "int32 [G^3/32] words of `view count >= min_views`: what OccupancyGrid.set_allowed takes");

  // ---- OccupancyGrid -----------------------------------------------------------------------------
  py::class_<OccupancyGrid, std::shared_ptr<OccupancyGrid>>(m, "OccupancyGrid")
    .def(
      py::init([](int64_t resolution, const std::string & dev) {
        return std::make_shared<OccupancyGrid>(resolution, parse_device(dev));
      }),
      py::arg("resolution") = 128, py::arg("device") = "")
    .def(
      "update",
      [](OccupancyGrid & g, Hash3DAnchored & field, float threshold, float decay,
         const c10::optional<Tensor> & probe) { g.update(field, threshold, decay, opt_tensor(probe)); },
      py::arg("field"), py::arg("threshold") = OccupancyGrid::kDefaultThreshold,
      py::arg("decay") = OccupancyGrid::kDefaultDecay, py::arg("probe") = py::none(),
      "density = max(density * decay, sigma(probe)); bit = density > threshold")
    .def("set_bits", &OccupancyGrid::set_bits, "bool [G,G,G], indexed [cz][cy][cx]")
    .def("bits", &OccupancyGrid::bits)
    .def("density", &OccupancyGrid::density)
    .def("occupied", &OccupancyGrid::occupied, "raw points [n,3] -> bool [n]")
    .def("fraction", &OccupancyGrid::fraction)
    .def_property_readonly("resolution", &OccupancyGrid::resolution)
    .def_property_readonly("words", &OccupancyGrid::words)
    .def(
      "set_allowed", &OccupancyGrid::set_allowed, py::arg("words"),
      "int32 [G^3/32] words (camera_visibility): no bit outside them is ever on while they are set")
    .def("clear_allowed", &OccupancyGrid::clear_allowed)
    .def(
      "allowed",
      [](const OccupancyGrid & g) {
        return g.allowed().defined() ? c10::optional<Tensor>(g.allowed()) : c10::nullopt;
      },
      "the allowed words, or None")
    .def(
      "carve_to_cameras",
      [](OccupancyGrid & g, const Tensor & poses, const Tensor & intr, int64_t h, int64_t w,
         const f2n::VisibilityOptions & opts, const c10::optional<Tensor> & dist,
         const f2n::PixelMask * mask) {
        g.carve_to_cameras(poses, intr, h, w, opts, opt_tensor(dist), mask);
      },
      py::arg("poses"), py::arg("intrinsics"), py::arg("h"), py::arg("w"),
      py::arg("opts") = f2n::VisibilityOptions(), py::arg("dist") = py::none(),
      py::arg("mask") = py::none(),
      "set_allowed(camera_visibility(...)) at the grid's own resolution")
    .def_property_readonly_static(
      "DEFAULT_THRESHOLD", [](py::object) { return OccupancyGrid::kDefaultThreshold; })
    .def_property_readonly_static(
      "DEFAULT_DECAY", [](py::object) { return OccupancyGrid::kDefaultDecay; });

  // ---- Renderer ----------------------------------------------------------------------------------
  py::class_<RenderResult>(m, "RenderResult")
    .def_readonly("colors", &RenderResult::colors)
    .def_readonly("depths", &RenderResult::depths)
    .def_property_readonly("weights", [](const RenderResult & r) { return tensor_or_none(r.weights); })
    .def_readonly("idx_start_end", &RenderResult::idx_start_end)
    .def_property_readonly(
      "weight_var", [](const RenderResult & r) { return tensor_or_none(r.weight_var); })
    .def_property_readonly(
      "weight_dist", [](const RenderResult & r) { return tensor_or_none(r.weight_dist); })
    .def_property_readonly(
      "depth_terms", [](const RenderResult & r) { return tensor_or_none(r.depth_terms); },
      "[n_rays, 3] line-of-sight depth terms, or None unless render_for_loss got a depth_target")
    .def_property_readonly(
      "normals", [](const RenderResult & r) { return tensor_or_none(r.normals); },
      "[n_rays, 3] sum of w n^ over the kept samples, or None when RendererOptions::normals is off")
    .def_property_readonly(
      "opacity", [](const RenderResult & r) { return tensor_or_none(r.opacity); },
      "[n_rays] sum of the kept samples' weights, or None unless render_for_loss got want_opacity");
  py::class_<f2n::RaySupervision>(m, "RaySupervision")
    .def(
      py::init([](const c10::optional<Tensor> & ray_weight, const c10::optional<Tensor> & alpha,
                  float opacity_weight, bool want_colors, bool composite_target) {
        return f2n::RaySupervision{
          opt_tensor(ray_weight), opt_tensor(alpha), opacity_weight, want_colors, composite_target};
      }),
      py::arg("ray_weight") = py::none(), py::arg("alpha") = py::none(),
      py::arg("opacity_weight") = 0.f, py::arg("want_colors") = false,
      py::arg("composite_target") = true,
      "per-ray weights [n_rays], alpha targets [n_rays], the weight of the opacity term, whether "
      "train_step_supervised hands the render's colours back, and whether the colour target is "
      "a gt + (1 - a) bg (True) or gt itself with alpha feeding the opacity term alone (False: what "
      "a learned background needs)")
    .def_property_readonly(
      "ray_weight", [](const f2n::RaySupervision & s) { return tensor_or_none(s.ray_weight); })
    .def_property_readonly(
      "alpha", [](const f2n::RaySupervision & s) { return tensor_or_none(s.alpha); })
    .def_readwrite("opacity_weight", &f2n::RaySupervision::opacity_weight)
    .def_readwrite("want_colors", &f2n::RaySupervision::want_colors)
    .def_readwrite("composite_target", &f2n::RaySupervision::composite_target);
  py::class_<f2n::PatchLoss>(m, "PatchLoss")
    .def(
      py::init([](int patch, float ssim_weight, const c10::optional<Tensor> & patch_weight) {
        return f2n::PatchLoss{patch, ssim_weight, opt_tensor(patch_weight)};
      }),
      py::arg("patch") = 0, py::arg("ssim_weight") = 0.f, py::arg("patch_weight") = py::none(),
      "the patch side P (the rays are n_patches * P^2, patch-major), the weight of the D-SSIM term "
      "and per-patch weights [n_patches]; patch 0 or weight 0: no term")
    .def_readwrite("patch", &f2n::PatchLoss::patch)
    .def_readwrite("ssim_weight", &f2n::PatchLoss::ssim_weight)
    .def_property_readonly(
      "patch_weight", [](const f2n::PatchLoss & p) { return tensor_or_none(p.patch_weight); });
  py::class_<f2n::RobustLoss>(m, "RobustLoss")
    .def(
      py::init([](float quantile, float box_thresh, float nbhd_thresh, int patch, int nbhd) {
        return f2n::RobustLoss{quantile, box_thresh, nbhd_thresh, patch, nbhd};
      }),
      py::arg("quantile") = 1.f, py::arg("box_thresh") = .5f, py::arg("nbhd_thresh") = .6f,
      py::arg("patch") = 0, py::arg("nbhd") = 8,
      "the trimmed colour loss of f2n_robust_weights: the quantile of the residuals kept (>= 1: off), "
      "the thresholds of the 3 x 3 box and of the block vote, the patch side P (0: scattered rays) "
      "and the side of a block")
    .def_readwrite("quantile", &f2n::RobustLoss::quantile)
    .def_readwrite("box_thresh", &f2n::RobustLoss::box_thresh)
    .def_readwrite("nbhd_thresh", &f2n::RobustLoss::nbhd_thresh)
    .def_readwrite("patch", &f2n::RobustLoss::patch)
    .def_readwrite("nbhd", &f2n::RobustLoss::nbhd);
  m.def(
    "robust_weights",
    [](const Tensor & colors, const Tensor & target, const f2n::RobustLoss & opt,
       const c10::optional<Tensor> & ray_weight) {
      f2n::RobustWeights w = f2n::robust_weights(colors, target, opt_tensor(ray_weight), opt);
      return py::make_tuple(w.weight, w.omega, w.stats);
    },
    py::arg("colors"), py::arg("target"), py::arg("opt"), py::arg("ray_weight") = py::none(),
    "f2n_robust_weights: colors, target [n,3], ray_weight [n] | None -> (weight [n] f32, omega [n] "
    "u8, stats [4] = {T, N_c, sum of the pixel labels, sum of the final labels}); no host read");
  py::class_<f2n::DepthLossOptions>(m, "DepthLossOptions")
    .def(
      py::init([](float empty, float near, float expected, float eps) {
        return f2n::DepthLossOptions{empty, near, expected, eps};
      }),
      py::arg("empty") = 0.f, py::arg("near") = 0.f, py::arg("expected") = 0.f, py::arg("eps") = 0.f,
      "weights of the three line-of-sight depth terms and the half-width of the surface band")
    .def_readwrite("empty", &f2n::DepthLossOptions::empty)
    .def_readwrite("near", &f2n::DepthLossOptions::near)
    .def_readwrite("expected", &f2n::DepthLossOptions::expected)
    .def_readwrite("eps", &f2n::DepthLossOptions::eps);
  py::class_<Renderer, std::shared_ptr<Renderer>>(m, "Renderer")
    .def(
      py::init([](int n_images, int64_t L, int64_t F, int64_t log2_T, int64_t stride,
                  int max_samples, float step, bool fused, const std::string & dev) {
        RendererOptions o;
        o.field = field_options(L, F, log2_T, stride, dev);
        o.sampler.max_samples = max_samples;
        o.sampler.step = step;
        o.fused = fused;
        return std::make_shared<Renderer>(n_images, o);
      }),
      py::arg("n_images"), py::arg("n_levels") = 16, py::arg("n_channels") = 2,
      py::arg("log2_table") = 19, py::arg("level_stride") = 0,
      py::arg("max_samples") = MAX_SAMPLE_PER_RAY, py::arg("step") = 1.0f / 256,
      py::arg("fused") = true, py::arg("device") = "")
    .def(
      "render",
      [](Renderer & r, const Tensor & o, const Tensor & d, const c10::optional<Tensor> & emb_idx,
         const std::string & mode, const c10::optional<Tensor> & noise,
         const c10::optional<Tensor> & bg) {
        RenderResult res;
        {
          py::gil_scoped_release no_gil;
          res = r.render(
            o, d, opt_tensor(emb_idx), parse_mode(mode), opt_tensor(noise), opt_tensor(bg));
        }
        return result_tuple(res);
      },
      py::arg("rays_o"), py::arg("rays_d"), py::arg("emb_idx") = py::none(),
      py::arg("mode") = "validate", py::arg("noise") = py::none(), py::arg("bg_color") = py::none())
    .def(
      "render_for_loss",
      [](Renderer & r, const Tensor & o, const Tensor & d, const c10::optional<Tensor> & emb_idx,
         const std::string & mode, const c10::optional<Tensor> & noise,
         const c10::optional<Tensor> & bg, bool want_dist,
         const c10::optional<Tensor> & depth_target, float depth_eps) -> py::tuple {
        const LossOutputs want{want_dist, opt_tensor(depth_target), depth_eps};
        RenderResult res;
        {
          py::gil_scoped_release no_gil;
          res = r.render_for_loss(
            o, d, opt_tensor(emb_idx), parse_mode(mode), opt_tensor(noise), opt_tensor(bg), want);
        }
        if (depth_target.has_value())
          return py::make_tuple(
            res.colors, res.depths, tensor_or_none(res.weights), res.idx_start_end,
            tensor_or_none(res.weight_var), tensor_or_none(res.weight_dist),
            tensor_or_none(res.depth_terms));
        return py::make_tuple(
          res.colors, res.depths, tensor_or_none(res.weights), res.idx_start_end,
          tensor_or_none(res.weight_var), tensor_or_none(res.weight_dist));
      },
      py::arg("rays_o"), py::arg("rays_d"), py::arg("emb_idx") = py::none(),
      py::arg("mode") = "train", py::arg("noise") = py::none(), py::arg("bg_color") = py::none(),
      py::arg("want_dist") = false, py::arg("depth_target") = py::none(),
      py::arg("depth_eps") = 0.f,
      "(colors, depths, weights | None, idx_start_end, weight_var | None, weight_dist | None): see "
      "Renderer::render_for_loss.  NOTE THE ARITY: the tuple has these six elements unless a "
      "depth_target [n_rays] is passed; then, and only then, it has a SEVENTH, depth_terms "
      "[n_rays, 3].  Callers written before depth supervision keep unpacking six; a caller that "
      "passes a target unpacks seven.  render_for_loss_result returns the RenderResult itself, with "
      "every field by name (None where undefined), whatever was asked for.")
    .def(
      "render_for_loss_result",
      [](Renderer & r, const Tensor & o, const Tensor & d, const c10::optional<Tensor> & emb_idx,
         const std::string & mode, const c10::optional<Tensor> & noise,
         const c10::optional<Tensor> & bg, bool want_dist,
         const c10::optional<Tensor> & depth_target, float depth_eps, bool want_opacity) {
        const LossOutputs want{want_dist, opt_tensor(depth_target), depth_eps, want_opacity};
        py::gil_scoped_release no_gil;
        return r.render_for_loss(
          o, d, opt_tensor(emb_idx), parse_mode(mode), opt_tensor(noise), opt_tensor(bg), want);
      },
      py::arg("rays_o"), py::arg("rays_d"), py::arg("emb_idx") = py::none(),
      py::arg("mode") = "train", py::arg("noise") = py::none(), py::arg("bg_color") = py::none(),
      py::arg("want_dist") = false, py::arg("depth_target") = py::none(),
      py::arg("depth_eps") = 0.f, py::arg("want_opacity") = false,
      "render_for_loss handing back the RenderResult: colors, depths, weights, idx_start_end, "
      "weight_var, weight_dist, depth_terms, normals, opacity by name (None where undefined)")
    .def(
      "render_rays",
      [](Renderer & r, const Tensor & o, const Tensor & d, const c10::optional<Tensor> & emb_idx,
         const std::string & mode, const c10::optional<Tensor> & noise,
         const c10::optional<Tensor> & bg) {
        py::gil_scoped_release no_gil;
        return r.render_rays(
          o, d, opt_tensor(emb_idx), parse_mode(mode), opt_tensor(noise), opt_tensor(bg));
      },
      py::arg("rays_o"), py::arg("rays_d"), py::arg("emb_idx") = py::none(),
      py::arg("mode") = "validate", py::arg("noise") = py::none(), py::arg("bg_color") = py::none(),
      "the no-grad render as one kernel: (colors, depths, last_trans, kept); see Renderer::render_rays")
    .def(
      "render_result",
      [](Renderer & r, const Tensor & o, const Tensor & d, const c10::optional<Tensor> & emb_idx,
         const std::string & mode, const c10::optional<Tensor> & noise,
         const c10::optional<Tensor> & bg) {
        py::gil_scoped_release no_gil;
        return r.render(o, d, opt_tensor(emb_idx), parse_mode(mode), opt_tensor(noise), opt_tensor(bg));
      },
      py::arg("rays_o"), py::arg("rays_d"), py::arg("emb_idx") = py::none(),
      py::arg("mode") = "validate", py::arg("noise") = py::none(), py::arg("bg_color") = py::none(),
      "render() handing back the RenderResult itself: colors, depths, weights, idx_start_end and, "
      "after set_normals(True), normals (None otherwise)")
    .def("set_normals", &Renderer::set_normals,
         "RendererOptions::normals: render() also composites the kept samples' surface normals")
    .def_property_readonly(
      "normals", [](const Renderer & r) { return r.options_.normals; },
      "RendererOptions::normals as set_normals left it")
    .def("render_all_rays", &Renderer::render_all_rays, py::call_guard<py::gil_scoped_release>())
    .def("render_all_rays_with_normals", &Renderer::render_all_rays_with_normals,
         py::call_guard<py::gil_scoped_release>(), py::arg("rays_o"), py::arg("rays_d"),
         py::arg("batch_size"), "(colors [n,3], depths [n,1], normals [n,3])")
    .def(
      "render_image_with_normals",
      [](Renderer & r, const Tensor & pose, const Tensor & intr, int h, int w, int batch_size,
         const c10::optional<Tensor> & dist) {
        py::gil_scoped_release no_gil;
        return r.render_image_with_normals(pose, intr, h, w, batch_size, opt_tensor(dist));
      },
      py::arg("pose"), py::arg("intrinsic"), py::arg("h"), py::arg("w"), py::arg("batch_size"),
      py::arg("dist") = py::none(), "(colors [h,w,3], depths [h,w,3], normals [h,w,3])")
    .def(
      "render_image",
      [](Renderer & r, const Tensor & pose, const Tensor & intr, int h, int w, int batch_size,
         const c10::optional<Tensor> & dist) {
        py::gil_scoped_release no_gil;
        return r.render_image(pose, intr, h, w, batch_size, opt_tensor(dist));
      },
      py::arg("pose"), py::arg("intrinsic"), py::arg("h"), py::arg("w"), py::arg("batch_size"),
      py::arg("dist") = py::none())
    .def(
      "train_step",
      [](Renderer & r, const Tensor & o, const Tensor & d, const Tensor & emb_idx, const Tensor & gt,
         float var_loss_weight, const c10::optional<Tensor> & noise,
         const c10::optional<Tensor> & bg, bool backward, float dist_loss_weight,
         const c10::optional<Tensor> & depth_target, const f2n::DepthLossOptions & depth_loss) {
        const f2n::TrainStepResult out = run_train_step(
          r, o, d, emb_idx, gt, var_loss_weight, noise, bg, backward, dist_loss_weight, depth_target,
          depth_loss);
        return py::make_tuple(out.loss, out.sq_err_sum, out.n_values, out.n_samples);
      },
      py::arg("rays_o"), py::arg("rays_d"), py::arg("emb_idx"), py::arg("gt_colors"),
      py::arg("var_loss_weight") = 0.f, py::arg("noise") = py::none(),
      py::arg("bg_color") = py::none(), py::arg("backward") = true,
      py::arg("dist_loss_weight") = 0.f, py::arg("depth_target") = py::none(),
      py::arg("depth_loss") = f2n::DepthLossOptions(),
      "reference train_manager.cpp:76-107 without the optimiser step; dist_loss_weight > 0 adds the "
      "distortion loss (its mean: last_dist_loss); depth_target [n_rays] with a DepthLossOptions "
      "that has a non-zero weight adds the line-of-sight depth terms (their means: last_depth_loss)")
    .def(
      "train_step_supervised",
      [](Renderer & r, const Tensor & o, const Tensor & d, const Tensor & emb_idx, const Tensor & gt,
         const f2n::RaySupervision & sup, float var_loss_weight,
         const c10::optional<Tensor> & noise, const c10::optional<Tensor> & bg, bool backward,
         float dist_loss_weight, const c10::optional<Tensor> & depth_target,
         const f2n::DepthLossOptions & depth_loss) {
        const f2n::TrainStepResult out = run_train_step(
          r, o, d, emb_idx, gt, var_loss_weight, noise, bg, backward, dist_loss_weight, depth_target,
          depth_loss, sup);
        if (sup.want_colors)
          return py::make_tuple(
            out.loss, out.sq_err_sum, out.n_values, out.n_samples, tensor_or_none(out.weight_sum),
            out.colors);
        return py::make_tuple(
          out.loss, out.sq_err_sum, out.n_values, out.n_samples, tensor_or_none(out.weight_sum));
      },
      py::arg("rays_o"), py::arg("rays_d"), py::arg("emb_idx"), py::arg("gt_colors"),
      py::arg("sup"), py::arg("var_loss_weight") = 0.f, py::arg("noise") = py::none(),
      py::arg("bg_color") = py::none(), py::arg("backward") = true,
      py::arg("dist_loss_weight") = 0.f, py::arg("depth_target") = py::none(),
      py::arg("depth_loss") = f2n::DepthLossOptions(),
      "train_step with a RaySupervision (masked rays, alpha targets): (loss, sq_err_sum, n_values, "
      "n_samples, weight_sum | None).  A RaySupervision without ray_weight and alpha is train_step "
      "itself, launch for launch; the opacity term's mean is left in last_opacity_loss.  NOTE THE "
      "ARITY: with sup.want_colors the tuple has a sixth element, the render's colours [n_rays, 3], "
      "detached")
    .def(
      "train_step_patches",
      [](Renderer & r, const Tensor & o, const Tensor & d, const Tensor & emb_idx, const Tensor & gt,
         const f2n::PatchLoss & patch, const f2n::RaySupervision & sup, float var_loss_weight,
         const c10::optional<Tensor> & noise, const c10::optional<Tensor> & bg, bool backward,
         float dist_loss_weight, const c10::optional<Tensor> & depth_target,
         const f2n::DepthLossOptions & depth_loss) {
        const f2n::TrainStepResult out = run_train_step(
          r, o, d, emb_idx, gt, var_loss_weight, noise, bg, backward, dist_loss_weight, depth_target,
          depth_loss, sup, patch);
        return py::make_tuple(
          out.loss, out.sq_err_sum, out.n_values, out.n_samples, tensor_or_none(out.weight_sum),
          tensor_or_none(out.colors));
      },
      py::arg("rays_o"), py::arg("rays_d"), py::arg("emb_idx"), py::arg("gt_colors"),
      py::arg("patch"), py::arg("sup") = f2n::RaySupervision(), py::arg("var_loss_weight") = 0.f,
      py::arg("noise") = py::none(), py::arg("bg_color") = py::none(), py::arg("backward") = true,
      py::arg("dist_loss_weight") = 0.f, py::arg("depth_target") = py::none(),
      py::arg("depth_loss") = f2n::DepthLossOptions(),
      "train_step with a PatchLoss (a D-SSIM term on patches; its unweighted mean: last_ssim_loss) "
      "and an optional RaySupervision: always six elements, (loss, sq_err_sum, n_values, "
      "n_samples, weight_sum | None, colors | None).  patch 0 or ssim_weight 0 is "
      "train_step_supervised, launch for launch")
    .def(
      "train_step_robust",
      [](Renderer & r, const Tensor & o, const Tensor & d, const Tensor & emb_idx, const Tensor & gt,
         const f2n::RobustLoss & robust, const f2n::PatchLoss & patch,
         const f2n::RaySupervision & sup, float var_loss_weight,
         const c10::optional<Tensor> & noise, const c10::optional<Tensor> & bg, bool backward,
         float dist_loss_weight, const c10::optional<Tensor> & depth_target,
         const f2n::DepthLossOptions & depth_loss) {
        const f2n::TrainStepResult out = run_train_step(
          r, o, d, emb_idx, gt, var_loss_weight, noise, bg, backward, dist_loss_weight, depth_target,
          depth_loss, sup, patch, robust);
        return py::make_tuple(
          out.loss, out.sq_err_sum, out.n_values, out.n_samples, tensor_or_none(out.weight_sum),
          tensor_or_none(out.colors), tensor_or_none(out.robust_weight),
          tensor_or_none(out.robust_stats));
      },
      py::arg("rays_o"), py::arg("rays_d"), py::arg("emb_idx"), py::arg("gt_colors"),
      py::arg("robust"), py::arg("patch") = f2n::PatchLoss(),
      py::arg("sup") = f2n::RaySupervision(), py::arg("var_loss_weight") = 0.f,
      py::arg("noise") = py::none(), py::arg("bg_color") = py::none(), py::arg("backward") = true,
      py::arg("dist_loss_weight") = 0.f, py::arg("depth_target") = py::none(),
      py::arg("depth_loss") = f2n::DepthLossOptions(),
      "train_step with a RobustLoss (the trimmed colour loss: rays the render cannot explain are "
      "dropped from every per-ray term), an optional PatchLoss and RaySupervision: always eight "
      "elements, (loss, sq_err_sum, n_values, n_samples, weight_sum | None, colors | None, "
      "robust_weight | None, robust_stats | None).  quantile >= 1 is train_step_patches, launch for "
      "launch")
    .def("named_parameters", [](Renderer & r) { return named_params(r); })
    .def("zero_grad", [](Renderer & r) { r.zero_grad(); })
    .def(
      "grads",
      [](Renderer & r) {
        py::dict d;
        for (auto & kv : r.named_parameters()) d[py::str(kv.key())] = grad_or_none(kv.value());
        return d;
      })
    .def(
      "set_occupancy",
      [](Renderer & r, std::shared_ptr<OccupancyGrid> g) { r.set_occupancy(std::move(g)); },
      py::arg("grid").none(true), "attach an occupancy grid (None = off): see Renderer::set_occupancy")
    .def_property_readonly("occupancy", [](Renderer & r) { return r.occupancy(); })
    .def(
      "set_background",
      [](Renderer & r, std::shared_ptr<f2n::EnvMap> e) { r.set_background(std::move(e)); },
      py::arg("env").none(true),
      "attach a learned background (None = off): see Renderer::set_background")
    .def_property_readonly("background", [](Renderer & r) { return r.background(); })
    .def("set_fused", [](Renderer & r, bool f) { r.options_.fused = f; })
    .def("set_fused_shade", [](Renderer & r, bool f) { r.options_.fused_shade = f; })
    .def("set_dense_first_pass", [](Renderer & r, int m) { r.options_.dense_first_pass = m; })
    .def("set_speculate_dense", [](Renderer & r, bool f) { r.options_.speculate_dense = f; })
    .def("set_pixel_tiles", [](Renderer & r, int b) { r.options_.pixel_tiles = b; })
    .def("set_fused_ray_grad", [](Renderer & r, bool f) { r.options_.fused_ray_grad = f; },
         "rays that require grad take the fused path: see RendererOptions::fused_ray_grad")
    .def("set_exact_ray_grad", [](Renderer & r, bool on) { r.scene_field_->set_exact_point_grad(on); },
         "the scene field's Hash3DAnchoredOptions::exact_point_grad, on every route")
    .def("set_level_weights", &Renderer::set_level_weights, py::arg("weights"),
         "per-level weights [L] >= 0 of the scene field, on every route: see Renderer::set_level_weights")
    .def("set_coarse_to_fine", &Renderer::set_coarse_to_fine, py::arg("alpha"),
         "the weights of f2n_level_weights for a progress alpha in [1, L]")
    .def("clear_level_weights", &Renderer::clear_level_weights)
    .def("level_weights", [](const Renderer & r) { return tensor_or_none(r.scene_field_->level_weights()); })
    .def("active_levels", [](const Renderer & r) { return r.scene_field_->active_levels(); })
    .def("set_skip_masked_levels",
         [](Renderer & r, bool on) { r.scene_field_->options_.skip_masked_levels = on; },
         "the scene field's Hash3DAnchoredOptions::skip_masked_levels")
    .def("set_margin_min_samples", [](Renderer & r, int64_t n) { r.options_.margin_min_samples = n; })
    .def("set_ray_order_min_rays", [](Renderer & r, int64_t n) { r.options_.ray_order_min_rays = n; },
         "dense first pass: bucket the rays from this many on (RendererOptions::ray_order_min_rays)")
    .def("set_one_pass", &Renderer::set_one_pass,
         "render_all_rays / render_image in one kernel per chunk: see RendererOptions::one_pass")
    .def("one_pass_applies", &Renderer::one_pass_applies)
    .def_property_readonly(
      "one_pass_head", [](const Renderer & r) { return r.options_.one_pass_head; },
      "RendererOptions::one_pass_head as set_one_pass_head left it")
    .def("set_one_pass_head", &Renderer::set_one_pass_head,
         "how the one-pass render walks a ray: 0 one wavefront per ray (default), -1 whole rays eight "
         "to a wavefront, a positive multiple of 64 = head then tail; see RendererOptions::one_pass_head")
    .def("set_deferred_check", [](Renderer & r, bool f) { r.options_.deferred_check = f; },
         "no host read in render(): see RendererOptions::deferred_check")
    .def("deferred_check_ok", &Renderer::deferred_check_ok)
    .def_property_readonly(
      "last_dist_loss", [](const Renderer & r) { return tensor_or_none(r.last_dist_loss_); },
      "mean weight_dist of the last train_step with dist_loss_weight != 0 (device scalar) or None")
    .def_property_readonly(
      "last_depth_loss", [](const Renderer & r) { return tensor_or_none(r.last_depth_loss_); },
      "[3] means over the valid rays of the depth terms of the last train_step that had them, or None")
    .def_property_readonly(
      "last_opacity_loss", [](const Renderer & r) { return tensor_or_none(r.last_opacity_loss_); },
      "weighted mean of (opacity - alpha)^2 of the last train_step that had the term, or None")
    .def_property_readonly(
      "last_ssim_loss", [](const Renderer & r) { return tensor_or_none(r.last_ssim_loss_); },
      "unweighted mean of 1 - SSIM_b of the last train_step with an active PatchLoss, or None")
    .def_readonly("last_kept_fraction", &Renderer::last_kept_fraction_)
    .def_readonly("last_n_samples", &Renderer::last_n_samples_)
    .def_property_readonly("scene_field", [](Renderer & r) { return r.scene_field_; })
    .def_property_readonly("shader", [](Renderer & r) { return r.shader_; })
    .def_property_readonly("pts_sampler", [](Renderer & r) { return r.pts_sampler_; })
    .def(
      "save", [](std::shared_ptr<Renderer> r, const std::string & path) { torch::save(r, path); })
    .def("load", [](std::shared_ptr<Renderer> r, const std::string & path) { torch::load(r, path); })
    .def(
      "make_adam",
      [](Renderer & r, float lr) {
        AdamHandle h;
        h.opt = std::make_shared<torch::optim::Adam>(r.optim_param_groups(lr));
        return h;
      },
      "torch::optim::Adam over optim_param_groups(lr) (reference train_manager.cpp:55)")
    .def(
      "make_fused_adam",
      [](Renderer & r, float lr) {
        AdamHandle h;
        h.opt = std::make_shared<FusedAdam>(r.optim_param_groups(lr), r.scene_field_);
        return h;
      },
      "FusedAdam over the same groups: one kernel per parameter, emits the table's f16 shadow");

  // ---- mesh extraction ---------------------------------------------------------------------------
  m.attr("DENSITY_SHIFT") = f2n::kDensityShift;
  m.def(
    "density_lattice",
    [](Hash3DAnchored & field, const std::array<float, 3> & lo, const std::array<float, 3> & step,
       const std::array<int64_t, 3> & dims) {
      py::gil_scoped_release no_gil;
      return f2n::density_lattice(field, lo, step, dims);
    },
    py::arg("field"), py::arg("lo"), py::arg("step"), py::arg("dims"),
    "f2n_density_lattice: the density logit [nz,ny,nx] at lo + i * step, dims = (nx, ny, nz)");
  m.def(
    "marching_tets",
    [](const Tensor & values, float level, const std::array<float, 3> & lo,
       const std::array<float, 3> & step) {
      f2n::Mesh mesh;
      {
        py::gil_scoped_release no_gil;
        mesh = f2n::marching_tets(values, level, lo, step);
      }
      return py::make_tuple(mesh.vertices, mesh.triangles);
    },
    py::arg("values"), py::arg("level"), py::arg("lo"), py::arg("step"),
    "marching tetrahedra on values [nz,ny,nx] -> (vertices [V,3] f32, triangles [T,3] i32)");
  m.def(
    "extract_mesh",
    [](Renderer & r, const std::array<float, 3> & lo, const std::array<float, 3> & hi,
       const std::array<int64_t, 3> & dims, float sigma_level, bool with_normals) {
      f2n::Mesh mesh;
      {
        py::gil_scoped_release no_gil;
        mesh = f2n::extract_mesh(r, lo, hi, dims, sigma_level, with_normals);
      }
      return py::make_tuple(mesh.vertices, mesh.triangles, tensor_or_none(mesh.normals));
    },
    py::arg("renderer"), py::arg("lo"), py::arg("hi"), py::arg("dims"), py::arg("sigma_level"),
    py::arg("with_normals") = false,
    "the surface density == sigma_level inside [lo, hi] -> (vertices, triangles, normals | None)");
  m.def(
    "save_ply",
    [](const std::string & path, const Tensor & vertices, const Tensor & triangles,
       const c10::optional<Tensor> & normals) {
      f2n::save_ply(path, vertices, triangles, opt_tensor(normals));
    },
    py::arg("path"), py::arg("vertices"), py::arg("triangles"), py::arg("normals") = py::none(),
    "binary little-endian PLY 1.0: x y z [nx ny nz], faces as uchar 3 + three int32");

  // ---- scene files: cams_meta.tsv, scene normalisation, inference_params.yaml
  m.def("read_cams_meta", [](const std::string & path) {
    f2n::CamsMeta c = f2n::read_cams_meta(path);
    return py::make_tuple(c.poses, c.intrinsics, c.dist_params, c.bounds);
  });
  m.def("normalize_scene", [](const torch::Tensor & poses) {
    f2n::SceneNormalisation n = f2n::normalize_scene(poses);
    return py::make_tuple(n.poses, n.center, n.radius);
  });
  m.def(
    "save_inference_params",
    [](const std::string & dir, int n_images, int height, int width, const torch::Tensor & intrinsic,
       const torch::Tensor & center, float radius) {
      f2n::InferenceParams p;
      p.n_images = n_images;
      p.height = height;
      p.width = width;
      p.intrinsic = intrinsic;
      p.normalizing_center = center;
      p.normalizing_radius = radius;
      f2n::save_inference_params(dir, p);
    });
  m.def("load_inference_params", [](const std::string & dir) {
    f2n::InferenceParams p = f2n::load_inference_params(dir);
    return py::make_tuple(
      p.n_images, p.height, p.width, p.intrinsic, p.normalizing_center, p.normalizing_radius);
  });

  // ---- Localizer ---------------------------------------------------------------------------------
  m.def(
    "perturb_poses",
    [](const Tensor & pose, const Tensor & noise, const std::array<float, 6> & sigmas) {
      return f2n::perturb_poses(pose, noise, sigmas);
    },
    py::arg("pose"), py::arg("noise"), py::arg("sigmas"),
    "f2n_perturb_poses: sigmas = (pos x, y, z in the NeRF frame, rot x, y, z in degrees)");
  m.def("pose_scores", &f2n::pose_scores, py::arg("colors"), py::arg("image"), py::arg("ij"),
        "f2n_pose_scores -> (loss [P], weights [P])");
  m.def("average_pose", &f2n::average_pose, py::arg("poses"), py::arg("weights"),
        "f2n_average_pose -> [3,4]");

  py::class_<LocalizerParam>(m, "LocalizerParam")
    .def(py::init<>())
    .def_readwrite("train_result_dir", &LocalizerParam::train_result_dir)
    .def_readwrite("render_pixel_num", &LocalizerParam::render_pixel_num)
    .def_readwrite("noise_position_x", &LocalizerParam::noise_position_x)
    .def_readwrite("noise_position_y", &LocalizerParam::noise_position_y)
    .def_readwrite("noise_position_z", &LocalizerParam::noise_position_z)
    .def_readwrite("noise_rotation_x", &LocalizerParam::noise_rotation_x)
    .def_readwrite("noise_rotation_y", &LocalizerParam::noise_rotation_y)
    .def_readwrite("noise_rotation_z", &LocalizerParam::noise_rotation_z)
    .def_readwrite("resize_factor", &LocalizerParam::resize_factor)
    .def_readwrite("one_pass", &LocalizerParam::one_pass)
    .def_readwrite("one_pass_head", &LocalizerParam::one_pass_head)
    .def_readwrite("dist_params", &LocalizerParam::dist_params)
    .def_readwrite("exact_ray_grad", &LocalizerParam::exact_ray_grad)
    .def_readwrite("level_alpha", &LocalizerParam::level_alpha);

  py::class_<Localizer, std::shared_ptr<Localizer>>(m, "Localizer")
    .def(py::init<const LocalizerParam &>(), py::arg("param"),
         "from param.train_result_dir: inference_params.yaml + checkpoints/latest/renderer.pt")
    .def(
      py::init<const LocalizerParam &, std::shared_ptr<Renderer>, const Tensor &, int, int,
               const Tensor &, float>(),
      py::arg("param"), py::arg("renderer"), py::arg("intrinsic"), py::arg("height"),
      py::arg("width"), py::arg("center"), py::arg("radius"))
    .def("render_image", &Localizer::render_image, py::call_guard<py::gil_scoped_release>())
    .def("set_level_alpha", &Localizer::set_level_alpha, py::arg("alpha"),
         "LocalizerParam::level_alpha afterwards: < 0 clears the renderer's level weights")
    .def(
      "optimize_pose_by_random_search",
      [](Localizer & l, const Tensor & pose, const Tensor & image, int64_t n, float coeff,
         const c10::optional<Tensor> & noise) {
        std::vector<Particle> particles;
        {
          py::gil_scoped_release no_gil;
          particles = l.optimize_pose_by_random_search(pose, image, n, coeff, opt_tensor(noise));
        }
        return particle_list(particles);
      },
      py::arg("initial_pose"), py::arg("image"), py::arg("particle_num"), py::arg("noise_coeff"),
      py::arg("noise") = py::none(), "-> [(pose [3,4], weight)] * particle_num")
    .def(
      "random_search",
      [](Localizer & l, const Tensor & pose, const Tensor & image, int64_t n, float coeff,
         const c10::optional<Tensor> & noise) {
        py::gil_scoped_release no_gil;
        return l.random_search(pose, image, n, coeff, opt_tensor(noise));
      },
      py::arg("initial_pose"), py::arg("image"), py::arg("particle_num"), py::arg("noise_coeff"),
      py::arg("noise") = py::none(), "-> (poses [P,3,4], weights [P]) on the device, no host read")
    .def(
      "optimize_pose_by_differential",
      [](Localizer & l, const Tensor & pose, const Tensor & image, int64_t iterations) {
        // loss.backward() runs the autograd engine, which must not be entered holding the GIL
        py::gil_scoped_release no_gil;
        return l.optimize_pose_by_differential(pose, image, iterations);
      },
      py::arg("initial_pose"), py::arg("image"), py::arg("iteration_num"))
    .def(
      "evaluate_poses",
      [](Localizer & l, const Tensor & poses, const Tensor & image, const c10::optional<Tensor> & ij) {
        py::gil_scoped_release no_gil;
        return l.evaluate_poses(poses, image, opt_tensor(ij));
      },
      py::arg("poses"), py::arg("image"), py::arg("ij") = py::none())
    .def(
      "evaluate_poses_full",
      [](Localizer & l, const Tensor & poses, const Tensor & image, const c10::optional<Tensor> & ij) {
        Localizer::PoseScores s;
        {
          py::gil_scoped_release no_gil;
          s = l.evaluate_poses_full(poses, image, opt_tensor(ij));
        }
        return py::make_tuple(s.weights, s.loss, s.colors, s.ij);
      },
      py::arg("poses"), py::arg("image"), py::arg("ij") = py::none(),
      "-> (weights [P], loss [P], colors [P,K,3], ij [K,2])")
    .def(
      "pose_rays",
      [](Localizer & l, const Tensor & poses, const Tensor & ij) {
        Rays r = l.pose_rays(poses, ij);
        return py::make_tuple(r.origins, r.dirs);
      },
      "the rays evaluate_poses renders, pose-major")
    .def_static(
      "calc_average_pose",
      [](const py::object & particles, const c10::optional<Tensor> & weights) {
        if (weights.has_value())
          return Localizer::calc_average_pose(particles.cast<Tensor>(), *weights);
        std::vector<Particle> v;
        for (py::handle h : particles) {
          auto t = h.cast<py::tuple>();
          v.push_back({t[0].cast<Tensor>(), t[1].cast<float>()});
        }
        return Localizer::calc_average_pose(v);
      },
      py::arg("particles"), py::arg("weights") = py::none(),
      "calc_average_pose([(pose, weight), ...]) or calc_average_pose(poses [P,3,4], weights [P])")
    .def("world2camera", &Localizer::world2camera)
    .def("camera2world", &Localizer::camera2world)
    .def("noise_sigmas", &Localizer::noise_sigmas)
    .def("radius", &Localizer::radius)
    .def("infer_height", &Localizer::infer_height)
    .def("infer_width", &Localizer::infer_width)
    .def_property_readonly("renderer", &Localizer::renderer)
    .def_property_readonly("intrinsic", [](Localizer & l) { return l.intrinsic(); });

  // ---- EnvMap ------------------------------------------------------------------------------------
  py::class_<f2n::EnvMap, std::shared_ptr<f2n::EnvMap>>(m, "EnvMap")
    .def(py::init([](int64_t resolution, const std::string & dev) {
           return std::make_shared<f2n::EnvMap>(resolution, parse_device(dev));
         }),
         py::arg("resolution"), py::arg("device") = "",
         "a learned background: a cube map [6,R,R,3] of colour logits, zeros; see env_map.hpp")
    .def("query", &f2n::EnvMap::query, py::arg("dirs"),
         "bg [n,3] of dirs [n,3], differentiable in the texture")
    .def("flags", &f2n::EnvMap::flags, py::call_guard<py::gil_scoped_release>(),
         "bit 0: a non-finite gradient was dropped, bit 1: a contribution was capped; a host read "
         "that resets the flags")
    .def(
      "make_adam",
      [](f2n::EnvMap & e, float lr) {
        AdamHandle h;
        h.opt = std::make_shared<torch::optim::Adam>(e.optim_param_groups(lr));
        return h;
      },
      "torch::optim::Adam over optim_param_groups(lr)")
    .def("zero_grad", [](f2n::EnvMap & e) { e.zero_grad(); })
    .def_property_readonly("resolution", &f2n::EnvMap::resolution)
    .def_property_readonly("texture", [](f2n::EnvMap & e) { return e.texture_; })
    .def_property_readonly("acc", [](f2n::EnvMap & e) { return e.acc_; },
                           "int64 [6*R*R*3]: the fixed-point sums, zero between backwards")
    .def(
      "save",
      [](std::shared_ptr<f2n::EnvMap> e, const std::string & path) { torch::save(e, path); })
    .def(
      "load",
      [](std::shared_ptr<f2n::EnvMap> e, const std::string & path) { torch::load(e, path); });

  // ---- PoseRefiner -------------------------------------------------------------------------------
  py::class_<PoseRefiner, std::shared_ptr<PoseRefiner>>(m, "PoseRefiner")
    .def(py::init([](const Tensor & base) { return std::make_shared<PoseRefiner>(base); }),
         py::arg("base_poses"), "per-image SE(3) corrections of base_poses [E,3|4,4]; see pose_refiner.hpp")
    .def("poses", &PoseRefiner::poses, "the refined poses [E,3,4], differentiable in delta")
    .def("set_fixed", &PoseRefiner::set_fixed, py::arg("mask"))
    .def(
      "sample_random_rays",
      [](PoseRefiner & r, const Tensor & intr, int h, int w, int64_t n,
         const c10::optional<Tensor> & images, const c10::optional<Tensor> & dist,
         const c10::optional<Tensor> & cam_idx, const c10::optional<Tensor> & ij) {
        auto [rays, gt, cam] = r.sample_random_rays(
          intr, h, w, n, opt_tensor(images), opt_tensor(dist), opt_tensor(cam_idx), opt_tensor(ij));
        return py::make_tuple(rays.origins, rays.dirs, gt, cam);
      },
      py::arg("intrinsics"), py::arg("h"), py::arg("w"), py::arg("batch_size"),
      py::arg("images") = py::none(), py::arg("dist") = py::none(), py::arg("cam_idx") = py::none(),
      py::arg("ij") = py::none())
    .def(
      "make_adam",
      [](PoseRefiner & r, float lr) {
        AdamHandle h;
        h.opt = std::make_shared<torch::optim::Adam>(r.optim_param_groups(lr));
        return h;
      },
      "torch::optim::Adam over optim_param_groups(lr)")
    .def("correction_norms", &PoseRefiner::correction_norms, "[E,2]: |omega|, |tau|")
    .def("zero_grad", [](PoseRefiner & r) { r.zero_grad(); })
    .def_property_readonly("n_cameras", &PoseRefiner::n_cameras)
    .def_property_readonly("delta", [](PoseRefiner & r) { return r.delta_; })
    .def_property_readonly("base", [](PoseRefiner & r) { return r.base_; })
    .def_property_readonly("fixed", [](PoseRefiner & r) { return r.fixed_; })
    .def(
      "save",
      [](std::shared_ptr<PoseRefiner> r, const std::string & path) { torch::save(r, path); })
    .def(
      "load",
      [](std::shared_ptr<PoseRefiner> r, const std::string & path) { torch::load(r, path); });

  // ---- IntrinsicsRefiner -------------------------------------------------------------------------
  py::class_<IntrinsicsRefiner, std::shared_ptr<IntrinsicsRefiner>>(m, "IntrinsicsRefiner")
    .def(py::init([](const Tensor & base_K, const c10::optional<Tensor> & base_dist,
                     const c10::optional<Tensor> & group) {
           return std::make_shared<IntrinsicsRefiner>(base_K, opt_tensor(base_dist), opt_tensor(group));
         }),
         py::arg("base_intrinsics"), py::arg("base_dist") = py::none(), py::arg("group") = py::none(),
         "a shared correction of (fx, fy, cx, cy, k1, k2, p1, p2) per physical camera; see "
         "intrinsics_refiner.hpp")
    .def("intrinsics", &IntrinsicsRefiner::intrinsics,
         "the effective intrinsics [E,3,3], differentiable in gamma")
    .def("dist", &IntrinsicsRefiner::dist, "the effective (k1, k2, p1, p2) [E,4], differentiable in gamma")
    .def(
      "calibration",
      [](IntrinsicsRefiner & r) {
        auto [K, D] = r.calibration();
        return py::make_tuple(K, D);
      },
      "(intrinsics, dist) from one launch")
    .def("set_learned", &IntrinsicsRefiner::set_learned, py::arg("mask"),
         "mask: 8 bools for (fx, fy, cx, cy, k1, k2, p1, p2)")
    .def("set_fixed", &IntrinsicsRefiner::set_fixed, py::arg("image_mask"))
    .def(
      "sample_random_rays",
      [](IntrinsicsRefiner & r, const Tensor & poses, int h, int w, int64_t n,
         const c10::optional<Tensor> & images, const c10::optional<Tensor> & cam_idx,
         const c10::optional<Tensor> & ij) {
        auto [rays, gt, cam] = r.sample_random_rays(
          poses, h, w, n, opt_tensor(images), opt_tensor(cam_idx), opt_tensor(ij));
        return py::make_tuple(rays.origins, rays.dirs, gt, cam);
      },
      py::arg("poses"), py::arg("h"), py::arg("w"), py::arg("batch_size"),
      py::arg("images") = py::none(), py::arg("cam_idx") = py::none(), py::arg("ij") = py::none())
    .def(
      "make_adam",
      [](IntrinsicsRefiner & r, float lr) {
        AdamHandle h;
        h.opt = std::make_shared<torch::optim::Adam>(r.optim_param_groups(lr));
        return h;
      },
      "torch::optim::Adam over optim_param_groups(lr)")
    .def("corrections", &IntrinsicsRefiner::corrections,
         "[E,8]: effective minus base (fx, fy, cx, cy, k1, k2, p1, p2)")
    .def("zero_grad", [](IntrinsicsRefiner & r) { r.zero_grad(); })
    .def_property_readonly("n_images", &IntrinsicsRefiner::n_images)
    .def_property_readonly("n_groups", &IntrinsicsRefiner::n_groups)
    .def_property_readonly("gamma", [](IntrinsicsRefiner & r) { return r.gamma_; })
    .def_property_readonly("base_K", [](IntrinsicsRefiner & r) { return r.base_K_; })
    .def_property_readonly("base_dist", [](IntrinsicsRefiner & r) { return r.base_dist_; })
    .def_property_readonly("group", [](IntrinsicsRefiner & r) { return r.group_; })
    .def_property_readonly("learn", [](IntrinsicsRefiner & r) { return r.learn_; })
    .def(
      "save",
      [](std::shared_ptr<IntrinsicsRefiner> r, const std::string & path) { torch::save(r, path); })
    .def(
      "load",
      [](std::shared_ptr<IntrinsicsRefiner> r, const std::string & path) { torch::load(r, path); });

  py::class_<AdamHandle>(m, "Adam")
    .def("step", [](AdamHandle & h) { h.opt->step(); }, py::call_guard<py::gil_scoped_release>())
    .def("zero_grad", [](AdamHandle & h) { h.opt->zero_grad(); })
    .def("n_groups", [](AdamHandle & h) { return h.opt->param_groups().size(); })
    .def("set_lr", [](AdamHandle & h, double lr) {
      for (auto & g : h.opt->param_groups())
        static_cast<torch::optim::AdamOptions &>(g.options()).lr(lr);
    });
}
