// mesh.cpp -- see mesh.hpp.
#include "mesh.hpp"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <vector>

#include "kernel_timer.hpp"

namespace f2n
{

namespace
{

void check_lattice(const std::array<int64_t, 3> & dims, const std::array<float, 3> & step)
{
  for (int a = 0; a < 3; a++) {
    TORCH_CHECK(dims[a] >= 2, "a lattice needs at least 2 vertices along every axis");
    TORCH_CHECK(step[a] > 0.f, "lattice steps must be positive");
  }
  TORCH_CHECK(
    dims[0] < ((int64_t)1 << 31) && dims[1] < ((int64_t)1 << 31) && dims[2] < ((int64_t)1 << 31) &&
      dims[0] * dims[1] < ((int64_t)1 << 31) && dims[0] * dims[1] * dims[2] < ((int64_t)1 << 31),
    "a lattice holds fewer than 2^31 vertices");
}

}  // namespace

Tensor density_lattice(
  Hash3DAnchored & field, const std::array<float, 3> & lo, const std::array<float, 3> & step,
  const std::array<int64_t, 3> & dims)
{
  torch::NoGradGuard no_grad;
  check_lattice(dims, step);
  TORCH_CHECK(
    field.feat_pool_.is_cuda(),
    "the field must live on the GPU: the F2-NeRF hot path has no CPU implementation in this library");
  const Tensor table16 = field.table_f16();
  const FieldArgs g = field.kernel_args(table16);
  const auto head = field.density_head();
  Tensor logit = torch::empty({dims[2], dims[1], dims[0]}, float_on(table16.device()));
  void * stream = current_stream(table16);
  ScopedKernelTimer timer("density_lattice", stream, (double)logit.numel());
  check(
    f2n_density_lattice(
      g.table, g.primes, g.bias, g.mul, head.first.data_ptr<float>(),
      head.second.data_ptr<float>(), logit.data_ptr<float>(), lo[0], lo[1], lo[2], step[0], step[1],
      step[2], (int)dims[0], (int)dims[1], (int)dims[2], g.L_walk, g.F, g.T, g.level_stride, stream),
    "f2n_density_lattice");
  return logit;
}

Mesh marching_tets(
  const Tensor & values_in, float level, const std::array<float, 3> & lo,
  const std::array<float, 3> & step)
{
  torch::NoGradGuard no_grad;
  const Tensor values = dev_f32(values_in.detach(), "values");
  TORCH_CHECK(values.dim() == 3, "values must be [nz, ny, nx]");
  const std::array<int64_t, 3> dims = {values.size(2), values.size(1), values.size(0)};
  check_lattice(dims, step);
  const int nx = (int)dims[0], ny = (int)dims[1], nz = (int)dims[2];
  const int64_t n = values.numel();
  const auto u8 = torch::TensorOptions().dtype(torch::kUInt8).device(values.device());
  Tensor mask = torch::empty({n}, u8), vcount = torch::empty({n}, u8), tcount = torch::empty({n}, u8);
  void * stream = current_stream(values);
  ScopedKernelTimer timer("marching_tets", stream, (double)n);
  check(
    f2n_mesh_count(
      values.data_ptr<float>(), mask.data_ptr<uint8_t>(), vcount.data_ptr<uint8_t>(),
      tcount.data_ptr<uint8_t>(), nx, ny, nz, level, stream),
    "f2n_mesh_count");
  // exclusive scans in int64 (plumbing), then the one host read
  const Tensor vincl = torch::cumsum(vcount, 0, torch::kInt64);
  const Tensor tincl = torch::cumsum(tcount, 0, torch::kInt64);
  const Tensor totals = torch::stack({vincl[n - 1], tincl[n - 1]}).cpu();
  const int64_t V = totals[0].item<int64_t>(), T = totals[1].item<int64_t>();
  TORCH_CHECK(
    V < ((int64_t)1 << 31) && 3 * T < ((int64_t)1 << 31), "the mesh has ", V, " vertices and ", T,
    " triangles: more than int32 indices hold; extract a coarser lattice or a smaller box");
  Mesh mesh;
  mesh.vertices = torch::empty({V, 3}, values.options());
  mesh.triangles = torch::empty({T, 3}, int_on(values.device()));
  if (V == 0 && T == 0) return mesh;
  const Tensor voff = vincl - vcount, toff = tincl - tcount;
  check(
    f2n_mesh_emit(
      values.data_ptr<float>(), mask.data_ptr<uint8_t>(), voff.data_ptr<int64_t>(),
      toff.data_ptr<int64_t>(), mesh.vertices.data_ptr<float>(),
      mesh.triangles.data_ptr<int32_t>(), V, T, lo[0], lo[1], lo[2], step[0], step[1], step[2],
      level, nx, ny, nz, stream),
    "f2n_mesh_emit");
  return mesh;
}

Mesh extract_mesh(
  Renderer & renderer, const std::array<float, 3> & lo, const std::array<float, 3> & hi,
  const std::array<int64_t, 3> & dims, float sigma_level, bool with_normals)
{
  torch::NoGradGuard no_grad;
  TORCH_CHECK(sigma_level > 0.f, "sigma_level must be positive");
  std::array<float, 3> step;
  for (int a = 0; a < 3; a++) {
    TORCH_CHECK(dims[a] >= 2, "a lattice needs at least 2 vertices along every axis");
    TORCH_CHECK(hi[a] > lo[a], "the box must have hi > lo along every axis");
    step[a] = (hi[a] - lo[a]) / (float)(dims[a] - 1);
  }
  const float level = (float)std::log((double)sigma_level) + kDensityShift;
  Hash3DAnchored & field = *renderer.scene_field_;
  Mesh mesh = marching_tets(density_lattice(field, lo, step, dims), level, lo, step);
  if (!with_normals) return mesh;
  if (mesh.vertices.size(0) == 0) {
    mesh.normals = torch::empty({0, 3}, mesh.vertices.options());
    return mesh;
  }
  const Tensor g = field.density_grad(mesh.vertices);
  const Tensor len = (g * g).sum(1, /*keepdim=*/true).sqrt();
  mesh.normals = torch::where(len > 0, -g / len, torch::zeros_like(g)).contiguous();
  return mesh;
}

void save_ply(
  const std::string & path, const Tensor & vertices_in, const Tensor & triangles_in,
  const Tensor & normals_in)
{
  TORCH_CHECK(
    vertices_in.defined() && vertices_in.dim() == 2 && vertices_in.size(1) == 3 &&
      vertices_in.scalar_type() == torch::kFloat32,
    "vertices must be [V, 3] float32");
  TORCH_CHECK(
    triangles_in.defined() && triangles_in.dim() == 2 && triangles_in.size(1) == 3 &&
      triangles_in.scalar_type() == torch::kInt32,
    "triangles must be [T, 3] int32");
  const bool with_normals = normals_in.defined();
  TORCH_CHECK(
    !with_normals ||
      (normals_in.dim() == 2 && normals_in.size(0) == vertices_in.size(0) &&
       normals_in.size(1) == 3 && normals_in.scalar_type() == torch::kFloat32),
    "normals must be [V, 3] float32");
  const uint16_t probe = 1;
  TORCH_CHECK(
    *reinterpret_cast<const uint8_t *>(&probe) == 1, "save_ply writes the host's byte order: little-endian only");
  const int64_t V = vertices_in.size(0), T = triangles_in.size(0);
  Tensor rows = vertices_in.detach().cpu();
  if (with_normals) rows = torch::cat({rows, normals_in.detach().cpu()}, 1);
  rows = rows.contiguous();
  const Tensor tri = triangles_in.detach().cpu().contiguous();

  std::ofstream out(path, std::ios::binary | std::ios::trunc);
  TORCH_CHECK(out.good(), "cannot open ", path, " for writing");
  out << "ply\nformat binary_little_endian 1.0\ncomment density level set, marching tetrahedra\n"
      << "element vertex " << V << "\nproperty float x\nproperty float y\nproperty float z\n";
  if (with_normals) out << "property float nx\nproperty float ny\nproperty float nz\n";
  out << "element face " << T << "\nproperty list uchar int vertex_indices\nend_header\n";
  out.write(reinterpret_cast<const char *>(rows.data_ptr<float>()), (std::streamsize)(rows.numel() * 4));
  std::vector<char> faces((size_t)T * 13);
  const int32_t * idx = tri.data_ptr<int32_t>();
  for (int64_t t = 0; t < T; t++) {
    faces[(size_t)t * 13] = 3;
    std::memcpy(&faces[(size_t)t * 13 + 1], idx + 3 * t, 12);
  }
  out.write(faces.data(), (std::streamsize)faces.size());
  out.close();
  TORCH_CHECK(out.good(), "writing ", path, " failed");
}

}  // namespace f2n
