// mesh.hpp -- a triangle mesh of the trained density: the logit on a lattice (f2n_density_lattice),
// marching tetrahedra on it (f2n_mesh_count, f2n_mesh_emit) and a PLY writer.
//
// The reference has no counterpart: everything it knows about geometry is per ray
// (src/renderer.cpp:58-90).  Nothing here touches Renderer::render*; the Renderer is only asked for
// its field.  Conventions of the mesh (orders, tetrahedra, winding): mesh.hip's header comment.
#pragma once

#include <array>
#include <string>

#include "common.hpp"
#include "hash_3d_anchored.hpp"
#include "renderer.hpp"

namespace f2n
{

// density = exp(logit - kDensityShift): the shift every render route passes to its kernels
// (reference src/renderer.cpp:62, TruncExp(x - 3)).
constexpr float kDensityShift = 3.f;

struct Mesh
{
  Tensor vertices;   // [V, 3] f32
  Tensor triangles;  // [T, 3] i32, (b - a) x (c - a) points from density above the level to below it
  Tensor normals;    // [V, 3] f32 or undefined
};

// Density logit (shift not subtracted) on the lattice lo + i * step, i < dims, per axis (x, y, z)
// -> [nz, ny, nx], x fastest.  dims >= 2 each, fewer than 2^31 vertices, steps > 0.
Tensor density_lattice(
  Hash3DAnchored & field, const std::array<float, 3> & lo, const std::array<float, 3> & step,
  const std::array<int64_t, 3> & dims);

// The level set values == level of any [nz, ny, nx] f32 lattice on the GPU; inside is value > level.
// One host read (the two totals).  No crossing: two empty tensors.
Mesh marching_tets(
  const Tensor & values, float level, const std::array<float, 3> & lo,
  const std::array<float, 3> & step);

// The surface density == sigma_level of the renderer's field inside the box [lo, hi], sampled on
// dims (x, y, z) vertices: step = (hi - lo) / (dims - 1), level = (float)log((double)sigma_level) +
// kDensityShift.  with_normals: normals = -g / |g| of Hash3DAnchored::density_grad at the vertices
// (pointing out of the dense side, as the triangles' winding does), zero where |g| is not positive.
Mesh extract_mesh(
  Renderer & renderer, const std::array<float, 3> & lo, const std::array<float, 3> & hi,
  const std::array<int64_t, 3> & dims, float sigma_level, bool with_normals);

// Binary little-endian PLY 1.0: float32 x y z [nx ny nz] per vertex, uchar 3 + three int32 per face.
// Tensors on either device.
void save_ply(
  const std::string & path, const Tensor & vertices, const Tensor & triangles,
  const Tensor & normals = Tensor());

}  // namespace f2n
