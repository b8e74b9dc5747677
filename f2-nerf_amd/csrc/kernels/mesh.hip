// mesh.hip -- marching tetrahedra on a scalar lattice: an indexed triangle mesh of the level set
// values == level, welded by construction.  Independent of the field: values is any [nz, ny, nx] f32.
// The reference has no mesher (its geometry is per ray, src/renderer.cpp:58-90).
//
//   f2n_mesh_count  one lane per lattice vertex, lanes along x: the vertex's 7-bit crossing mask, its
//                   number of mesh vertices and its cell's number of triangles.
//   f2n_mesh_emit   the same mapping, after exclusive scans of the two counts (host): writes the
//                   vertices and the triangles at their scanned places.  Every store is checked
//                   against the totals it is given.
//
// Conventions, fixed here once (tests/mesh_model.py restates them):
//   lattice   vertex (x, y, z) has lattice index (z ny + y) nx + x, position fmaf((float)i, step, lo)
//             per axis, and is INSIDE iff value > level (NaN is outside).
//   edges     direction d = dx + 2 dy + 4 dz in 1..7; vertex a owns the edges a -> a + d whose far end
//             exists.  An owned edge whose ends differ carries one mesh vertex (mask bit d - 1):
//             t = (level - s_a) / (s_b - s_a), t = 0.5 if !(t >= 0 && t <= 1),
//             p = fmaf(t, p_b - p_a, p_a) per axis.  Vertices are ordered by (owner, d); the index of
//             (owner, d) is voff[owner] + popcount(mask[owner] & ((1 << (d - 1)) - 1)).
//   cells     cell = its low-corner vertex, six Kuhn tetrahedra 0, c1, c2, 7 (corners as direction
//             bits) in the lexicographic order of the axes' permutations:
//               k: 0 xyz (1, 3) +   1 xzy (1, 5) -   2 yxz (2, 3) -   3 yzx (2, 6) +   4 zxy (4, 5) +
//                  5 zyx (4, 6) -        (c1, c2) and the sign of det[c1, c2, 7]
//             local corners 0..3 in that order, local edges 0..5 = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).
//   triangles for a positive tetrahedron (a negative one swaps the 2nd and 3rd vertex):
//               one inside corner p, q < r < s the others with r, s swapped if (p q r s) is odd:
//                 (pq, pr, ps); one outside corner p: (pq, ps, pr);
//               two inside P < Q, R < S the others swapped if (P Q R S) is odd: the quad PR PS QS QR
//                 split along PR - QS: (PR, PS, QS) then (PR, QS, QR).
//             (b - a) x (c - a) points from the inside corners to the outside ones.  Triangles are
//             ordered by (cell, tetrahedron, triangle).  kCases packs this table: 3 bits per local
//             edge, triangle 0 in bits 0-8, triangle 1 in bits 9-17, the count in bits 18-19.
#include "common.hiph"

namespace
{

__constant__ const uint32_t kCases[16] = {
  0x0,     0x40088, 0x400e0, 0x9c311, 0x40159, 0xab4c2, 0x8d160, 0x40162,
  0x4012a, 0xa5148, 0xaa683, 0x400e9, 0x94319, 0x40118, 0x40050, 0x0};

template <int K>
struct Tet
{
  static constexpr int c1 = (K < 2) ? 1 : (K < 4) ? 2 : 4;
  static constexpr int c2 = (K == 0 || K == 2) ? 3 : (K == 1 || K == 4) ? 5 : 6;
  static constexpr bool positive = (K == 0 || K == 3 || K == 4);
};

struct LatticeVertex
{
  int64_t i;
  int x, y, z;
  bool ex, ey, ez;  // the neighbour at +1 along the axis exists
};

__device__ __forceinline__ bool lattice_vertex(int nx, int ny, int nz, LatticeVertex & v)
{
  // (fewer than 2^31 vertices: 32-bit divisions)
  const uint32_t i = blockIdx.x * (uint32_t)F2N_BLOCK + threadIdx.x;
  if (i >= (uint32_t)nx * (uint32_t)ny * (uint32_t)nz) return false;
  const uint32_t yz = i / (uint32_t)nx;
  v.i = i;
  v.x = (int)(i - yz * (uint32_t)nx);
  v.y = (int)(yz % (uint32_t)ny);
  v.z = (int)(yz / (uint32_t)ny);
  v.ex = v.x + 1 < nx;
  v.ey = v.y + 1 < ny;
  v.ez = v.z + 1 < nz;
  return true;
}

// Offset of cell corner c from the vertex, with a step along an axis dropped where the lattice ends:
// no load leaves the lattice.  (Such a corner is another vertex, not the one asked for:
// crossing_mask takes the edges to it out again, and cells are formed only where all three exist.)
template <int C>
__device__ __forceinline__ int64_t corner_offset(const LatticeVertex & v, int nx, int ny)
{
  return (((C & 1) && v.ex) ? 1 : 0) + (((C & 2) && v.ey) ? (int64_t)nx : 0) +
         (((C & 4) && v.ez) ? (int64_t)nx * ny : 0);
}

__device__ __forceinline__ void load_corners(
  const float * __restrict__ values, const LatticeVertex & v, int nx, int ny, float s[8])
{
  s[0] = values[v.i + corner_offset<0>(v, nx, ny)];
  s[1] = values[v.i + corner_offset<1>(v, nx, ny)];
  s[2] = values[v.i + corner_offset<2>(v, nx, ny)];
  s[3] = values[v.i + corner_offset<3>(v, nx, ny)];
  s[4] = values[v.i + corner_offset<4>(v, nx, ny)];
  s[5] = values[v.i + corner_offset<5>(v, nx, ny)];
  s[6] = values[v.i + corner_offset<6>(v, nx, ny)];
  s[7] = values[v.i + corner_offset<7>(v, nx, ny)];
}

// bit c = corner c is inside
__device__ __forceinline__ uint32_t inside_bits(const float s[8], float level)
{
  uint32_t in = 0;
#pragma unroll
  for (int c = 0; c < 8; c++) in |= (s[c] > level ? 1u : 0u) << c;
  return in;
}

// bit d - 1 = the edge to corner d exists and crosses
__device__ __forceinline__ uint32_t crossing_mask(uint32_t in, const LatticeVertex & v)
{
  const uint32_t exists = (v.ex ? 0x7fu : 0x2au) & (v.ey ? 0x7fu : 0x19u) & (v.ez ? 0x7fu : 0x07u);
  return ((in >> 1) ^ (0u - (in & 1u))) & exists;
}

template <int K>
__device__ __forceinline__ uint32_t tet_code(uint32_t in)
{
  return (in & 1u) | (((in >> Tet<K>::c1) & 1u) << 1) | (((in >> Tet<K>::c2) & 1u) << 2) |
         (((in >> 7) & 1u) << 3);
}

__global__ __launch_bounds__(F2N_BLOCK) void mesh_count_kernel(
  const float * __restrict__ values, uint8_t * __restrict__ mask, uint8_t * __restrict__ vcount,
  uint8_t * __restrict__ tcount, int nx, int ny, int nz, float level)
{
  LatticeVertex v;
  if (!lattice_vertex(nx, ny, nz, v)) return;
  float s[8];
  load_corners(values, v, nx, ny, s);
  const uint32_t in = inside_bits(s, level);
  const uint32_t m = crossing_mask(in, v);
  uint32_t tris = 0;
  if (v.ex && v.ey && v.ez) {
    tris = (kCases[tet_code<0>(in)] >> 18) + (kCases[tet_code<1>(in)] >> 18) +
           (kCases[tet_code<2>(in)] >> 18) + (kCases[tet_code<3>(in)] >> 18) +
           (kCases[tet_code<4>(in)] >> 18) + (kCases[tet_code<5>(in)] >> 18);
  }
  mask[v.i] = (uint8_t)m;
  vcount[v.i] = (uint8_t)__popc(m);
  tcount[v.i] = (uint8_t)tris;
}

__device__ __forceinline__ int64_t pick6(
  uint32_t e, int64_t a0, int64_t a1, int64_t a2, int64_t a3, int64_t a4, int64_t a5)
{
  return e == 0 ? a0 : e == 1 ? a1 : e == 2 ? a2 : e == 3 ? a3 : e == 4 ? a4 : a5;
}

// Index of the mesh vertex on the edge from cell corner A to cell corner B (A a subset of B).
template <int A, int B>
__device__ __forceinline__ int64_t edge_vertex(const int64_t vo[7], const uint32_t mk[7])
{
  return vo[A] + __popc(mk[A] & ((1u << (B - A - 1)) - 1u));
}

template <int K>
__device__ __forceinline__ void emit_tet(
  uint32_t in, const int64_t vo[7], const uint32_t mk[7], int32_t * __restrict__ triangles,
  int64_t n_triangles, int64_t & slot)
{
  constexpr int c1 = Tet<K>::c1, c2 = Tet<K>::c2;
  const uint32_t word = kCases[tet_code<K>(in)];
  const uint32_t n = word >> 18;
  if (n == 0) return;
  const int64_t e0 = edge_vertex<0, c1>(vo, mk), e1 = edge_vertex<0, c2>(vo, mk),
                e2 = edge_vertex<0, 7>(vo, mk), e3 = edge_vertex<c1, c2>(vo, mk),
                e4 = edge_vertex<c1, 7>(vo, mk), e5 = edge_vertex<c2, 7>(vo, mk);
#pragma unroll
  for (int j = 0; j < 2; j++) {
    if ((uint32_t)j >= n) break;
    const uint32_t tri = word >> (9 * j);
    const int64_t a = pick6(tri & 7u, e0, e1, e2, e3, e4, e5);
    int64_t b = pick6((tri >> 3) & 7u, e0, e1, e2, e3, e4, e5);
    int64_t c = pick6((tri >> 6) & 7u, e0, e1, e2, e3, e4, e5);
    if (!Tet<K>::positive) {
      const int64_t t = b;
      b = c;
      c = t;
    }
    if (slot >= 0 && slot < n_triangles) {
      triangles[3 * slot] = (int32_t)a;
      triangles[3 * slot + 1] = (int32_t)b;
      triangles[3 * slot + 2] = (int32_t)c;
    }
    slot++;
  }
}

template <int D>
__device__ __forceinline__ void emit_vertex(
  uint32_t m, const float s[8], float level, const float pa[3], const float pb[3],
  float * __restrict__ vertices, int64_t n_vertices, int64_t & idx)
{
  if (!((m >> (D - 1)) & 1u)) return;
  float t = (level - s[0]) / (s[D] - s[0]);
  if (!(t >= 0.f && t <= 1.f)) t = 0.5f;
  if (idx >= 0 && idx < n_vertices) {
    vertices[3 * idx] = (D & 1) ? fmaf(t, pb[0] - pa[0], pa[0]) : pa[0];
    vertices[3 * idx + 1] = (D & 2) ? fmaf(t, pb[1] - pa[1], pa[1]) : pa[1];
    vertices[3 * idx + 2] = (D & 4) ? fmaf(t, pb[2] - pa[2], pa[2]) : pa[2];
  }
  idx++;
}

__global__ __launch_bounds__(F2N_BLOCK) void mesh_emit_kernel(
  const float * __restrict__ values, const uint8_t * __restrict__ mask,
  const int64_t * __restrict__ voff, const int64_t * __restrict__ toff,
  float * __restrict__ vertices, int32_t * __restrict__ triangles, int64_t n_vertices,
  int64_t n_triangles, float lo_x, float lo_y, float lo_z, float step_x, float step_y, float step_z,
  float level, int nx, int ny, int nz)
{
  LatticeVertex v;
  if (!lattice_vertex(nx, ny, nz, v)) return;
  float s[8];
  load_corners(values, v, nx, ny, s);
  const uint32_t m = mask[v.i];
  if (m) {
    const float pa[3] = {
      fmaf((float)v.x, step_x, lo_x), fmaf((float)v.y, step_y, lo_y), fmaf((float)v.z, step_z, lo_z)};
    const float pb[3] = {
      fmaf((float)(v.x + 1), step_x, lo_x), fmaf((float)(v.y + 1), step_y, lo_y),
      fmaf((float)(v.z + 1), step_z, lo_z)};
    int64_t idx = voff[v.i];
    emit_vertex<1>(m, s, level, pa, pb, vertices, n_vertices, idx);
    emit_vertex<2>(m, s, level, pa, pb, vertices, n_vertices, idx);
    emit_vertex<3>(m, s, level, pa, pb, vertices, n_vertices, idx);
    emit_vertex<4>(m, s, level, pa, pb, vertices, n_vertices, idx);
    emit_vertex<5>(m, s, level, pa, pb, vertices, n_vertices, idx);
    emit_vertex<6>(m, s, level, pa, pb, vertices, n_vertices, idx);
    emit_vertex<7>(m, s, level, pa, pb, vertices, n_vertices, idx);
  }
  if (!(v.ex && v.ey && v.ez)) return;
  const uint32_t in = inside_bits(s, level);
  if (in == 0u || in == 0xffu) return;  // no corner differs from corner 0: no tetrahedron is mixed
  // the seven corners that own an edge of this cell (corner 7 owns none); all of them exist here
  int64_t vo[7];
  uint32_t mk[7];
#pragma unroll
  for (int c = 0; c < 7; c++) {
    const int64_t at = v.i + ((c & 1) ? 1 : 0) + ((c & 2) ? (int64_t)nx : 0) +
                       ((c & 4) ? (int64_t)nx * ny : 0);
    vo[c] = voff[at];
    mk[c] = mask[at];
  }
  int64_t slot = toff[v.i];
  emit_tet<0>(in, vo, mk, triangles, n_triangles, slot);
  emit_tet<1>(in, vo, mk, triangles, n_triangles, slot);
  emit_tet<2>(in, vo, mk, triangles, n_triangles, slot);
  emit_tet<3>(in, vo, mk, triangles, n_triangles, slot);
  emit_tet<4>(in, vo, mk, triangles, n_triangles, slot);
  emit_tet<5>(in, vo, mk, triangles, n_triangles, slot);
}

int lattice_status(int nx, int ny, int nz)
{
  if (nx < 2 || ny < 2 || nz < 2) return F2N_E_INVALID_ARG;
  if ((int64_t)nx * ny >= ((int64_t)1 << 31) || (int64_t)nx * ny * nz >= ((int64_t)1 << 31))
    return F2N_E_INVALID_ARG;
  return F2N_OK;
}

}  // namespace

extern "C" int f2n_mesh_count(
  const float * values, uint8_t * mask, uint8_t * vcount, uint8_t * tcount, int nx, int ny, int nz,
  float level, void * stream)
{
  if (const int st = lattice_status(nx, ny, nz)) return st;
  if (!values || !mask || !vcount || !tcount) return F2N_E_INVALID_ARG;
  const int64_t n = (int64_t)nx * ny * nz;
  hipLaunchKernelGGL(
    mesh_count_kernel, dim3(f2n_div_up(n, F2N_BLOCK)), dim3(F2N_BLOCK), 0, (hipStream_t)stream,
    values, mask, vcount, tcount, nx, ny, nz, level);
  return f2n_launch_status();
}

extern "C" int f2n_mesh_emit(
  const float * values, const uint8_t * mask, const int64_t * voff, const int64_t * toff,
  float * vertices, int32_t * triangles, int64_t n_vertices, int64_t n_triangles, float lo_x,
  float lo_y, float lo_z, float step_x, float step_y, float step_z, float level, int nx, int ny,
  int nz, void * stream)
{
  if (const int st = lattice_status(nx, ny, nz)) return st;
  if (!(step_x > 0.f) || !(step_y > 0.f) || !(step_z > 0.f)) return F2N_E_INVALID_ARG;
  if (n_vertices < 0 || n_triangles < 0) return F2N_E_INVALID_ARG;
  if (n_vertices >= ((int64_t)1 << 31) || 3 * n_triangles >= ((int64_t)1 << 31))
    return F2N_E_UNSUPPORTED;
  if (n_vertices == 0 && n_triangles == 0) return F2N_OK;
  // a triangle has three vertices, a vertex lies on at least one triangle
  if (n_vertices == 0 || n_triangles == 0) return F2N_E_INVALID_ARG;
  if (!values || !mask || !voff || !toff || !vertices || !triangles) return F2N_E_INVALID_ARG;
  const int64_t n = (int64_t)nx * ny * nz;
  hipLaunchKernelGGL(
    mesh_emit_kernel, dim3(f2n_div_up(n, F2N_BLOCK)), dim3(F2N_BLOCK), 0, (hipStream_t)stream,
    values, mask, voff, toff, vertices, triangles, n_vertices, n_triangles, lo_x, lo_y, lo_z, step_x,
    step_y, step_z, level, nx, ny, nz);
  return f2n_launch_status();
}
