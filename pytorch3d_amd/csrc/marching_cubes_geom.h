// marching_cubes_geom.h -- the pieces of marching cubes shared by the kernels and the host loop of marching_cubes.hip (as box3d_geom.h
// is shared by box3d.hip's): the inside test, the vertex on a crossed lattice edge, the distinctness test of two vertices and the map
// to local coordinates.  The contract of the reference's compiled CPU operator (implicit_abi.h: p3di_marching_cubes_*): plain float32
// expressions, every product and sum a rounding of its own (the build has -ffp-contract=off), an IEEE division.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define P3D_HD __host__ __device__ __forceinline__
#else
#define P3D_HD inline
#endif

namespace p3d {

constexpr float kMcEps = 1e-5f;

// a corner is inside iff its value is below the isolevel, strictly; NaN on either side: outside
P3D_HD bool mc_inside(float value, float iso) { return value < iso; }

// The vertex on the edge from lattice point (x, y, z), value v1, one step along `axis` (0 = x, 1 = y, 2 = z) to the point of value v2.
// All three coordinates go through p1 (1 - r) + p2 r, the two that do not vary included: c (1 - r) + c r is not always c.
P3D_HD void mc_edge_vertex(float iso, float v1, float v2, int x, int y, int z, int axis, float out[3]) {
  const float p1[3] = {(float)x, (float)y, (float)z};
  const float p2[3] = {(float)(x + (axis == 0)), (float)(y + (axis == 1)), (float)(z + (axis == 2))};
  int snap = 0;  // 1: the vertex is p1, 2: it is p2
  if (fabsf(iso - v1) < kMcEps) {
    snap = 1;
  } else if (fabsf(iso - v2) < kMcEps) {
    snap = 2;
  } else if (fabsf(v1 - v2) < kMcEps) {
    snap = 1;
  }
  const float r = (iso - v1) / (v2 - v1);
  const float s = 1.0f - r;
  for (int c = 0; c < 3; ++c) out[c] = snap == 1 ? p1[c] : snap == 2 ? p2[c] : p1[c] * s + p2[c] * r;
}

// the reference's Vertex::operator!=: at least 1e-5 apart in some coordinate (a NaN difference: not apart).  A triangle is kept iff
// its three vertices differ pairwise by this test.
P3D_HD bool mc_differ(const float* a, const float* b) {
  return fabsf(a[0] - b[0]) >= kMcEps || fabsf(a[1] - b[1]) >= kMcEps || fabsf(a[2] - b[2]) >= kMcEps;
}

// world coordinate c on an axis of `size` lattice points -> [-1, 1]: c / ((size - 1) / 2) - 1
P3D_HD float mc_local(float c, int size) { return c / ((float)(size - 1) * 0.5f) - 1.0f; }

}  // namespace p3d
