// vec3.h -- the float 3-vector of the loss kernels (normals.hip, mesh_losses.hip, point_mesh_geom.h, point_mesh.hip) and quiet_nan().
// Every helper is the float32 operations it spells, in that operand order, one per written operation (-ffp-contract=off): callers
// that are compared with the reference bit for bit rely on it.  Host and device, so that point_mesh_geom.h compiles for both.
#pragma once

#include <math.h>

#include "p3d_common.h"

#define P3D_V3_FN __host__ __device__ __forceinline__

namespace p3d {

struct V3 {
  float x, y, z;
};
P3D_V3_FN V3 mk(float x, float y, float z) { return V3{x, y, z}; }
P3D_V3_FN V3 load3(const float* p) { return V3{p[0], p[1], p[2]}; }
P3D_V3_FN void store3(float* p, V3 a) { p[0] = a.x, p[1] = a.y, p[2] = a.z; }
P3D_V3_FN V3 operator+(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
P3D_V3_FN V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
P3D_V3_FN V3 operator-(V3 a) { return V3{-a.x, -a.y, -a.z}; }
P3D_V3_FN V3 operator*(V3 a, float s) { return V3{a.x * s, a.y * s, a.z * s}; }
P3D_V3_FN V3 operator*(float s, V3 a) { return V3{s * a.x, s * a.y, s * a.z}; }
P3D_V3_FN V3 operator/(V3 a, float s) { return V3{a.x / s, a.y / s, a.z / s}; }
P3D_V3_FN float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
P3D_V3_FN V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
P3D_V3_FN float norm3(V3 a) { return sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }

P3D_V3_FN float quiet_nan() { return __builtin_bit_cast(float, 0x7fc00000u); }

}  // namespace p3d
