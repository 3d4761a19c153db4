// face_gather.h -- `face_verts[f] = verts_packed[faces_packed[f]]` for ONE face, and the per-face record that goes with it.
//
// Shared by the stand-alone gather (gather.hip: p3d_gather_face_verts_pre) and by the count pass of the binning when the
// rasterizer's entry takes packed vertices (binning.hip: bin_count_kernel<kTriangles, true, true>): the two must write the same
// bytes, so there is one function for the index rules and one for what is stored.
#pragma once

#include "p3d_geom.h"

namespace p3d {

// Indices follow torch indexing: a negative id wraps once (v + V).  torch device-asserts on ids still out of range; here nothing
// outside `verts` is ever touched and the corner gets NaN coordinates (visible downstream, never silent garbage).
__device__ __forceinline__ void gather_face_corners(const float* __restrict__ verts, const int64_t* __restrict__ faces, int64_t V,
                                                    int64_t f, float c[9]) {
  const float nan = __int_as_float(0x7fc00000);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int64_t v = faces[f * 3 + k];
    if (v < 0) v += V;
    const bool ok = v >= 0 && v < V;
    const float* s = verts + (ok ? v : 0) * 3;
    c[3 * k + 0] = ok ? s[0] : nan;
    c[3 * k + 1] = ok ? s[1] : nan;
    c[3 * k + 2] = ok ? s[2] : nan;
  }
}

// face_verts[f] = c; face_pre[f] = the record of p3d_geom.h: BwdFacePre (face_pre null: none)
__device__ __forceinline__ void store_face(const float c[9], int64_t f, float* __restrict__ face_verts, float4* __restrict__ face_pre) {
  float* d = face_verts + f * 9;
#pragma unroll
  for (int k = 0; k < 9; ++k) d[k] = c[k];
  if (face_pre != nullptr) {
    const BwdFacePre r = bwd_face_pre_make(mk3(c[0], c[1], c[2]), mk3(c[3], c[4], c[5]), mk3(c[6], c[7], c[8]));
    face_pre[f] = make_float4(r.inv_area, r.inv_l01, r.inv_l02, r.inv_l12);
  }
}

}  // namespace p3d
