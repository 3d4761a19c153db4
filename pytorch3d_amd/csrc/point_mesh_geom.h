// point_mesh_geom.h -- squared distances point -> segment and point -> triangle in 3D and their gradients, float32
// (pytorch3d/csrc/utils/geometry_utils.h: PointLine3Distance*, PointTriangle3Distance*, IsInsideTriangle; the formulas restated).
// Shared by the forward kernels of point_mesh.hip, its backward and the ordered backward of ordered_bwd.hip, so that forward and
// backward take the same branch for the same pair.  Every operation is a float32 operation of its own (-ffp-contract=off).
//
// What depends on the primitive alone lives in a record (Seg, Tri) that is built once -- per tile for a target, per lane for a query
// -- by make_seg / make_tri and holds the very float32 values a per-pair evaluation would compute.
//   segment   l2 = |v1 - v0|^2 <= 1e-8: the distance to v1.  Else the distance to v0 + clamp(t, 0, 1) (v1 - v0).
//   triangle  with n the unit normal, t = (v0 - p) . n and p0 = p + t n: "inside" when the face's area is at least
//             min_triangle_area, |n| > 1e-8 and the three barycentric coordinates of p0 lie in [0, 1]; then the distance is t^2.
//             Otherwise the smallest of the three edge distances; the backward picks the edge by the cascade e01, e02, e12 with <=.
#pragma once

#include <float.h>

#include "vec3.h"

namespace p3d {
namespace pm {

#define P3D_PM_FN __host__ __device__ __forceinline__

constexpr float kEps = 1e-8f;  // kEpsilon and vEpsilon of geometry_utils.h

enum Kind { kPoint = 0, kSeg = 1, kTri = 2 };
__host__ __device__ constexpr int kind_floats(int kind) { return kind == kPoint ? 3 : (kind == kSeg ? 6 : 9); }

struct Seg {
  V3 v0, v1, d;  // d = v1 - v0
  float l2;      // d . d
};

struct Tri {
  V3 v0, v1, v2;
  V3 e01, e02, e12;               // v1 - v0, v2 - v0, v2 - v1
  V3 n;                           // cross(e02, e01) / (|.| + 1e-8)
  float d00, d01, d11, l12;       // e01.e01, e01.e02, e02.e02, e12.e12 (d00, d11, l12: the edges' squared lengths)
  float denom;                    // d00 d11 - d01 d01 + 1e-8
  float norm;                     // |cross(e02, e01)|
  float ok;                       // 1: area >= min_triangle_area and norm > 1e-8 (the inside branch is possible), else 0
};

P3D_PM_FN Seg make_seg(V3 v0, V3 v1) {
  Seg s;
  s.v0 = v0, s.v1 = v1, s.d = v1 - v0;
  s.l2 = dot(s.d, s.d);
  return s;
}

P3D_PM_FN Tri make_tri(V3 v0, V3 v1, V3 v2, double min_triangle_area) {
  Tri f;
  f.v0 = v0, f.v1 = v1, f.v2 = v2;
  f.e01 = v1 - v0, f.e02 = v2 - v0, f.e12 = v2 - v1;
  const V3 raw = cross(f.e02, f.e01);
  f.norm = sqrtf(dot(raw, raw));
  f.n = raw / (f.norm + kEps);
  const V3 c = cross(f.e01, f.e02);
  const double area = (double)hypotf(c.x, hypotf(c.y, c.z)) / 2.0;
  f.d00 = dot(f.e01, f.e01), f.d01 = dot(f.e01, f.e02), f.d11 = dot(f.e02, f.e02), f.l12 = dot(f.e12, f.e12);
  f.denom = f.d00 * f.d11 - f.d01 * f.d01 + kEps;
  f.ok = (!(area < min_triangle_area) && f.norm > kEps) ? 1.0f : 0.0f;
  return f;
}

// |p - segment|^2 from the segment's record
P3D_PM_FN float seg_dist_parts(V3 p, V3 v0, V3 v1, V3 d, float l2) {
  const V3 pv1 = p - v1;
  const float at_v1 = dot(pv1, pv1);
  const float t = dot(d, p - v0) / l2;
  const float tt = fminf(fmaxf(t, 0.0f), 1.0f);
  const V3 diff = p - (v0 + tt * d);
  const float on = dot(diff, diff);
  return l2 <= kEps ? at_v1 : on;
}
P3D_PM_FN float seg_dist(V3 p, const Seg& s) { return seg_dist_parts(p, s.v0, s.v1, s.d, s.l2); }

// The plane part of a (point, triangle) pair: t and whether the distance is t^2
P3D_PM_FN bool tri_inside(V3 p, const Tri& f, float* t_out) {
  const float t = dot(f.v0 - p, f.n);
  const V3 p0 = p + t * f.n;
  const V3 p2 = p0 - f.v0;
  const float d20 = dot(p2, f.e01), d21 = dot(p2, f.e02);
  const float w1 = (f.d11 * d20 - f.d01 * d21) / f.denom;
  const float w2 = (f.d00 * d21 - f.d01 * d20) / f.denom;
  const float w0 = 1.0f - w1 - w2;
  *t_out = t;
  return f.ok != 0.0f && 0.0f <= w0 && w0 <= 1.0f && 0.0f <= w1 && w1 <= 1.0f && 0.0f <= w2 && w2 <= 1.0f;
}

P3D_PM_FN float tri_dist(V3 p, const Tri& f) {
  float t;
  const bool inside = tri_inside(p, f, &t);
  const float e01 = seg_dist_parts(p, f.v0, f.v1, f.e01, f.d00);
  const float e02 = seg_dist_parts(p, f.v0, f.v2, f.e02, f.d11);
  const float e12 = seg_dist_parts(p, f.v1, f.v2, f.e12, f.l12);
  float dist = (e01 > e02) ? e02 : e01;
  dist = (dist > e12) ? e12 : dist;
  return inside ? t * t : dist;
}

// ---- gradients: of g * distance with respect to the point and the primitive's vertices ------------------------------------------
struct SegGrad {
  V3 p, v0, v1;
};
struct TriGrad {
  V3 p, v0, v1, v2;
};

P3D_PM_FN SegGrad seg_backward(V3 p, V3 v0, V3 v1, float g) {
  const V3 zero = mk(0.0f, 0.0f, 0.0f);
  SegGrad r{zero, zero, zero};
  const V3 d = v1 - v0, pv0 = p - v0;
  const float t_bot = dot(d, d), t_top = dot(d, pv0);
  const float tt = t_top / t_bot;
  if (t_bot < kEps) {  // v0 == v1: the distance is read as half of each end's
    r.p = (g * 2.0f) * pv0;
    r.v0 = -0.5f * r.p;
    r.v1 = r.v0;
  } else if (tt < 0.0f) {
    r.p = (g * 2.0f) * pv0;
    r.v0 = -1.0f * r.p;
  } else if (tt > 1.0f) {
    r.p = (g * 2.0f) * (p - v1);
    r.v1 = -1.0f * r.p;
  } else {
    const V3 diff = p - (v0 + tt * d);
    const V3 base = (g * 2.0f) * diff;
    const float bd = dot(base, d);
    r.p = base - (bd * d) / t_bot;
    const V3 dtt_v0 = (((-1.0f * d) - pv0) + ((2.0f * tt) * d)) / t_bot;
    r.v0 = ((-1.0f + tt) * base) - (bd * dtt_v0);
    const V3 dtt_v1 = (pv0 - ((2.0f * tt) * d)) / t_bot;
    r.v1 = ((-bd) * dtt_v1) - (tt * base);
  }
  return r;
}

P3D_PM_FN TriGrad tri_backward(V3 p, const Tri& f, float g) {
  const V3 zero = mk(0.0f, 0.0f, 0.0f);
  TriGrad r{zero, zero, zero, zero};
  float t;
  if (tri_inside(p, f, &t)) {
    const V3 raw = cross(f.e02, f.e01);
    const V3 v0p = f.v0 - p, diff = t * f.n;
    r.p = ((-2.0f * g) * t) * f.n;
    const V3 gn = ((2.0f * g) * t) * (v0p + diff);  // with respect to the unit normal
    // through a / (|a| + 1e-8)
    const float an = f.norm + kEps;
    const V3 o = raw / an;
    const V3 graw = mk(gn.x * (1.0f - o.x * o.x) / an + gn.y * (-o.x * o.y) / an + gn.z * (-o.x * o.z) / an,
                       gn.x * (-o.x * o.y) / an + gn.y * (1.0f - o.y * o.y) / an + gn.z * (-o.y * o.z) / an,
                       gn.x * (-o.x * o.z) / an + gn.y * (-o.y * o.z) / an + gn.z * (1.0f - o.z * o.z) / an);
    // through cross(a, b), a = e02, b = e01
    const V3 a = f.e02, b = f.e01;
    const V3 ga = mk(-graw.y * b.z + graw.z * b.y, graw.x * b.z - graw.z * b.x, -graw.x * b.y + graw.y * b.x);
    const V3 gb = mk(graw.y * a.z - graw.z * a.y, -graw.x * a.z + graw.z * a.x, graw.x * a.y - graw.y * a.x);
    r.v0 = (((g * 2.0f) * t) * f.n) - (ga + gb);
    r.v1 = gb;
    r.v2 = ga;
    return r;
  }
  const float e01 = seg_dist_parts(p, f.v0, f.v1, f.e01, f.d00);
  const float e02 = seg_dist_parts(p, f.v0, f.v2, f.e02, f.d11);
  const float e12 = seg_dist_parts(p, f.v1, f.v2, f.e12, f.l12);
  if (e01 <= e02 && e01 <= e12) {
    const SegGrad s = seg_backward(p, f.v0, f.v1, g);
    r.p = s.p, r.v0 = s.v0, r.v1 = s.v1;
  } else if (e02 <= e01 && e02 <= e12) {
    const SegGrad s = seg_backward(p, f.v0, f.v2, g);
    r.p = s.p, r.v0 = s.v0, r.v2 = s.v1;
  } else if (e12 <= e01 && e12 <= e02) {
    const SegGrad s = seg_backward(p, f.v1, f.v2, g);
    r.p = s.p, r.v1 = s.v0, r.v2 = s.v1;
  }
  return r;
}

// The gradient of one (point, primitive) pair, flattened: gp[3] and gprim[3 * corners], PRIM in {kSeg, kTri}
template <int PRIM>
P3D_PM_FN void pair_backward(const float* point, const float* prim, float g, double min_triangle_area, float* gp, float* gprim) {
  const V3 p = load3(point);
  if (PRIM == kSeg) {
    const SegGrad s = seg_backward(p, load3(prim), load3(prim + 3), g);
    gp[0] = s.p.x, gp[1] = s.p.y, gp[2] = s.p.z;
    gprim[0] = s.v0.x, gprim[1] = s.v0.y, gprim[2] = s.v0.z, gprim[3] = s.v1.x, gprim[4] = s.v1.y, gprim[5] = s.v1.z;
  } else {
    const TriGrad s = tri_backward(p, make_tri(load3(prim), load3(prim + 3), load3(prim + 6), min_triangle_area), g);
    gp[0] = s.p.x, gp[1] = s.p.y, gp[2] = s.p.z;
    gprim[0] = s.v0.x, gprim[1] = s.v0.y, gprim[2] = s.v0.z, gprim[3] = s.v1.x, gprim[4] = s.v1.y, gprim[5] = s.v1.z;
    gprim[6] = s.v2.x, gprim[7] = s.v2.y, gprim[8] = s.v2.z;
  }
}

// ---- the hits of a backward: query q met target idxs[q] ---------------------------------------------------------------------------
// With the first-index arrays a query's batch element is found by a search over them: an element without targets has no hit
// (nothing of `targets` is read for it), and elem_scale multiplies the upstream gradient.  Without them every idxs[q] in [0, T)
// is a hit.
struct Hits {
  const float* queries;
  const float* targets;
  const int64_t* idxs;
  const float* grad_dists;          // (Q) or NULL: 1
  const float* elem_scale;          // (N) or NULL: 1; needs the first-index arrays
  const int64_t* query_first_idx;   // (N) or NULL
  const int64_t* target_first_idx;  // (N) or NULL
  int64_t N, Q, T;
  int query_kind, target_kind;
  double min_triangle_area;

  // the target of query q, or -1; *g: the upstream gradient of its distance
  __device__ __forceinline__ int64_t target(int64_t q, float* g) const {
    float up = grad_dists ? grad_dists[q] : 1.0f;
    if (query_first_idx && target_first_idx && N > 0) {
      int64_t lo = 0, hi = N;  // the last element whose first index is <= q
      while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (query_first_idx[mid] <= q) lo = mid;
        else hi = mid;
      }
      const int64_t t0 = target_first_idx[lo], t1 = lo + 1 < N ? target_first_idx[lo + 1] : T;
      if (t1 <= t0) return -1;
      if (elem_scale) up = up * elem_scale[lo];
    }
    *g = up;
    const int64_t t = idxs[q];
    return (t >= 0 && t < T) ? t : -1;
  }

  // gq[kind_floats(QK)], gt[kind_floats(TK)] of the hit (q, t)
  template <int QK, int TK>
  __device__ __forceinline__ void grads(int64_t q, int64_t t, float g, float* gq, float* gt) const {
    if constexpr (QK == kPoint) pair_backward<TK>(queries + q * 3, targets + t * kind_floats(TK), g, min_triangle_area, gq, gt);
    else pair_backward<QK>(targets + t * 3, queries + q * kind_floats(QK), g, min_triangle_area, gt, gq);
  }
};

}  // namespace pm
}  // namespace p3d
