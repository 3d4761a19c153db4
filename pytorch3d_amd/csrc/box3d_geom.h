// box3d_geom.h -- the geometry of box3d_overlap (box3d.hip: the kernels and the host loop), by the contract of the reference's compiled
// CPU operator (pytorch3d/csrc/iou_box3d/iou_box3d_cpu.cpp over iou_utils.h).  Host and device; every function is the float32
// operations it spells, in that order (-ffp-contract=off), and holds a handful of V3 -- nothing indexed by a list position.
//   * the reference's epsilons are doubles: a float is compared with 1 - 1e-3, 1e-3 and 1e-4 AS DOUBLES (the comparisons below widen);
//     only kEpsilon meets fmaxf and is the float 1e-8f.
//   * TriNormal / PlaneNormal: the CPU operator never updates its running maximum (`max_dist` stays -1), so the normal is that of the
//     LAST vertex pair whose cross product has a norm > -1, i.e. the last pair, unless that norm is a NaN.  last_pair_normal walks
//     the pairs backwards and stops at the first that passes: the same choice.  (The CUDA file keeps the maximum in an int; the
//     recorded results this package is held to come from the CPU operator.)
#pragma once

#include "vec3.h"

namespace p3d {
namespace box3d {

constexpr double kDEps = 1e-3;   // dEpsilon: on |cos|
constexpr double kAEps = 1e-4;   // aEpsilon: the face area of the coplanar rule
constexpr float kKEps = 1e-8f;   // kEpsilon: u / max(|u|, kEpsilon)
constexpr int kTris = 12, kPlanes = 6;
constexpr int kTriFloats = 9;    // a list entry: three vertices
constexpr int kPlaneFloats = 18;  // a stored plane: centre, inward normal, four vertices

struct Tri {
  V3 a, b, c;
};
// a quad face of a box with its centre and the unit normal that points at the box's centre
struct Plane {
  V3 ctr, n, v[4];
};

// c ? x : y per component (a conditional on the structs themselves selects between their addresses and keeps them in memory)
P3D_V3_FN V3 pick(bool c, V3 x, V3 y) { return V3{c ? x.x : y.x, c ? x.y : y.y, c ? x.z : y.z}; }
P3D_V3_FN Tri load_tri(const float* p) { return Tri{load3(p), load3(p + 3), load3(p + 6)}; }
P3D_V3_FN void store_tri(float* p, const Tri& t) { store3(p, t.a), store3(p + 3, t.b), store3(p + 6, t.c); }

// _TRIS / _PLANES: the corner indices, packed four bits each (corner k of entry e: (word >> 4 k) & 7)
P3D_V3_FN int tri_corner(int t, int k) {
  const unsigned short w[kTris] = {0x210, 0x230, 0x654, 0x764, 0x651, 0x261, 0x740, 0x370, 0x623, 0x763, 0x510, 0x540};
  return (w[t] >> (4 * k)) & 7;
}
P3D_V3_FN int plane_corner(int p, int k) {
  const unsigned short w[kPlanes] = {0x3210, 0x7623, 0x4510, 0x4730, 0x2651, 0x7654};
  return (w[p] >> (4 * k)) & 7;
}
P3D_V3_FN Tri box_tri(const float* box, int t) {
  return Tri{load3(box + 3 * tri_corner(t, 0)), load3(box + 3 * tri_corner(t, 1)), load3(box + 3 * tri_corner(t, 2))};
}

// at::mean(box, 0) as torch's CPU sum adds eight rows (four accumulators, row k and row k + 4 each, then added in order): the tree
// the recorded box volumes -- hence the IoUs -- carry; / 8 is exact
P3D_V3_FN V3 box_center(const float* box) {
  V3 s = load3(box) + load3(box + 12);
  for (int k = 1; k < 4; ++k) s = s + (load3(box + 3 * k) + load3(box + 3 * k + 12));
  return s / 8.0f;
}

P3D_V3_FN V3 unit_normal(V3 e0, V3 e1) {
  const V3 n = cross(e0, e1);
  return n / fmaxf(norm3(n), kKEps);
}

// see the head of the file: the normal of the last pair (i < j) of d[0..n) whose cross product has a norm > -1
template <int N>
P3D_V3_FN V3 last_pair_normal(const V3 (&d)[N]) {
#pragma unroll
  for (int i = N - 2; i >= 0; --i)
#pragma unroll
    for (int j = N - 1; j > i; --j)
      if (norm3(cross(d[i], d[j])) > -1.0f) return unit_normal(d[i], d[j]);
  return mk(0.0f, 0.0f, 0.0f);
}

P3D_V3_FN V3 tri_normal(const Tri& t) {
  const V3 ctr = (t.a + t.b + t.c) / 3.0f;
  const V3 d[3] = {t.a - ctr, t.b - ctr, t.c - ctr};
  return last_pair_normal(d);
}

// FaceArea
P3D_V3_FN float tri_area(const Tri& t) { return norm3(cross(t.b - t.a, t.c - t.a)) / 2.0f; }

// GetBoxPlanes + PlaneCenter + PlaneNormalDirection for face p of `box` whose centre is `center`
P3D_V3_FN Plane box_plane(const float* box, int p, V3 center) {
  Plane pl;
  for (int k = 0; k < 4; ++k) pl.v[k] = load3(box + 3 * plane_corner(p, k));
  pl.ctr = (pl.v[0] + pl.v[1] + pl.v[2] + pl.v[3]) / 4.0f;
  const V3 d[4] = {pl.v[0] - pl.ctr, pl.v[1] - pl.ctr, pl.v[2] - pl.ctr, pl.v[3] - pl.ctr};
  pl.n = last_pair_normal(d);
  if (dot(center - pl.ctr, pl.n) < 0.0f) pl.n = -1.0f * pl.n;
  return pl;
}
P3D_V3_FN void store_plane(float* p, const Plane& pl) {
  store3(p, pl.ctr), store3(p + 3, pl.n);
  for (int k = 0; k < 4; ++k) store3(p + 6 + 3 * k, pl.v[k]);
}
P3D_V3_FN Plane load_plane(const float* p) {
  return Plane{load3(p), load3(p + 3), {load3(p + 6), load3(p + 9), load3(p + 12), load3(p + 15)}};
}

// ArgMaxVerts + the unit vector between the two: the FIRST pair (a outer, b inner) with the largest distance
template <int NB>
P3D_V3_FN V3 farthest_direction(const Tri& t, const V3 (&b)[NB]) {
  const V3 a[3] = {t.a, t.b, t.c};
  V3 am = mk(0.0f, 0.0f, 0.0f), bm = am;
  float best = -1.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const float dist = norm3(a[i] - b[j]);
      if (dist > best) am = a[i], bm = b[j], best = dist;
    }
  const V3 d = am - bm;
  return d / fmaxf(norm3(d), kKEps);
}

// IsCoplanarTriPlane, the parallel test first (the second has no side effect)
P3D_V3_FN bool coplanar_tri_plane(const Tri& t, const Plane& pl) {
  if (!((double)fabsf(dot(tri_normal(t), pl.n)) > 1 - kDEps)) return false;
  return (double)fabsf(dot(farthest_direction(t, pl.v), pl.n)) < kDEps;
}

// IsCoplanarTriTri with both normals given
P3D_V3_FN bool parallel_normals(V3 n1, V3 n2) { return (double)fabsf(dot(n1, n2)) > 1 - kDEps; }
P3D_V3_FN bool coplanar_tri_tri_far(const Tri& t1, V3 n1, const Tri& t2, V3 n2) {
  const V3 b[3] = {t2.a, t2.b, t2.c};
  const V3 d = farthest_direction(t1, b);
  return (double)fabsf(dot(d, n1)) < kDEps || (double)fabsf(dot(d, n2)) < kDEps;
}

// PlaneEdgeIntersection: the midpoint when the edge runs along the plane
P3D_V3_FN V3 edge_hit(const Plane& pl, V3 p0, V3 p1) {
  V3 direc = p1 - p0;
  direc = direc / fmaxf(norm3(direc), kKEps);
  V3 p = (p1 + p0) / 2.0f;
  if ((double)fabsf(dot(direc, pl.n)) >= kDEps) {
    const float top = -1.0f * dot(p0 - pl.ctr, pl.n);
    const float bot = dot(p1 - p0, pl.n);
    const float a = top / bot;
    p = p0 + a * (p1 - p0);
  }
  return p;
}

P3D_V3_FN bool inside(const Plane& pl, V3 p) { return dot(p - pl.ctr, pl.n) >= 0.0f; }

// ClipTriByPlane: the number of triangles (0, 1, 2) written to o0, o1, in the reference's order
P3D_V3_FN int clip_tri(const Tri& t, const Plane& pl, Tri& o0, Tri& o1) {
  o0 = t, o1 = t;
  if (coplanar_tri_plane(t, pl)) return 1;
  const bool in0 = inside(pl, t.a), in1 = inside(pl, t.b), in2 = inside(pl, t.c);
  const int nin = (int)in0 + (int)in1 + (int)in2;
  if (nin == 3) return 1;
  if (nin == 0) return 0;
  // two in (ClipTriByPlaneOneOut): p, q inside, r outside -> {p, pr, qr}, {p, qr, q}
  // one in (ClipTriByPlaneTwoOut): p inside, q, r outside -> {p, pq, pr}
  const V3 A = t.a, B = t.b, C = t.c;
  const bool two = nin == 2;
  const V3 p = two ? pick(!in0, B, A) : pick(in0, A, pick(in2, C, B));
  const V3 q = two ? pick(!in2, B, C) : pick(in0, B, A);
  const V3 r = two ? pick(!in2, C, pick(!in1, B, A)) : pick(in2, B, C);
  const V3 h1 = edge_hit(pl, p, pick(two, r, q));
  const V3 h2 = edge_hit(pl, pick(two, q, p), r);
  o0 = Tri{p, h1, h2};
  o1 = Tri{p, h2, q};
  return two ? 2 : 1;
}

// PolyhedronCenter's term: the face centre, per coordinate (v0 + v1 + v2) / 3
P3D_V3_FN V3 face_center(const Tri& t) { return mk((t.a.x + t.b.x + t.c.x) / 3.0f, (t.a.y + t.b.y + t.c.y) / 3.0f, (t.a.z + t.b.z + t.c.z) / 3.0f); }

// BoxVolume's term: |v0 . (v1 x v2)| / 6 about `center`
P3D_V3_FN float tet_term(const Tri& t, V3 center) {
  const V3 v0 = t.a - center, v1 = t.b - center, v2 = t.c - center;
  return fabsf(dot(v0, cross(v1, v2))) / 6.0f;
}

}  // namespace box3d
}  // namespace p3d
