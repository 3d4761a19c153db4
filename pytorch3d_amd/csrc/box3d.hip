// box3d.hip -- box3d_overlap: the exact intersection volume and IoU of every pair of two sets of oriented 3D boxes
// (pytorch3d/ops/iou_box3d.py over csrc/iou_box3d/iou_box3d_cpu.cpp).  include/p3d_amd.h has the contract, box3d_geom.h the geometry.
//
// ONE WAVE PER PAIR.  A pair's three fragment lists -- the finished box-1 side, and two buffers that a clipping step reads and writes
// in turn -- are 9 floats per triangle in memory the wave owns: LDS (box3d_lds_kernel, four waves per workgroup, `capacity` <= 64
// triangles per list) or the wave's slab of the workspace (box3d_slab_kernel, P3D_BOX3D_SLAB_CAPACITY).  The same code runs both:
//   clip_list   one plane across a whole list, one lane per fragment and 64 fragments per round: a lane emits 0, 1 or 2 triangles and
//               two ballots place them behind those of the lanes below it -- the reference's order (source fragment, then output slot);
//   the coplanar rule  box-2 fragments across the lanes, a loop over the box-1 fragments whose normal and area were stored once: the
//               test for parallel normals first, the nine distances only in the lanes that pass it;
//   ordered_sum the face centres and the tetrahedron terms are computed one per lane and added by every lane in list order
//               (v_readlane of lane 0, 1, 2, ...): the reference's sequential sums, the same bits on every run, stream and launch shape.
// A list that would outgrow `capacity` truncates nothing: the pair's index is appended to a list in the workspace (one integer atomic
// on its length; no result depends on the order) and box3d_slab_kernel, always launched behind the first kernel, reads the length on
// the device and redoes those pairs.  THE SLAB CANNOT OVERFLOW: clipping a triangle by a plane yields at most 2 triangles, so the 12
// triangles of a box are at most 12 * 2^6 = 768 = P3D_BOX3D_SLAB_CAPACITY after its 6 planes, and every intermediate list is shorter.
// No host sync, no float atomic.
#include <vector>

#include "box3d_geom.h"

namespace p3d {
namespace {

using namespace box3d;

constexpr int kGroupWaves = P3D_BOX3D_WAVES_PER_GROUP;
constexpr int kLdsCap = P3D_BOX3D_LDS_CAPACITY;
constexpr int kSlabCap = P3D_BOX3D_SLAB_CAPACITY;
constexpr int kSlabChunks = kSlabCap / kWave;
static_assert(kLdsCap == kWave, "the LDS kernel keeps one keep-mask per wave: a list is one round of lanes");
static_assert(kSlabCap == kTris * 64 && kSlabCap % kWave == 0, "12 triangles, doubled by each of 6 planes at the most");
constexpr int kListFloats = 3 * kTriFloats + 4;  // per unit of capacity: three lists and the (normal, area) of the box-1 side
constexpr size_t kHeaderBytes = 256;             // the workspace's head: the length of the overflow list

// a wave's working memory
struct Lists {
  float *f1, *a, *b, *nrm;
  int cap;
};
__device__ __forceinline__ Lists carve(float* base, int cap) {
  return Lists{base, base + cap * kTriFloats, base + 2 * cap * kTriFloats, base + 3 * cap * kTriFloats, cap};
}

// the wave's own stores before its next loads (LDS and the slab alike: one wave, one CU)
__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float lane_value(float x, int k) {  // k wave-uniform
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), k));
}

// src[0..n) through one plane into dst; the new length, or -1 where it would pass cap (dst is then partly written, never past cap)
__device__ __forceinline__ int clip_list(const float* src, int n, float* dst, int cap, const Plane& pl, int lane) {
  int n_out = 0;
  for (int base = 0; base < n; base += kWave) {
    const int i = base + lane;
    int cnt = 0;
    Tri o0, o1;
    if (i < n) cnt = clip_tri(load_tri(src + i * kTriFloats), pl, o0, o1);
    const unsigned long long m1 = __ballot(cnt >= 1), m2 = __ballot(cnt == 2);
    const int total = __popcll(m1) + __popcll(m2);
    if (n_out + total > cap) return -1;
    const int at = n_out + mask_rank(m1) + mask_rank(m2);
    if (cnt >= 1) store_tri(dst + at * kTriFloats, o0);
    if (cnt == 2) store_tri(dst + (at + 1) * kTriFloats, o1);
    n_out += total;
  }
  wave_fence();
  return n_out;
}

// list[0..n) through the six planes at `planes`, ping-pong with `other`; the result is back in `list`
__device__ __forceinline__ int clip_box(float* list, float* other, int n, const float* planes, int cap, int lane) {
  float *from = list, *to = other;
  for (int p = 0; p < kPlanes; ++p) {
    n = clip_list(from, n, to, cap, load_plane(planes + p * kPlaneFloats), lane);
    if (n < 0) return -1;
    float* h = from;
    from = to, to = h;
  }
  return n;
}

// term(t) of every fragment of the box-1 list and of the kept box-2 fragments, added in list order to (0, 0, 0)
template <class Term>
__device__ __forceinline__ V3 ordered_sum(const Lists& L, int n1, int n2, const unsigned long long* keep, int lane, Term term) {
  V3 acc = mk(0.0f, 0.0f, 0.0f);
  for (int side = 0; side < 2; ++side) {
    const float* list = side == 0 ? L.f1 : L.a;
    const int n = side == 0 ? n1 : n2;
    for (int base = 0, c = 0; base < n; base += kWave, ++c) {
      const int i = base + lane;
      V3 t = mk(0.0f, 0.0f, 0.0f);
      if (i < n) t = term(load_tri(list + i * kTriFloats));
      const unsigned long long m = side == 0 ? ~0ull : keep[c];
      const int cnt = n - base < kWave ? n - base : kWave;
      for (int k = 0; k < cnt; ++k) {
        if ((m >> k) & 1ull) acc = acc + mk(lane_value(t.x, k), lane_value(t.y, k), lane_value(t.z, k));
      }
    }
  }
  return acc;
}

// One pair by one wave.  false: a list passed L.cap (nothing of the pair is decided).  planes: 12 stored planes, keep: one mask per
// 64 box-2 fragments -- both the wave's own LDS.
__device__ __forceinline__ bool pair_overlap(const float* box1, const float* box2, const Lists& L, float* planes, unsigned long long* keep,
                                             int lane, float& vol, float& iou) {
  const V3 c1 = box_center(box1), c2 = box_center(box2);
  float t1 = 0.0f, t2 = 0.0f;
  if (lane < kTris) {
    const bool first = lane < kPlanes;
    store_plane(planes + lane * kPlaneFloats, box_plane(first ? box1 : box2, first ? lane : lane - kPlanes, first ? c1 : c2));
    const Tri a = box_tri(box1, lane), b = box_tri(box2, lane);
    t1 = tet_term(a, c1), t2 = tet_term(b, c2);
    store_tri(L.f1 + lane * kTriFloats, a);
    store_tri(L.a + lane * kTriFloats, b);
  }
  float vol1 = 0.0f, vol2 = 0.0f;  // BoxVolume: twelve terms in order
  for (int k = 0; k < kTris; ++k) vol1 = vol1 + lane_value(t1, k), vol2 = vol2 + lane_value(t2, k);
  wave_fence();
  const int n1 = clip_box(L.f1, L.b, kTris, planes + kPlanes * kPlaneFloats, L.cap, lane);  // box 1's triangles, box 2's planes
  if (n1 < 0) return false;
  const int n2 = clip_box(L.a, L.b, kTris, planes, L.cap, lane);
  if (n2 < 0) return false;
  vol = 0.0f, iou = 0.0f;
  if (n1 + n2 == 0) return true;
  for (int i = lane; i < n1; i += kWave) {
    const Tri t = load_tri(L.f1 + i * kTriFloats);
    const V3 n = tri_normal(t);
    float* o = L.nrm + i * 4;
    o[0] = n.x, o[1] = n.y, o[2] = n.z, o[3] = tri_area(t);
  }
  wave_fence();
  int kept = 0;
  for (int base = 0, c = 0; base < n2; base += kWave, ++c) {
    const int j = base + lane;
    bool keep_it = j < n2;
    const Tri tb = load_tri(L.a + (keep_it ? j : 0) * kTriFloats);
    const V3 nb = tri_normal(tb);
    for (int i = 0; i < n1; ++i) {
      const float* o = L.nrm + i * 4;
      if (!((double)o[3] > kAEps)) continue;  // wave-uniform
      const V3 na = load3(o);
      if (keep_it && parallel_normals(na, nb) && coplanar_tri_tri_far(load_tri(L.f1 + i * kTriFloats), na, tb, nb)) keep_it = false;
    }
    const unsigned long long m = __ballot(keep_it);
    if (lane == 0) keep[c] = m;
    kept += __popcll(m);
  }
  wave_fence();
  const float count = (float)(n1 + kept);
  const V3 s = ordered_sum(L, n1, n2, keep, lane, [](const Tri& t) { return face_center(t); });
  const V3 center = mk(s.x / count, s.y / count, s.z / count);
  vol = ordered_sum(L, n1, n2, keep, lane, [center](const Tri& t) { return mk(tet_term(t, center), 0.0f, 0.0f); }).x;
  iou = vol / (vol1 + vol2 - vol);
  return true;
}

// grid: up to P3D_BOX3D_MAX_GROUPS workgroups of four waves; wave w of workgroup g takes the pairs 4 g + w, + 4 gridDim.x, ...
__global__ __launch_bounds__(kGroupWaves* kWave) void box3d_lds_kernel(const float* __restrict__ boxes1, const float* __restrict__ boxes2,
                                                                       int64_t M, int64_t pairs, int cap, float* __restrict__ vol,
                                                                       float* __restrict__ iou, unsigned* __restrict__ overflow_count,
                                                                       unsigned* __restrict__ overflow_list) {
  __shared__ float sh_lists[kGroupWaves][kLdsCap * kListFloats];
  __shared__ float sh_planes[kGroupWaves][2 * kPlanes * kPlaneFloats];
  __shared__ unsigned long long sh_keep[kGroupWaves];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  const Lists L = carve(sh_lists[wave], cap);
  for (int64_t pair = (int64_t)blockIdx.x * kGroupWaves + wave; pair < pairs; pair += (int64_t)gridDim.x * kGroupWaves) {
    float v, u;
    const bool done = pair_overlap(boxes1 + pair / M * 24, boxes2 + pair % M * 24, L, sh_planes[wave], &sh_keep[wave], lane, v, u);
    if (lane == 0) {
      if (done) vol[pair] = v, iou[pair] = u;
      else overflow_list[atomicAdd(overflow_count, 1u)] = (unsigned)pair;
    }
    wave_fence();  // the next pair overwrites the lists
  }
}

// grid: `gridDim.x` workgroups of one wave, each with a slab of kSlabCap * kListFloats floats; wave g redoes the pairs
// overflow_list[g], [g + gridDim.x], ... below *overflow_count
__global__ __launch_bounds__(kWave) void box3d_slab_kernel(const float* __restrict__ boxes1, const float* __restrict__ boxes2, int64_t M,
                                                           float* __restrict__ vol, float* __restrict__ iou,
                                                           const unsigned* __restrict__ overflow_count,
                                                           const unsigned* __restrict__ overflow_list, float* __restrict__ slabs) {
  __shared__ float sh_planes[2 * kPlanes * kPlaneFloats];
  __shared__ unsigned long long sh_keep[kSlabChunks];
  const int lane = (int)threadIdx.x;
  const unsigned count = *overflow_count;
  const Lists L = carve(slabs + (size_t)blockIdx.x * kSlabCap * kListFloats, kSlabCap);
  for (unsigned k = blockIdx.x; k < count; k += gridDim.x) {
    const int64_t pair = overflow_list[k];
    float v, u;
    if (!pair_overlap(boxes1 + pair / M * 24, boxes2 + pair % M * 24, L, sh_planes, sh_keep, lane, v, u)) v = u = quiet_nan();  // (see the head of the file: cannot happen)
    if (lane == 0) vol[pair] = v, iou[pair] = u;
    wave_fence();
  }
}

int64_t slab_waves(int64_t pairs) { return pairs < P3D_BOX3D_SLAB_WAVES ? pairs : P3D_BOX3D_SLAB_WAVES; }

// ---- the host path: a plain loop over the pairs on the same geometry --------------------------------------------------------------
std::vector<Tri> host_clip_box(const float* box, const Plane (&planes)[kPlanes]) {
  std::vector<Tri> cur, next;
  for (int t = 0; t < kTris; ++t) cur.push_back(box_tri(box, t));
  for (int p = 0; p < kPlanes; ++p) {
    next.clear();
    for (const Tri& t : cur) {
      Tri o0, o1;
      const int cnt = clip_tri(t, planes[p], o0, o1);
      if (cnt >= 1) next.push_back(o0);
      if (cnt == 2) next.push_back(o1);
    }
    cur.swap(next);
  }
  return cur;
}

float host_box_volume(const float* box, V3 center) {
  float v = 0.0f;
  for (int t = 0; t < kTris; ++t) v = v + tet_term(box_tri(box, t), center);
  return v;
}

void host_pair(const float* box1, const float* box2, float& vol, float& iou) {
  const V3 c1 = box_center(box1), c2 = box_center(box2);
  Plane planes1[kPlanes], planes2[kPlanes];
  for (int p = 0; p < kPlanes; ++p) planes1[p] = box_plane(box1, p, c1), planes2[p] = box_plane(box2, p, c2);
  std::vector<Tri> poly = host_clip_box(box1, planes2);
  const std::vector<Tri> side2 = host_clip_box(box2, planes1);
  const size_t n1 = poly.size();
  std::vector<V3> normal1(n1);
  std::vector<float> area1(n1);
  for (size_t i = 0; i < n1; ++i) normal1[i] = tri_normal(poly[i]), area1[i] = tri_area(poly[i]);
  for (const Tri& tb : side2) {
    const V3 nb = tri_normal(tb);
    bool keep_it = true;
    for (size_t i = 0; i < n1 && keep_it; ++i) {
      if ((double)area1[i] > kAEps && parallel_normals(normal1[i], nb) && coplanar_tri_tri_far(poly[i], normal1[i], tb, nb)) keep_it = false;
    }
    if (keep_it) poly.push_back(tb);
  }
  vol = 0.0f, iou = 0.0f;
  if (poly.empty()) return;
  V3 s = mk(0.0f, 0.0f, 0.0f);
  for (const Tri& t : poly) s = s + face_center(t);
  const float count = (float)poly.size();
  const V3 center = mk(s.x / count, s.y / count, s.z / count);
  for (const Tri& t : poly) vol = vol + tet_term(t, center);
  iou = vol / (host_box_volume(box1, c1) + host_box_volume(box2, c2) - vol);
}

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API size_t p3d_iou_box3d_workspace_bytes(int64_t N, int64_t M) {
  if (N <= 0 || M <= 0 || N > INT32_MAX / M) return 0;
  const int64_t pairs = N * M;
  return kHeaderBytes + align_up((size_t)pairs * sizeof(unsigned), 256) + (size_t)slab_waves(pairs) * kSlabCap * kListFloats * sizeof(float);
}

P3D_API int p3d_iou_box3d(const float* boxes1, const float* boxes2, int64_t N, int64_t M, int lds_capacity, float* vol, float* iou,
                          void* workspace, size_t workspace_bytes, p3d_stream_t stream) {
  if (N < 0 || M < 0 || lds_capacity < kTris || lds_capacity > kLdsCap) return P3D_ERR_INVALID_ARG;
  if (N == 0 || M == 0) return P3D_OK;
  if (N > INT32_MAX / M) return P3D_ERR_UNSUPPORTED;  // (pair indices are 32 bits in the overflow list)
  if (!boxes1 || !boxes2 || !vol || !iou || !workspace) return P3D_ERR_INVALID_ARG;
  if (workspace_bytes < p3d_iou_box3d_workspace_bytes(N, M)) return P3D_ERR_WORKSPACE;
  const int64_t pairs = N * M;
  char* ws = static_cast<char*>(workspace);
  unsigned* count = reinterpret_cast<unsigned*>(ws);
  unsigned* list = reinterpret_cast<unsigned*>(ws + kHeaderBytes);
  float* slabs = reinterpret_cast<float*>(ws + kHeaderBytes + align_up((size_t)pairs * sizeof(unsigned), 256));
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(count, 0, kHeaderBytes, s) != hipSuccess) return P3D_ERR_LAUNCH;
  int64_t groups = ceil_div(pairs, kGroupWaves);
  if (groups > P3D_BOX3D_MAX_GROUPS) groups = P3D_BOX3D_MAX_GROUPS;
  {
    LaunchScope ls("box3d_lds", s);
    box3d_lds_kernel<<<(unsigned)groups, kGroupWaves * kWave, 0, s>>>(boxes1, boxes2, M, pairs, lds_capacity, vol, iou, count, list);
  }
  {
    LaunchScope ls("box3d_slab", s);
    box3d_slab_kernel<<<(unsigned)slab_waves(pairs), kWave, 0, s>>>(boxes1, boxes2, M, vol, iou, count, list, slabs);
  }
  return launch_status();
}

P3D_API int p3d_iou_box3d_host(const float* boxes1, const float* boxes2, int64_t N, int64_t M, float* vol, float* iou) {
  if (N < 0 || M < 0) return P3D_ERR_INVALID_ARG;
  if (N == 0 || M == 0) return P3D_OK;
  if (!boxes1 || !boxes2 || !vol || !iou) return P3D_ERR_INVALID_ARG;
  for (int64_t n = 0; n < N; ++n)
    for (int64_t m = 0; m < M; ++m) host_pair(boxes1 + n * 24, boxes2 + m * 24, vol[n * M + m], iou[n * M + m]);
  return P3D_OK;
}
