// point_mesh.hip -- brute-force distances between the points of a cloud and the faces / edges of its mesh, forward and backward
// (pytorch3d/loss/point_mesh_distance.py over csrc/point_mesh/point_mesh_cpu.cpp's contract).  include/p3d_amd.h has the contract.
//
// Forward: the loop shape of knn.hip.  ONE LANE PER QUERY OBJECT -- a point, a segment or a triangle, its record (point_mesh_geom.h)
// in registers -- and 64 consecutive objects of ONE batch element per wave.  The target index of the scan is wave-uniform: a wave
// stages kTile = 64 targets of its element in LDS, lane l building the record of target l ONCE per tile (for a triangle: edges, their
// squared lengths, unit normal, |n|, the small-area flag, d00 d01 d11 and the barycentric denominator), and every lane then reads the
// same record with ds_read_b128 -- identical addresses broadcast.  Point targets are a structure of arrays read four at a time, as in
// knn.hip.  A tile's tail up to a multiple of four holds NaN records: a NaN distance fails every `<=`, so the loop has no remainder
// code.  The scan ascends with `<=`: among equal distances the LARGEST target index wins, which makes the result a minimum under
// the total order (distance, -index) and so independent of how the targets are split.
//
// Split: a workgroup is S in {1, 2, 4, 8} waves that share the same 64 queries; wave w takes the tiles w, w + S, ... into an LDS
// region of its own and wave 0 merges the S (distance, index) pairs through LDS by the same order.  Bit-equal for every S.
//
// Fused loss: wave 0 also multiplies a query's distance by its element's weight and sums the wave; a second launch (one block per
// element) adds an element's wave partials: the fixed tree of fixed_sum.h with a wave of 64 queries at level 1.  No float atomic in
// the forward.
//
// Backward: one lane per query, the hit (query, idxs[query]) from point_mesh_geom.h.  The query side is a plain store (or add) to the
// query's own row.  The target side goes through LDS and leaves as float atomics with lane = hit * values + value, so the 3 / 6 / 9
// values of one hit come from adjacent lanes (profiles/microbench/global_atomic_mi355x.txt); its ordered form is in ordered_bwd.hip.
#include "fixed_sum.h"
#include "point_mesh_geom.h"

namespace p3d {

// ordered_bwd.hip: the target side of the backward as an ordered segmented sum over the hits sorted by target
size_t point_mesh_ordered_bytes(int target_kind, int64_t Q);
int point_mesh_ordered_scatter(const pm::Hits& h, const int64_t* sorted, int accumulate, float* grad_targets, void* workspace,
                               hipStream_t s);

namespace {

using namespace pm;

constexpr int kTile = P3D_POINT_MESH_TILE;
constexpr int kMaxSplit = 8;
static_assert(kTile == kWave, "lane l builds the record of target l of a tile");

// float4 per staged record
__host__ __device__ constexpr int rec4(int kind) { return kind == kSeg ? 3 : 7; }
__host__ __device__ constexpr size_t tile_bytes(int kind) { return kind == kPoint ? 3 * kTile * sizeof(float) : (size_t)kTile * rec4(kind) * 16; }

__device__ __forceinline__ void put(float4* dst, const Seg& s) {
  dst[0] = make_float4(s.v0.x, s.v0.y, s.v0.z, s.v1.x);
  dst[1] = make_float4(s.v1.y, s.v1.z, s.d.x, s.d.y);
  dst[2] = make_float4(s.d.z, s.l2, 0.0f, 0.0f);
}
__device__ __forceinline__ void get(const float4* src, Seg& s) {
  const float4 a = src[0], b = src[1], c = src[2];
  s.v0 = mk(a.x, a.y, a.z), s.v1 = mk(a.w, b.x, b.y), s.d = mk(b.z, b.w, c.x), s.l2 = c.y;
}
__device__ __forceinline__ void put(float4* dst, const Tri& f) {
  dst[0] = make_float4(f.v0.x, f.v0.y, f.v0.z, f.v1.x);
  dst[1] = make_float4(f.v1.y, f.v1.z, f.v2.x, f.v2.y);
  dst[2] = make_float4(f.v2.z, f.e01.x, f.e01.y, f.e01.z);
  dst[3] = make_float4(f.e02.x, f.e02.y, f.e02.z, f.e12.x);
  dst[4] = make_float4(f.e12.y, f.e12.z, f.n.x, f.n.y);
  dst[5] = make_float4(f.n.z, f.d00, f.d01, f.d11);
  dst[6] = make_float4(f.l12, f.denom, f.norm, f.ok);
}
__device__ __forceinline__ void get(const float4* src, Tri& f) {
  const float4 a = src[0], b = src[1], c = src[2], d = src[3], e = src[4], g = src[5], h = src[6];
  f.v0 = mk(a.x, a.y, a.z), f.v1 = mk(a.w, b.x, b.y), f.v2 = mk(b.z, b.w, c.x);
  f.e01 = mk(c.y, c.z, c.w), f.e02 = mk(d.x, d.y, d.z), f.e12 = mk(d.w, e.x, e.y), f.n = mk(e.z, e.w, g.x);
  f.d00 = g.y, f.d01 = g.z, f.d11 = g.w, f.l12 = h.x, f.denom = h.y, f.norm = h.z, f.ok = h.w;
}

// a primitive in registers, from its packed floats (all NaN for the tail of a tile)
template <int KIND>
struct Prim;
template <>
struct Prim<kPoint> {
  V3 p;
  __device__ __forceinline__ void load(const float* src, double) { p = load3(src); }
};
template <>
struct Prim<kSeg> {
  Seg r;
  __device__ __forceinline__ void load(const float* src, double) { r = make_seg(load3(src), load3(src + 3)); }
};
template <>
struct Prim<kTri> {
  Tri r;
  __device__ __forceinline__ void load(const float* src, double min_area) { r = make_tri(load3(src), load3(src + 3), load3(src + 6), min_area); }
};

__device__ __forceinline__ float pair_dist(V3 p, const Seg& s) { return seg_dist(p, s); }
__device__ __forceinline__ float pair_dist(V3 p, const Tri& f) { return tri_dist(p, f); }

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// grid: N * blocks_per_elem workgroups of S waves (blockDim.x = 64 S); dynamic LDS: S tiles + S * 64 (float, int) merge slots.
// partials != NULL: the loss terms of the workgroup's 64 queries.
template <int QK, int TK>
__global__ __launch_bounds__(64 * kMaxSplit) void pm_forward_kernel(const float* __restrict__ queries, const float* __restrict__ targets,
                                                                    const int64_t* __restrict__ qfirst, const int64_t* __restrict__ tfirst,
                                                                    int64_t N, int64_t Q, int64_t T, int64_t blocks_per_elem,
                                                                    double min_area, const float* __restrict__ weights,
                                                                    float* __restrict__ dists, int64_t* __restrict__ idxs,
                                                                    float* __restrict__ partials) {
  extern __shared__ float4 smem[];
  constexpr int QF = kind_floats(QK), TF = kind_floats(TK);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, S = blockDim.x >> 6;
  const int64_t n = blockIdx.x / blocks_per_elem, b = blockIdx.x % blocks_per_elem;
  const int64_t q0 = clamp64(qfirst[n], 0, Q), q1 = n + 1 < N ? clamp64(qfirst[n + 1], q0, Q) : Q;
  const int64_t t0 = clamp64(tfirst[n], 0, T), t1 = n + 1 < N ? clamp64(tfirst[n + 1], t0, T) : T;
  const int64_t qcount = q1 - q0;
  if (b * kWave >= qcount) {  // uniform over the workgroup: rows past the element's count
    if (partials && threadIdx.x == 0) partials[blockIdx.x] = 0.0f;
    return;
  }
  const int64_t i = b * kWave + lane;
  const bool live = i < qcount;
  Prim<QK> q;
  q.load(queries + (q0 + (live ? i : 0)) * QF, min_area);

  float best_d = FLT_MAX;
  int best_j = -1;
  const int tcount = (int)(t1 - t0);  // T <= INT32_MAX
  const int ntiles = (tcount + kTile - 1) / kTile;
  char* const mine = reinterpret_cast<char*>(smem) + (size_t)w * tile_bytes(TK);
  for (int tile0 = 0; tile0 < ntiles; tile0 += S) {  // the same trip count for every wave of the workgroup
    const int j0 = (tile0 + w) * kTile;
    const int tn = tile0 + w < ntiles ? (tcount - j0 < kTile ? tcount - j0 : kTile) : 0, tn4 = (tn + 3) & ~3;
    __syncthreads();  // the waves are done with the tiles before
    if (lane < tn4) {
      if constexpr (TK == kPoint) {
        float* soa = reinterpret_cast<float*>(mine);
        const float* src = targets + (t0 + j0 + lane) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) soa[c * kTile + lane] = lane < tn ? src[c] : quiet_nan();
      } else {
        float v[TF];
        const float* src = targets + (t0 + j0 + lane) * TF;
#pragma unroll
        for (int c = 0; c < TF; ++c) v[c] = lane < tn ? src[c] : quiet_nan();
        Prim<TK> rec;
        rec.load(v, min_area);
        put(reinterpret_cast<float4*>(mine) + lane * rec4(TK), rec.r);
      }
    }
    __syncthreads();
    for (int t = 0; t < tn4; t += 4) {
      if constexpr (TK == kPoint) {
        const float* soa = reinterpret_cast<const float*>(mine);
        const float4 x = *reinterpret_cast<const float4*>(soa + t), y = *reinterpret_cast<const float4*>(soa + kTile + t),
                     z = *reinterpret_cast<const float4*>(soa + 2 * kTile + t);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const V3 p = mk(u == 0 ? x.x : (u == 1 ? x.y : (u == 2 ? x.z : x.w)), u == 0 ? y.x : (u == 1 ? y.y : (u == 2 ? y.z : y.w)),
                          u == 0 ? z.x : (u == 1 ? z.y : (u == 2 ? z.z : z.w)));
          const float dn = pair_dist(p, q.r);
          const bool better = dn <= best_d;
          best_d = better ? dn : best_d;
          best_j = better ? j0 + t + u : best_j;
        }
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          Prim<TK> rec;
          get(reinterpret_cast<const float4*>(mine) + (t + u) * rec4(TK), rec.r);
          const float dn = pair_dist(q.p, rec.r);
          const bool better = dn <= best_d;
          best_d = better ? dn : best_d;
          best_j = better ? j0 + t + u : best_j;
        }
      }
    }
  }
  if (S > 1) {  // uniform
    float* md = reinterpret_cast<float*>(reinterpret_cast<char*>(smem) + (size_t)S * tile_bytes(TK));
    int* mj = reinterpret_cast<int*>(md + S * kWave);
    md[w * kWave + lane] = best_d;
    mj[w * kWave + lane] = best_j;
    __syncthreads();
    if (w != 0) return;
    for (int s = 1; s < S; ++s) {
      const float d = md[s * kWave + lane];
      const int j = mj[s * kWave + lane];
      const bool better = d < best_d || (d == best_d && j > best_j);
      best_d = better ? d : best_d;
      best_j = better ? j : best_j;
    }
  }
  if (live) {
    dists[q0 + i] = best_d;
    idxs[q0 + i] = best_j >= 0 ? t0 + best_j : 0;
  }
  if (partials) {  // uniform
    float term = live ? best_d * (weights ? weights[n] : 1.0f) : 0.0f;
    // fixed_sum.h's wave_sum, written out: through the call the compiler lays out this kernel's tail differently (11 instructions
    // fewer in all four instantiations), and the kernel is held to its recorded instruction count
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) term += __shfl_xor(term, d);
    if (lane == 0) partials[blockIdx.x] = term;
  }
}

// the last step of segment_sum_kernel over an element's wave partials: nothing
struct ElementSum {
  __device__ __forceinline__ float operator()(int64_t, float s) const { return s; }
};

// One lane per query; a block of 256 = four waves, each with an LDS slab of its own for the target side.
template <int QK, int TK>
__global__ __launch_bounds__(256) void pm_backward_kernel(Hits h, int accumulate_query, float* __restrict__ grad_queries,
                                                          float* __restrict__ grad_targets) {
  constexpr int QF = kind_floats(QK), TF = kind_floats(TK);
  __shared__ float slab[4][kWave * TF];
  __shared__ int64_t hit_target[4][kWave];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float g = 0.0f;
  const int64_t t = q < h.Q ? h.target(q, &g) : -1;
  float gq[QF], gt[TF];
#pragma unroll
  for (int c = 0; c < QF; ++c) gq[c] = 0.0f;
#pragma unroll
  for (int c = 0; c < TF; ++c) gt[c] = 0.0f;
  if (t >= 0) h.grads<QK, TK>(q, t, g, gq, gt);
  if (grad_queries && q < h.Q) {
#pragma unroll
    for (int c = 0; c < QF; ++c) grad_queries[q * QF + c] = accumulate_query ? grad_queries[q * QF + c] + gq[c] : gq[c];
  }
  if (!grad_targets) return;  // uniform
#pragma unroll
  for (int c = 0; c < TF; ++c) slab[w][lane * TF + c] = gt[c];
  hit_target[w][lane] = t;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < TF; ++k) {
    const int flat = k * kWave + lane, hit = flat / TF, c = flat % TF;
    const int64_t tt = hit_target[w][hit];
    if (tt >= 0) atomicAdd(grad_targets + tt * TF + c, slab[w][flat]);
  }
}

int cu_count() {
  static int cached[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cached[dev] == 0) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    cached[dev] = v;
  }
  return cached[dev];
}

// S waves per workgroup: doubled while every wave still finds a SIMD of its own (4 per CU) and a tile of its own
int auto_split(int64_t blocks, int64_t T) {
  const int64_t simds = 4ll * cu_count(), tiles = ceil_div(T, kTile);
  int S = 1;
  while (S < kMaxSplit && blocks * (2 * S) <= simds && 2 * S <= tiles) S *= 2;
  return S;
}

bool kinds_ok(int qk, int tk) {
  return (qk == kPoint && (tk == kSeg || tk == kTri)) || (tk == kPoint && (qk == kSeg || qk == kTri));
}

template <int QK, int TK>
int launch_forward(const float* queries, const float* targets, const int64_t* qfirst, const int64_t* tfirst, int64_t N, int64_t Q,
                   int64_t T, int64_t bpe, double min_area, int S, const float* weights, float* dists, int64_t* idxs, float* partials,
                   hipStream_t s) {
  const size_t lds = (size_t)S * tile_bytes(TK) + (size_t)S * kWave * 8;
  pm_forward_kernel<QK, TK><<<(unsigned)(N * bpe), 64 * S, lds, s>>>(queries, targets, qfirst, tfirst, N, Q, T, bpe, min_area, weights,
                                                                    dists, idxs, partials);
  return launch_status();
}

template <int QK, int TK>
int launch_backward(const Hits& h, int accumulate_query, float* gq, float* gt, hipStream_t s) {
  pm_backward_kernel<QK, TK><<<(unsigned)ceil_div(h.Q, 256), 256, 0, s>>>(h, accumulate_query, gq, gt);
  return launch_status();
}

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API size_t p3d_point_mesh_forward_workspace_bytes(int64_t N, int64_t max_queries) {
  return N <= 0 || max_queries <= 0 ? 0 : (size_t)N * (size_t)ceil_div(max_queries, kWave) * sizeof(float);
}

P3D_API int p3d_point_mesh_forward(int query_kind, int target_kind, const float* queries, const float* targets,
                                   const int64_t* query_first_idx, const int64_t* target_first_idx, int64_t N, int64_t Q, int64_t T,
                                   int64_t max_queries, double min_triangle_area, int split, const float* weights, float* dists,
                                   int64_t* idxs, float* sums, void* workspace, size_t workspace_bytes, p3d_stream_t stream) {
  if (!kinds_ok(query_kind, target_kind)) return P3D_ERR_INVALID_ARG;
  if (N < 0 || Q < 0 || T < 0 || max_queries < 0 || Q > INT32_MAX || T > INT32_MAX || N > INT32_MAX) return P3D_ERR_INVALID_ARG;
  if (split != 0 && split != 1 && split != 2 && split != 4 && split != 8) return P3D_ERR_INVALID_ARG;
  if (max_queries > Q) max_queries = Q;
  if (N > 0 && (!query_first_idx || !target_first_idx)) return P3D_ERR_INVALID_ARG;
  if (Q > 0 && (!queries || !dists || !idxs || (T > 0 && !targets))) return P3D_ERR_INVALID_ARG;
  if (Q > 0 && (N == 0 || max_queries == 0)) return P3D_ERR_INVALID_ARG;  // rows nobody would write
  if (sums && N > 0 && max_queries > 0 &&
      (!workspace || workspace_bytes < p3d_point_mesh_forward_workspace_bytes(N, max_queries)))
    return P3D_ERR_WORKSPACE;
  if (N == 0) return P3D_OK;
  const int64_t bpe = ceil_div(max_queries, kWave), blocks = N * bpe;
  if (blocks > 0x7fffffffll) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  float* partials = sums ? static_cast<float*>(workspace) : nullptr;
  if (blocks > 0) {
    const int S = split ? split : auto_split(blocks, T);
    LaunchScope ls(query_kind == kPoint ? (target_kind == kTri ? "point_face_forward" : "point_edge_forward")
                                        : (query_kind == kTri ? "face_point_forward" : "edge_point_forward"), s);
    int rc;
#define P3D_PM_FWD(QK, TK) \
  launch_forward<QK, TK>(queries, targets, query_first_idx, target_first_idx, N, Q, T, bpe, min_triangle_area, S, weights, dists, idxs, partials, s)
    if (query_kind == kPoint) rc = target_kind == kTri ? P3D_PM_FWD(kPoint, kTri) : P3D_PM_FWD(kPoint, kSeg);
    else rc = query_kind == kTri ? P3D_PM_FWD(kTri, kPoint) : P3D_PM_FWD(kSeg, kPoint);
#undef P3D_PM_FWD
    if (rc != P3D_OK) return rc;
  }
  if (sums) {
    LaunchScope ls("point_mesh_element_sum", s);
    segment_sum_kernel<<<(unsigned)N, 256, 0, s>>>(partials, bpe, ElementSum{}, sums);
    return launch_status();
  }
  return P3D_OK;
}

P3D_API size_t p3d_point_mesh_backward_workspace_bytes(int target_kind, int64_t Q) {
  return Q <= 0 ? 0 : point_mesh_ordered_bytes(target_kind, Q);
}

P3D_API int p3d_point_mesh_backward(int query_kind, int target_kind, const float* queries, const float* targets, const int64_t* idxs,
                                    const float* grad_dists, const float* elem_scale, const int64_t* query_first_idx,
                                    const int64_t* target_first_idx, int64_t N, int64_t Q, int64_t T, double min_triangle_area,
                                    unsigned flags, const int64_t* sorted_hits, float* grad_queries, float* grad_targets, void* workspace,
                                    size_t workspace_bytes, p3d_stream_t stream) {
  if (!kinds_ok(query_kind, target_kind)) return P3D_ERR_INVALID_ARG;
  if (N < 0 || Q < 0 || T < 0 || Q > INT32_MAX || T > INT32_MAX || N > INT32_MAX) return P3D_ERR_INVALID_ARG;
  if ((query_first_idx == nullptr) != (target_first_idx == nullptr)) return P3D_ERR_INVALID_ARG;
  if (elem_scale && !query_first_idx) return P3D_ERR_INVALID_ARG;
  if (Q > 0 && (!queries || !idxs || (T > 0 && !targets))) return P3D_ERR_INVALID_ARG;
  if (sorted_hits && grad_targets && Q > 0 && T > 0 &&
      (!workspace || workspace_bytes < p3d_point_mesh_backward_workspace_bytes(target_kind, Q)))
    return P3D_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int TF = kind_floats(target_kind);
  const bool acc_t = (flags & P3D_POINT_MESH_ACCUMULATE_TARGETS) != 0, acc_q = (flags & P3D_POINT_MESH_ACCUMULATE_QUERIES) != 0;
  const bool ordered = sorted_hits != nullptr && grad_targets != nullptr;
  if (grad_targets && T > 0 && !acc_t &&
      hipMemsetAsync(grad_targets, 0, (size_t)T * TF * sizeof(float), s) != hipSuccess)
    return P3D_ERR_LAUNCH;
  if (Q == 0) return P3D_OK;
  Hits h;
  h.queries = queries, h.targets = targets, h.idxs = idxs, h.grad_dists = grad_dists, h.elem_scale = elem_scale;
  h.query_first_idx = query_first_idx, h.target_first_idx = target_first_idx;
  h.N = query_first_idx ? N : 0, h.Q = Q, h.T = T, h.query_kind = query_kind, h.target_kind = target_kind;
  h.min_triangle_area = min_triangle_area;
  float* atomic_targets = ordered || T == 0 ? nullptr : grad_targets;
  if (grad_queries || atomic_targets) {
    LaunchScope ls("point_mesh_backward", s);
    int rc;
    if (query_kind == kPoint) rc = target_kind == kTri ? launch_backward<kPoint, kTri>(h, acc_q, grad_queries, atomic_targets, s)
                                                       : launch_backward<kPoint, kSeg>(h, acc_q, grad_queries, atomic_targets, s);
    else rc = query_kind == kTri ? launch_backward<kTri, kPoint>(h, acc_q, grad_queries, atomic_targets, s)
                                 : launch_backward<kSeg, kPoint>(h, acc_q, grad_queries, atomic_targets, s);
    if (rc != P3D_OK) return rc;
  }
  if (ordered && T > 0) return point_mesh_ordered_scatter(h, sorted_hits, 1, grad_targets, workspace, s);
  return P3D_OK;
}
