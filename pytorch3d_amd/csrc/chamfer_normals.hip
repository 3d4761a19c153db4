// chamfer_normals.hip -- chamfer_distance with normals (pytorch3d/loss/chamfer.py), both directions, forward and backward.
// csrc/implicit_abi.h has the contract.
//
// Forward, ONE launch: the workgroups of x -> y, then those of y -> x.  A workgroup is 64 queries of one cloud (ONE LANE PER QUERY,
//   the query in registers) and S in {1, 2, 4, 8} waves that hold the SAME 64 queries and scan consecutive slices of the far cloud,
//   each through an LDS tile of its own (structure of arrays, four points per ds_read_b128, identical addresses broadcast; a
//   tile's tail up to a multiple of four is NaN, which fails every `<`).  The distance is knn.hip's pair_dist<3, NORM>: per
//   coordinate the difference, squared or absolute, added in coordinate order, unfused.  The waves' winners meet in LDS and wave 0
//   takes the least by the total order (dist, j); inside a wave strict `<` over ascending j is that order, so idx and the distance
//   have knn_kernel<3, NORM, 1>'s bits for every S.  Every wave goes round the tile loop the same number of times (a wave whose
//   slice has ended, or is empty because lengths < S, stages nothing): the workgroup barriers are uniform.
//   Epilogue, wave 0, still a lane per query: the far normal at the winner, the cosine by the contract below, the row mask and
//   the cloud's weight on both terms; idx, and either the two per-point terms or the wave's sums of both (wave_sum).
// Cloud sums, one launch, a workgroup per cloud: the four series of wave partials (2 terms x 2 directions) through the tree of
//   fixed_sum.h (segment_sum_kernel's: strided in ascending order, then block_sum_256), the division by the length, the two
//   directions added.  No float atomic and no host read in the forward.
// Backward, two launches.  near: a lane per (direction, n, i) writes the row's own gradients -- point and normal -- into EVERY
//   entry of the four outputs, so nothing is zero-filled in front.  far: lane = hit * 6 + value (point 0..2, normal 3..5), ten hits
//   per wave; consecutive hits of one target are summed inside the wave by a segmented scan and the last hit of a run issues the
//   float atomics from six adjacent lanes (knn.hip's scatter at six values; profiles/microbench/global_atomic_mi355x.txt).
//
// The cosine (F.cosine_similarity(u, v, dim=2, eps)): a = u / max(|u|, eps), b = v / max(|v|, eps), c = (a0 b0 + a1 b1) + a2 b2,
// |u| = sqrt((u0 u0 + u1 u1) + u2 u2), every operation a float32 rounding of its own.  Its gradient as autograd has it: through the
// quotient and through the norm wherever |u| > 0 -- torch clamps the norm in place outside the graph, so the clamp stops nothing;
// the norm's own gradient at |u| == 0 is 0.
#include "fixed_sum.h"
#include "implicit_abi.h"
#include "knn_grad.h"
#include "vec3.h"

namespace p3d {
namespace {

constexpr int kTile = P3D_KNN_TILE;
static_assert(kTile % 4 == 0, "a tile is read four points at a time");
constexpr int kMaxSplit = P3D_CHAMFER_NORMALS_MAX_SPLIT;
constexpr float kCosEps = 1e-6f;
constexpr int kValues = 6;               // of a hit in the far scatter: point (3), normal (3)
constexpr int kHits = kWave / kValues;   // hits per wave

// the two clouds with their normals; direction 0 reads them as given, direction 1 swapped
struct Clouds {
  const float *x, *y, *xn, *yn;
  const int64_t *lx, *ly;
  int64_t N, P1, P2;
};

struct Side {
  const float *a, *b, *an, *bn;  // near points, far points, near normals, far normals
  const int64_t *la, *lb;
  int64_t PA, PB;
};

__device__ __forceinline__ Side side_of(const Clouds& c, int dir) {
  if (dir == 0) return Side{c.x, c.y, c.xn, c.yn, c.lx, c.ly, c.P1, c.P2};
  return Side{c.y, c.x, c.yn, c.xn, c.ly, c.lx, c.P2, c.P1};
}

template <int NORM>
__device__ __forceinline__ float coord_term(float x, float y) {
  const float d = x - y;
  return NORM == 2 ? d * d : fabsf(d);
}

struct Unit {
  V3 a;        // v / max(|v|, eps)
  float n, m;  // |v|, max(|v|, eps)
};

__device__ __forceinline__ Unit unit_of(V3 v) {
  Unit u;
  u.n = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
  u.m = u.n < kCosEps ? kCosEps : u.n;
  u.a = mk(v.x / u.m, v.y / u.m, v.z / u.m);
  return u;
}

__device__ __forceinline__ float dot_in_order(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

__device__ __forceinline__ float cosine(V3 u, V3 v) { return dot_in_order(unit_of(u).a, unit_of(v).a); }

// d(1 - |c|) / dc, or d(1 - c) / dc: abs has derivative 0 at c == 0
__device__ __forceinline__ float term_slope(float c, int abs_cosine) {
  if (!abs_cosine) return -1.0f;
  return c > 0.0f ? -1.0f : (c < 0.0f ? 1.0f : 0.0f);
}

// what v receives from the gradient ga of its unit vector a = v / m: ga / m through the quotient and, where |v| > 0, the
// quotient's gradient of m through the norm (m counts as the norm itself, clamped or not)
__device__ __forceinline__ V3 through_unit(V3 v, const Unit& u, V3 ga) {
  V3 g = mk(ga.x / u.m, ga.y / u.m, ga.z / u.m);
  if (u.n > 0.0f) {
    const float gm = -dot_in_order(ga, u.a) / u.m;
    g = g + mk(gm * (v.x / u.n), gm * (v.y / u.n), gm * (v.z / u.n));
  }
  return g;
}

// grid: blocks_x workgroups of direction 0, then those of direction 1; S waves each.  terms (per-point mode) or partials (sums)
// is NULL.  partials: [direction][term][n][block of the cloud].
template <int NORM, int S>
__global__ __launch_bounds__(64 * S) void chamfer_normals_fwd_kernel(Clouds c, const float* __restrict__ weights, int64_t blocks_x,
                                                                     int64_t bpc_x, int64_t bpc_y, int abs_cosine,
                                                                     int64_t* __restrict__ idx_x, int64_t* __restrict__ idx_y,
                                                                     float* __restrict__ dist_x, float* __restrict__ norm_x,
                                                                     float* __restrict__ dist_y, float* __restrict__ norm_y,
                                                                     float* __restrict__ partials) {
  __shared__ __align__(16) float tile[S][3][kTile];
  __shared__ float win_d[S][kWave];
  __shared__ int win_j[S][kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int dir = (int64_t)blockIdx.x >= blocks_x ? 1 : 0;  // uniform
  const Side s = side_of(c, dir);
  const int64_t bpc = dir ? bpc_y : bpc_x, block = (int64_t)blockIdx.x - (dir ? blocks_x : 0);
  const int64_t n = block / bpc, b = block % bpc;
  const int64_t i = b * kWave + lane;
  const int64_t len1 = knn::cloud_length(s.la, n, s.PA), len2 = knn::cloud_length(s.lb, n, s.PB);
  const bool live = i < len1, row = i < s.PA;
  const V3 q = live ? load3(s.a + (n * s.PA + i) * 3) : mk(0.0f, 0.0f, 0.0f);
  float best_d = __builtin_inff();
  int best_j = -1;
  const int64_t scan = b * kWave < len1 ? len2 : 0;  // uniform: a workgroup of padding rows scans nothing
  const int64_t per = (scan + S - 1) / S;
  const int64_t lo = wave * per < scan ? wave * per : scan, hi = lo + per < scan ? lo + per : scan;  // this wave's slice
  for (int64_t r0 = 0; r0 < per; r0 += kTile) {  // the same rounds in every wave
    const int64_t j0 = lo + r0;
    const int tn = j0 < hi ? (int)(hi - j0 < kTile ? hi - j0 : kTile) : 0, tn4 = (tn + 3) & ~3;
    __syncthreads();  // the wave is done with the tile before
    const float* src = s.b + (n * s.PB + j0) * 3;
    for (int e = lane; e < tn * 3; e += kWave) tile[wave][e % 3][e / 3] = src[e];
    if (lane < tn4 - tn) {
#pragma unroll
      for (int k = 0; k < 3; ++k) tile[wave][k][tn + lane] = quiet_nan();
    }
    __syncthreads();
    for (int t = 0; t < tn4; t += 4) {
      float4 v[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] = *reinterpret_cast<const float4*>(&tile[wave][k][t]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float y[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) y[k] = u == 0 ? v[k].x : (u == 1 ? v[k].y : (u == 2 ? v[k].z : v[k].w));
        float dn = coord_term<NORM>(q.x, y[0]);  // knn.hip's pair_dist<3, NORM>
        dn = dn + coord_term<NORM>(q.y, y[1]);
        dn = dn + coord_term<NORM>(q.z, y[2]);
        const bool better = dn < best_d;
        best_d = better ? dn : best_d;
        best_j = better ? (int)j0 + t + u : best_j;
      }
    }
  }
  if (S > 1) {
    win_d[wave][lane] = best_d, win_j[wave][lane] = best_j;
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int v = 1; v < S; ++v) {
      const float d = win_d[v][lane];
      const int j = win_j[v][lane];
      // the total order (dist, smaller j); a wave that found nothing (j < 0) never wins
      const bool better = j >= 0 && (best_j < 0 || d < best_d || (d == best_d && j < best_j));
      best_d = better ? d : best_d;
      best_j = better ? j : best_j;
    }
  }
  const bool found = live && len2 > 0;
  const int64_t j = found && best_j >= 0 ? (int64_t)best_j : 0;  // knn.hip's index-0 rule
  const float w = weights ? weights[n] : 1.0f;
  float dterm = 0.0f, nterm = 0.0f;
  if (live) {
    // an empty far cloud leaves a zero normal behind (knn_gather's mask): cosine 0
    const V3 far = found ? load3(s.bn + (n * s.PB + j) * 3) : mk(0.0f, 0.0f, 0.0f);
    const float cs = cosine(load3(s.an + (n * s.PA + i) * 3), far);
    nterm = (1.0f - (abs_cosine ? fabsf(cs) : cs)) * w;
    dterm = (found ? best_d : 0.0f) * w;
  }
  if (row) {
    (dir ? idx_y : idx_x)[n * s.PA + i] = j;
    if (!partials) (dir ? dist_y : dist_x)[n * s.PA + i] = dterm, (dir ? norm_y : norm_x)[n * s.PA + i] = nterm;
  }
  if (partials) {  // uniform
    const float sd = wave_sum(dterm), sn = wave_sum(nterm);
    float* out = partials + (dir ? 2 * c.N * bpc_x : 0);
    if (lane == 0) out[n * bpc + b] = sd, out[(c.N + n) * bpc + b] = sn;
  }
}

// segment_sum_kernel's tree over one cloud's wave partials; every lane of the block calls it, thread 0 uses it
__device__ __forceinline__ float cloud_sum(const float* __restrict__ partials, int64_t per_cloud) {
  float acc = 0.0f;
  for (int64_t k = threadIdx.x; k < per_cloud; k += 256) acc += partials[k];
  const float s = block_sum_256(acc);
  __syncthreads();  // block_sum_256's four words are free again
  return s;
}

// grid: one workgroup of 256 per cloud.  sums (N, 2): the distance and the normal loss of the cloud
__global__ __launch_bounds__(256) void chamfer_normals_sum_kernel(const float* __restrict__ partials, const int64_t* __restrict__ lx,
                                                                  const int64_t* __restrict__ ly, int64_t N, int64_t P1, int64_t P2,
                                                                  int64_t bpc_x, int64_t bpc_y, int single, int point_mean,
                                                                  float* __restrict__ sums) {
  const int64_t n = blockIdx.x;
  const float* py = partials + 2 * N * bpc_x;
  float v[4];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    v[q] = cloud_sum(partials + (q * N + n) * bpc_x, bpc_x);
    v[2 + q] = single ? 0.0f : cloud_sum(py + (q * N + n) * bpc_y, bpc_y);
  }
  if (threadIdx.x != 0) return;
  if (point_mean) {
    const int64_t l1 = knn::cloud_length(lx, n, P1), l2 = knn::cloud_length(ly, n, P2);
    const float d1 = (float)(l1 < 1 ? 1 : l1), d2 = (float)(l2 < 1 ? 1 : l2);
    v[0] = v[0] / d1, v[1] = v[1] / d1, v[2] = v[2] / d2, v[3] = v[3] / d2;
  }
  sums[n * 2 + 0] = single ? v[0] : v[0] + v[2];
  sums[n * 2 + 1] = single ? v[1] : v[1] + v[3];
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
struct Back {
  Clouds c;
  const int64_t *idx_x, *idx_y;
  const float* cloud_grad;  // (2 terms, N): the upstream gradients of the clouds' two losses, or NULL (1)
  const float* weights;     // (N) or NULL (1)
  const float *gdx, *gnx, *gdy, *gny;  // per-point upstream gradients of the four term tensors, each may be NULL (1)
  int norm, abs_cosine, point_mean;

  // hit r of direction dir: the row n * PA + i.  False where the row is padding or has no neighbour; else the far row j, the
  // gradient of the near point (the far point's is its negative) and of the two normals.
  __device__ __forceinline__ bool hit(int dir, int64_t r, int64_t* target, V3* gp, V3* g_near, V3* g_far) const {
    const Side s = side_of(c, dir);
    const int64_t n = r / s.PA, i = r % s.PA;
    const int64_t len1 = knn::cloud_length(s.la, n, s.PA);
    if (i >= len1 || knn::cloud_length(s.lb, n, s.PB) <= 0) return false;
    const int64_t j = (dir ? idx_y : idx_x)[r];
    if (j < 0 || j >= s.PB) return false;
    const float* gd = dir ? gdy : gdx;
    const float* gn = dir ? gny : gnx;
    float ud = gd ? gd[r] : 1.0f, un = gn ? gn[r] : 1.0f;
    // the forward's steps backwards: the cloud's gradient, the mean's divisor (len1 >= 1 here), the weight
    if (cloud_grad) ud = ud * cloud_grad[n], un = un * cloud_grad[c.N + n];
    if (point_mean) ud = ud / (float)len1, un = un / (float)len1;
    if (weights) ud = ud * weights[n], un = un * weights[n];
    const int64_t t = n * s.PB + j;
    *target = t;
    const V3 a = load3(s.a + r * 3), b = load3(s.b + t * 3);
    *gp = mk(knn::grad_term(ud, a.x, b.x, norm), knn::grad_term(ud, a.y, b.y, norm), knn::grad_term(ud, a.z, b.z, norm));
    const V3 u = load3(s.an + r * 3), v = load3(s.bn + t * 3);
    const Unit uu = unit_of(u), uv = unit_of(v);
    const float gc = un * term_slope(dot_in_order(uu.a, uv.a), abs_cosine);
    *g_near = through_unit(u, uu, gc * uv.a);
    *g_far = through_unit(v, uv, gc * uu.a);
    return true;
  }
};

// one lane per (direction, n, i): every entry of the four gradients is written (NULL: skipped).  `single`: the rows of y get zeros
__global__ __launch_bounds__(256) void chamfer_normals_bwd_near_kernel(Back k, int single, float* __restrict__ grad_x,
                                                                       float* __restrict__ grad_y, float* __restrict__ grad_xn,
                                                                       float* __restrict__ grad_yn) {
  const int64_t rows_x = k.c.N * k.c.P1, rows = rows_x + k.c.N * k.c.P2;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < rows; e += (int64_t)gridDim.x * 256) {
    const int dir = e >= rows_x ? 1 : 0;
    const int64_t r = dir ? e - rows_x : e;
    V3 gp = mk(0.0f, 0.0f, 0.0f), gn = gp, gf;
    int64_t t;
    if (!(dir && single)) k.hit(dir, r, &t, &gp, &gn, &gf);  // a row without a hit keeps its zeros
    float* p = dir ? grad_y : grad_x;
    float* q = dir ? grad_yn : grad_xn;
    if (p) store3(p + r * 3, gp);
    if (q) store3(q + r * 3, gn);
  }
}

// lane = hit * 6 + value; a wave owns ten consecutive hits of the hits of direction 0 followed by those of direction 1 (the last
// four lanes idle).  A hit of x -> y adds to y's rows, one of y -> x to x's: targets are numbered N * P2 apart.
__global__ __launch_bounds__(256) void chamfer_normals_bwd_far_kernel(Back k, int64_t hits, int64_t nwaves, float* __restrict__ grad_x,
                                                                      float* __restrict__ grad_y, float* __restrict__ grad_xn,
                                                                      float* __restrict__ grad_yn) {
  const int lane = threadIdx.x & 63, hw = lane / kValues, val = lane % kValues;
  const int first = hw * kValues;  // the lane of this hit's value 0
  const int64_t rows_x = k.c.N * k.c.P1, far_y = k.c.N * k.c.P2;
  for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < nwaves; w += (int64_t)gridDim.x * 4) {  // wave-uniform
    const int64_t e = w * kHits + hw;
    const int dir = e >= rows_x ? 1 : 0;
    int64_t t = -1;
    float v = 0.0f;
    if (hw < kHits && e < hits) {
      V3 gp, gn, gf;
      int64_t row;
      if (k.hit(dir, dir ? e - rows_x : e, &row, &gp, &gn, &gf)) {
        t = dir ? far_y + row : row;
        const float six[kValues] = {-gp.x, -gp.y, -gp.z, gf.x, gf.y, gf.z};
        v = val == 0 ? six[0] : val == 1 ? six[1] : val == 2 ? six[2] : val == 3 ? six[3] : val == 4 ? six[4] : six[5];
      }
    }
    // a run: consecutive hits of the wave with one target; lanes without a hit are runs of their own (knn.hip's scatter)
    const int64_t before = __shfl_up(t, kValues);
    const bool head = hw == 0 || before != t || t < 0;
    const unsigned long long heads = __ballot(head && val == 0);
    const int start = (63 - __clzll((long long)(heads & ((2ull << first) - 1ull)))) / kValues;  // first hit of this lane's run
#pragma unroll
    for (int d = 1; d < kHits; d <<= 1) {
      const float below = __shfl_up(v, d * kValues);
      if (hw - d >= start) v += below;
    }
    const int64_t after = __shfl_down(t, kValues);
    const bool tail = hw + 1 >= kHits || after != t;
    if (t >= 0 && tail) {
      const bool to_x = t >= far_y;
      const int64_t row = to_x ? t - far_y : t;
      float* dst = val < 3 ? (to_x ? grad_x : grad_y) : (to_x ? grad_xn : grad_yn);
      if (dst) atomicAdd(dst + row * 3 + (val < 3 ? val : val - 3), v);
    }
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

// the waves of a workgroup, from profiles/chamfer_normals_mi355x.txt: as many as the longer far cloud has full tiles, up to 8 -- the
// split won at every measured launch size, 158 to 20 096 workgroups -- but 4 once 8 would put more than two waves on every SIMD
// (there 8 measured 0.5 - 4 % behind 4)
int auto_split(int64_t blocks, int64_t far) {
  const int64_t simds = 4ll * cu_count(), tiles = ceil_div(far, kTile);
  int S = 1;
  while (S < kMaxSplit && 2 * S <= tiles) S *= 2;
  if (S == 8 && blocks * 8 > 2 * simds) S = 4;
  return S;
}

struct Sizes {
  int64_t bpc_x, bpc_y, blocks_x, blocks;
};

// every index within an int64 with room, a neighbour's j within an int32, the grid within 2^31
bool sizes_ok(int64_t N, int64_t P1, int64_t P2, int single, Sizes* z) {
  if (N < 0 || P1 < 0 || P2 < 0 || P1 > INT32_MAX || P2 > INT32_MAX || N > INT32_MAX) return false;
  z->bpc_x = ceil_div(P1, kWave), z->bpc_y = ceil_div(P2, kWave);
  const int64_t per = z->bpc_x + z->bpc_y;
  if (N > 0 && per > 0x7fffffffll / 16 / N) return false;  // also N (P1 + P2) * 6 lanes of the scatter within an int64 by far
  z->blocks_x = N * z->bpc_x;
  z->blocks = z->blocks_x + (single ? 0 : N * z->bpc_y);
  return true;
}

bool split_ok(int split) { return split == 0 || split == 1 || split == 2 || split == 4 || split == 8; }

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API size_t p3di_chamfer_normals_forward_workspace_bytes(int64_t N, int64_t P1, int64_t P2) {
  Sizes z;
  if (!sizes_ok(N, P1, P2, 0, &z)) return 0;
  return (size_t)(2 * N * (z.bpc_x + z.bpc_y)) * sizeof(float);
}

P3D_API int p3di_chamfer_normals_forward(const float* x, const float* y, const float* x_normals, const float* y_normals,
                                         const int64_t* x_lengths, const int64_t* y_lengths, const float* weights, int64_t N, int64_t P1,
                                         int64_t P2, int norm, int abs_cosine, int single_directional, int point_reduction, int split,
                                         int64_t* idx_x, int64_t* idx_y, float* dist_x, float* normal_x, float* dist_y, float* normal_y,
                                         float* sums, void* workspace, size_t workspace_bytes, p3d_stream_t stream) {
  Sizes z;
  const int single = single_directional != 0;
  if (!sizes_ok(N, P1, P2, single, &z) || !split_ok(split) || (norm != 1 && norm != 2) || point_reduction < 0 || point_reduction > 2)
    return P3D_ERR_INVALID_ARG;
  if (N == 0) return P3D_OK;
  const bool reduced = point_reduction != 0;
  if (P1 > 0 && (!x || !x_normals || !idx_x || (!reduced && (!dist_x || !normal_x)))) return P3D_ERR_INVALID_ARG;
  if (P2 > 0 && (!y || !y_normals || (!single && (!idx_y || (!reduced && (!dist_y || !normal_y)))))) return P3D_ERR_INVALID_ARG;
  if (reduced && !sums) return P3D_ERR_INVALID_ARG;
  if (reduced && z.bpc_x + z.bpc_y > 0 &&
      (!workspace || workspace_bytes < p3di_chamfer_normals_forward_workspace_bytes(N, P1, P2)))
    return P3D_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* partials = reduced ? static_cast<float*>(workspace) : nullptr;
  const Clouds c{x, y, x_normals, y_normals, x_lengths, y_lengths, N, P1, P2};
  if (z.blocks > 0) {
    LaunchScope ls("chamfer_normals_forward", st);
    const int S = split ? split : auto_split(z.blocks, single || P2 > P1 ? P2 : P1);
    const unsigned g = (unsigned)z.blocks;
#define P3D_CHAMFER_NORMALS(NORM, SPLIT)                                                                                            \
  chamfer_normals_fwd_kernel<NORM, SPLIT><<<g, 64 * SPLIT, 0, st>>>(c, weights, z.blocks_x, z.bpc_x, z.bpc_y, abs_cosine, idx_x, idx_y, \
                                                                    dist_x, normal_x, dist_y, normal_y, partials)
#define P3D_CHAMFER_NORMALS_S(NORM)       \
  if (S == 1) P3D_CHAMFER_NORMALS(NORM, 1);      \
  else if (S == 2) P3D_CHAMFER_NORMALS(NORM, 2); \
  else if (S == 4) P3D_CHAMFER_NORMALS(NORM, 4); \
  else P3D_CHAMFER_NORMALS(NORM, 8)
    if (norm == 2) {
      P3D_CHAMFER_NORMALS_S(2);
    } else {
      P3D_CHAMFER_NORMALS_S(1);
    }
#undef P3D_CHAMFER_NORMALS_S
#undef P3D_CHAMFER_NORMALS
    const int rc = launch_status();
    if (rc != P3D_OK) return rc;
  }
  if (reduced) {
    LaunchScope ls("chamfer_normals_cloud_sum", st);
    chamfer_normals_sum_kernel<<<(unsigned)N, 256, 0, st>>>(partials, x_lengths, y_lengths, N, P1, P2, z.bpc_x, z.bpc_y, single,
                                                            point_reduction == 2, sums);
    return launch_status();
  }
  return P3D_OK;
}

P3D_API int p3di_chamfer_normals_backward(const float* x, const float* y, const float* x_normals, const float* y_normals,
                                          const int64_t* x_lengths, const int64_t* y_lengths, const int64_t* idx_x, const int64_t* idx_y,
                                          const float* weights, const float* cloud_grad, const float* grad_dist_x,
                                          const float* grad_normal_x, const float* grad_dist_y, const float* grad_normal_y, int64_t N,
                                          int64_t P1, int64_t P2, int norm, int abs_cosine, int single_directional, int point_mean, float* grad_x, float* grad_y, float* grad_x_normals,
                                          float* grad_y_normals, p3d_stream_t stream) {
  Sizes z;
  const int single = single_directional != 0;
  if (!sizes_ok(N, P1, P2, single, &z) || (norm != 1 && norm != 2)) return P3D_ERR_INVALID_ARG;
  if (N * (P1 + P2) == 0) return P3D_OK;
  if (P1 == 0 || P2 == 0) return P3D_ERR_INVALID_ARG;  // nothing to pair: the caller answers with zeros
  if (!x || !y || !x_normals || !y_normals || !idx_x || (!single && !idx_y)) return P3D_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  Back k;
  k.c = Clouds{x, y, x_normals, y_normals, x_lengths, y_lengths, N, P1, P2};
  k.idx_x = idx_x, k.idx_y = idx_y, k.cloud_grad = cloud_grad, k.weights = weights;
  k.gdx = grad_dist_x, k.gnx = grad_normal_x, k.gdy = grad_dist_y, k.gny = grad_normal_y;
  k.norm = norm, k.abs_cosine = abs_cosine, k.point_mean = point_mean != 0;
  {
    LaunchScope ls("chamfer_normals_backward_near", st);
    chamfer_normals_bwd_near_kernel<<<stream_blocks(N * (P1 + P2)), 256, 0, st>>>(k, single, grad_x, grad_y, grad_x_normals, grad_y_normals);
    const int rc = launch_status();
    if (rc != P3D_OK) return rc;
  }
  const bool from_x = grad_y || grad_y_normals, from_y = !single && (grad_x || grad_x_normals);  // which direction's hits land somewhere
  if (!from_x && !from_y) return P3D_OK;
  const int64_t hits = N * P1 + (from_y ? N * P2 : 0);
  const int64_t nwaves = ceil_div(hits, kHits);
  LaunchScope ls("chamfer_normals_backward_far", st);
  chamfer_normals_bwd_far_kernel<<<stream_blocks(nwaves * kWave), 256, 0, st>>>(k, hits, nwaves, from_y ? grad_x : nullptr, grad_y,
                                                                                 from_y ? grad_x_normals : nullptr, grad_y_normals);
  return launch_status();
}
