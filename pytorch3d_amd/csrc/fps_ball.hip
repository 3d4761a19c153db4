// fps_ball.hip -- farthest point sampling and ball query over padded point clouds (pytorch3d/ops/sample_farthest_points.py over
// sample_farthest_points_cpu.cpp's contract, pytorch3d/ops/ball_query.py).  include/p3d_amd.h has the contract.
//
// Farthest point sampling is a chain of K dependent steps, each a distance update plus an arg-max over a whole cloud.  ONE
// WORKGROUP PER CLOUD and nothing between workgroups: no spin, no ticket, no cooperative launch -- a small N uses few CUs.
//   register form   T lanes (64 .. 1024, chosen on the host from P alone) hold R in {1, 2, 4, 8, 16} points each -- coordinates
//                   and running minimum distance in VGPRs, point r * T + tid in slot r -- so a cloud of up to 16 384 points
//                   never leaves the register file.  One step: (1) every held point's minimum takes its distance to the last
//                   selected point, and the lane keeps its best (distance, index, coordinates), slots ascending with a strict >;
//                   (2) the wave's best: the maximum by four DPP rounds inside each row of 16 lanes and a read of the four rows,
//                   then in the same way the lowest index among the lanes that hold it; (3) the lane
//                   that owns the wave's winner writes (distance, index, coordinates) into the wave's LDS slot; (4) ONE
//                   barrier; (5) every wave reads all slots, one slot per lane, and reduces them redundantly with the same DPP
//                   rounds: every lane then has the next selected point AND its coordinates without a second barrier or a global
//                   read.  The slots are double-buffered by step parity: a wave can only write a slot again after the barrier of the
//                   step in between, which every wave reaches after it has read the slot.
//   workspace form  P > 16 384: the same workgroup of 1024 lanes and the same reduction; the minimum distances live in a row of
//                   the workspace (N, P) and the points are re-read (from L2) every step.
// The order is total: the larger minimum wins, equal minima go to the LOWER index (std::max_element's first maximum).  A selected
// point needs no mask: its distance to itself is 0.  Padding slots hold a minimum of -1, below every real one, and never change:
// no distance is < -1 and a NaN distance fails the comparison.  A minimum is never NaN (d < m ? d : m from +inf), so as long as
// a cloud has one point the winner is a real index whatever the coordinates hold.
//
// Ball query is the layout of knn.hip's forward -- one lane per query, one wave per workgroup, p2 staged per P3D_KNN_TILE points
// in LDS as structure of arrays and broadcast, the tile's tail filled with NaN -- with a per-lane COUNT in place of the queue: pair
// j, ascending, is a hit when dist2 < radius2 (strictly) and the row is not full; the lane stores it at slot `count` directly
// (rows go to memory: K defaults to 500).  The wave leaves the scan when a ballot shows every live lane full.  The slots behind
// a row's count are written row by row, the lanes along k.
#include "knn_grad.h"
#include "vec3.h"

namespace p3d {
namespace {

constexpr int kTile = P3D_KNN_TILE;
constexpr int kFpsMaxLanes = 1024;
constexpr int kFpsMaxWaves = kFpsMaxLanes / kWave;
static_assert(kTile % 4 == 0, "a tile is read four points at a time");
static_assert(P3D_FPS_REGISTER_POINTS == kFpsMaxLanes * 16, "the top rung is 16 points per lane of the largest workgroup");

__device__ __forceinline__ float pos_inf() { return __int_as_float(0x7f800000); }

// the squared distance: per coordinate the difference and its square, accumulated in coordinate order, NOT fused
template <int D>
__device__ __forceinline__ float dist2(const float (&a)[D], const float (&b)[D]) {
  const float d0 = a[0] - b[0];
  float s = d0 * d0;
#pragma unroll
  for (int c = 1; c < D; ++c) {
    const float d = a[c] - b[c];
    s = s + d * d;
  }
  return s;
}

// ---- farthest point sampling ----------------------------------------------------------------------------------------------------
constexpr int kNoPoint = 0x7fffffff;  // the index of "nothing": loses every tie

// The selection order on (minimum, index): the larger minimum, then the lower index.  A minimum is +0 or above, +inf included, and
// "nothing" is -1: as SIGNED integers the bit patterns of those floats compare like the floats, so the reductions below run on
// integers (v_max_i32 / v_min_i32 take the DPP operand directly and need no NaN handling).
template <int CTRL>
__device__ __forceinline__ int dpp(int x) {
  return __builtin_amdgcn_update_dpp(x, x, CTRL, 0xf, 0xf, true);  // every lane of these patterns has a source: bound_ctrl never acts
}

// every lane of a row of 16 gets the row's maximum / minimum: lane ^ 1, lane ^ 2 (quad_perm), then the mirrored half row and row.
// All 64 lanes must be active.
__device__ __forceinline__ int row_max(int x) {
  x = max(x, dpp<0xB1>(x));   // quad_perm [1, 0, 3, 2]
  x = max(x, dpp<0x4E>(x));   // quad_perm [2, 3, 0, 1]
  x = max(x, dpp<0x141>(x));  // row_half_mirror
  return max(x, dpp<0x140>(x));  // row_mirror
}
__device__ __forceinline__ int row_min(int x) {
  x = min(x, dpp<0xB1>(x));
  x = min(x, dpp<0x4E>(x));
  x = min(x, dpp<0x141>(x));
  return min(x, dpp<0x140>(x));
}
__device__ __forceinline__ int rows_max(int x) {  // wave-uniform, of the four rows' values
  const int a = max(__builtin_amdgcn_readlane(x, 0), __builtin_amdgcn_readlane(x, 16));
  const int b = max(__builtin_amdgcn_readlane(x, 32), __builtin_amdgcn_readlane(x, 48));
  return max(a, b);
}
__device__ __forceinline__ int rows_min(int x) {
  const int a = min(__builtin_amdgcn_readlane(x, 0), __builtin_amdgcn_readlane(x, 16));
  const int b = min(__builtin_amdgcn_readlane(x, 32), __builtin_amdgcn_readlane(x, 48));
  return min(a, b);
}

// wave-uniform: the wave's best -- the largest minimum, and among the lanes that hold it the lowest index
__device__ __forceinline__ void wave_best(float& d, int& i) {
  const int k = __float_as_int(d);
  const int wk = rows_max(row_max(k));
  i = rows_min(row_min(k == wk ? i : kNoPoint));
  d = __int_as_float(wk);
}

struct FpsSlots {
  float4 head[2][kFpsMaxWaves];  // (distance, index bits, x, y) by step parity and wave
  float z[2][kFpsMaxWaves];
};

// Steps (3) to (5) of the header: the lane's best (bd, bi, bc) in, the workgroup's best out -- index returned, coordinates in sel.
// point i lives in lane i % T: its wave is (i % T) / 64.
template <int D, int T>
__device__ __forceinline__ int fps_select(FpsSlots& slots, int parity, float bd, int bi, const float (&bc)[D], float (&sel)[D]) {
  constexpr int W = T / kWave;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float wd = bd;
  int wi = bi;
  wave_best(wd, wi);
  if (W == 1) {
    // the owner's coordinates straight from its lane
    const int owner = __builtin_amdgcn_readfirstlane(wi == kNoPoint ? 0 : (wi & 63));
#pragma unroll
    for (int c = 0; c < D; ++c) sel[c] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bc[c]), owner));
    return wi;
  }
  if (bi == wi) {  // one lane, or every lane of a wave of padding (all the same values)
    slots.head[parity][wave] = make_float4(wd, __int_as_float(wi), bc[0], bc[1]);
    if (D == 3) slots.z[parity][wave] = bc[D - 1];
  }
  __syncthreads();
  float4 h = make_float4(-1.0f, __int_as_float(kNoPoint), 0.0f, 0.0f);
  float z = 0.0f;
  if (lane < W) {
    h = slots.head[parity][lane];
    if (D == 3) z = slots.z[parity][lane];
  }
  // W <= 16: one row of lanes holds every slot
  const int k = __float_as_int(h.x);
  const int gk = __builtin_amdgcn_readfirstlane(row_max(k));
  const int gi = __builtin_amdgcn_readfirstlane(row_min(k == gk ? __float_as_int(h.y) : kNoPoint));
  const int owner = gi == kNoPoint ? 0 : ((gi & (T - 1)) >> 6);
  sel[0] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(h.z), owner));
  sel[1] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(h.w), owner));
  if (D == 3) sel[D - 1] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(z), owner));
  return gi;
}

// what a cloud's row of idx holds: count = min(K[n], length) entries, the first one start (clamped into the cloud)
struct FpsRow {
  int64_t len, count, start;
};
__device__ __forceinline__ FpsRow fps_row(const int64_t* __restrict__ lengths, const int64_t* __restrict__ K,
                                          const int64_t* __restrict__ start_idxs, int64_t n, int64_t P, int64_t max_K) {
  FpsRow r;
  r.len = knn::cloud_length(lengths, n, P);
  int64_t k = K ? K[n] : max_K;
  k = k < 0 ? 0 : (k > max_K ? max_K : k);
  r.count = k < r.len ? k : r.len;
  const int64_t s = start_idxs ? start_idxs[n] : 0;
  r.start = s < 0 ? 0 : (s >= r.len ? (r.len > 0 ? r.len - 1 : 0) : s);
  return r;
}

// grid: N workgroups of T lanes; P <= T * R
template <int D, int T, int R>
__global__ __launch_bounds__(T) void fps_register_kernel(const float* __restrict__ points, const int64_t* __restrict__ lengths,
                                                         const int64_t* __restrict__ K, const int64_t* __restrict__ start_idxs, int64_t P,
                                                         int64_t max_K, int64_t* __restrict__ idx) {
  __shared__ __align__(16) FpsSlots slots;
  const int tid = threadIdx.x;
  const int64_t n = blockIdx.x;
  const FpsRow row = fps_row(lengths, K, start_idxs, n, P, max_K);
  const float* cloud = points + n * P * D;
  int64_t* out = idx + n * max_K;
  float p[R][D], m[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = r * T + tid;
    const bool held = i < row.len;
#pragma unroll
    for (int c = 0; c < D; ++c) p[r][c] = held ? cloud[(int64_t)i * D + c] : 0.0f;
    m[r] = held ? pos_inf() : -1.0f;
  }
  float sel[D];
  if (row.count > 0) {
#pragma unroll
    for (int c = 0; c < D; ++c) sel[c] = cloud[row.start * D + c];
    if (tid == 0) out[0] = row.start;
  }
  for (int64_t s = 1; s < row.count; ++s) {  // workgroup-uniform
    float bd = -1.0f, bc[D];
    int bi = kNoPoint;
#pragma unroll
    for (int c = 0; c < D; ++c) bc[c] = 0.0f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float d = dist2<D>(sel, p[r]);
      m[r] = d < m[r] ? d : m[r];
      const bool b = m[r] > bd;  // slots ascend in index: a later equal minimum does not displace
      bd = b ? m[r] : bd;
      bi = b ? r * T + tid : bi;
#pragma unroll
      for (int c = 0; c < D; ++c) bc[c] = b ? p[r][c] : bc[c];
    }
    const int gi = fps_select<D, T>(slots, (int)(s & 1), bd, bi, bc, sel);
    if (tid == 0) out[s] = gi;
  }
  for (int64_t s = (row.count > 0 ? row.count : 0) + tid; s < max_K; s += T) out[s] = -1;
}

// grid: N workgroups of 1024 lanes; any P.  mins: (N, P) floats of the workspace, written at step 1 before they are read.
template <int D>
__global__ __launch_bounds__(kFpsMaxLanes) void fps_workspace_kernel(const float* __restrict__ points, const int64_t* __restrict__ lengths,
                                                                     const int64_t* __restrict__ K, const int64_t* __restrict__ start_idxs,
                                                                     int64_t P, int64_t max_K, float* __restrict__ mins,
                                                                     int64_t* __restrict__ idx) {
  constexpr int T = kFpsMaxLanes;
  __shared__ __align__(16) FpsSlots slots;
  const int tid = threadIdx.x;
  const int64_t n = blockIdx.x;
  const FpsRow row = fps_row(lengths, K, start_idxs, n, P, max_K);
  const float* cloud = points + n * P * D;
  float* mine = mins + n * P;
  int64_t* out = idx + n * max_K;
  const int len = (int)row.len;
  float sel[D];
  if (row.count > 0) {
#pragma unroll
    for (int c = 0; c < D; ++c) sel[c] = cloud[row.start * D + c];
    if (tid == 0) out[0] = row.start;
  }
  for (int64_t s = 1; s < row.count; ++s) {
    float bd = -1.0f, bc[D];
    int bi = kNoPoint;
#pragma unroll
    for (int c = 0; c < D; ++c) bc[c] = 0.0f;
    for (int i = tid; i < len; i += T) {  // ascending in index; a lane reads and writes only its own entries of the row
      float x[D];
#pragma unroll
      for (int c = 0; c < D; ++c) x[c] = cloud[(int64_t)i * D + c];
      const float d = dist2<D>(sel, x);
      const float before_m = s == 1 ? pos_inf() : mine[i];
      const float mi = d < before_m ? d : before_m;
      mine[i] = mi;
      const bool b = mi > bd;
      bd = b ? mi : bd;
      bi = b ? i : bi;
#pragma unroll
      for (int c = 0; c < D; ++c) bc[c] = b ? x[c] : bc[c];
    }
    const int gi = fps_select<D, T>(slots, (int)(s & 1), bd, bi, bc, sel);
    if (tid == 0) out[s] = gi;
  }
  for (int64_t s = (row.count > 0 ? row.count : 0) + tid; s < max_K; s += T) out[s] = -1;
}

template <int D>
int launch_fps(const float* points, const int64_t* lengths, const int64_t* K, const int64_t* start, int64_t N, int64_t P, int64_t max_K,
               int64_t* idx, float* mins, hipStream_t s) {
  const unsigned g = (unsigned)N;
#define P3D_FPS_LAUNCH(T, R) fps_register_kernel<D, T, R><<<g, T, 0, s>>>(points, lengths, K, start, P, max_K, idx)
  if (P <= 64) P3D_FPS_LAUNCH(64, 1);
  else if (P <= 128) P3D_FPS_LAUNCH(128, 1);
  else if (P <= 256) P3D_FPS_LAUNCH(256, 1);
  else if (P <= 512) P3D_FPS_LAUNCH(512, 1);
  else if (P <= 1024) P3D_FPS_LAUNCH(1024, 1);
  else if (P <= 2048) P3D_FPS_LAUNCH(1024, 2);
  else if (P <= 4096) P3D_FPS_LAUNCH(1024, 4);
  else if (P <= 8192) P3D_FPS_LAUNCH(1024, 8);
  else if (P <= P3D_FPS_REGISTER_POINTS) P3D_FPS_LAUNCH(1024, 16);
  else fps_workspace_kernel<D><<<g, kFpsMaxLanes, 0, s>>>(points, lengths, K, start, P, max_K, mins, idx);
#undef P3D_FPS_LAUNCH
  return launch_status();
}

// ---- ball query -------------------------------------------------------------------------------------------------------------------
// grid: N * blocks_per_cloud workgroups of one wave
template <int D>
__global__ __launch_bounds__(64) void ball_query_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                        const int64_t* __restrict__ lengths1, const int64_t* __restrict__ lengths2,
                                                        int64_t P1, int64_t P2, int K, float radius2, int64_t blocks_per_cloud,
                                                        int64_t* __restrict__ idx, float* __restrict__ dists) {
  __shared__ __align__(16) float tile[D][kTile];
  const int lane = threadIdx.x;
  const int64_t n = blockIdx.x / blocks_per_cloud, b = blockIdx.x % blocks_per_cloud;
  const int64_t i0 = b * kWave, i = i0 + lane;
  const int64_t len1 = knn::cloud_length(lengths1, n, P1), len2 = knn::cloud_length(lengths2, n, P2);
  const bool live = i < len1;
  float q[D];
#pragma unroll
  for (int c = 0; c < D; ++c) q[c] = live ? p1[(n * P1 + i) * D + c] : 0.0f;
  const int64_t mine = (n * P1 + (live ? i : i0)) * K;  // the row this lane appends to
  int count = 0;
  const int64_t scan = i0 < len1 ? len2 : 0;  // wave-uniform: a wave of padding rows scans nothing
  bool full = false;                          // wave-uniform: every live row holds K hits
  for (int64_t j0 = 0; j0 < scan && !full; j0 += kTile) {
    const int tn = (int)(scan - j0 < kTile ? scan - j0 : kTile), tn4 = (tn + 3) & ~3;
    __syncthreads();  // the wave is done with the tile before
    const float* src = p2 + (n * P2 + j0) * D;
    for (int e = lane; e < tn * D; e += kWave) tile[e % D][e / D] = src[e];
    if (lane < tn4 - tn) {
#pragma unroll
      for (int c = 0; c < D; ++c) tile[c][tn + lane] = quiet_nan();
    }
    __syncthreads();
    for (int t = 0; t < tn4 && !full; t += 4) {
      float4 v[D];
#pragma unroll
      for (int c = 0; c < D; ++c) v[c] = *reinterpret_cast<const float4*>(&tile[c][t]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float y[D];
#pragma unroll
        for (int c = 0; c < D; ++c) y[c] = u == 0 ? v[c].x : (u == 1 ? v[c].y : (u == 2 ? v[c].z : v[c].w));
        const float dn = dist2<D>(q, y);
        if (live && count < K && dn < radius2) {  // a NaN distance (the tile's tail among them) is no hit
          idx[mine + count] = j0 + t + u;
          dists[mine + count] = dn;
          ++count;
        }
      }
      full = __ballot(live && count < K) == 0ull;
    }
  }
  // behind a row's count: -1 / 0, row by row with the lanes along k (rows past lengths1 have a count of 0)
  const int rows = (int)(P1 - i0 < kWave ? P1 - i0 : kWave);
  for (int r = 0; r < rows; ++r) {
    const int from = __shfl(count, r);
    const int64_t base = (n * P1 + i0 + r) * K;
    for (int k = from + lane; k < K; k += kWave) {
      idx[base + k] = -1;
      dists[base + k] = 0.0f;
    }
  }
}

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API size_t p3d_sample_farthest_points_workspace_bytes(int64_t N, int64_t P) {
  return N <= 0 || P <= P3D_FPS_REGISTER_POINTS ? 0 : (size_t)N * (size_t)P * sizeof(float);
}

P3D_API int p3d_sample_farthest_points(const float* points, const int64_t* lengths, const int64_t* K, const int64_t* start_idxs,
                                       int64_t N, int64_t P, int D, int64_t max_K, int64_t* idx, void* workspace,
                                       size_t workspace_bytes, p3d_stream_t stream) {
  if (N < 0 || P < 0 || P > INT32_MAX || max_K < 0 || D < 1 || N > 0x7fffffffll) return P3D_ERR_INVALID_ARG;
  if (N > 0 && ((P > 0 && P > INT64_MAX / 16 / N) || (max_K > 0 && max_K > INT64_MAX / 16 / N))) return P3D_ERR_INVALID_ARG;
  if (D != 2 && D != 3) return P3D_ERR_UNSUPPORTED;
  if (N == 0 || P == 0 || max_K == 0) return P3D_OK;
  if (!points || !idx) return P3D_ERR_INVALID_ARG;
  const size_t need = p3d_sample_farthest_points_workspace_bytes(N, P);
  if (need > 0 && (!workspace || workspace_bytes < need)) return P3D_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls(need > 0 ? "sample_farthest_points_workspace" : "sample_farthest_points", s);
  float* mins = static_cast<float*>(workspace);
  return D == 3 ? launch_fps<3>(points, lengths, K, start_idxs, N, P, max_K, idx, mins, s)
                : launch_fps<2>(points, lengths, K, start_idxs, N, P, max_K, idx, mins, s);
}

P3D_API int p3d_ball_query(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2, int64_t N, int64_t P1,
                           int64_t P2, int D, int K, float radius, int64_t* idx, float* dists, p3d_stream_t stream) {
  if (N < 0 || P1 < 0 || P2 < 0 || P1 > INT32_MAX || P2 > INT32_MAX || K < 1 || D < 1) return P3D_ERR_INVALID_ARG;
  const int64_t per_cloud = (P1 > P2 ? P1 : P2) * (int64_t)K * 4;
  if (N > 0 && per_cloud > INT64_MAX / 4 / N) return P3D_ERR_INVALID_ARG;
  if (D != 2 && D != 3) return P3D_ERR_UNSUPPORTED;
  if (N * P1 == 0) return P3D_OK;
  if (!p1 || !idx || !dists || (P2 > 0 && !p2)) return P3D_ERR_INVALID_ARG;
  const int64_t bpc = ceil_div(P1, kWave), blocks = N * bpc;
  if (blocks > 0x7fffffffll) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const float radius2 = radius * radius;  // float32, as the reference's `float radius`
  LaunchScope ls("ball_query", s);
  if (D == 3) ball_query_kernel<3><<<(unsigned)blocks, 64, 0, s>>>(p1, p2, lengths1, lengths2, P1, P2, K, radius2, bpc, idx, dists);
  else ball_query_kernel<2><<<(unsigned)blocks, 64, 0, s>>>(p1, p2, lengths1, lengths2, P1, P2, K, radius2, bpc, idx, dists);
  return launch_status();
}
