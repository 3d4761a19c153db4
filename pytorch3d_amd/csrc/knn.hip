// knn.hip -- brute-force K nearest neighbours between padded point clouds and the chamfer sums on top of K = 1, forward and
// backward (pytorch3d/ops/knn.py over knn_cpu.cpp's contract, pytorch3d/loss/chamfer.py).  include/p3d_amd.h has the contract.
//
// Forward: ONE LANE PER QUERY, the query in registers, one wave (64 queries of one cloud) per workgroup.  The p2 index of the scan
// is wave-uniform: the wave stages kTile points of its cloud's p2 in LDS as structure of arrays and every lane reads the same four
// points with one ds_read_b128 per coordinate -- identical addresses broadcast, no bank conflict.  A tile's tail up to a multiple
// of four is filled with NaN coordinates: a NaN distance fails every `<`, so the loop needs no remainder code.
//   K = 1 (chamfer)  no queue: compare and two selects per pair; for D = 3 that is 3 sub, 3 mul, 2 add, 1 cmp, 2 cndmask.
//   K > 1            a sorted queue (knn_queue.h) of KQ in {2, 4, 8, 16, 32} (distance, index) pairs in registers.  A candidate is looked at only
//                    when some lane of the wave beats its current worst (one ballot per pair); the insert is a fully unrolled,
//                    branch-free shift: slot s takes its left neighbour where that one is larger than the candidate, else the
//                    candidate where it itself is larger.  Strict comparisons and ascending j give the (dist, j) order: an equal
//                    distance met later never displaces or overtakes an earlier one.
// A distance is the per-coordinate difference, squared or absolute, accumulated in coordinate order, each a float32 operation of
// its own: NOT fused (-ffp-contract=off), the same in every instantiation.
// One wave per workgroup keeps 1 x 5000 x 5000 at 79 workgroups instead of 20 and needs no workgroup barrier beyond the wave's own;
// the tile is re-staged per wave from L2 (D * 2 KiB per 512 x 64 pairs).
//
// Chamfer: the K = 1 kernel also multiplies a query's distance by its cloud's weight and sums the wave; a second launch (one block
// per cloud) adds a cloud's wave partials: the fixed tree of fixed_sum.h with a wave of 64 queries at level 1.  No float atomic in
// the forward.
//
// Backward: grad_p1 is a gather (one lane per (n, i), k ascending).  grad_p2 is a scatter with float atomics, lane = hit * D +
// coordinate so that the D values of one hit leave from adjacent lanes (profiles/microbench/global_atomic_mi355x.txt), after
// consecutive hits of one point have been summed inside the wave; its ordered form is in ordered_bwd.hip.  All three take a hit's
// terms from knn_grad.h.
#include "fixed_sum.h"
#include "knn_grad.h"
#include "knn_queue.h"
#include "vec3.h"

namespace p3d {
namespace {

constexpr int kTile = P3D_KNN_TILE;
static_assert(kTile % 4 == 0, "a tile is read four points at a time");

template <int NORM>
__device__ __forceinline__ float coord_term(float x, float y) {
  const float d = x - y;
  return NORM == 2 ? d * d : fabsf(d);
}

template <int D, int NORM>
__device__ __forceinline__ float pair_dist(const float (&q)[D], const float (&y)[D]) {
  float s = coord_term<NORM>(q[0], y[0]);
#pragma unroll
  for (int c = 1; c < D; ++c) s = s + coord_term<NORM>(q[c], y[c]);
  return s;
}

// grid: N * blocks_per_cloud workgroups of one wave.  K <= KQ.  partials != NULL (KQ == 1 only): the chamfer terms of the wave.
template <int D, int NORM, int KQ>
__global__ __launch_bounds__(64) void knn_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                 const int64_t* __restrict__ lengths1, const int64_t* __restrict__ lengths2, int64_t P1,
                                                 int64_t P2, int K, int64_t blocks_per_cloud, const float* __restrict__ weights,
                                                 int64_t* __restrict__ idx, float* __restrict__ dists, float* __restrict__ partials) {
  __shared__ __align__(16) float tile[D][kTile];
  const int lane = threadIdx.x;
  const int64_t n = blockIdx.x / blocks_per_cloud, b = blockIdx.x % blocks_per_cloud;
  const int64_t i = b * kWave + lane;
  const int64_t len1 = knn::cloud_length(lengths1, n, P1), len2 = knn::cloud_length(lengths2, n, P2);
  const bool live = i < len1;
  float q[D];
#pragma unroll
  for (int c = 0; c < D; ++c) q[c] = live ? p1[(n * P1 + i) * D + c] : 0.0f;
  Queue<KQ> best;
  best.init();
  const int64_t scan = b * kWave < len1 ? len2 : 0;  // wave-uniform: a wave of padding rows scans nothing
  for (int64_t j0 = 0; j0 < scan; j0 += kTile) {
    const int tn = (int)(scan - j0 < kTile ? scan - j0 : kTile), tn4 = (tn + 3) & ~3;
    __syncthreads();  // the wave is done with the tile before
    const float* src = p2 + (n * P2 + j0) * D;
    for (int e = lane; e < tn * D; e += kWave) tile[e % D][e / D] = src[e];
    if (lane < tn4 - tn) {
#pragma unroll
      for (int c = 0; c < D; ++c) tile[c][tn + lane] = quiet_nan();
    }
    __syncthreads();
    for (int t = 0; t < tn4; t += 4) {
      float4 v[D];
#pragma unroll
      for (int c = 0; c < D; ++c) v[c] = *reinterpret_cast<const float4*>(&tile[c][t]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float y[D];
#pragma unroll
        for (int c = 0; c < D; ++c) y[c] = u == 0 ? v[c].x : (u == 1 ? v[c].y : (u == 2 ? v[c].z : v[c].w));
        const float dn = pair_dist<D, NORM>(q, y);
        const int jn = (int)j0 + t + u;
        if constexpr (KQ == 1) {
          const bool better = dn < best.d[0];
          best.d[0] = better ? dn : best.d[0];
          best.j[0] = better ? jn : best.j[0];
        } else {
          if (__ballot(best.wants(dn)) != 0ull) best.insert(dn, jn);
        }
      }
    }
  }
  const int found = (int)(len2 < K ? len2 : K);
  if (i < P1) {
    const int64_t row = (n * P1 + i) * K;
#pragma unroll
    for (int k = 0; k < KQ; ++k) {
      if (k < K) {
        const bool slot = live && k < found;
        idx[row + k] = slot && best.j[k] >= 0 ? (int64_t)best.j[k] : 0;
        dists[row + k] = slot ? best.d[k] : 0.0f;
      }
    }
  }
  if constexpr (KQ == 1) {
    if (partials) {  // wave-uniform
      const float w = weights ? weights[n] : 1.0f;
      const float term = wave_sum(live && found > 0 ? best.d[0] * w : 0.0f);
      if (lane == 0) partials[blockIdx.x] = term;
    }
  }
}

// the last step of segment_sum_kernel over a cloud's wave partials: for point_mean, cham_x /= x_lengths.clamp(min=1)
struct CloudMean {
  const int64_t* lengths1;
  int64_t P1;
  int point_mean;
  __device__ __forceinline__ float operator()(int64_t n, float s) const {
    if (!point_mean) return s;
    const int64_t len1 = knn::cloud_length(lengths1, n, P1);
    return s / (float)(len1 < 1 ? 1 : len1);
  }
};

// grad_p1: one lane per (n, i); every entry written
template <int D>
__global__ __launch_bounds__(256) void knn_bwd_gather_kernel(knn::Hits h, float* __restrict__ grad_p1) {
  const int64_t rows = h.N * h.P1;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256) {
    float acc[D];
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] = 0.0f;
    for (int k = 0; k < h.K; ++k) {
      const int64_t e = r * h.K + k, t = h.target(e);
      if (t < 0) continue;
      const float g = h.upstream(e);
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] += h.term(e, t, c, g);
    }
#pragma unroll
    for (int c = 0; c < D; ++c) grad_p1[r * D + c] = acc[c];
  }
}

// grad_p2: lane = hit * D + coordinate, a wave owns kWave / D consecutive hits (the last 64 % D lanes idle).  Consecutive hits of
// one p2 point -- a cloud that many queries share one neighbour of -- are first summed inside the wave by a segmented scan over the
// run (ordered_sum.h's), and the last hit of a run issues the atomics: its D adjacent lanes.  Runs of one hit, the common case, go
// through unchanged.  The scan is written out here, in ordered_sum.h (pass1_kernel) and in transform.hip on purpose: hoisted into a
// shared helper it compiled ordered::pass1_kernel<Op> to 2-3 % more instructions (ordered_sum.h has the figures).
template <int D>
__global__ __launch_bounds__(256) void knn_bwd_scatter_kernel(knn::Hits h, int64_t nwaves, float* __restrict__ grad_p2) {
  constexpr int kHits = kWave / D;  // hits per wave
  const int lane = threadIdx.x & 63, hw = lane / D, c = lane % D;
  const int first = hw * D;  // the lane of this hit's coordinate 0
  const int64_t hits = h.N * h.P1 * h.K;
  for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < nwaves; w += (int64_t)gridDim.x * 4) {  // wave-uniform
    const int64_t e = w * kHits + hw;
    const bool mine = hw < kHits && e < hits;
    const int64_t t = mine ? h.target(e) : -1;
    float v = t >= 0 ? -h.term(e, t, c, h.upstream(e)) : 0.0f;
    // a run: consecutive hits of the wave with one target; lanes without a hit are runs of their own
    const int64_t before = __shfl_up(t, D);
    const bool head = hw == 0 || before != t || t < 0;
    const unsigned long long heads = __ballot(head && c == 0);
    const int start = (63 - __clzll((long long)(heads & ((2ull << first) - 1ull)))) / D;  // first hit of this lane's run
#pragma unroll
    for (int d = 1; d < kHits; d <<= 1) {
      const float below = __shfl_up(v, d * D);
      if (hw - d >= start) v += below;
    }
    const int64_t after = __shfl_down(t, D);
    const bool tail = hw + 1 >= kHits || after != t;
    if (t >= 0 && tail) atomicAdd(grad_p2 + t * D + c, v);
  }
}

// every index the kernels form must fit an int64 comfortably and a hit's j an int32
bool sizes_ok(int64_t N, int64_t P1, int64_t P2, int K) {
  if (N < 0 || P1 < 0 || P2 < 0 || P2 > INT32_MAX || P1 > INT32_MAX) return false;
  const int64_t per_cloud = (P1 > P2 ? P1 : P2) * (int64_t)(K > 0 ? K : 1) * 4;
  return N == 0 || per_cloud <= INT64_MAX / 4 / N;
}

template <int D, int NORM>
int launch_forward_dn(const float* p1, const float* p2, const int64_t* l1, const int64_t* l2, int64_t N, int64_t P1, int64_t P2, int K,
                      const float* weights, int64_t* idx, float* dists, float* partials, hipStream_t s) {
  const int64_t bpc = ceil_div(P1, kWave), blocks = N * bpc;
  if (blocks > 0x7fffffffll) return P3D_ERR_INVALID_ARG;
  const unsigned g = (unsigned)blocks;
#define P3D_KNN_LAUNCH(KQ) knn_kernel<D, NORM, KQ><<<g, 64, 0, s>>>(p1, p2, l1, l2, P1, P2, K, bpc, weights, idx, dists, partials)
  if (K == 1) P3D_KNN_LAUNCH(1);
  else if (K <= 2) P3D_KNN_LAUNCH(2);
  else if (K <= 4) P3D_KNN_LAUNCH(4);
  else if (K <= 8) P3D_KNN_LAUNCH(8);
  else if (K <= 16) P3D_KNN_LAUNCH(16);
  else P3D_KNN_LAUNCH(32);
#undef P3D_KNN_LAUNCH
  return launch_status();
}

int launch_forward(const float* p1, const float* p2, const int64_t* l1, const int64_t* l2, int64_t N, int64_t P1, int64_t P2, int D, int K,
                   int norm, const float* weights, int64_t* idx, float* dists, float* partials, hipStream_t s) {
  if (D == 3) {
    return norm == 2 ? launch_forward_dn<3, 2>(p1, p2, l1, l2, N, P1, P2, K, weights, idx, dists, partials, s)
                     : launch_forward_dn<3, 1>(p1, p2, l1, l2, N, P1, P2, K, weights, idx, dists, partials, s);
  }
  return norm == 2 ? launch_forward_dn<2, 2>(p1, p2, l1, l2, N, P1, P2, K, weights, idx, dists, partials, s)
                   : launch_forward_dn<2, 1>(p1, p2, l1, l2, N, P1, P2, K, weights, idx, dists, partials, s);
}

int check_forward(const float* p1, const float* p2, int64_t N, int64_t P1, int64_t P2, int D, int K, int norm, const int64_t* idx,
                  const float* dists) {
  if (!sizes_ok(N, P1, P2, K) || (norm != 1 && norm != 2) || K < 1 || D < 1) return P3D_ERR_INVALID_ARG;
  if ((D != 2 && D != 3) || K > P3D_KNN_MAX_K) return P3D_ERR_UNSUPPORTED;
  if (N * P1 > 0 && (!p1 || !idx || !dists || (P2 > 0 && !p2))) return P3D_ERR_INVALID_ARG;
  return P3D_OK;
}

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API int p3d_knn_points_forward(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2, int64_t N,
                                   int64_t P1, int64_t P2, int D, int K, int norm, int64_t* idx, float* dists, p3d_stream_t stream) {
  const int st = check_forward(p1, p2, N, P1, P2, D, K, norm, idx, dists);
  if (st != P3D_OK || N * P1 == 0) return st;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls(K == 1 ? "knn_forward_k1" : "knn_forward", s);
  return launch_forward(p1, p2, lengths1, lengths2, N, P1, P2, D, K, norm, nullptr, idx, dists, nullptr, s);
}

P3D_API size_t p3d_chamfer_forward_workspace_bytes(int64_t N, int64_t P1) {
  return N <= 0 || P1 <= 0 ? 0 : (size_t)N * (size_t)ceil_div(P1, kWave) * sizeof(float);
}

P3D_API int p3d_chamfer_forward(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2, const float* weights,
                                int64_t N, int64_t P1, int64_t P2, int D, int norm, int point_mean, int64_t* idx, float* dists,
                                float* sums, void* workspace, size_t workspace_bytes, p3d_stream_t stream) {
  const int st = check_forward(p1, p2, N, P1, P2, D, 1, norm, idx, dists);
  if (st != P3D_OK || N == 0) return st;
  if (!sums) return P3D_ERR_INVALID_ARG;
  if (P1 > 0 && (!workspace || workspace_bytes < p3d_chamfer_forward_workspace_bytes(N, P1))) return P3D_ERR_WORKSPACE;
  if (N > 0x7fffffffll) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  float* partials = static_cast<float*>(workspace);
  if (P1 > 0) {
    LaunchScope ls("chamfer_forward_k1", s);
    const int rc = launch_forward(p1, p2, lengths1, lengths2, N, P1, P2, D, 1, norm, weights, idx, dists, partials, s);
    if (rc != P3D_OK) return rc;
  }
  LaunchScope ls("chamfer_cloud_sum", s);
  segment_sum_kernel<<<(unsigned)N, 256, 0, s>>>(partials, ceil_div(P1, kWave), CloudMean{lengths1, P1, point_mean}, sums);
  return launch_status();
}

P3D_API int p3d_knn_points_backward(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2, const int64_t* idx,
                                    const float* grad_dists, const float* cloud_scale, int64_t N, int64_t P1, int64_t P2, int D, int K,
                                    int norm, unsigned flags, float* grad_p1, float* grad_p2, p3d_stream_t stream) {
  if (!sizes_ok(N, P1, P2, K) || (norm != 1 && norm != 2) || K < 1 || D < 1) return P3D_ERR_INVALID_ARG;
  if (D != 2 && D != 3) return P3D_ERR_UNSUPPORTED;
  const int64_t hits = N * P1 * K;
  if (hits > 0 && P2 > 0 && (!p1 || !p2 || !idx)) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  knn::Hits h;
  h.p1 = p1, h.p2 = p2, h.lengths1 = lengths1, h.lengths2 = lengths2, h.idx = idx, h.grad_dists = grad_dists, h.cloud_scale = cloud_scale;
  h.N = N, h.P1 = P1, h.P2 = P2, h.D = D, h.K = K, h.norm = norm;
  if (grad_p1 && N * P1 > 0) {
    if (P2 == 0) {
      if (hipMemsetAsync(grad_p1, 0, (size_t)(N * P1 * D) * sizeof(float), s) != hipSuccess) return P3D_ERR_LAUNCH;
    } else {
      LaunchScope ls("knn_backward_gather", s);
      if (D == 3) knn_bwd_gather_kernel<3><<<stream_blocks(N * P1), 256, 0, s>>>(h, grad_p1);
      else knn_bwd_gather_kernel<2><<<stream_blocks(N * P1), 256, 0, s>>>(h, grad_p1);
      const int rc = launch_status();
      if (rc != P3D_OK) return rc;
    }
  }
  if (grad_p2 && N * P2 > 0) {
    if (!(flags & P3D_KNN_ACCUMULATE_P2) &&
        hipMemsetAsync(grad_p2, 0, (size_t)(N * P2 * D) * sizeof(float), s) != hipSuccess)
      return P3D_ERR_LAUNCH;
    if (hits > 0) {
      LaunchScope ls("knn_backward_scatter", s);
      const int64_t nwaves = ceil_div(hits, kWave / D);
      if (D == 3) knn_bwd_scatter_kernel<3><<<stream_blocks(nwaves * kWave), 256, 0, s>>>(h, nwaves, grad_p2);
      else knn_bwd_scatter_kernel<2><<<stream_blocks(nwaves * kWave), 256, 0, s>>>(h, nwaves, grad_p2);
      return launch_status();
    }
  }
  return P3D_OK;
}
