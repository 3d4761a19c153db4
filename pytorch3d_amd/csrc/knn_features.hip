// knn_features.hip -- K nearest neighbours between padded clouds of FEATURE points, 4 <= D <= 256, squared L2, forward and backward
// (pytorch3d/ops/knn.py at the point dimensions knn.hip does not take).  implicit_abi.h has the contract; DESIGN 8.29 the figures.
//
// The contract's distance is knn.hip's: per coordinate the difference, squared, accumulated in coordinate order, each a float32
// operation of its own.  The cross term of |q|^2 + |y|^2 - 2 q.y is a GEMM, but its rounding error scales with the norms, not with
// the distance, so it only SCREENS: a pair is dropped when even the most favourable reading of the screen value cannot beat the
// query's current worst neighbour; every other pair is evaluated by the contract's arithmetic and offered to the queue.  The result
// is that of the exact scan over all pairs, whatever the screen lets through.
//
// Split.  A wave owns 32 consecutive queries of one cloud, a workgroup of 4 waves 128 (2 waves / 64 where 4 query blocks and two
// tiles pass 160 KB of LDS: D > 178).  The workgroup walks its cloud's p2 in tiles of 32 targets; a tile is staged once for all
// waves, rows padded to the odd stride Dp + 1 (Dp: D rounded up to even, the pad column 0), and tile it + 1 is copied into the
// other buffer before tile it is screened: one barrier per tile.
// Screen.  Per (wave, tile) one 32 x 32 block of y.q over Dp / 2 v_mfma_f32_32x32x2_f32, A = the tile (lane l: target l % 32,
// coordinate 2 k + l / 32), B = the wave's query block from LDS in the same form: lane l then holds, for query l % 32, the 16
// targets 8 (r / 4) + 4 (l / 32) + r % 4.  16 accumulator registers whatever D.  |q|^2 once per wave, |y|^2 by a pre-pass into the
// workspace.
// Rescore.  The survivors of a block are compacted by ballot into the wave's list (query << 5 | target); one lane per entry
// recomputes the distance from the two staged rows (different rows at one coordinate: the odd stride keeps them in different
// banks) into the wave's exact[query][target].
// Queues.  Lane q < 32 keeps the sorted queue of query q in registers (knn_queue.h) and takes its survivors from exact[] in
// ascending target, tiles in ascending j0: a query's candidates arrive in ascending j whatever the tile size, wave count or grid,
// so the queue's strict comparisons give the (dist, j) order as in knn.hip, and a NaN or a distance that does not beat the worst is
// never inserted.
//
// Backward (runtime D): grad_p1 a gather, one lane per (row, coordinate), k ascending; grad_p2 float atomics with lane = hit * D +
// coordinate.  Both take a hit's term from knn_grad.h.
#include "implicit_abi.h"
#include "knn_grad.h"
#include "knn_queue.h"

namespace p3d {
namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int kBlock = 32;                // queries of a wave and targets of a tile: one MFMA block
constexpr int kExactStride = kBlock + 1;  // exact[query][target], odd
constexpr size_t kLdsBytes = 160 * 1024;  // per CU on gfx950

// The screen's error bound E = c(D) (|q|^2 + |y|^2) + kAbsolute, with u = 2^-24 and every multiply and add rounding at most once
// with relative error u, in ANY summation order (the matrix instruction's is not documented; fewer roundings only help).  Write
// S = |q|^2 + |y|^2 in real numbers, d the real distance of the two float32 points; d <= 2 S and sum_c |q_c y_c| <= S / 2.
//   the two norms      a term passes one multiply and at most D - 1 adds, all terms >= 0:           error <= D u S
//   the cross term     a term passes one multiply and at most Dp <= D + 1 adds (the accumulator's
//                      first add included): error <= (D + 2) u S / 2, and the screen doubles it:    error <= (D + 2) u S
//   t = fl(nq + ny), s = fl(t - 2 dot): two roundings of values <= S and <= 2 S:                    error <= 3 u S
//   the contract's distance   a term is fl(fl(x - y)^2), three roundings, then at most D - 1 adds,
//                      all terms >= 0: error <= (D + 2) u d <= (2 D + 4) u S
//   fl(s - E) and the roundings inside E                                                            error <= 3 u S
// together (4 D + 12) u S up to terms of second order, which are below D u = 2^-16 of that.  c(D) = 2 (4 D + 12) u: the factor 2
// pays for the second order, for E being formed from the computed norms and for everything not thought of.  kAbsolute stands for
// results flushed to zero: at most 4 D + 8 operations lose at most 2^-126 each, below 2^-115.
// So when fl(s - E) > worst, the contract's distance is > worst and the queue would not take the pair.
constexpr float kAbsolute = 0x1p-100f;
float screen_factor(int D) { return ldexpf((float)(8 * D + 24), -24); }

// the dynamic LDS of a workgroup of `waves` waves, in floats from its start
struct Layout {
  int stride;  // of a query or tile row
  int tiles;   // two tiles of kBlock rows behind the waves * kBlock query rows (rows contiguous: one loop clears the pad column)
  int ynorm;   // two rows of kBlock |y|^2
  int exact;   // per wave kBlock * kExactStride
  int list;    // per wave kBlock * kBlock uint16: kBlock * kBlock / 2 floats
  int end;
};
__host__ __device__ inline Layout layout(int D, int waves) {
  Layout L;
  L.stride = ((D + 1) & ~1) + 1;
  L.tiles = waves * kBlock * L.stride;
  L.ynorm = L.tiles + 2 * kBlock * L.stride;
  L.exact = L.ynorm + 2 * kBlock;
  L.list = L.exact + waves * kBlock * kExactStride;
  L.end = L.list + waves * kBlock * kBlock / 2;
  return L;
}
int waves_for(int D) { return (size_t)layout(D, 4).end * sizeof(float) <= kLdsBytes ? 4 : 2; }

// this wave's LDS writes before its next LDS reads: in-order in hardware, the fence is for the compiler
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// |y|^2 of every p2 row, one lane per row
__global__ __launch_bounds__(256) void knn_features_norms_kernel(const float* __restrict__ p2, int64_t rows, int D, float* __restrict__ out) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256) {
    float s = 0.0f;
    for (int c = 0; c < D; ++c) s = s + p2[r * D + c] * p2[r * D + c];
    out[r] = s;
  }
}

// Copies `count` consecutive floats of rows of D into LDS rows of `stride`: element e of lane tid, tid + threads, ... lies at
// (row, col), advanced without a division per element.
struct Cursor {
  int row, col, drow, dcol;
  __device__ __forceinline__ Cursor(int tid, int threads, int D) : row(tid / D), col(tid % D), drow(threads / D), dcol(threads % D) {}
  __device__ __forceinline__ void next(int D) {
    row += drow, col += dcol;
    if (col >= D) col -= D, ++row;
  }
};

// grid: N * blocks_per_cloud workgroups of 2 or 4 waves; K <= KQ; LDS: layout(D, waves)
// amdgpu_waves_per_eu(2): at most 256 registers, which also makes the compiler keep the accumulators in VGPRs (no AGPR copies)
template <int KQ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void knn_features_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                           const int64_t* __restrict__ lengths1, const int64_t* __restrict__ lengths2,
                                                           const float* __restrict__ ynorms, int64_t P1, int64_t P2, int D, int K,
                                                           int64_t blocks_per_cloud, float cD, int64_t* __restrict__ idx,
                                                           float* __restrict__ dists) {
  extern __shared__ __align__(16) float smem[];
  const int tid = threadIdx.x, threads = blockDim.x, waves = threads >> 6, wave = tid >> 6, lane = tid & 63;
  const int ql = lane & 31, hi = lane >> 5;
  const Layout L = layout(D, waves);
  const int stride = L.stride;
  float* const qrows = smem + wave * kBlock * stride;
  float* const exact = smem + L.exact + wave * kBlock * kExactStride;
  unsigned short* const list = reinterpret_cast<unsigned short*>(smem + L.list) + wave * kBlock * kBlock;

  const int64_t n = blockIdx.x / blocks_per_cloud, b = blockIdx.x % blocks_per_cloud;
  const int64_t row0 = b * (waves * kBlock);
  const int64_t len1 = knn::cloud_length(lengths1, n, P1), len2 = knn::cloud_length(lengths2, n, P2);
  const int64_t scan = row0 < len1 ? len2 : 0;  // workgroup-uniform: padding rows scan nothing

  if (scan > 0) {
    if (D & 1) {
      for (int r = tid; r < (waves + 2) * kBlock; r += threads) smem[r * stride + D] = 0.0f;
    }
    Cursor at(tid, threads, D);
    for (int e = tid; e < waves * kBlock * D; e += threads, at.next(D)) {
      const int64_t i = row0 + at.row;
      smem[at.row * stride + at.col] = i < len1 ? p1[(n * P1 + i) * D + at.col] : 0.0f;
    }
  }
  // tile it into buffer it & 1
  auto stage = [&](int64_t it) {
    const int64_t j0 = it * kBlock;
    const int tn = (int)(scan - j0 < kBlock ? scan - j0 : kBlock);
    float* const dst = smem + L.tiles + (int)(it & 1) * kBlock * stride;
    const float* const src = p2 + (n * P2 + j0) * D;
    Cursor to(tid, threads, D);
    for (int e = tid; e < tn * D; e += threads, to.next(D)) dst[to.row * stride + to.col] = src[e];
    if (tid < tn) smem[L.ynorm + (int)(it & 1) * kBlock + tid] = ynorms[n * P2 + j0 + tid];
  };
  const int64_t ntiles = (scan + kBlock - 1) / kBlock;
  if (ntiles > 0) stage(0);
  __syncthreads();

  const int64_t mine = row0 + wave * kBlock + ql;  // both lanes of a pair: the query of this lane's accumulators
  const bool live = mine < len1;
  const bool wave_live = row0 + wave * kBlock < len1;  // wave-uniform
  float nq = 0.0f;
  if (scan > 0 && wave_live) {
    for (int c = 0; c < D; ++c) nq = nq + qrows[ql * stride + c] * qrows[ql * stride + c];
  }
  Queue<KQ> best;
  best.init();
  const int steps = (D + 1) >> 1;

  for (int64_t it = 0; it < ntiles; ++it) {
    if (it + 1 < ntiles) stage(it + 1);
    if (wave_live) {
      const int64_t j0 = it * kBlock;
      const int tn = (int)(scan - j0 < kBlock ? scan - j0 : kBlock);
      const float* const tile = smem + L.tiles + (int)(it & 1) * kBlock * stride;
      const float* const yn = smem + L.ynorm + (int)(it & 1) * kBlock;
      // ---- screen: acc[r] = y[8 (r / 4) + 4 hi + r % 4] . q[ql]
      const float* const arow = tile + ql * stride + hi;
      const float* const brow = qrows + ql * stride + hi;
      floatx16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
      int k = 0;
      for (; k + 4 <= steps; k += 4) {  // a chunk of 8 coordinates: the eight LDS reads leave before the first instruction waits
        float a[4], bq[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = arow[2 * (k + u)], bq[u] = brow[2 * (k + u)];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], bq[u], acc, 0, 0, 0);
      }
      for (; k < steps; ++k) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[2 * k], brow[2 * k], acc, 0, 0, 0);
      const float worst = __shfl(best.d[KQ - 1], ql);  // the owner's, for both lanes of the pair
      int count = 0;        // wave-uniform: entries of the list
      unsigned mask = 0u;   // this lane's survivors by target
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int t = 8 * (r / 4) + 4 * hi + (r % 4);
        const float sum = nq + yn[t];
        const float s = sum - 2.0f * acc[r];
        const float E = cD * sum + kAbsolute;
        // dropped only on a finite screen value that is surely too large: NaN and infinities fall through to the exact path
        const bool drop = (s - E > worst) && (fabsf(s) < pos_inf());
        const bool keep = live && t < tn && !drop;
        const unsigned long long votes = __ballot(keep);
        if (keep) {
          list[count + mask_rank(votes)] = (unsigned short)(ql << 5 | t);
          mask |= 1u << t;
        }
        count += __popcll(votes);
      }
      mask |= (unsigned)__shfl_xor((int)mask, 32);
      wave_sync();
      // ---- rescore: the contract's arithmetic, one lane per survivor
      for (int e = lane; e < count; e += kWave) {
        const int q = list[e] >> 5, t = list[e] & 31;
        const float* const x = qrows + q * stride;
        const float* const y = tile + t * stride;
        float d = x[0] - y[0];
        float s = d * d;
        for (int c = 1; c < D; ++c) {
          d = x[c] - y[c];
          s = s + d * d;
        }
        exact[q * kExactStride + t] = s;
      }
      wave_sync();
      // ---- queues: lane q < 32 takes the survivors of query q in ascending target
      if (hi) mask = 0u;
      while (__ballot(mask != 0u) != 0ull) {
        const int t = mask ? __builtin_ctz(mask) : 0;
        const float dn = mask ? exact[ql * kExactStride + t] : __int_as_float(0x7fc00000);
        mask &= mask - 1u;
        const int jn = (int)j0 + t;
        if constexpr (KQ == 1) {
          const bool better = dn < best.d[0];
          best.d[0] = better ? dn : best.d[0];
          best.j[0] = better ? jn : best.j[0];
        } else {
          if (__ballot(best.wants(dn)) != 0ull) best.insert(dn, jn);
        }
      }
    }
    __syncthreads();  // everyone is done with tile it, and tile it + 1 is in place
  }

  const int found = (int)(len2 < K ? len2 : K);
  if (hi == 0 && mine < P1) {
    const int64_t row = (n * P1 + mine) * K;
#pragma unroll
    for (int k = 0; k < KQ; ++k) {
      if (k < K) {
        const bool slot = live && k < found;
        idx[row + k] = slot && best.j[k] >= 0 ? (int64_t)best.j[k] : 0;
        dists[row + k] = slot ? best.d[k] : 0.0f;
      }
    }
  }
}

// grad_p1: one lane per (row, coordinate), k ascending; every entry written
__global__ __launch_bounds__(256) void knn_features_bwd_gather_kernel(knn::Hits h, float* __restrict__ grad_p1) {
  const int64_t total = h.N * h.P1 * h.D;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
    const int64_t r = v / h.D;
    const int c = (int)(v % h.D);
    float acc = 0.0f;
    for (int k = 0; k < h.K; ++k) {
      const int64_t e = r * h.K + k, t = h.target(e);
      if (t >= 0) acc += h.term(e, t, c, h.upstream(e));
    }
    grad_p1[v] = acc;
  }
}

// grad_p2: lane = hit * D + coordinate, the D values of a hit leave from adjacent lanes
__global__ __launch_bounds__(256) void knn_features_bwd_scatter_kernel(knn::Hits h, float* __restrict__ grad_p2) {
  const int64_t total = h.N * h.P1 * h.K * h.D;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
    const int64_t e = v / h.D, t = h.target(e);
    const int c = (int)(v % h.D);
    if (t >= 0) atomicAdd(grad_p2 + t * h.D + c, -h.term(e, t, c, h.upstream(e)));
  }
}

// in place of hipMemsetAsync: a fill that a captured graph replays like any other kernel
__global__ __launch_bounds__(256) void knn_features_zero_kernel(float* __restrict__ out, int64_t count) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < count; v += (int64_t)gridDim.x * 256) out[v] = 0.0f;
}

// every index the kernels form fits an int64 comfortably, a hit's j an int32
bool sizes_ok(int64_t N, int64_t P1, int64_t P2, int D, int K) {
  if (N < 0 || P1 < 0 || P2 < 0 || P2 > INT32_MAX || P1 > INT32_MAX || D < 1 || K < 1) return false;
  const int64_t per_cloud = (P1 > P2 ? P1 : P2) * (int64_t)(K > D ? K : D) * 4;
  return N == 0 || per_cloud <= INT64_MAX / 64 / N;
}
bool supported(int D, int K) { return D >= P3D_KNN_FEATURES_MIN_D && D <= P3D_KNN_FEATURES_MAX_D && K <= P3D_KNN_MAX_K; }

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API size_t p3di_knn_features_forward_workspace_bytes(int64_t N, int64_t P2, int D) {
  (void)D;
  return N <= 0 || P2 <= 0 ? 0 : (size_t)N * (size_t)P2 * sizeof(float);
}

P3D_API int p3di_knn_features_forward(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2, int64_t N,
                                      int64_t P1, int64_t P2, int D, int K, int64_t* idx, float* dists, void* workspace,
                                      size_t workspace_bytes, p3d_stream_t stream) {
  if (!sizes_ok(N, P1, P2, D, K)) return P3D_ERR_INVALID_ARG;
  if (!supported(D, K)) return P3D_ERR_UNSUPPORTED;
  if (N * P1 == 0) return P3D_OK;
  if (!p1 || !idx || !dists || (P2 > 0 && !p2)) return P3D_ERR_INVALID_ARG;
  if (P2 > 0 && (!workspace || workspace_bytes < p3di_knn_features_forward_workspace_bytes(N, P2, D))) return P3D_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* ynorms = static_cast<float*>(workspace);
  if (P2 > 0) {
    LaunchScope ls("knn_features_norms", s);
    knn_features_norms_kernel<<<stream_blocks(N * P2), 256, 0, s>>>(p2, N * P2, D, ynorms);
    const int rc = launch_status();
    if (rc != P3D_OK) return rc;
  }
  const int waves = waves_for(D);
  const int64_t bpc = ceil_div(P1, waves * kBlock), blocks = N * bpc;
  if (blocks > 0x7fffffffll) return P3D_ERR_INVALID_ARG;
  const size_t lds = (size_t)layout(D, waves).end * sizeof(float);
  const float cD = screen_factor(D);
  LaunchScope ls("knn_features_forward", s);
  // the attribute belongs to the function on the current device: set on every launch, no global state in this library
#define P3D_KNN_FEATURES_LAUNCH(KQ)                                                                                                  \
  do {                                                                                                                               \
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_features_kernel<KQ>), hipFuncAttributeMaxDynamicSharedMemorySize,     \
                            (int)lds) != hipSuccess)                                                                                 \
      return P3D_ERR_LAUNCH;                                                                                                         \
    knn_features_kernel<KQ><<<(unsigned)blocks, waves * kWave, lds, s>>>(p1, p2, lengths1, lengths2, ynorms, P1, P2, D, K, bpc, cD,  \
                                                                        idx, dists);                                                 \
  } while (0)
  if (K == 1) P3D_KNN_FEATURES_LAUNCH(1);
  else if (K <= 2) P3D_KNN_FEATURES_LAUNCH(2);
  else if (K <= 4) P3D_KNN_FEATURES_LAUNCH(4);
  else if (K <= 8) P3D_KNN_FEATURES_LAUNCH(8);
  else if (K <= 16) P3D_KNN_FEATURES_LAUNCH(16);
  else if (K <= 20) P3D_KNN_FEATURES_LAUNCH(20);
  else P3D_KNN_FEATURES_LAUNCH(32);
#undef P3D_KNN_FEATURES_LAUNCH
  return launch_status();
}

P3D_API int p3di_knn_features_backward(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2,
                                       const int64_t* idx, const float* grad_dists, int64_t N, int64_t P1, int64_t P2, int D, int K,
                                       unsigned flags, float* grad_p1, float* grad_p2, p3d_stream_t stream) {
  if (!sizes_ok(N, P1, P2, D, K)) return P3D_ERR_INVALID_ARG;
  if (!supported(D, K)) return P3D_ERR_UNSUPPORTED;
  const int64_t hits = N * P1 * K;
  if (hits > 0 && P2 > 0 && (!p1 || !p2 || !idx)) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  knn::Hits h;
  h.p1 = p1, h.p2 = p2, h.lengths1 = lengths1, h.lengths2 = lengths2, h.idx = idx, h.grad_dists = grad_dists, h.cloud_scale = nullptr;
  h.N = N, h.P1 = P1, h.P2 = P2, h.D = D, h.K = K, h.norm = 2;
  if (grad_p1 && N * P1 > 0) {
    LaunchScope ls("knn_features_backward_gather", s);
    if (P2 == 0) knn_features_zero_kernel<<<stream_blocks(N * P1 * D), 256, 0, s>>>(grad_p1, N * P1 * D);
    else knn_features_bwd_gather_kernel<<<stream_blocks(N * P1 * D), 256, 0, s>>>(h, grad_p1);
    const int rc = launch_status();
    if (rc != P3D_OK) return rc;
  }
  if (grad_p2 && N * P2 > 0) {
    LaunchScope ls("knn_features_backward_scatter", s);
    if (!(flags & P3D_KNN_ACCUMULATE_P2)) knn_features_zero_kernel<<<stream_blocks(N * P2 * D), 256, 0, s>>>(grad_p2, N * P2 * D);
    if (hits > 0) knn_features_bwd_scatter_kernel<<<stream_blocks(hits * D), 256, 0, s>>>(h, grad_p2);
    return launch_status();
  }
  return P3D_OK;
}
