// points_alignment.hip -- iterative closest point and the alignment of corresponding points (Umeyama) between padded point clouds
// (pytorch3d/ops/points_alignment.py).  csrc/implicit_abi.h has the contract.
//
// One ICP iteration is six launches and nothing of it returns to the host but one int:
//   match    ONE LANE PER X POINT, 64 points of one cloud per workgroup, the scan of knn.hip for K = 1: the point is moved by the
//            cloud's current (R, T, s) in registers -- Xt = s * (sum_c x_c R[c][.]) + T, c ascending, every operation a float32
//            rounding of its own (-ffp-contract=off) --, Y is staged in LDS tiles of kTile points as structure of arrays and every
//            lane reads the same four points per ds_read_b128 (identical addresses broadcast).  A workgroup is S in {1, 2, 4, 8}
//            waves that hold the SAME 64 points and scan consecutive slices of Y, each into a tile of its own; the waves' winners
//            meet in LDS and wave 0 takes the least by the total order (dist, j).  Within a wave `<` over ascending j is that order,
//            so the result has the same bits for every S, and they are knn.hip's.  Every wave goes round the tile loop the same
//            number of times (a wave whose slice has ended stages nothing), so the workgroup barriers are uniform.
//            Wave 0 then gathers the neighbour and leaves the wave's sums of w, w y and (first iteration only) w x.
//   means    one workgroup per cloud: the fixed tree of fixed_sum.h over the wave partials -> Xmu, Ymu, sum w.
//   moments  one lane per X point: Xc = (x - Xmu) w, Yc = (y - Ymu) w, the nine products Xc Yc^T and Xc . Xc, summed per wave.
//            CENTRED, as the reference: a cloud far from the origin loses nothing to cancellation.
//   solve    one workgroup per cloud: the tree over the moment partials, the float32 quotients by the total weight, then ONE LANE
//            in float64: a one-sided Jacobi singular value decomposition of the 3 x 3 covariance, the reflection fix, scale and
//            translation, each result rounded to float32 once.
//   rmse     one lane per X point: the new transform, the old neighbour, w |Xt - y|^2 summed per wave; Xt is stored.
//   finish   one workgroup: per cloud the tree, the root, the relative decrease against the iteration before, and the AND over the
//            clouds into the int the host reads.
// No atomic.  Every sum is a wave_sum at level 1 and the strided-then-block tree of fixed_sum.h at level 2: the same bits on every
// run, stream and process.  corresponding_points_alignment is sums (match without the scan), means, moments, solve.
#include "fixed_sum.h"
#include "implicit_abi.h"
#include "knn_grad.h"
#include "knn_queue.h"
#include "vec3.h"

namespace p3d {
namespace {

constexpr int kTile = P3D_KNN_TILE;
static_assert(kTile % 4 == 0, "a tile is read four points at a time");
constexpr int kMaxSplit = P3D_ICP_MAX_SPLIT;
constexpr int kSums = 7;      // w, w y (3), w x (3)
constexpr int kMoments = 10;  // Xc Yc^T row-major (9), Xc . Xc
constexpr int kMu = 8;        // Xmu (3), Ymu (3), sum w, unused
constexpr float kRmseEps = 1e-9f;
constexpr double kAmbiguous = 1e-15;  // AMBIGUOUS_ROT_SINGULAR_THR

struct Rts {
  float r[9], t[3], s;
};

__device__ __forceinline__ Rts load_rts(const float* __restrict__ R, const float* __restrict__ T, const float* __restrict__ s, int64_t n) {
  Rts m;
#pragma unroll
  for (int k = 0; k < 9; ++k) m.r[k] = R[n * 9 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) m.t[k] = T[n * 3 + k];
  m.s = s[n];
  return m;
}

// s * (x R) + T: the row vector times R, c ascending
__device__ __forceinline__ V3 transform(const Rts& m, V3 x) {
  float o[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float acc = x.x * m.r[k];
    acc = acc + x.y * m.r[3 + k];
    acc = acc + x.z * m.r[6 + k];
    o[k] = m.s * acc + m.t[k];
  }
  return mk(o[0], o[1], o[2]);
}

// the weight of row i of cloud n: the length mask (NULL: ones) times the given weight (NULL: one)
__device__ __forceinline__ float row_weight(const int64_t* __restrict__ mask_len, const float* __restrict__ w, int64_t n, int64_t i,
                                            int64_t P1) {
  const float m = i < knn::cloud_length(mask_len, n, P1) ? 1.0f : 0.0f;
  return w ? m * w[n * P1 + i] : m;
}

// y of row i: its neighbour (zeros where the cloud of Y is empty, as knn_gather leaves them), or, without idx, row i of Y
__device__ __forceinline__ V3 partner(const float* __restrict__ Y, const int64_t* __restrict__ idx, const int64_t* __restrict__ lengths2,
                                      int64_t n, int64_t i, int64_t P1, int64_t P2) {
  if (!idx) return load3(Y + (n * P2 + i) * 3);
  if (knn::cloud_length(lengths2, n, P2) <= 0) return mk(0.0f, 0.0f, 0.0f);
  return load3(Y + (n * P2 + idx[n * P1 + i]) * 3);
}

// the wave's sums of w, w y and, where asked for, w x; a lane outside the rows holds wt = 0 and finite x, y
__device__ __forceinline__ void store_sums(float wt, V3 x, V3 y, bool want_x, float* __restrict__ out, int lane) {
  const float s0 = wave_sum(wt);
  const float y0 = wave_sum(wt * y.x), y1 = wave_sum(wt * y.y), y2 = wave_sum(wt * y.z);
  if (lane == 0) out[0] = s0, out[1] = y0, out[2] = y1, out[3] = y2;
  if (want_x) {  // uniform
    const float x0 = wave_sum(wt * x.x), x1 = wave_sum(wt * x.y), x2 = wave_sum(wt * x.z);
    if (lane == 0) out[4] = x0, out[5] = x1, out[6] = x2;
  }
}

// grid: N * blocks_per_cloud workgroups of S waves
template <int S>
__global__ __launch_bounds__(64 * S) void icp_match_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                           const int64_t* __restrict__ lengths1, const int64_t* __restrict__ lengths2,
                                                           const int64_t* __restrict__ mask_len, const float* __restrict__ w,
                                                           const float* __restrict__ R, const float* __restrict__ T,
                                                           const float* __restrict__ s, int64_t P1, int64_t P2, int64_t blocks_per_cloud,
                                                           int want_x, int64_t* __restrict__ idx, float* __restrict__ sums) {
  __shared__ __align__(16) float tile[S][3][kTile];
  __shared__ float win_d[S][kWave];
  __shared__ int win_j[S][kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = blockIdx.x / blocks_per_cloud, b = blockIdx.x % blocks_per_cloud;
  const int64_t i = b * kWave + lane;
  const int64_t len1 = knn::cloud_length(lengths1, n, P1), len2 = knn::cloud_length(lengths2, n, P2);
  const bool live = i < len1, row = i < P1;
  const V3 x = row ? load3(X + (n * P1 + i) * 3) : mk(0.0f, 0.0f, 0.0f);
  V3 q = x;
  if (R) q = transform(load_rts(R, T, s, n), x);
  if (!live) q = mk(0.0f, 0.0f, 0.0f);
  float best_d = pos_inf();
  int best_j = -1;
  const int64_t scan = b * kWave < len1 ? len2 : 0;  // uniform: a workgroup of padding rows scans nothing
  const int64_t per = (scan + S - 1) / S;
  const int64_t lo = wave * per < scan ? wave * per : scan, hi = lo + per < scan ? lo + per : scan;  // this wave's slice of Y
  for (int64_t r0 = 0; r0 < per; r0 += kTile) {  // the same rounds in every wave
    const int64_t j0 = lo + r0;
    const int tn = j0 < hi ? (int)(hi - j0 < kTile ? hi - j0 : kTile) : 0, tn4 = (tn + 3) & ~3;
    __syncthreads();  // the wave is done with the tile before
    const float* src = Y + (n * P2 + j0) * 3;
    for (int e = lane; e < tn * 3; e += kWave) tile[wave][e % 3][e / 3] = src[e];
    if (lane < tn4 - tn) {
#pragma unroll
      for (int c = 0; c < 3; ++c) tile[wave][c][tn + lane] = quiet_nan();  // a NaN distance fails every `<`
    }
    __syncthreads();
    for (int t = 0; t < tn4; t += 4) {
      float4 v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = *reinterpret_cast<const float4*>(&tile[wave][c][t]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float y[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) y[c] = u == 0 ? v[c].x : (u == 1 ? v[c].y : (u == 2 ? v[c].z : v[c].w));
        const float dx = q.x - y[0], dy = q.y - y[1], dz = q.z - y[2];
        const float dn = dx * dx + dy * dy + dz * dz;  // knn.hip's pair_dist<3, 2>
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
  const int64_t j = live && len2 > 0 && best_j >= 0 ? (int64_t)best_j : 0;  // knn.hip's index-0 rule
  if (row) idx[n * P1 + i] = j;
  const V3 y = row && len2 > 0 ? load3(Y + (n * P2 + j) * 3) : mk(0.0f, 0.0f, 0.0f);
  const float wt = row ? row_weight(mask_len, w, n, i, P1) : 0.0f;
  store_sums(wt, x, y, want_x != 0, sums + (int64_t)blockIdx.x * kSums, lane);
}

// corresponding points: the sums of match without the scan.  grid: N * blocks_per_cloud workgroups of one wave
__global__ __launch_bounds__(64) void pair_sums_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                       const int64_t* __restrict__ mask_len, const float* __restrict__ w, int64_t P1,
                                                       int64_t blocks_per_cloud, float* __restrict__ sums) {
  const int lane = threadIdx.x;
  const int64_t n = blockIdx.x / blocks_per_cloud, i = (blockIdx.x % blocks_per_cloud) * kWave + lane;
  const bool row = i < P1;
  const V3 x = row ? load3(X + (n * P1 + i) * 3) : mk(0.0f, 0.0f, 0.0f);
  const V3 y = row ? load3(Y + (n * P1 + i) * 3) : mk(0.0f, 0.0f, 0.0f);
  const float wt = row ? row_weight(mask_len, w, n, i, P1) : 0.0f;
  store_sums(wt, x, y, true, sums + (int64_t)blockIdx.x * kSums, lane);
}

// segment_sum_kernel's tree over entry q of a cloud's records of `stride` floats; every lane of the block calls it, thread 0 uses it
__device__ __forceinline__ float cloud_sum(const float* __restrict__ partials, int64_t per_cloud, int stride, int q) {
  float acc = 0.0f;
  for (int64_t k = threadIdx.x; k < per_cloud; k += 256) acc += partials[k * stride + q];
  const float s = block_sum_256(acc);
  __syncthreads();  // block_sum_256's four words are free again
  return s;
}

// grid: one workgroup of 256 per cloud.  uniform: no mask and no weights -- the reference's plain mean over P1 rows
__global__ __launch_bounds__(256) void means_kernel(const float* __restrict__ sums, int64_t per_cloud, int64_t P1, int uniform, int want_x,
                                                    float eps, float* __restrict__ mu) {
  const int64_t n = blockIdx.x;
  float v[kSums];
#pragma unroll
  for (int q = 0; q < kSums; ++q) v[q] = q < 4 || want_x ? cloud_sum(sums + n * per_cloud * kSums, per_cloud, kSums, q) : 0.0f;
  if (threadIdx.x != 0) return;
  float* m = mu + n * kMu;
  const float total = uniform ? (float)P1 : v[0];
  const float den = uniform ? total : fmaxf(total, eps);
  m[3] = v[1] / den, m[4] = v[2] / den, m[5] = v[3] / den, m[6] = total;
  if (want_x) m[0] = v[4] / den, m[1] = v[5] / den, m[2] = v[6] / den;
}

// grid: N * blocks_per_cloud workgroups of one wave
__global__ __launch_bounds__(64) void moments_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                     const int64_t* __restrict__ idx, const int64_t* __restrict__ lengths2,
                                                     const int64_t* __restrict__ mask_len, const float* __restrict__ w,
                                                     const float* __restrict__ mu, int weighted, int64_t P1, int64_t P2,
                                                     int64_t blocks_per_cloud, float* __restrict__ moments) {
  const int lane = threadIdx.x;
  const int64_t n = blockIdx.x / blocks_per_cloud, i = (blockIdx.x % blocks_per_cloud) * kWave + lane;
  float t[kMoments];
#pragma unroll
  for (int k = 0; k < kMoments; ++k) t[k] = 0.0f;
  if (i < P1) {
    const float* m = mu + n * kMu;
    V3 xc = load3(X + (n * P1 + i) * 3) - mk(m[0], m[1], m[2]);
    V3 yc = partner(Y, idx, lengths2, n, i, P1, P2) - mk(m[3], m[4], m[5]);
    if (weighted) {  // uniform: the reference multiplies only where it has weights
      const float wt = row_weight(mask_len, w, n, i, P1);
      xc = xc * wt, yc = yc * wt;  // the weight enters every product squared, as in the reference
    }
    t[0] = xc.x * yc.x, t[1] = xc.x * yc.y, t[2] = xc.x * yc.z;
    t[3] = xc.y * yc.x, t[4] = xc.y * yc.y, t[5] = xc.y * yc.z;
    t[6] = xc.z * yc.x, t[7] = xc.z * yc.y, t[8] = xc.z * yc.z;
    t[9] = (xc.x * xc.x + xc.y * xc.y) + xc.z * xc.z;
  }
#pragma unroll
  for (int k = 0; k < kMoments; ++k) {
    const float sum = wave_sum(t[k]);
    if (lane == 0) moments[(int64_t)blockIdx.x * kMoments + k] = sum;
  }
}

// ---- the 3 x 3 decomposition, one lane, float64 ------------------------------------------------------------------------------------
struct M3 {
  double c[3][3];  // c[j]: column j
};

__device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// one rotation of the one-sided Jacobi iteration: columns P and Q of g are made orthogonal, v follows
template <int P, int Q>
__device__ __forceinline__ bool jacobi_rotate(M3& g, M3& v) {
  const double alpha = dot3(g.c[P], g.c[P]), beta = dot3(g.c[Q], g.c[Q]), gamma = dot3(g.c[P], g.c[Q]);
  if (gamma == 0.0 || fabs(gamma) <= 1e-17 * sqrt(alpha * beta)) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double gp = g.c[P][k], gq = g.c[Q][k], vp = v.c[P][k], vq = v.c[Q][k];
    g.c[P][k] = cs * gp - sn * gq, g.c[Q][k] = sn * gp + cs * gq;
    v.c[P][k] = cs * vp - sn * vq, v.c[Q][k] = sn * vp + cs * vq;
  }
  return true;
}

template <int P, int Q>
__device__ __forceinline__ void order_columns(M3& g, M3& v, double (&sig)[3]) {
  if (sig[P] >= sig[Q]) return;
  const double h = sig[P];
  sig[P] = sig[Q], sig[Q] = h;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a = g.c[P][k], b = v.c[P][k];
    g.c[P][k] = g.c[Q][k], g.c[Q][k] = a;
    v.c[P][k] = v.c[Q][k], v.c[Q][k] = b;
  }
}

__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1], o[1] = a[2] * b[0] - a[0] * b[2], o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ double det3(const M3& m) {
  double x[3];
  cross3(m.c[1], m.c[2], x);
  return dot3(m.c[0], x);
}

// a (row-major) = U diag(sig) V^T with sig descending and U, V orthogonal (their COLUMNS in u.c[j], v.c[j]).  A column of U whose
// singular value is nothing against the largest is completed to an orthonormal basis: a zero matrix gives U = V = I.
__device__ void svd3(const double (&a)[9], M3& u, double (&sig)[3], M3& v) {
  M3 g;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
#pragma unroll
    for (int k = 0; k < 3; ++k) g.c[j][k] = a[k * 3 + j], v.c[j][k] = j == k ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < 30; ++sweep) {
    const bool r01 = jacobi_rotate<0, 1>(g, v), r02 = jacobi_rotate<0, 2>(g, v), r12 = jacobi_rotate<1, 2>(g, v);
    if (!(r01 || r02 || r12)) break;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) sig[j] = sqrt(dot3(g.c[j], g.c[j]));
  order_columns<0, 1>(g, v, sig), order_columns<1, 2>(g, v, sig), order_columns<0, 1>(g, v, sig);
  const double tiny = 1e-14 * sig[0];
  if (!(sig[0] > 0.0)) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
      for (int k = 0; k < 3; ++k) u.c[j][k] = j == k ? 1.0 : 0.0;
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) u.c[0][k] = g.c[0][k] / sig[0];
  if (sig[1] > tiny) {
#pragma unroll
    for (int k = 0; k < 3; ++k) u.c[1][k] = g.c[1][k] / sig[1];
  } else {  // rank one: any unit vector orthogonal to u0 -- from the axis u0 has least of
    const double a0 = fabs(u.c[0][0]), a1 = fabs(u.c[0][1]), a2 = fabs(u.c[0][2]);
    const int axis = a0 <= a1 && a0 <= a2 ? 0 : (a1 <= a2 ? 1 : 2);
    const double ua = axis == 0 ? u.c[0][0] : (axis == 1 ? u.c[0][1] : u.c[0][2]);
    double e[3], len2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = (k == axis ? 1.0 : 0.0) - ua * u.c[0][k], len2 += e[k] * e[k];
    const double len = sqrt(len2);
#pragma unroll
    for (int k = 0; k < 3; ++k) u.c[1][k] = e[k] / len;
  }
  if (sig[2] > tiny) {
#pragma unroll
    for (int k = 0; k < 3; ++k) u.c[2][k] = g.c[2][k] / sig[2];
  } else {
    cross3(u.c[0], u.c[1], u.c[2]);
  }
}

// grid: one workgroup of 256 per cloud
__global__ __launch_bounds__(256) void solve_kernel(const float* __restrict__ moments, int64_t per_cloud, const float* __restrict__ mu,
                                                    int uniform, unsigned flags, float eps, float* __restrict__ R, float* __restrict__ T,
                                                    float* __restrict__ s_out, int32_t* __restrict__ status) {
  const int64_t n = blockIdx.x;
  float m[kMoments];
#pragma unroll
  for (int q = 0; q < kMoments; ++q) m[q] = cloud_sum(moments + n * per_cloud * kMoments, per_cloud, kMoments, q);
  if (threadIdx.x != 0) return;
  const float* c = mu + n * kMu;
  const float total = uniform ? fmaxf(c[6], 1.0f) : fmaxf(c[6], eps);  // clamp(num_points, 1) or clamp(sum w, eps)
  double a[9], sig[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) a[k] = (double)(m[k] / total);  // the float32 covariance, as the reference decomposes it
  M3 u, v;
  svd3(a, u, sig, v);
  if (sig[0] <= kAmbiguous || sig[1] <= kAmbiguous || sig[2] <= kAmbiguous) status[1] = 1;
  const double e = (flags & P3D_ALIGN_ALLOW_REFLECTION) ? 1.0 : det3(u) * det3(v);  // det(U V^T)
  double r[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) r[i * 3 + j] = (u.c[0][i] * v.c[0][j] + u.c[1][i] * v.c[1][j]) + e * (u.c[2][i] * v.c[2][j]);
  }
  double scale = 1.0;
  if (flags & P3D_ALIGN_ESTIMATE_SCALE) scale = ((sig[0] + sig[1]) + e * sig[2]) / (double)fmaxf(m[9] / total, eps);
#pragma unroll
  for (int k = 0; k < 9; ++k) R[n * 9 + k] = (float)r[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double xr = ((double)c[0] * r[k] + (double)c[1] * r[3 + k]) + (double)c[2] * r[6 + k];
    T[n * 3 + k] = (float)((double)c[3 + k] - scale * xr);
  }
  s_out[n] = (float)scale;
}

// grid: N * blocks_per_cloud workgroups of one wave
__global__ __launch_bounds__(64) void rmse_kernel(const float* __restrict__ X, const float* __restrict__ Y, const int64_t* __restrict__ idx,
                                                  const int64_t* __restrict__ lengths2, const int64_t* __restrict__ mask_len,
                                                  const float* __restrict__ R, const float* __restrict__ T, const float* __restrict__ s,
                                                  int64_t P1, int64_t P2, int64_t blocks_per_cloud, float* __restrict__ Xt,
                                                  float* __restrict__ partials) {
  const int lane = threadIdx.x;
  const int64_t n = blockIdx.x / blocks_per_cloud, i = (blockIdx.x % blocks_per_cloud) * kWave + lane;
  float term = 0.0f;
  if (i < P1) {
    const V3 xt = transform(load_rts(R, T, s, n), load3(X + (n * P1 + i) * 3));
    store3(Xt + (n * P1 + i) * 3, xt);
    const V3 d = xt - partner(Y, idx, lengths2, n, i, P1, P2);
    term = ((d.x * d.x + d.y * d.y) + d.z * d.z) * row_weight(mask_len, nullptr, n, i, P1);
  }
  term = wave_sum(term);
  if (lane == 0) partials[blockIdx.x] = term;
}

// grid: ONE workgroup of 256.  prev == NULL: the first iteration, whose relative decrease is 1
__global__ __launch_bounds__(256) void finish_kernel(const float* __restrict__ partials, int64_t N, int64_t per_cloud,
                                                     const float* __restrict__ mu, const float* __restrict__ prev, float thr,
                                                     float* __restrict__ rmse, int32_t* __restrict__ status) {
  int all = 1;
  for (int64_t n = 0; n < N; ++n) {
    const float sum = cloud_sum(partials + n * per_cloud, per_cloud, 1, 0);
    if (threadIdx.x == 0) {
      const float e = sqrtf(sum / fmaxf(mu[n * kMu + 6], kRmseEps));
      rmse[n] = e;
      const float relative = prev ? (prev[n] - e) / prev[n] : 1.0f;  // 0 / 0: NaN, never converged -- as the reference
      all &= relative <= thr ? 1 : 0;
    }
  }
  if (threadIdx.x == 0) status[0] = all;
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

// the waves of a workgroup: doubled while the launch leaves SIMDs idle and every wave still has a tile of its own to scan
int auto_split(int64_t blocks, int64_t P2) {
  const int64_t simds = 4ll * cu_count(), tiles = ceil_div(P2, kTile);
  int S = 1;
  while (S < kMaxSplit && blocks * (2 * S) <= simds && 2 * S <= tiles) S *= 2;
  return S;
}

struct Sizes {
  int64_t bpc, blocks;
};

// every index within an int64 with room, a neighbour's j within an int32, the grid within 2^31
bool sizes_ok(int64_t N, int64_t P1, int64_t P2, Sizes* out) {
  if (N < 0 || P1 < 0 || P2 < 0 || P1 > INT32_MAX || P2 > INT32_MAX || N > INT32_MAX) return false;
  out->bpc = ceil_div(P1, kWave);
  if (N > 0 && out->bpc > 0x7fffffffll / N) return false;
  out->blocks = N * out->bpc;
  return true;
}

struct Workspace {
  float *sums, *mu, *moments, *rm;
  bool ok;
  Workspace(void* p, size_t bytes, int64_t N, int64_t bpc) {
    Arena a(p, bytes);
    sums = a.take<float>((size_t)(N * bpc) * kSums), mu = a.take<float>((size_t)N * kMu);
    moments = a.take<float>((size_t)(N * bpc) * kMoments), rm = a.take<float>((size_t)(N * bpc));
    ok = p != nullptr && a.ok();
  }
};

int launch_match(const float* X, const float* Y, const int64_t* l1, const int64_t* l2, const int64_t* mask_len, const float* w,
                 const float* R, const float* T, const float* s, int64_t P1, int64_t P2, Sizes z, int split, int want_x, int64_t* idx,
                 float* sums, hipStream_t st) {
  const int S = split ? split : auto_split(z.blocks, P2);
  const unsigned g = (unsigned)z.blocks;
#define P3D_ICP_MATCH(SPLIT) \
  icp_match_kernel<SPLIT><<<g, 64 * SPLIT, 0, st>>>(X, Y, l1, l2, mask_len, w, R, T, s, P1, P2, z.bpc, want_x, idx, sums)
  if (S == 1) P3D_ICP_MATCH(1);
  else if (S == 2) P3D_ICP_MATCH(2);
  else if (S == 4) P3D_ICP_MATCH(4);
  else P3D_ICP_MATCH(8);
#undef P3D_ICP_MATCH
  return launch_status();
}

bool split_ok(int split) { return split == 0 || split == 1 || split == 2 || split == 4 || split == 8; }

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API size_t p3di_icp_workspace_bytes(int64_t N, int64_t P1) {
  Sizes z;
  if (!sizes_ok(N, P1, 0, &z) || z.blocks == 0) return 0;
  Arena a(nullptr, 0);  // Workspace's layout
  a.take<float>((size_t)z.blocks * kSums), a.take<float>((size_t)N * kMu), a.take<float>((size_t)z.blocks * kMoments);
  a.take<float>((size_t)z.blocks);
  return a.off;
}

P3D_API int p3di_icp_match(const float* X, const float* Y, const int64_t* lengths1, const int64_t* lengths2, const float* R, const float* T,
                           const float* s, int64_t N, int64_t P1, int64_t P2, int split, int64_t* idx, void* workspace,
                           size_t workspace_bytes, p3d_stream_t stream) {
  Sizes z;
  if (!sizes_ok(N, P1, P2, &z) || !split_ok(split)) return P3D_ERR_INVALID_ARG;
  if (z.blocks == 0) return P3D_OK;
  if (!X || !idx || (P2 > 0 && !Y) || ((R != nullptr) != (T != nullptr)) || ((R != nullptr) != (s != nullptr))) return P3D_ERR_INVALID_ARG;
  Workspace ws(workspace, workspace_bytes, N, z.bpc);
  if (!ws.ok) return P3D_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  LaunchScope ls("icp_match", st);
  return launch_match(X, Y, lengths1, lengths2, nullptr, nullptr, R, T, s, P1, P2, z, split, 1, idx, ws.sums, st);
}

P3D_API int p3di_icp_iteration(const float* X, const float* Y, const int64_t* lengths1, const int64_t* lengths2, const int64_t* mask_len,
                               const float* R_in, const float* T_in, const float* s_in, const float* rmse_prev, int64_t N, int64_t P1,
                               int64_t P2, int split, unsigned flags, float relative_rmse_thr, float* R_out, float* T_out, float* s_out,
                               int64_t* idx, float* Xt, float* rmse, int32_t* status, void* workspace, size_t workspace_bytes,
                               p3d_stream_t stream) {
  Sizes z;
  if (!sizes_ok(N, P1, P2, &z) || !split_ok(split) || (flags & ~(P3D_ALIGN_ESTIMATE_SCALE | P3D_ALIGN_ALLOW_REFLECTION)))
    return P3D_ERR_INVALID_ARG;
  if (z.blocks == 0) return P3D_ERR_INVALID_ARG;  // an empty batch has no iteration: the caller answers it
  if (!X || (P2 > 0 && !Y) || !R_out || !T_out || !s_out || !idx || !Xt || !rmse || !status) return P3D_ERR_INVALID_ARG;
  if (((R_in != nullptr) != (T_in != nullptr)) || ((R_in != nullptr) != (s_in != nullptr))) return P3D_ERR_INVALID_ARG;
  Workspace ws(workspace, workspace_bytes, N, z.bpc);
  if (!ws.ok) return P3D_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int first = rmse_prev == nullptr;
  const unsigned g = (unsigned)z.blocks, clouds = (unsigned)N;
  const float eps = 1e-9f;  // corresponding_points_alignment's default, which the reference's loop never changes
  int rc;
  {
    LaunchScope ls("icp_match", st);
    rc = launch_match(X, Y, lengths1, lengths2, mask_len, nullptr, R_in, T_in, s_in, P1, P2, z, split, first, idx, ws.sums, st);
    if (rc != P3D_OK) return rc;
  }
  {
    LaunchScope ls("icp_means", st);
    means_kernel<<<clouds, 256, 0, st>>>(ws.sums, z.bpc, P1, mask_len == nullptr, first, eps, ws.mu);
    if ((rc = launch_status()) != P3D_OK) return rc;
  }
  {
    LaunchScope ls("icp_moments", st);
    moments_kernel<<<g, 64, 0, st>>>(X, Y, idx, lengths2, mask_len, nullptr, ws.mu, mask_len != nullptr, P1, P2, z.bpc, ws.moments);
    if ((rc = launch_status()) != P3D_OK) return rc;
  }
  {
    LaunchScope ls("icp_solve", st);
    // the loop always passes a mask as weights: clamp(sum w, eps), never clamp(num_points, 1) -- the same number for P1 >= 1
    solve_kernel<<<clouds, 256, 0, st>>>(ws.moments, z.bpc, ws.mu, 0, flags, eps, R_out, T_out, s_out, status);
    if ((rc = launch_status()) != P3D_OK) return rc;
  }
  {
    LaunchScope ls("icp_rmse", st);
    rmse_kernel<<<g, 64, 0, st>>>(X, Y, idx, lengths2, mask_len, R_out, T_out, s_out, P1, P2, z.bpc, Xt, ws.rm);
    if ((rc = launch_status()) != P3D_OK) return rc;
  }
  LaunchScope ls("icp_finish", st);
  finish_kernel<<<1, 256, 0, st>>>(ws.rm, N, z.bpc, ws.mu, rmse_prev, relative_rmse_thr, rmse, status);
  return launch_status();
}

P3D_API int p3di_points_alignment(const float* X, const float* Y, const int64_t* mask_len, const float* weights, int64_t N, int64_t P,
                                  unsigned flags, float eps, float* R, float* T, float* s, int32_t* status, void* workspace,
                                  size_t workspace_bytes, p3d_stream_t stream) {
  Sizes z;
  if (!sizes_ok(N, P, P, &z) || (flags & ~(P3D_ALIGN_ESTIMATE_SCALE | P3D_ALIGN_ALLOW_REFLECTION)) || z.blocks == 0)
    return P3D_ERR_INVALID_ARG;
  if (!X || !Y || !R || !T || !s || !status) return P3D_ERR_INVALID_ARG;
  Workspace ws(workspace, workspace_bytes, N, z.bpc);
  if (!ws.ok) return P3D_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const unsigned g = (unsigned)z.blocks, clouds = (unsigned)N;
  const int uniform = mask_len == nullptr && weights == nullptr;
  int rc;
  {
    LaunchScope ls("align_sums", st);
    pair_sums_kernel<<<g, 64, 0, st>>>(X, Y, mask_len, weights, P, z.bpc, ws.sums);
    if ((rc = launch_status()) != P3D_OK) return rc;
  }
  {
    LaunchScope ls("icp_means", st);
    means_kernel<<<clouds, 256, 0, st>>>(ws.sums, z.bpc, P, uniform, 1, eps, ws.mu);
    if ((rc = launch_status()) != P3D_OK) return rc;
  }
  {
    LaunchScope ls("icp_moments", st);
    moments_kernel<<<g, 64, 0, st>>>(X, Y, nullptr, nullptr, mask_len, weights, ws.mu, !uniform, P, P, z.bpc, ws.moments);
    if ((rc = launch_status()) != P3D_OK) return rc;
  }
  LaunchScope ls("icp_solve", st);
  solve_kernel<<<clouds, 256, 0, st>>>(ws.moments, z.bpc, ws.mu, uniform, flags, eps, R, T, s, status);
  return launch_status();
}
