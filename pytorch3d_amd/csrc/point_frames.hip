// point_frames.hip -- per-point covariances, curvatures and local coordinate frames of padded point clouds in one launch
// (pytorch3d/ops/points_normals.py over ops/utils.py get_point_covariances and common/workaround/symeig3x3.py).  include/p3d_amd.h
// has the contract.
//
// ONE LANE PER QUERY POINT, one wave (64 queries of one cloud) per workgroup, the scan of knn.hip: the cloud is staged in LDS tiles
// of kTile points as structure of arrays, every lane reads the same four points per ds_read_b128, and the K smallest (dist, j) pairs
// of a lane live in the register queue of knn_queue.h, KQ in {2, 4, 8, 16, 32, 64}.  A squared distance is pair_dist's: per
// coordinate the difference and its square, accumulated in coordinate order, NOT fused (-ffp-contract=off).
// After the scan the queue's indices go to LDS (the tile's bytes, k-major: lane-consecutive addresses), the queue's registers are
// dead, and the rest runs in rolled loops over k ascending, each neighbour gathered from global memory (L2):
//   the neighbourhood mean, then the mean of the centred outer products: float32, sequential in k;
//   the eigenvalues and eigenvectors by the reference's regularised closed form (sym3_eig below), operation for operation;
//   with P3D_FRAMES_DISAMBIGUATE the sign votes of column 0 and column 2 over the same neighbours, and column 1 = n x z.
// Nothing of size K per point leaves the chip unless idx_out is asked for.  No atomics, nothing between workgroups: the same bits on
// every run and stream.
#include "knn_grad.h"
#include "knn_queue.h"
#include "vec3.h"

namespace p3d {
namespace {

constexpr int kTile = P3D_KNN_TILE;
static_assert(kTile % 4 == 0, "a tile is read four points at a time");
constexpr float kEps = 1.1920928955078125e-07f;           // torch.finfo(torch.float32).eps
constexpr float kSixEps = 7.152557373046875e-07f;         // 6 * eps: the width of the blend towards the sorted diagonal
constexpr float kTwoPiThirds = 2.0943951023931953f;       // 2 * pi / 3
constexpr float kNormalizeEps = 1e-12f;                   // torch.nn.functional.normalize

// a symmetric 3 x 3 matrix: the upper triangle
struct Sym3 {
  float a00, a01, a02, a11, a12, a22;
};

__device__ __forceinline__ float sign_nz(float x) { return x > 0.0f ? 1.0f : -1.0f; }  // _sign_without_zero
__device__ __forceinline__ float sq3(V3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
__device__ __forceinline__ Sym3 minus_diag(Sym3 a, float s) { return Sym3{a.a00 - s, a.a01, a.a02, a.a11 - s, a.a12, a.a22 - s}; }

// _get_ev0: the cross product of two rows with the largest squared norm, all three regularised by +-eps in the sign of the FIRST
__device__ __forceinline__ V3 first_eigenvector(Sym3 c) {
  const V3 r0 = mk(c.a00, c.a01, c.a02), r1 = mk(c.a01, c.a11, c.a12), r2 = mk(c.a02, c.a12, c.a22);
  V3 r01 = cross(r0, r1), r12 = cross(r1, r2), r02 = cross(r0, r2);
  const V3 reg = mk(kEps * sign_nz(r01.x), kEps * sign_nz(r01.y), kEps * sign_nz(r01.z));
  r01 = r01 + reg, r12 = r12 + reg, r02 = r02 + reg;
  const float n01 = sq3(r01), n12 = sq3(r12), n02 = sq3(r02);
  V3 best = r01;
  float nb = n01;
  if (n12 > nb) best = r12, nb = n12;  // argmax: the first of equal norms
  if (n02 > nb) best = r02, nb = n02;
  return best / sqrtf(nb);
}

// _get_uv: {u, v, w} right-handed and orthonormal; u is w turned by pi / 2 about the axis of its smallest component
__device__ __forceinline__ void complete_basis(V3 w, V3& u, V3& v) {
  const float ax = fabsf(w.x), ay = fabsf(w.y), az = fabsf(w.z);
  int axis = 0;
  float am = ax;
  if (ay < am) axis = 1, am = ay;  // argmin: the first of equal components
  if (az < am) axis = 2;
  const V3 t = axis == 0 ? mk(0.0f, -w.z, w.y) : (axis == 1 ? mk(-w.z, 0.0f, w.x) : mk(-w.y, w.x, 0.0f));
  u = t / fmaxf(sqrtf(sq3(t)), kNormalizeEps);
  v = cross(w, u);
}

// _get_ev1: the eigenvector of the second eigenvalue inside span{u, v}
__device__ __forceinline__ V3 second_eigenvector(Sym3 c, V3 u, V3 v) {
  const V3 c0 = mk(c.a00, c.a01, c.a02), c1 = mk(c.a01, c.a11, c.a12), c2 = mk(c.a02, c.a12, c.a22);  // columns = rows
  const V3 tu = mk(dot(u, c0), dot(u, c1), dot(u, c2)), tv = mk(dot(v, c0), dot(v, c1), dot(v, c2));     // [u v]^T C
  const float m00 = dot(tu, u), m01 = dot(tu, v), m10 = dot(tv, u), m11 = dot(tv, v);
  const float acute = sign_nz(m00 * m10 + m01 * m11);
  float rs0 = m00 + acute * m10, rs1 = m01 + acute * m11;
  const float reg = kEps * sign_nz(rs0);
  rs0 = rs0 + reg, rs1 = rs1 + reg;
  const float t0 = rs1, t1 = -rs0;  // rowspace @ [[0, -1], [1, 0]]
  const float nrm = fmaxf(sqrtf(t0 * t0 + t1 * t1), kNormalizeEps);
  return u * (t0 / nrm) + v * (t1 / nrm);
}

// symeig3x3(inputs, eigenvectors=True): val ascending, vec[c] the eigenvector of val[c].  NOT a true eigen-decomposition: p1 is
// clamped at eps, r at +-(1 - eps), and the eigenvalues are blended towards the sorted diagonal by exp(-(p1 / (6 eps))^2).
__device__ __forceinline__ void sym3_eig(Sym3 a, float (&val)[3], V3 (&vec)[3]) {
  const float q = ((a.a00 + a.a11) + a.a22) / 3.0f;
  // the reference's (sum of all squares - sum of the diagonal's) / 2 without its cancellation: the same number, and that
  // difference was the largest single source of float32 error in the curvatures
  const float p1 = a.a01 * a.a01 + a.a02 * a.a02 + a.a12 * a.a12;
  const float d0 = a.a00 - q, d1 = a.a11 - q, d2 = a.a22 - q;
  const float p2 = (d0 * d0 + d1 * d1 + d2 * d2) + 2.0f * fmaxf(p1, kEps);
  const float p = sqrtf(p2 / 6.0f);
  const float b00 = d0 / p, b11 = d1 / p, b22 = d2 / p, b01 = a.a01 / p, b02 = a.a02 / p, b12 = a.a12 / p;
  const float det = b00 * (b11 * b22 - b12 * b12) - b01 * (b01 * b22 - b12 * b02) + b02 * (b01 * b12 - b11 * b02);
  const float r = fminf(fmaxf(det / 2.0f, -1.0f + kEps), 1.0f - kEps);
  const float phi = acosf(r) / 3.0f;
  const float eig1 = q + (2.0f * p) * cosf(phi);
  const float eig2 = q + (2.0f * p) * cosf(phi + kTwoPiThirds);
  const float eig3 = 3.0f * q - eig1 - eig2;
  const float t = p1 / kSixEps;
  const float blend = expf(-(t * t));
  // the diagonal, ascending
  float s0 = a.a00, s1 = a.a11, s2 = a.a22, h;
  if (s1 < s0) h = s0, s0 = s1, s1 = h;
  if (s2 < s1) h = s1, s1 = s2, s2 = h;
  if (s1 < s0) h = s0, s0 = s1, s1 = h;
  val[0] = blend * s0 + (1.0f - blend) * eig2;
  val[1] = blend * s1 + (1.0f - blend) * eig3;
  val[2] = blend * s2 + (1.0f - blend) * eig1;
  // the set built from the better separated end: (val0, val1) or (val2, val1); the other set is never looked at
  const bool low = val[1] - val[0] > val[2] - val[1];
  const V3 e0 = first_eigenvector(minus_diag(a, low ? val[0] : val[2]));
  V3 u, v;
  complete_basis(e0, u, v);
  const V3 e1 = second_eigenvector(minus_diag(a, val[1]), u, v);
  const V3 e2 = cross(e0, e1);
  vec[0] = low ? e0 : e2, vec[1] = e1, vec[2] = low ? e2 : e0;
}

// grid: N * blocks_per_cloud workgroups of one wave.  K <= KQ.
template <int KQ>
__global__ __launch_bounds__(64) void point_frames_kernel(const float* __restrict__ pts, const int64_t* __restrict__ lengths, int64_t P,
                                                          int K, int64_t blocks_per_cloud, unsigned flags, float* __restrict__ curv,
                                                          float* __restrict__ frames, float* __restrict__ cov_out,
                                                          int64_t* __restrict__ idx_out) {
  __shared__ __align__(16) union {
    float tile[3][kTile];  // the scan: a tile of the cloud
    int nbr[KQ][kWave];    // after it: the lanes' neighbour lists, k-major
  } sh;
  const int lane = threadIdx.x;
  const int64_t n = blockIdx.x / blocks_per_cloud, b = blockIdx.x % blocks_per_cloud;
  const int64_t i = b * kWave + lane;
  const int64_t len = knn::cloud_length(lengths, n, P);
  const bool live = i < len;
  const float* cloud = pts + n * P * 3;
  float q[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) q[c] = live ? cloud[i * 3 + c] : 0.0f;
  Queue<KQ> best;
  best.init();
  const int64_t scan = b * kWave < len ? len : 0;  // wave-uniform: a wave of padding rows scans nothing
  for (int64_t j0 = 0; j0 < scan; j0 += kTile) {
    const int tn = (int)(scan - j0 < kTile ? scan - j0 : kTile), tn4 = (tn + 3) & ~3;
    __syncthreads();  // the wave is done with the tile before
    const float* src = cloud + j0 * 3;
    for (int e = lane; e < tn * 3; e += kWave) sh.tile[e % 3][e / 3] = src[e];
    if (lane < tn4 - tn) {
#pragma unroll
      for (int c = 0; c < 3; ++c) sh.tile[c][tn + lane] = quiet_nan();  // a NaN distance fails every `<`
    }
    __syncthreads();
    for (int t = 0; t < tn4; t += 4) {
      float4 v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = *reinterpret_cast<const float4*>(&sh.tile[c][t]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float y[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) y[c] = u == 0 ? v[c].x : (u == 1 ? v[c].y : (u == 2 ? v[c].z : v[c].w));
        const float dx = q[0] - y[0], dy = q[1] - y[1], dz = q[2] - y[2];
        const float dn = dx * dx + dy * dy + dz * dz;
        if (__ballot(best.wants(dn)) != 0ull) best.insert(dn, (int)j0 + t + u);
      }
    }
  }
  __syncthreads();  // the last tile is done: its bytes become the neighbour lists
#pragma unroll
  for (int k = 0; k < KQ; ++k) sh.nbr[k][lane] = best.j[k] < 0 ? (int)(live ? i : 0) : best.j[k];  // a lane reads back its own column
  // (a slot below kn is empty only where NaN coordinates kept candidates out -- outside the contract; it then names the row itself,
  // so that no gather leaves the cloud)
  if (i >= P) return;
  const int64_t row = n * P + i;
  const int kn = live ? (int)(len < K ? len : K) : 0;  // a cloud shorter than K: all of it
  if (idx_out) {
    for (int k = 0; k < K; ++k) idx_out[row * K + k] = k < kn ? (int64_t)sh.nbr[k][lane] : 0;
  }
  // get_point_covariances: the mean of the neighbours, then the mean of the centred outer products
  V3 sum = mk(0.0f, 0.0f, 0.0f);
  for (int k = 0; k < kn; ++k) sum = sum + load3(cloud + (int64_t)sh.nbr[k][lane] * 3);
  const float count = (float)kn;
  const V3 mean = sum / count;
  Sym3 c = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int k = 0; k < kn; ++k) {
    const V3 d = load3(cloud + (int64_t)sh.nbr[k][lane] * 3) - mean;
    c.a00 = c.a00 + d.x * d.x, c.a01 = c.a01 + d.x * d.y, c.a02 = c.a02 + d.x * d.z;
    c.a11 = c.a11 + d.y * d.y, c.a12 = c.a12 + d.y * d.z, c.a22 = c.a22 + d.z * d.z;
  }
  if (live) c = Sym3{c.a00 / count, c.a01 / count, c.a02 / count, c.a11 / count, c.a12 / count, c.a22 / count};
  if (cov_out) {
    float* o = cov_out + row * 9;
    o[0] = c.a00, o[1] = c.a01, o[2] = c.a02, o[3] = c.a01, o[4] = c.a11, o[5] = c.a12, o[6] = c.a02, o[7] = c.a12, o[8] = c.a22;
  }
  if (!frames) return;  // (curv and frames come together)
  float val[3] = {0.0f, 0.0f, 0.0f};
  V3 vec[3] = {mk(0.0f, 0.0f, 0.0f), mk(0.0f, 0.0f, 0.0f), mk(0.0f, 0.0f, 0.0f)};
  if (live) {
    sym3_eig(c, val, vec);
    if (flags & P3D_FRAMES_DISAMBIGUATE) {
      // _disambiguate_vector_directions for the normal and the main curvature: a vector that fewer than half of the neighbours
      // lie in front of is turned round
      const V3 x = mk(q[0], q[1], q[2]);
      int front_n = 0, front_z = 0;
      for (int k = 0; k < kn; ++k) {
        const V3 d = load3(cloud + (int64_t)sh.nbr[k][lane] * 3) - x;
        front_n += vec[0].x * d.x + vec[0].y * d.y + vec[0].z * d.z > 0.0f ? 1 : 0;
        front_z += vec[2].x * d.x + vec[2].y * d.y + vec[2].z * d.z > 0.0f ? 1 : 0;
      }
      const float half = 0.5f * count;
      if ((float)front_n < half) vec[0] = -vec[0];
      if ((float)front_z < half) vec[2] = -vec[2];
      vec[1] = cross(vec[0], vec[2]);
    }
  }
  store3(curv + row * 3, mk(val[0], val[1], val[2]));
  float* f = frames + row * 9;  // the vectors are the COLUMNS
  f[0] = vec[0].x, f[1] = vec[1].x, f[2] = vec[2].x;
  f[3] = vec[0].y, f[4] = vec[1].y, f[5] = vec[2].y;
  f[6] = vec[0].z, f[7] = vec[1].z, f[8] = vec[2].z;
}

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API int64_t p3d_point_frames_workgroups(int64_t N, int64_t P) {
  if (N <= 0 || P <= 0) return 0;
  const int64_t bpc = ceil_div(P, (int64_t)P3D_FRAMES_ROWS_PER_GROUP);
  return bpc > 0x7fffffffll / N ? -1 : N * bpc;
}

P3D_API int p3d_point_frames(const float* points, const int64_t* lengths, int64_t N, int64_t P, int D, int K, unsigned flags,
                             float* curvatures, float* frames, float* cov_out, int64_t* idx_out, p3d_stream_t stream) {
  if (N < 0 || P < 0 || P > INT32_MAX || (flags & ~P3D_FRAMES_DISAMBIGUATE)) return P3D_ERR_INVALID_ARG;
  if (D != 3 || K < 1 || K > P3D_FRAMES_MAX_K) return P3D_ERR_UNSUPPORTED;
  if ((curvatures == nullptr) != (frames == nullptr)) return P3D_ERR_INVALID_ARG;
  if (N * P == 0) return P3D_OK;
  if (!points || (!frames && !cov_out && !idx_out)) return P3D_ERR_INVALID_ARG;
  static_assert(P3D_FRAMES_ROWS_PER_GROUP == kWave, "one wave of queries per workgroup");
  const int64_t bpc = ceil_div(P, kWave), groups = p3d_point_frames_workgroups(N, P);
  if (groups < 0) return P3D_ERR_INVALID_ARG;
  const unsigned g = (unsigned)groups;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("point_frames", s);
#define P3D_FRAMES_LAUNCH(KQ) \
  point_frames_kernel<KQ><<<g, 64, 0, s>>>(points, lengths, P, K, bpc, flags, curvatures, frames, cov_out, idx_out)
  if (K <= 2) P3D_FRAMES_LAUNCH(2);
  else if (K <= 4) P3D_FRAMES_LAUNCH(4);
  else if (K <= 8) P3D_FRAMES_LAUNCH(8);
  else if (K <= 16) P3D_FRAMES_LAUNCH(16);
  else if (K <= 32) P3D_FRAMES_LAUNCH(32);
  else P3D_FRAMES_LAUNCH(64);
#undef P3D_FRAMES_LAUNCH
  return launch_status();
}
