// ordered_bwd.hip -- the deterministic backwards (torch.use_deterministic_algorithms(True)): the scatters of the mesh and point
// rasterizers, the face-vertex gather, the compositors and interpolate_face_attributes as ordered segmented sums
// (ordered_sum.h) instead of float atomics.  The caller hands over the samples that hold a primitive, sorted by primitive
// (stable), and a workspace; every gradient is then a pure function of the inputs, bit for bit.  DESIGN.md section 8.8.
#include "knn_grad.h"
#include "ordered_sum.h"
#include "p3d_geom.h"
#include "point_mesh_geom.h"

namespace p3d {
namespace {

using ordered::partial_bytes;

constexpr float kEpsAlpha = 1e-9f;  // alpha_composite.cu:20
constexpr float kEpsNorm = 1e-4f;   // norm_weighted_sum.cu:20

// ---- meshes: the nine partials of a (pixel, k) sample, by the device function of the atomic kernels ---------------------------
struct MeshOp {
  static constexpr int R = 9;
  int64_t nsamples, nkeys;
  const float* face_verts;
  const int64_t* p2f;
  const float *gz, *gb, *gd;
  int H, W, K, persp, clip;
  float* out;  // (F, 9)
  __device__ int64_t key(int64_t s) const { return p2f[s]; }
  __device__ void row(int64_t s, int f, int, float (&r)[R]) const {
    const int64_t pix = s / K;
    const int x = (int)(pix % W), y = (int)((pix / W) % H);
    const f2 p = mk2(pix_to_ndc(W - 1 - x, W, H), pix_to_ndc(H - 1 - y, H, W));  // rasterize_meshes.cu:458-462
    const float* g = face_verts + (int64_t)f * 9;
    const FaceGrad fg = face_sample_bwd(mk3(g[0], g[1], g[2]), mk3(g[3], g[4], g[5]), mk3(g[6], g[7], g[8]), p, gz[s],
                                        mk3(gb[s * 3], gb[s * 3 + 1], gb[s * 3 + 2]), gd[s], persp != 0, clip != 0, false);
#pragma unroll
    for (int i = 0; i < R; ++i) r[i] = fg.g[i];
  }
  __device__ void store(int f, int, const float (&r)[R]) const {
#pragma unroll
    for (int i = 0; i < R; ++i) out[(int64_t)f * 9 + i] = r[i];
  }
};

// ---- verts[faces]'s backward: corner c of the (F, 3) faces adds row c of grad_face_verts to its vertex -------------------------
struct CornerOp {
  static constexpr int R = 3;
  int64_t nsamples, nkeys;  // 3 F corners, V vertices
  const float* src;         // (3 F, 3)
  const int64_t* faces;
  float* out;               // (V, 3)
  __device__ int64_t key(int64_t c) const {
    const int64_t v = faces[c];
    return v < 0 ? v + nkeys : v;  // torch indexing: a negative id wraps once (gather.hip)
  }
  __device__ void row(int64_t c, int, int, float (&r)[R]) const {
    r[0] = src[c * 3], r[1] = src[c * 3 + 1], r[2] = src[c * 3 + 2];
  }
  __device__ void store(int v, int, const float (&r)[R]) const {
    out[(int64_t)v * 3] = r[0], out[(int64_t)v * 3 + 1] = r[1], out[(int64_t)v * 3 + 2] = r[2];
  }
};

// ---- nearest neighbours: hit e of idx (N, P1, K) adds minus its row of knn_grad.h to p2 point n * P2 + idx[e] ----------------------
struct KnnOp {
  static constexpr int R = 3;  // D is 2 or 3; a row's third float stays 0 for D = 2
  int64_t nsamples, nkeys;     // N P1 K hits, N P2 points
  knn::Hits h;
  int accumulate;              // add to what out holds (every key is stored once, so the order of the sum stays fixed)
  float* out;                  // (N P2, D)
  __device__ int64_t key(int64_t e) const { return h.target(e); }
  __device__ void row(int64_t e, int t, int, float (&r)[R]) const {
    const float g = h.upstream(e);
    for (int c = 0; c < h.D; ++c) r[c] = -h.term(e, t, c, g);
  }
  __device__ void store(int t, int, const float (&r)[R]) const {
    float* o = out + (int64_t)t * h.D;
    for (int c = 0; c < h.D; ++c) o[c] = accumulate ? o[c] + r[c] : r[c];
  }
};

// ---- point-mesh distances: query q adds the target part of its pair's gradient (point_mesh_geom.h) to target idxs[q] -----------------
template <int QK, int TK>
struct PointMeshOp {
  static constexpr int R = pm::kind_floats(TK);
  int64_t nsamples, nkeys;  // Q queries, T targets
  pm::Hits h;
  int accumulate;
  float* out;  // (T, R)
  // the recorded index also for a query whose element has no targets (its row is zero): it must not cut a segment in two
  __device__ int64_t key(int64_t q) const { return h.idxs[q]; }
  __device__ void row(int64_t q, int, int, float (&r)[R]) const {
    float g = 0.0f;
    const int64_t t = h.target(q, &g);
    if (t < 0) return;
    float gq[pm::kind_floats(QK)];
    h.grads<QK, TK>(q, t, g, gq, r);
  }
  __device__ void store(int t, int, const float (&r)[R]) const {
    float* o = out + (int64_t)t * R;
#pragma unroll
    for (int c = 0; c < R; ++c) o[c] = accumulate ? o[c] + r[c] : r[c];
  }
};

// ---- sample_points_from_meshes: sample s adds w_k grad_sample to corner k of its face and grad_normal to the face's normal sum ------
struct SampleOp {
  static constexpr int R = 12;
  int64_t nsamples, nkeys;  // N S samples, F faces
  const int64_t* face_idxs;
  const float *bary, *gs, *gn;  // gn NULL: the row's last three stay 0 and are not stored
  int nv;                       // floats of a stored row: 9 or 12
  float* out;                   // (F, nv)
  __device__ int64_t key(int64_t s) const { return face_idxs[s]; }
  __device__ void row(int64_t s, int, int, float (&r)[R]) const {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float w = bary[s * 3 + k];
      r[3 * k] = w * gs[s * 3], r[3 * k + 1] = w * gs[s * 3 + 1], r[3 * k + 2] = w * gs[s * 3 + 2];
    }
    if (gn) r[9] = gn[s * 3], r[10] = gn[s * 3 + 1], r[11] = gn[s * 3 + 2];
  }
  __device__ void store(int f, int, const float (&r)[R]) const {
    float* o = out + (int64_t)f * nv;
#pragma unroll
    for (int i = 0; i < R; ++i)
      if (i < nv) o[i] = r[i];
  }
};

// ---- points: (2 gd dx, 2 gd dy, gz) per entry (rasterize_points.cu:389-405) ---------------------------------------------------
struct PointOp {
  static constexpr int R = 3;
  int64_t nsamples, nkeys;
  const float* points;
  const int32_t* idxs;
  const float *gz, *gd;
  int H, W, K;
  float* out;  // (P, 3)
  __device__ int64_t key(int64_t s) const { return idxs[s]; }
  __device__ void row(int64_t s, int p, int, float (&r)[R]) const {
    const int64_t pix = s / K;
    const int x = (int)(pix % W), y = (int)((pix / W) % H);
    const float xf = pix_to_ndc(W - 1 - x, W, H), yf = pix_to_ndc(H - 1 - y, H, W);
    const float g = gd[s];
    r[0] = 2.0f * g * (points[(int64_t)p * 3] - xf);
    r[1] = 2.0f * g * (points[(int64_t)p * 3 + 1] - yf);
    r[2] = gz[s];
  }
  __device__ void store(int p, int, const float (&r)[R]) const {
    out[(int64_t)p * 3] = r[0], out[(int64_t)p * 3 + 1] = r[1], out[(int64_t)p * 3 + 2] = r[2];
  }
};

// ---- the compositors' per-pixel part: grad_alphas and each entry's weight on grad_features -------------------------------------
// One thread per pixel, nothing shared between pixels (composite.hip: composite_bwd_generic_kernel without its scatter).  Entry k of
// pixel (n, y, x) is read at n st[0] + k st[1] + y st[2] + x st[3]; grad_alphas and the weights are written at the strides `os`.
struct PixelArgs {
  const float* features;
  int64_t fs0, fs1;
  const float* alphas;   // or squared distances when from_dists (alpha = 1 - d * inv_r2: PointsRenderer's weights)
  const int64_t* idx64;  // one of the two
  const int32_t* idx32;
  const float* grad_out;
  int64_t as[4], is[4], gos[4], os[4];  // gos: (n, c, y, x) strides of grad_out
  int N, C, K, H, W, from_dists;
  int64_t P;
  float inv_r2;
  float* grad_alphas;
  float* weights;
};

__device__ __forceinline__ int pixel_id(const PixelArgs& a, int64_t i) {
  const int64_t v = a.idx64 ? a.idx64[i] : (int64_t)a.idx32[i];
  return (v >= 0 && v < a.P) ? (int)v : -1;
}
__device__ __forceinline__ float pixel_alpha(const PixelArgs& a, int64_t i) {
  const float v = a.alphas[i];
  return a.from_dists ? 1.0f - v * a.inv_r2 : v;
}

template <int MODE>
__global__ __launch_bounds__(256) void composite_pixel_kernel(PixelArgs a) {
  const int64_t npix = (int64_t)a.N * a.H * a.W;
  const int K = a.K, C = a.C;
  const int64_t HW = (int64_t)a.H * a.W;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < npix; t += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(t / HW);
    const int64_t yx = t % HW;
    const int y = (int)(yx / a.W), x = (int)(yx % a.W);
    const int64_t abase = n * a.as[0] + y * a.as[2] + x * a.as[3];
    const int64_t ibase = n * a.is[0] + y * a.is[2] + x * a.is[3];
    const int64_t obase = n * a.os[0] + y * a.os[2] + x * a.os[3];
    const float* go_p = a.grad_out + n * a.gos[0] + y * a.gos[2] + x * a.gos[3];
    float* ga_p = a.grad_alphas + obase;
    float* w_p = a.weights + obase;
    float sum_alpha = 0.0f, cum = 1.0f;
    for (int k = 0; k < K; ++k) {  // the weights: cum * alpha (alpha_composite.cu:113), alpha / sum, alpha
      ga_p[k * a.os[1]] = 0.0f;
      float w = 0.0f;
      if (pixel_id(a, ibase + k * a.is[1]) >= 0) {
        const float al = pixel_alpha(a, abase + k * a.as[1]);
        if (MODE == P3D_COMPOSITE_ALPHA) {
          w = cum * al;
          cum = cum * (1 - al);
        } else {
          w = al;
          sum_alpha += al;
        }
      }
      w_p[k * a.os[1]] = w;
    }
    if (MODE == P3D_COMPOSITE_NORM_SUM) {
      if (sum_alpha < kEpsNorm) sum_alpha = kEpsNorm;
      for (int k = 0; k < K; ++k) w_p[k * a.os[1]] = w_p[k * a.os[1]] / sum_alpha;
    }
    for (int c = 0; c < C; ++c) {
      const float* f = a.features + (int64_t)c * a.fs0;
      const float go = go_p[c * a.gos[1]];
      cum = 1.0f;
      float sum_af = 0.0f;
      if (MODE == P3D_COMPOSITE_NORM_SUM) {
        for (int k = 0; k < K; ++k) {
          const int id = pixel_id(a, ibase + k * a.is[1]);
          if (id >= 0) sum_af += pixel_alpha(a, abase + k * a.as[1]) * f[(int64_t)id * a.fs1];
        }
      }
      for (int k = 0; k < K; ++k) {
        const int id = pixel_id(a, ibase + k * a.is[1]);
        if (id < 0) continue;
        const float al = pixel_alpha(a, abase + k * a.as[1]);
        const float fv = f[(int64_t)id * a.fs1];
        if (MODE == P3D_COMPOSITE_ALPHA) {
          ga_p[k * a.os[1]] += cum * fv * go;
          const float back = -go * fv * cum * al;
          for (int tt = 0; tt < k; ++tt) {
            if (pixel_id(a, ibase + tt * a.is[1]) < 0) continue;
            ga_p[tt * a.os[1]] += back / (1 - pixel_alpha(a, abase + tt * a.as[1]) + kEpsAlpha);
          }
          cum = cum * (1 - al);
        } else if (MODE == P3D_COMPOSITE_NORM_SUM) {
          ga_p[k * a.os[1]] += (fv * sum_alpha - sum_af) / (sum_alpha * sum_alpha) * go;
        } else {
          ga_p[k * a.os[1]] += fv * go;
        }
      }
    }
  }
}

int launch_pixels(int mode, const PixelArgs& a, hipStream_t s) {
  int64_t blocks = ceil_div((int64_t)a.N * a.H * a.W, 256);
  if (blocks > 16384) blocks = 16384;
  if (blocks < 1) return P3D_OK;
  LaunchScope ls("composite_pixels_ordered", s);
  if (mode == P3D_COMPOSITE_ALPHA)
    composite_pixel_kernel<P3D_COMPOSITE_ALPHA><<<(unsigned)blocks, 256, 0, s>>>(a);
  else if (mode == P3D_COMPOSITE_NORM_SUM)
    composite_pixel_kernel<P3D_COMPOSITE_NORM_SUM><<<(unsigned)blocks, 256, 0, s>>>(a);
  else
    composite_pixel_kernel<P3D_COMPOSITE_SUM><<<(unsigned)blocks, 256, 0, s>>>(a);
  return launch_status();
}

// ---- compositors: entry s of the logical (N, K, H, W) tensors adds weight[s] * grad_out[n, :, y, x] to its point, four channels
// per chunk ---------------------------------------------------------------------------------------------------------------------
struct CompositeOp {
  static constexpr int R = 4;
  int64_t nsamples, nkeys;
  const int64_t* idx;
  int64_t is[4];
  const float* weights;   // (N, K, H, W) contiguous
  const float* grad_out;  // (N, C, H, W) contiguous
  int C, K, H, W;
  float* out;
  int64_t gs0, gs1;
  __device__ void where(int64_t s, int* n, int* k, int* y, int* x) const {
    *x = (int)(s % W);
    s /= W;
    *y = (int)(s % H);
    s /= H;
    *k = (int)(s % K);
    *n = (int)(s / K);
  }
  __device__ int64_t key(int64_t s) const {
    int n, k, y, x;
    where(s, &n, &k, &y, &x);
    return idx[n * is[0] + k * is[1] + y * is[2] + x * is[3]];
  }
  __device__ void row(int64_t s, int, int chunk, float (&r)[R]) const {
    int n, k, y, x;
    where(s, &n, &k, &y, &x);
    const float w = weights[s];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int c = chunk * R + j;
      if (c < C) r[j] = w * grad_out[(((int64_t)n * C + c) * H + y) * W + x];
    }
  }
  __device__ void store(int p, int chunk, const float (&r)[R]) const {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int c = chunk * R + j;
      if (c < C) out[c * gs0 + (int64_t)p * gs1] = r[j];
    }
  }
};

// ---- PointsRenderer's chain: both scatters of an entry in one row of 2 + C ------------------------------------------------------
template <int C>
struct SplatOp {
  static constexpr int R = 2 + C;
  int64_t nsamples, nkeys;
  const float* points;
  const int32_t* idxs;
  const float* grad_alphas;  // (N, H, W, K), from composite_pixel_kernel
  const float* weights;      // (N, H, W, K)
  const float* grad_images;  // (N, H, W, C)
  int H, W, K;
  float inv_r2;
  float *grad_points, *grad_features;
  __device__ int64_t key(int64_t s) const { return idxs[s]; }
  __device__ void row(int64_t s, int p, int, float (&r)[R]) const {
    const int64_t pix = s / K;
    const int x = (int)(pix % W), y = (int)((pix / W) % H);
    const float xf = pix_to_ndc(W - 1 - x, W, H), yf = pix_to_ndc(H - 1 - y, H, W);
    const float gd = -grad_alphas[s] * inv_r2;  // weights = 1 - dists / r^2 (renderer.py:62-64)
    r[0] = 2.0f * gd * (points[(int64_t)p * 3] - xf);
    r[1] = 2.0f * gd * (points[(int64_t)p * 3 + 1] - yf);
    const float w = weights[s];
#pragma unroll
    for (int c = 0; c < C; ++c) r[2 + c] = w * grad_images[pix * C + c];
  }
  __device__ void store(int p, int, const float (&r)[R]) const {
    grad_points[(int64_t)p * 3] = r[0], grad_points[(int64_t)p * 3 + 1] = r[1], grad_points[(int64_t)p * 3 + 2] = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) grad_features[(int64_t)p * C + c] = r[2 + c];
  }
};

// ---- interpolate_face_attributes: bary_i * grad_d into column i D + d of the face's row, four columns per chunk --------------------
struct InterpOp {
  static constexpr int R = 4;
  int64_t nsamples, nkeys;
  const int64_t* p2f;
  const float *bary, *gout;
  int D;
  float* out;  // (F, 3 D)
  __device__ int64_t key(int64_t s) const { return p2f[s]; }
  __device__ void row(int64_t s, int, int chunk, float (&r)[R]) const {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int col = chunk * R + j;
      if (col < 3 * D) r[j] = bary[s * 3 + col / D] * gout[s * D + col % D];
    }
  }
  __device__ void store(int f, int chunk, const float (&r)[R]) const {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int col = chunk * R + j;
      if (col < 3 * D) out[(int64_t)f * 3 * D + col] = r[j];
    }
  }
};

// grad_bary is per sample: no scatter (interp.hip: interp_bwd_kernel without its atomics)
__global__ __launch_bounds__(256) void interp_grad_bary_kernel(const int64_t* __restrict__ p2f, const float* __restrict__ attrs,
                                                               const float* __restrict__ gout, int64_t P, int64_t F, int64_t D,
                                                               float* __restrict__ gbary) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = p2f[p];
    float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
    if (f >= 0 && f < F) {
      const float* a = attrs + f * 3 * D;
      for (int64_t d = 0; d < D; ++d) {
        const float up = gout[p * D + d];
        g0 += a[d] * up;
        g1 += a[D + d] * up;
        g2 += a[2 * D + d] * up;
      }
    }
    gbary[p * 3 + 0] = g0;
    gbary[p * 3 + 1] = g1;
    gbary[p * 3 + 2] = g2;
  }
}

size_t floats_bytes(int64_t n) { return align_up((size_t)(n > 0 ? n : 0) * sizeof(float), 256); }

bool strides_planar_or_rows(const int64_t* st, int C, int64_t P, int64_t out[2]) {  // composite.hip: feature_strides_ok
  const int64_t planes[2] = {P, 1};
  if (st == nullptr) st = planes;
  const bool planar = (st[0] == P || C <= 1) && (st[1] == 1 || P <= 1);
  const bool rows = (st[0] == 1 || C <= 1) && (st[1] == C || P <= 1);
  if (!planar && !rows) return false;
  out[0] = planar ? P : 1;
  out[1] = planar ? 1 : C;
  return true;
}

}  // namespace

// ---- point-mesh distances (point_mesh.hip calls these) ---------------------------------------------------------------------------------
size_t point_mesh_ordered_bytes(int target_kind, int64_t Q) { return partial_bytes(Q, pm::kind_floats(target_kind), 1); }

template <int QK, int TK>
static int point_mesh_ordered_run(const pm::Hits& h, const int64_t* sorted, int accumulate, float* grad_targets, void* workspace,
                                  hipStream_t s) {
  PointMeshOp<QK, TK> op;
  op.nsamples = h.Q, op.nkeys = h.T, op.h = h, op.accumulate = accumulate, op.out = grad_targets;
  return ordered::run(op, sorted, h.Q, 1, workspace, s, "point_mesh_backward_ordered");
}

// the rows of grad_targets hold what the sum is added to (accumulate) or anything (then rows nobody hits must be zero already)
int point_mesh_ordered_scatter(const pm::Hits& h, const int64_t* sorted, int accumulate, float* grad_targets, void* workspace,
                               hipStream_t s) {
  if (h.query_kind == pm::kPoint) {
    return h.target_kind == pm::kTri ? point_mesh_ordered_run<pm::kPoint, pm::kTri>(h, sorted, accumulate, grad_targets, workspace, s)
                                     : point_mesh_ordered_run<pm::kPoint, pm::kSeg>(h, sorted, accumulate, grad_targets, workspace, s);
  }
  return h.query_kind == pm::kTri ? point_mesh_ordered_run<pm::kTri, pm::kPoint>(h, sorted, accumulate, grad_targets, workspace, s)
                                  : point_mesh_ordered_run<pm::kSeg, pm::kPoint>(h, sorted, accumulate, grad_targets, workspace, s);
}

// ---- sample_points_from_meshes (sample_points.hip calls these) --------------------------------------------------------------------------
size_t sample_points_ordered_bytes(int64_t num_sorted) { return partial_bytes(num_sorted, SampleOp::R, 1); }

// rows (F, nv) <- per face the sum of its samples' rows, `sorted` being the samples that hold a face sorted stably by face
int sample_points_ordered_rows(const int64_t* face_idxs, const float* bary, const float* grad_samples, const float* grad_normals,
                               const int64_t* sorted, int64_t num_sorted, int64_t num_samples, int64_t F, int nv, float* rows,
                               void* workspace, hipStream_t s) {
  const int st = ordered::fill_zero(rows, F * nv, s);
  if (st != P3D_OK) return st;
  SampleOp op;
  op.nsamples = num_samples, op.nkeys = F;
  op.face_idxs = face_idxs, op.bary = bary, op.gs = grad_samples, op.gn = grad_normals, op.nv = nv, op.out = rows;
  return ordered::run(op, sorted, num_sorted, 1, workspace, s, "sample_points_face_sums_ordered");
}

}  // namespace p3d

using namespace p3d;

// ---- meshes ------------------------------------------------------------------------------------------------------------------------
P3D_API size_t p3d_rasterize_meshes_backward_ordered_workspace_bytes(int64_t F, int through_faces, int64_t num_sorted) {
  if (F < 0 || num_sorted < 0) return 0;
  if (!through_faces) return partial_bytes(num_sorted, 9, 1);
  const size_t a = partial_bytes(num_sorted, 9, 1), b = partial_bytes(F * 3, 3, 1);
  return floats_bytes(F * 9) + (a > b ? a : b);
}

P3D_API int p3d_rasterize_meshes_backward_ordered(const float* face_verts, const int64_t* faces, const int64_t* p2f, const float* grad_zbuf,
                                                  const float* grad_bary, const float* grad_dists, const int64_t* sorted_samples,
                                                  int64_t num_sorted, const int64_t* sorted_corners, int64_t num_corners, int64_t F,
                                                  int64_t V, int N, int H, int W, int K, int persp, int clip, float* grad_out,
                                                  void* workspace, size_t workspace_bytes, p3d_stream_t stream) {
  if (F < 0 || V < 0 || N < 0 || H < 0 || W < 0 || K < 0 || num_sorted < 0 || num_corners < 0) return P3D_ERR_INVALID_ARG;
  const int64_t nsamples = (int64_t)N * H * W * K;
  if (num_sorted > nsamples || num_corners > F * 3) return P3D_ERR_INVALID_ARG;
  const int64_t out_floats = faces ? V * 3 : F * 9;
  if (out_floats == 0) return P3D_OK;
  if (!grad_out) return P3D_ERR_INVALID_ARG;
  if (num_sorted > 0 && (!face_verts || !p2f || !grad_zbuf || !grad_bary || !grad_dists || !sorted_samples)) return P3D_ERR_INVALID_ARG;
  if (faces && num_corners > 0 && !sorted_corners) return P3D_ERR_INVALID_ARG;
  if (workspace_bytes < p3d_rasterize_meshes_backward_ordered_workspace_bytes(F, faces != nullptr, num_sorted) ||
      (!workspace && (num_sorted > 0 || (faces && F > 0))))
    return P3D_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  int st = ordered::fill_zero(grad_out, out_floats, s);
  if (st != P3D_OK || F == 0) return st;
  float* per_face = faces ? static_cast<float*>(workspace) : grad_out;
  void* partials = faces ? static_cast<char*>(workspace) + floats_bytes(F * 9) : workspace;
  if (faces && (st = ordered::fill_zero(per_face, F * 9, s)) != P3D_OK) return st;
  MeshOp op;
  op.nsamples = nsamples, op.nkeys = F;
  op.face_verts = face_verts, op.p2f = p2f, op.gz = grad_zbuf, op.gb = grad_bary, op.gd = grad_dists;
  op.H = H, op.W = W, op.K = K, op.persp = persp, op.clip = clip;
  op.out = per_face;
  if ((st = ordered::run(op, sorted_samples, num_sorted, 1, partials, s, "mesh_backward_ordered")) != P3D_OK || !faces) return st;
  CornerOp co;
  co.nsamples = F * 3, co.nkeys = V;
  co.src = per_face, co.faces = faces, co.out = grad_out;
  return ordered::run(co, sorted_corners, num_corners, 1, partials, s, "scatter_face_grads_ordered");
}

P3D_API size_t p3d_scatter_face_grads_ordered_workspace_bytes(int64_t F) { return F < 0 ? 0 : partial_bytes(F * 3, 3, 1); }

P3D_API int p3d_scatter_face_grads_ordered(const float* grad_face_verts, const int64_t* faces, const int64_t* sorted_corners,
                                           int64_t num_corners, int64_t V, int64_t F, float* grad_verts, void* workspace,
                                           size_t workspace_bytes, p3d_stream_t stream) {
  if (V < 0 || F < 0 || num_corners < 0 || num_corners > F * 3) return P3D_ERR_INVALID_ARG;
  if (V == 0) return P3D_OK;
  if (!grad_verts) return P3D_ERR_INVALID_ARG;
  if (num_corners > 0 && (!grad_face_verts || !faces || !sorted_corners)) return P3D_ERR_INVALID_ARG;
  if (workspace_bytes < p3d_scatter_face_grads_ordered_workspace_bytes(F) || (!workspace && num_corners > 0)) return P3D_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int st = ordered::fill_zero(grad_verts, V * 3, s);
  if (st != P3D_OK) return st;
  CornerOp co;
  co.nsamples = F * 3, co.nkeys = V;
  co.src = grad_face_verts, co.faces = faces, co.out = grad_verts;
  return ordered::run(co, sorted_corners, num_corners, 1, workspace, s, "scatter_face_grads_ordered");
}

// ---- nearest neighbours --------------------------------------------------------------------------------------------------------------
P3D_API size_t p3d_knn_points_ordered_backward_workspace_bytes(int64_t num_sorted) {
  return num_sorted < 0 ? 0 : partial_bytes(num_sorted, 3, 1);
}

P3D_API int p3d_knn_points_ordered_backward(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2,
                                            const int64_t* idx, const float* grad_dists, const float* cloud_scale,
                                            const int64_t* sorted_samples, int64_t num_sorted, int64_t N, int64_t P1, int64_t P2, int D,
                                            int K, int norm, unsigned flags, float* grad_p2, void* workspace, size_t workspace_bytes,
                                            p3d_stream_t stream) {
  if (N < 0 || P1 < 0 || P2 < 0 || K < 1 || D < 1 || num_sorted < 0 || (norm != 1 && norm != 2)) return P3D_ERR_INVALID_ARG;
  if (D != 2 && D != 3) return P3D_ERR_UNSUPPORTED;
  // a key n * P2 + j is an int (ordered_sum.h)
  if (P2 > 0 && N > INT32_MAX / P2) return P3D_ERR_INVALID_ARG;
  if (P1 > 0 && N > 0 && (int64_t)K > INT64_MAX / 8 / P1 / N) return P3D_ERR_INVALID_ARG;
  const int64_t hits = N * P1 * K;
  if (num_sorted > hits) return P3D_ERR_INVALID_ARG;
  if (N * P2 == 0) return P3D_OK;
  if (!grad_p2) return P3D_ERR_INVALID_ARG;
  if (num_sorted > 0 && (!p1 || !p2 || !idx || !sorted_samples)) return P3D_ERR_INVALID_ARG;
  if (workspace_bytes < p3d_knn_points_ordered_backward_workspace_bytes(num_sorted) || (!workspace && num_sorted > 0)) return P3D_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int accumulate = (flags & P3D_KNN_ACCUMULATE_P2) != 0;
  if (!accumulate) {
    const int st = ordered::fill_zero(grad_p2, N * P2 * D, s);
    if (st != P3D_OK) return st;
  }
  KnnOp op;
  op.nsamples = hits, op.nkeys = N * P2;
  op.h.p1 = p1, op.h.p2 = p2, op.h.lengths1 = lengths1, op.h.lengths2 = lengths2, op.h.idx = idx, op.h.grad_dists = grad_dists;
  op.h.cloud_scale = cloud_scale, op.h.N = N, op.h.P1 = P1, op.h.P2 = P2, op.h.D = D, op.h.K = K, op.h.norm = norm;
  op.accumulate = accumulate, op.out = grad_p2;
  return ordered::run(op, sorted_samples, num_sorted, 1, workspace, s, "knn_backward_ordered");
}

// ---- points ------------------------------------------------------------------------------------------------------------------------
P3D_API size_t p3d_rasterize_points_backward_ordered_workspace_bytes(int64_t num_sorted) {
  return num_sorted < 0 ? 0 : partial_bytes(num_sorted, 3, 1);
}

P3D_API int p3d_rasterize_points_backward_ordered(const float* points, const int32_t* idxs, const float* grad_zbuf, const float* grad_dists,
                                                  const int64_t* sorted_samples, int64_t num_sorted, int64_t P, int N, int H, int W, int K,
                                                  float* grad_points, void* workspace, size_t workspace_bytes, p3d_stream_t stream) {
  if (P < 0 || N < 0 || H < 0 || W < 0 || K < 0 || num_sorted < 0) return P3D_ERR_INVALID_ARG;
  const int64_t nsamples = (int64_t)N * H * W * K;
  if (num_sorted > nsamples) return P3D_ERR_INVALID_ARG;
  if (P == 0) return P3D_OK;
  if (!grad_points) return P3D_ERR_INVALID_ARG;
  if (num_sorted > 0 && (!points || !idxs || !grad_zbuf || !grad_dists || !sorted_samples)) return P3D_ERR_INVALID_ARG;
  if (workspace_bytes < p3d_rasterize_points_backward_ordered_workspace_bytes(num_sorted) || (!workspace && num_sorted > 0))
    return P3D_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int st = ordered::fill_zero(grad_points, P * 3, s);
  if (st != P3D_OK) return st;
  PointOp op;
  op.nsamples = nsamples, op.nkeys = P;
  op.points = points, op.idxs = idxs, op.gz = grad_zbuf, op.gd = grad_dists;
  op.H = H, op.W = W, op.K = K;
  op.out = grad_points;
  return ordered::run(op, sorted_samples, num_sorted, 1, workspace, s, "points_backward_ordered");
}

P3D_API size_t p3d_rasterize_points_composite_backward_ordered_workspace_bytes(int N, int H, int W, int K, int C, int64_t num_sorted) {
  if (N < 0 || H < 0 || W < 0 || K < 0 || C < 1 || C > 4 || num_sorted < 0) return 0;
  return 2 * floats_bytes((int64_t)N * H * W * K) + partial_bytes(num_sorted, 2 + C, 1);
}

P3D_API int p3d_rasterize_points_composite_backward_ordered(int mode, const float* points, const float* features, const int32_t* idxs,
                                                            const float* dists, const float* grad_images, const int64_t* sorted_samples,
                                                            int64_t num_sorted, int64_t P, int C, int N, int H, int W, int K, float inv_r2,
                                                            float* grad_points, float* grad_features, void* workspace,
                                                            size_t workspace_bytes, p3d_stream_t stream) {
  if (P < 0 || N < 0 || H < 0 || W < 0 || K < 0 || C < 1 || C > 4 || num_sorted < 0) return P3D_ERR_INVALID_ARG;
  if (K > P3D_MAX_K) return P3D_ERR_K_TOO_LARGE;
  if (mode != P3D_COMPOSITE_ALPHA && mode != P3D_COMPOSITE_NORM_SUM) return P3D_ERR_INVALID_ARG;
  const int64_t nsamples = (int64_t)N * H * W * K;
  if (num_sorted > nsamples) return P3D_ERR_INVALID_ARG;
  if (P == 0) return P3D_OK;
  if (!grad_points || !grad_features) return P3D_ERR_INVALID_ARG;
  if (nsamples > 0 && (!points || !features || !idxs || !dists || !grad_images)) return P3D_ERR_INVALID_ARG;
  if (num_sorted > 0 && !sorted_samples) return P3D_ERR_INVALID_ARG;
  if (workspace_bytes < p3d_rasterize_points_composite_backward_ordered_workspace_bytes(N, H, W, K, C, num_sorted) ||
      (!workspace && nsamples > 0))
    return P3D_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  int st = ordered::fill_zero(grad_points, P * 3, s);
  if (st != P3D_OK) return st;
  if ((st = ordered::fill_zero(grad_features, P * C, s)) != P3D_OK || nsamples == 0) return st;
  float* ga = static_cast<float*>(workspace);
  float* wt = reinterpret_cast<float*>(static_cast<char*>(workspace) + floats_bytes(nsamples));
  void* partials = static_cast<char*>(workspace) + 2 * floats_bytes(nsamples);
  PixelArgs a{};
  a.features = features, a.fs0 = 1, a.fs1 = C;
  a.alphas = dists, a.idx32 = idxs, a.grad_out = grad_images;
  const int64_t hwk[4] = {(int64_t)H * W * K, 1, (int64_t)W * K, K};  // (n, k, y, x) strides of (N, H, W, K) memory
  for (int i = 0; i < 4; ++i) a.as[i] = a.is[i] = a.os[i] = hwk[i];
  a.gos[0] = (int64_t)H * W * C, a.gos[1] = 1, a.gos[2] = (int64_t)W * C, a.gos[3] = C;
  a.N = N, a.C = C, a.K = K, a.H = H, a.W = W, a.from_dists = 1, a.P = P, a.inv_r2 = inv_r2;
  a.grad_alphas = ga, a.weights = wt;
  if ((st = launch_pixels(mode, a, s)) != P3D_OK) return st;
#define P3D_SPLAT_ORDERED(C_)                                                                       \
  {                                                                                                 \
    SplatOp<C_> op;                                                                                 \
    op.nsamples = nsamples, op.nkeys = P;                                                           \
    op.points = points, op.idxs = idxs, op.grad_alphas = ga, op.weights = wt, op.grad_images = grad_images; \
    op.H = H, op.W = W, op.K = K, op.inv_r2 = inv_r2;                                               \
    op.grad_points = grad_points, op.grad_features = grad_features;                                 \
    return ordered::run(op, sorted_samples, num_sorted, 1, partials, s, "points_composite_bwd_ordered"); \
  }
  switch (C) {
    case 1: P3D_SPLAT_ORDERED(1)
    case 2: P3D_SPLAT_ORDERED(2)
    case 3: P3D_SPLAT_ORDERED(3)
    default: P3D_SPLAT_ORDERED(4)
  }
#undef P3D_SPLAT_ORDERED
}

// ---- compositors -------------------------------------------------------------------------------------------------------------------
P3D_API size_t p3d_composite_backward_ordered_workspace_bytes(int N, int K, int H, int W, int C, int64_t num_sorted) {
  if (N < 0 || K < 0 || H < 0 || W < 0 || C < 0 || num_sorted < 0) return 0;
  return floats_bytes((int64_t)N * K * H * W) + partial_bytes(num_sorted, 4, (C + 3) / 4);
}

P3D_API int p3d_composite_backward_ordered(int mode, const float* grad_outputs, const float* features, const int64_t feature_strides[2],
                                           const float* alphas, const int64_t* points_idx, const int64_t* sorted_samples,
                                           int64_t num_sorted, int N, int C, int64_t P, int K, int H, int W,
                                           const int64_t alphas_strides[4], const int64_t idx_strides[4], float* grad_features,
                                           const int64_t grad_feature_strides[2], float* grad_alphas, void* workspace,
                                           size_t workspace_bytes, p3d_stream_t stream) {
  if (mode < 0 || mode > 2 || N < 0 || C < 0 || K < 0 || H < 0 || W < 0 || P < 0 || num_sorted < 0) return P3D_ERR_INVALID_ARG;
  int64_t fst[2], gst[2];
  if (!strides_planar_or_rows(feature_strides, C, P, fst) || !strides_planar_or_rows(grad_feature_strides, C, P, gst))
    return P3D_ERR_INVALID_ARG;
  const int64_t nga = (int64_t)N * K * H * W;
  if (num_sorted > nga || (C + 3) / 4 > 65535) return P3D_ERR_INVALID_ARG;
  if ((int64_t)C * P > 0 && !grad_features) return P3D_ERR_INVALID_ARG;
  if (nga > 0 && (!grad_alphas || !alphas || !points_idx || !alphas_strides || !idx_strides)) return P3D_ERR_INVALID_ARG;
  if (nga > 0 && C > 0 && (!grad_outputs || !features)) return P3D_ERR_INVALID_ARG;
  if (num_sorted > 0 && !sorted_samples) return P3D_ERR_INVALID_ARG;
  if (workspace_bytes < p3d_composite_backward_ordered_workspace_bytes(N, K, H, W, C, num_sorted) || (!workspace && nga > 0))
    return P3D_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  int st = ordered::fill_zero(grad_features, (int64_t)C * P, s);
  if (st != P3D_OK || nga == 0) return st;
  float* wt = static_cast<float*>(workspace);
  void* partials = static_cast<char*>(workspace) + floats_bytes(nga);
  PixelArgs a{};
  a.features = features, a.fs0 = fst[0], a.fs1 = fst[1];
  a.alphas = alphas, a.idx64 = points_idx, a.grad_out = grad_outputs;
  const int64_t HW = (int64_t)H * W;
  for (int i = 0; i < 4; ++i) a.as[i] = alphas_strides[i], a.is[i] = idx_strides[i];
  a.os[0] = K * HW, a.os[1] = HW, a.os[2] = W, a.os[3] = 1;
  a.gos[0] = C * HW, a.gos[1] = HW, a.gos[2] = W, a.gos[3] = 1;
  a.N = N, a.C = C, a.K = K, a.H = H, a.W = W, a.from_dists = 0, a.P = P, a.inv_r2 = 0.0f;
  a.grad_alphas = grad_alphas, a.weights = wt;
  if ((st = launch_pixels(mode, a, s)) != P3D_OK || C == 0 || P == 0) return st;
  CompositeOp op;
  op.nsamples = nga, op.nkeys = P;
  op.idx = points_idx;
  for (int i = 0; i < 4; ++i) op.is[i] = idx_strides[i];
  op.weights = wt, op.grad_out = grad_outputs;
  op.C = C, op.K = K, op.H = H, op.W = W;
  op.out = grad_features, op.gs0 = gst[0], op.gs1 = gst[1];
  return ordered::run(op, sorted_samples, num_sorted, (C + 3) / 4, partials, s, "composite_bwd_ordered");
}

// ---- interpolate_face_attributes (float32) --------------------------------------------------------------------------------------------
P3D_API size_t p3d_interp_face_attrs_backward_ordered_workspace_bytes(int64_t D, int64_t num_sorted) {
  if (D < 0 || num_sorted < 0 || D > 65535) return 0;
  return partial_bytes(num_sorted, 4, (int)((3 * D + 3) / 4));
}

P3D_API int p3d_interp_face_attrs_backward_ordered(const int64_t* p2f, const float* bary, const float* attrs, const float* gout,
                                                   const int64_t* sorted_samples, int64_t num_sorted, int64_t P, int64_t F, int64_t D,
                                                   float* gbary, float* gattrs, void* workspace, size_t workspace_bytes,
                                                   p3d_stream_t stream) {
  if (P < 0 || F < 0 || D < 0 || D > 65535 || num_sorted < 0 || num_sorted > P) return P3D_ERR_INVALID_ARG;
  if (F * D > 0 && !gattrs) return P3D_ERR_INVALID_ARG;
  if (P > 0 && (!p2f || !bary || !gbary || (D > 0 && !gout) || (F > 0 && D > 0 && !attrs))) return P3D_ERR_INVALID_ARG;
  if (num_sorted > 0 && !sorted_samples) return P3D_ERR_INVALID_ARG;
  if (workspace_bytes < p3d_interp_face_attrs_backward_ordered_workspace_bytes(D, num_sorted) || (!workspace && num_sorted > 0 && D > 0))
    return P3D_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  int st = ordered::fill_zero(gattrs, F * 3 * D, s);
  if (st != P3D_OK || P == 0) return st;
  int64_t blocks = ceil_div(P, 256);
  if (blocks > 16384) blocks = 16384;
  {
    LaunchScope ls("interp_grad_bary_ordered", s);
    interp_grad_bary_kernel<<<(unsigned)blocks, 256, 0, s>>>(p2f, attrs, gout, P, F, D, gbary);
  }
  if ((st = launch_status()) != P3D_OK || F == 0 || D == 0) return st;
  InterpOp op;
  op.nsamples = P, op.nkeys = F;
  op.p2f = p2f, op.bary = bary, op.gout = gout, op.D = (int)D;
  op.out = gattrs;
  return ordered::run(op, sorted_samples, num_sorted, (int)((3 * D + 3) / 4), workspace, s, "interp_bwd_ordered");
}
