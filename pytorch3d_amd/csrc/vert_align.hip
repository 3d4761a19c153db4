// vert_align.hip -- image features pooled at vertex positions (pytorch3d/ops/vert_align.py: F.grid_sample per feature map, then
// squeeze / transpose / cat / gather).  include/p3d_amd.h has the contract; DESIGN.md 8.19.
//
// The contract is ATen's grid_sampler_2d restated in float32.  A normalised coordinate c on an axis of S pixels has the source
// coordinate ((c + 1) / 2) * (S - 1) with align_corners, ((c + 1) * S - 1) / 2 without.  Border padding clamps it to [0, S - 1]
// (NaN -> 0) and its gradient is 0 where it was at or beyond an end.  Bilinear: x0 = floor(ix), y0 = floor(iy), the corners nw, ne,
// sw, se with the weights (x0+1-ix)(y0+1-iy), (ix-x0)(y0+1-iy), (x0+1-ix)(iy-y0), (ix-x0)(iy-y0); the in-range corners are summed in
// that order from +0.  Nearest: round half to even, one corner of weight 1, no coordinate gradient.  Under zeros padding a source
// coordinate that is not finite or does not fit an int32 (tested as a float, before the conversion) makes the whole sample empty:
// a zero row and zero gradients.
//
// Forward: one launch per feature map writes that map's column block of the (rows, sum C) output; a row is a (n, v) pair, or -- with
// a padded-to-packed index -- a packed vertex, so padding rows are never sampled.  Map and verts are read through their strides.
// Lanes run over channels, several vertices share a wave when C is small; float4 per lane when the map is channels-last and
// C, strides and pointers allow it.
// Backward: grad_verts is a gather per vertex (the lanes' partial sums meet in a fixed shuffle tree; no atomics); grad_feats by
// float atomics with a sample's channels in adjacent lanes, or -- ordered form -- a keys kernel writes the pixel n*H*W + y*W + x of
// every (row, corner) sample, the caller sorts stably, and ordered_sum.h adds the rows of one pixel (channels in chunks of 4): the
// same bits on every run and stream.
#include "ordered_sum.h"

namespace p3d {
namespace {

constexpr float kTooLargeF = 2.0e9f;  // below 2^31: a source coordinate under it converts to int32 without overflow

struct Map {
  const float* p;
  int64_t sn, sc, sh, sw;  // element strides of (N, C, H, W)
  int64_t N, C, H, W;
};

struct GradMap {
  float* p;
  int64_t sn, sc, sh, sw;
};

struct Verts {
  const float* p;  // (N, V, >= 2): x = p[n sn + v sv], y = p[n sn + v sv + sd]
  int64_t sn, sv, sd;
  int64_t V;
  const int64_t* packed_idx;  // row r is the padded vertex packed_idx[r], or r itself
  int64_t n_rows;
};

struct Sample {
  int x[4], y[4];  // corners nw, ne, sw, se; nearest: corner 0 alone
  float w[4];
  bool ok[4];
  float dx[4], dy[4];  // d(out) / d(ix) = sum_k val_k dx[k], d(out) / d(iy) = sum_k val_k dy[k]
  float mx, my;        // d(ix) / d(cx), d(iy) / d(cy); 0 where border clipped, for nearest, and for an empty sample
};

// the source coordinate of c on an axis of S pixels; false: the sample is empty
__device__ __forceinline__ bool source(float c, int64_t S, unsigned flags, float& i, float& mult) {
  const float size = (float)S;
  if (flags & P3D_VERT_ALIGN_CORNERS) {
    i = ((c + 1.0f) / 2.0f) * (size - 1.0f);
    mult = (size - 1.0f) / 2.0f;
  } else {
    i = ((c + 1.0f) * size - 1.0f) / 2.0f;
    mult = size / 2.0f;
  }
  if (flags & P3D_VERT_ALIGN_BORDER) {
    if (!(i > 0.0f)) i = 0.0f, mult = 0.0f;  // NaN too
    else if (i >= size - 1.0f) i = size - 1.0f, mult = 0.0f;
    return true;
  }
  return fabsf(i) < kTooLargeF;  // NaN fails
}

__device__ __forceinline__ Sample make_sample(float cx, float cy, int64_t H, int64_t W, unsigned flags) {
  Sample s;
#pragma unroll
  for (int k = 0; k < 4; ++k) s.x[k] = s.y[k] = 0, s.w[k] = s.dx[k] = s.dy[k] = 0.0f, s.ok[k] = false;
  s.mx = s.my = 0.0f;
  float ix, iy, mx, my;
  const bool okx = source(cx, W, flags, ix, mx), oky = source(cy, H, flags, iy, my);
  if (!(okx && oky)) return s;
  if (flags & P3D_VERT_ALIGN_NEAREST) {
    s.x[0] = (int)rintf(ix);  // half to even
    s.y[0] = (int)rintf(iy);
    s.w[0] = 1.0f;
    s.ok[0] = s.x[0] >= 0 && s.y[0] >= 0 && s.x[0] < W && s.y[0] < H;
    return s;
  }
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy;
  const float wx1 = ix - fx, wx0 = (fx + 1.0f) - ix, wy1 = iy - fy, wy0 = (fy + 1.0f) - iy;
  s.x[0] = x0, s.y[0] = y0, s.w[0] = wx0 * wy0, s.dx[0] = -wy0, s.dy[0] = -wx0;
  s.x[1] = x0 + 1, s.y[1] = y0, s.w[1] = wx1 * wy0, s.dx[1] = wy0, s.dy[1] = -wx1;
  s.x[2] = x0, s.y[2] = y0 + 1, s.w[2] = wx0 * wy1, s.dx[2] = -wy1, s.dy[2] = wx0;
  s.x[3] = x0 + 1, s.y[3] = y0 + 1, s.w[3] = wx1 * wy1, s.dx[3] = wy1, s.dy[3] = wx1;
#pragma unroll
  for (int k = 0; k < 4; ++k) s.ok[k] = s.x[k] >= 0 && s.y[k] >= 0 && s.x[k] < W && s.y[k] < H;
  s.mx = mx, s.my = my;
  return s;
}

// row r -> (n, v) and its sample; false: no such vertex (an index outside the padded tensor): an empty sample
__device__ __forceinline__ bool row_sample(const Verts& vt, int64_t N, int64_t H, int64_t W, unsigned flags, int64_t r, int64_t& n,
                                           int64_t& v, Sample& s) {
  const int64_t i = vt.packed_idx ? vt.packed_idx[r] : r;
  if (i < 0 || i >= N * vt.V) {
    n = v = 0;
    s = make_sample(NAN, NAN, H, W, flags & ~P3D_VERT_ALIGN_BORDER);
    return false;
  }
  n = i / vt.V, v = i % vt.V;
  const float* q = vt.p + n * vt.sn + v * vt.sv;
  s = make_sample(q[0], q[vt.sd], H, W, flags);
  return true;
}

template <bool VEC>
struct Chan;
template <>
struct Chan<true> {
  using T = float4;
  static constexpr int kWidth = 4;
  static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ T load(const float* p) { return *reinterpret_cast<const float4*>(p); }
  static __device__ __forceinline__ void store(float* p, T v) { *reinterpret_cast<float4*>(p) = v; }
  static __device__ __forceinline__ T add_scaled(T a, T v, float w) {
    return make_float4(a.x + v.x * w, a.y + v.y * w, a.z + v.z * w, a.w + v.w * w);
  }
};
template <>
struct Chan<false> {
  using T = float;
  static constexpr int kWidth = 1;
  static __device__ __forceinline__ T zero() { return 0.f; }
  static __device__ __forceinline__ T load(const float* p) { return *p; }
  static __device__ __forceinline__ void store(float* p, T v) { *p = v; }
  static __device__ __forceinline__ T add_scaled(T a, T v, float w) { return a + v * w; }
};

struct Launch {
  int64_t units;  // float4s (VEC) or channels per row
  int lpr_log2;   // log2(lanes per row)
};

// VEC: sc == 1 and everything a multiple of 4 floats / 16 bytes (the entry decides)
template <bool VEC>
__global__ __launch_bounds__(256) void vert_align_fwd_kernel(Map m, Verts vt, Launch L, unsigned flags, float* __restrict__ out,
                                                             int64_t out_stride) {
  using Ch = Chan<VEC>;
  using T = typename Ch::T;
  const int lpr = 1 << L.lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t rows_per_group = 256 >> L.lpr_log2;
  const int64_t groups = (vt.n_rows + rows_per_group - 1) >> (8 - L.lpr_log2);
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t r = g * rows_per_group + (threadIdx.x >> L.lpr_log2);
    if (r >= vt.n_rows) continue;
    int64_t n, v;
    Sample s;
    row_sample(vt, m.N, m.H, m.W, flags, r, n, v, s);
    int64_t off[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) off[k] = s.ok[k] ? s.y[k] * m.sh + s.x[k] * m.sw : 0;
    const float* src = m.p + n * m.sn;
    for (int64_t u = lane; u < L.units; u += lpr) {
      const int64_t c = u * Ch::kWidth;
      const float* q = src + c * m.sc;
      T acc;
      if (flags & P3D_VERT_ALIGN_NEAREST) {
        const T val = Ch::load(q + off[0]);
        acc = s.ok[0] ? val : Ch::zero();
      } else {
        const T v0 = Ch::load(q + off[0]), v1 = Ch::load(q + off[1]), v2 = Ch::load(q + off[2]), v3 = Ch::load(q + off[3]);
        acc = Ch::zero();
        acc = s.ok[0] ? Ch::add_scaled(acc, v0, s.w[0]) : acc;
        acc = s.ok[1] ? Ch::add_scaled(acc, v1, s.w[1]) : acc;
        acc = s.ok[2] ? Ch::add_scaled(acc, v2, s.w[2]) : acc;
        acc = s.ok[3] ? Ch::add_scaled(acc, v3, s.w[3]) : acc;
      }
      Ch::store(out + r * out_stride + c, acc);
    }
  }
}

// grad_verts (N, V, 3) contiguous, ADDED to (the caller zero-fills once and runs one launch per map); grad_feat: zero-filled by the
// caller, float atomics (FEATS) or left alone.  One lane per channel, a fixed xor tree over the lanes of a row.
template <bool FEATS>
__global__ __launch_bounds__(256) void vert_align_bwd_kernel(Map m, Verts vt, Launch L, unsigned flags, const float* __restrict__ grad_out,
                                                             int64_t go_stride, GradMap gm, float* __restrict__ grad_verts) {
  const int lpr = 1 << L.lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t rows_per_group = 256 >> L.lpr_log2;
  const int64_t groups = (vt.n_rows + rows_per_group - 1) >> (8 - L.lpr_log2);
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t r = g * rows_per_group + (threadIdx.x >> L.lpr_log2);
    const bool live = r < vt.n_rows;  // (no early exit: the shuffles below want every lane of the wave)
    int64_t n = 0, v = 0;
    Sample s;
    bool vertex = false;
    if (live) vertex = row_sample(vt, m.N, m.H, m.W, flags, r, n, v, s);
    else s = make_sample(NAN, NAN, m.H, m.W, flags & ~P3D_VERT_ALIGN_BORDER);
    float gix = 0.0f, giy = 0.0f;
    if (live) {
      const float* src = m.p + n * m.sn;
      for (int64_t c = lane; c < m.C; c += lpr) {
        const float go = grad_out[r * go_stride + c];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!s.ok[k]) continue;
          if (FEATS) atomicAdd(gm.p + n * gm.sn + c * gm.sc + s.y[k] * gm.sh + s.x[k] * gm.sw, s.w[k] * go);
          if (grad_verts != nullptr && !(flags & P3D_VERT_ALIGN_NEAREST)) {
            const float val = src[c * m.sc + s.y[k] * m.sh + s.x[k] * m.sw];
            gix += val * s.dx[k] * go;
            giy += val * s.dy[k] * go;
          }
        }
      }
    }
    if (grad_verts != nullptr) {
      for (int d = lpr >> 1; d > 0; d >>= 1) {
        gix += __shfl_xor(gix, d);
        giy += __shfl_xor(giy, d);
      }
      if (live && vertex && lane == 0) {
        float* gv = grad_verts + (n * vt.V + v) * 3;
        gv[0] = gv[0] + s.mx * gix;
        gv[1] = gv[1] + s.my * giy;
      }
    }
  }
}

// sample 4 r + k: the pixel of corner k of row r, or none
__global__ __launch_bounds__(256) void vert_align_keys_kernel(Verts vt, int64_t N, int64_t H, int64_t W, unsigned flags, int* __restrict__ keys) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= vt.n_rows) return;
  int64_t n, v;
  Sample s;
  row_sample(vt, N, H, W, flags, r, n, v, s);
#pragma unroll
  for (int k = 0; k < 4; ++k) keys[r * 4 + k] = s.ok[k] ? (int)((n * H + s.y[k]) * W + s.x[k]) : ordered::kNone;
}

struct PixelOp {
  static constexpr int R = 4;
  Verts vt;
  int64_t N, C, H, W;
  unsigned flags;
  const float* grad_out;
  int64_t go_stride;
  GradMap gm;
  const int* keys;
  int64_t nsamples, nkeys;
  __device__ int64_t key(int64_t s) const { return keys[s]; }
  __device__ void row(int64_t s, int, int chunk, float (&r)[R]) const {
    int64_t n, v;
    Sample sm;
    const int64_t row = s >> 2;
    const int k = (int)(s & 3);
    row_sample(vt, N, H, W, flags, row, n, v, sm);
    float w = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) w = (j == k && sm.ok[j]) ? sm.w[j] : w;  // (no dynamic index into the register arrays)
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t c = (int64_t)chunk * R + i;
      if (c < C) r[i] = w * grad_out[row * go_stride + c];
    }
  }
  __device__ void store(int k, int chunk, const float (&r)[R]) const {
    int64_t p = k;
    const int64_t x = p % W;
    p /= W;
    const int64_t y = p % H, n = p / H;
    float* q = gm.p + n * gm.sn + y * gm.sh + x * gm.sw;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t c = (int64_t)chunk * R + i;
      if (c < C) q[c * gm.sc] = r[i];  // every (pixel, channel) is stored once; the caller zero-filled the rest
    }
  }
};

inline bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

Launch launch_of(int64_t units) {
  Launch L;
  L.units = units;
  L.lpr_log2 = 0;
  while (L.lpr_log2 < 6 && ((int64_t)1 << L.lpr_log2) < units) ++L.lpr_log2;
  return L;
}

unsigned grid_of(int64_t n_rows, const Launch& L) {
  int64_t groups = ceil_div(n_rows, (int64_t)256 >> L.lpr_log2);
  return (unsigned)(groups > P3D_VERT_ALIGN_MAX_GROUPS ? P3D_VERT_ALIGN_MAX_GROUPS : groups);
}

bool bad_verts(const float* verts, int64_t N, int64_t V, int64_t n_rows, const int64_t* packed_idx) {
  return N < 0 || V < 0 || n_rows < 0 || (n_rows > 0 && !verts) || (!packed_idx && n_rows > N * V);
}

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API int p3d_vert_align_forward(const float* feat, int64_t N, int64_t C, int64_t H, int64_t W, int64_t f_sn, int64_t f_sc, int64_t f_sh,
                                   int64_t f_sw, const float* verts, int64_t V, int64_t v_sn, int64_t v_sv, int64_t v_sd,
                                   const int64_t* packed_idx, int64_t n_rows, unsigned flags, float* out, int64_t out_stride,
                                   p3d_stream_t stream) {
  if (C < 0 || H < 0 || W < 0 || bad_verts(verts, N, V, n_rows, packed_idx) || (flags & ~7u) || H > INT32_MAX || W > INT32_MAX)
    return P3D_ERR_INVALID_ARG;
  if (n_rows == 0 || C == 0) return P3D_OK;
  if (!out || out_stride < C || !feat || H == 0 || W == 0) return P3D_ERR_INVALID_ARG;
  const Map m{feat, f_sn, f_sc, f_sh, f_sw, N, C, H, W};
  const Verts vt{verts, v_sn, v_sv, v_sd, V, packed_idx, n_rows};
  const bool vec = f_sc == 1 && C % 4 == 0 && f_sn % 4 == 0 && f_sh % 4 == 0 && f_sw % 4 == 0 && out_stride % 4 == 0 && aligned16(feat) &&
                   aligned16(out);
  const Launch L = launch_of(vec ? C / 4 : C);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("vert_align_forward", s);
  if (vec) vert_align_fwd_kernel<true><<<grid_of(n_rows, L), 256, 0, s>>>(m, vt, L, flags, out, out_stride);
  else vert_align_fwd_kernel<false><<<grid_of(n_rows, L), 256, 0, s>>>(m, vt, L, flags, out, out_stride);
  return launch_status();
}

P3D_API int p3d_vert_align_backward(const float* grad_out, int64_t go_stride, const float* feat, int64_t N, int64_t C, int64_t H, int64_t W,
                                    int64_t f_sn, int64_t f_sc, int64_t f_sh, int64_t f_sw, const float* verts, int64_t V, int64_t v_sn,
                                    int64_t v_sv, int64_t v_sd, const int64_t* packed_idx, int64_t n_rows, unsigned flags, float* grad_feat,
                                    int64_t g_sn, int64_t g_sc, int64_t g_sh, int64_t g_sw, float* grad_verts, p3d_stream_t stream) {
  if (C < 0 || H < 0 || W < 0 || bad_verts(verts, N, V, n_rows, packed_idx) || (flags & ~7u) || H > INT32_MAX || W > INT32_MAX)
    return P3D_ERR_INVALID_ARG;
  if (n_rows == 0 || C == 0 || (!grad_feat && !grad_verts)) return P3D_OK;
  if (!grad_out || go_stride < C || !feat || H == 0 || W == 0) return P3D_ERR_INVALID_ARG;
  const Map m{feat, f_sn, f_sc, f_sh, f_sw, N, C, H, W};
  const Verts vt{verts, v_sn, v_sv, v_sd, V, packed_idx, n_rows};
  const GradMap gm{grad_feat, g_sn, g_sc, g_sh, g_sw};
  const Launch L = launch_of(C);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("vert_align_backward", s);
  if (grad_feat) vert_align_bwd_kernel<true><<<grid_of(n_rows, L), 256, 0, s>>>(m, vt, L, flags, grad_out, go_stride, gm, grad_verts);
  else vert_align_bwd_kernel<false><<<grid_of(n_rows, L), 256, 0, s>>>(m, vt, L, flags, grad_out, go_stride, gm, grad_verts);
  return launch_status();
}

P3D_API size_t p3d_vert_align_workspace_bytes(int64_t n_rows, int64_t C) {
  if (n_rows <= 0 || C <= 0) return 0;
  return ordered::partial_bytes(n_rows * 4, PixelOp::R, (int)ceil_div(C, PixelOp::R));
}

P3D_API int p3d_vert_align_keys(int64_t N, int64_t H, int64_t W, const float* verts, int64_t V, int64_t v_sn, int64_t v_sv, int64_t v_sd,
                                const int64_t* packed_idx, int64_t n_rows, unsigned flags, int32_t* keys, p3d_stream_t stream) {
  if (H < 0 || W < 0 || bad_verts(verts, N, V, n_rows, packed_idx) || (flags & ~7u)) return P3D_ERR_INVALID_ARG;
  if (H > INT32_MAX || W > INT32_MAX || (double)N * (double)H * (double)W >= 2147483648.0 || n_rows > INT32_MAX / 4) return P3D_ERR_UNSUPPORTED;
  if (n_rows == 0) return P3D_OK;
  if (!keys || H == 0 || W == 0) return P3D_ERR_INVALID_ARG;
  const Verts vt{verts, v_sn, v_sv, v_sd, V, packed_idx, n_rows};
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("vert_align_keys", s);
  vert_align_keys_kernel<<<(unsigned)ceil_div(n_rows, 256), 256, 0, s>>>(vt, N, H, W, flags, keys);
  return launch_status();
}

P3D_API int p3d_vert_align_ordered_backward(const float* grad_out, int64_t go_stride, int64_t N, int64_t C, int64_t H, int64_t W,
                                            const float* verts, int64_t V, int64_t v_sn, int64_t v_sv, int64_t v_sd,
                                            const int64_t* packed_idx, int64_t n_rows, unsigned flags, const int32_t* keys,
                                            const int64_t* sorted_samples, float* grad_feat, int64_t g_sn, int64_t g_sc, int64_t g_sh,
                                            int64_t g_sw, void* workspace, size_t workspace_bytes, p3d_stream_t stream) {
  if (C < 0 || H < 0 || W < 0 || bad_verts(verts, N, V, n_rows, packed_idx) || (flags & ~7u)) return P3D_ERR_INVALID_ARG;
  if (H > INT32_MAX || W > INT32_MAX || (double)N * (double)H * (double)W >= 2147483648.0 || n_rows > INT32_MAX / 4) return P3D_ERR_UNSUPPORTED;
  if (n_rows == 0 || C == 0) return P3D_OK;
  if (!grad_out || go_stride < C || !keys || !sorted_samples || !grad_feat || H == 0 || W == 0) return P3D_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < p3d_vert_align_workspace_bytes(n_rows, C)) return P3D_ERR_WORKSPACE;
  const Verts vt{verts, v_sn, v_sv, v_sd, V, packed_idx, n_rows};
  const GradMap gm{grad_feat, g_sn, g_sc, g_sh, g_sw};
  const PixelOp op{vt, N, C, H, W, flags, grad_out, go_stride, gm, keys, n_rows * 4, N * H * W};
  return ordered::run(op, sorted_samples, n_rows * 4, (int)ceil_div(C, PixelOp::R), workspace, (hipStream_t)stream, "vert_align_ordered_backward");
}
