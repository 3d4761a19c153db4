// implicit.hip -- the two per-ray operators every implicit renderer of the reference ends in (pytorch3d/renderer/implicit):
// sample_pdf (hierarchical ray sampling) and emission-absorption / absorption-only raymarching, forward and backward.
// Contracts: implicit_abi.h.  No float atomic anywhere; every sum and product has an order fixed by the shapes alone.
//
// sample_pdf.  A workgroup of 256 lanes takes `rows` consecutive rows: their weights are one contiguous block, loaded coalesced into LDS
// at an ODD row stride (lanes that walk different rows at the same column hit different banks); `rows` lanes make the running sums in
// place, sequentially, because the bits of a sum decide the bin; then all lanes take the rows x S samples -- consecutive lanes,
// consecutive outputs -- through sample_pdf_one (sample_pdf_sample.h), the function the host loop calls too.  A row whose stride passes
// P3D_SAMPLE_PDF_LDS_FLOATS has its sums made by one lane per row into the workspace and is searched there by the same function.
//
// raymarching.  Lanes run ALONG the ray: a ray of P <= 64 points owns a segment of G = next_pow2(P) lanes (64 / G rays per wave), a
// longer one the whole wave and goes through chunks of 64 points with a carry.  The shifted absorption a_k = prod_{j <= k - s} x_j is an
// inclusive scan of y_k = x_{k-s} (1 for k < s): the shift is a second, cached read of the densities, not a cross-lane move, so it
// crosses chunk borders for free.  The scans are Hillis-Steele rounds of __shfl_up / __shfl_down within the segment, the per-ray sums
// xor butterflies (fixed_sum.h's wave_sum at G = 64, the same rounds cut at G below).  The backward divides nothing:
//     g_d_k = a_k g_w_k - L_k T_k + gO Pre_k Suf_k      (the opacity 1 - prod (1 - d) GROWS with d_k: its term is added)
// with L the exclusive prefix product of x, Pre / Suf the exclusive prefix / suffix products of 1 - d, and T the reverse affine scan
// T_k = g_w_{k+s} d_{k+s} + x_{k+1} T_{k+1} (elements (m, b), composed (m1 m2, b1 + m1 b2)).  Rays of more than one chunk run a first
// sweep that leaves the three prefix carries of every chunk in the workspace (written and read back by the same lane), then the chunks
// in reverse order.
#include "fixed_sum.h"
#include "implicit_abi.h"
#include "sample_pdf_sample.h"

namespace p3d {
namespace {

constexpr int kGroup = 256;

// ---- sample_pdf ---------------------------------------------------------------------------------------------------------------
int64_t pdf_stride(int64_t n_bins) { return n_bins | 1; }
bool pdf_in_lds(int64_t n_bins) { return pdf_stride(n_bins) <= P3D_SAMPLE_PDF_LDS_FLOATS; }
int pdf_rows(int64_t n_bins) {
  const int64_t fit = P3D_SAMPLE_PDF_LDS_FLOATS / pdf_stride(n_bins);
  return (int)(fit < P3D_SAMPLE_PDF_ROWS ? fit : P3D_SAMPLE_PDF_ROWS);
}

// grid: ceil(B / rows) workgroups of 256; dynamic LDS: rows * stride floats
__global__ __launch_bounds__(kGroup) void sample_pdf_lds_kernel(const float* __restrict__ bins, const float* __restrict__ weights,
                                                                float* __restrict__ outputs, int64_t B, int n_bins, int64_t S, float eps,
                                                                int rows, int stride) {
  extern __shared__ float sh_partial[];
  __shared__ float sh_total[P3D_SAMPLE_PDF_ROWS];
  const int64_t row0 = (int64_t)blockIdx.x * rows;
  const int here = (int)(B - row0 < rows ? B - row0 : rows);
  const float* w0 = weights + row0 * n_bins;
  for (int e = threadIdx.x; e < here * n_bins; e += kGroup) sh_partial[(e / n_bins) * stride + e % n_bins] = w0[e];
  __syncthreads();
  if ((int)threadIdx.x < here) {
    float* p = sh_partial + threadIdx.x * stride;
    float total = 0.0f;
    for (int i = 0; i < n_bins; ++i) {
      total = total + p[i];
      p[i] = total;
    }
    sh_total[threadIdx.x] = total + eps;
  }
  __syncthreads();
  float* out0 = outputs + row0 * S;
  for (int64_t e = threadIdx.x; e < here * S; e += kGroup) {
    const int r = (int)(e / S);
    out0[e] = sample_pdf_one(sh_partial + r * stride, w0 + (int64_t)r * n_bins, bins + (row0 + r) * ((int64_t)n_bins + 1), n_bins,
                             sh_total[r], eps, out0[e]);
  }
}

// one lane per row: the running sums into partial (B, n_bins)
__global__ __launch_bounds__(kGroup) void sample_pdf_sums_kernel(const float* __restrict__ weights, float* __restrict__ partial, int64_t B,
                                                                 int64_t n_bins) {
  const int64_t row = (int64_t)blockIdx.x * kGroup + threadIdx.x;
  if (row >= B) return;
  const float* w = weights + row * n_bins;
  float* p = partial + row * n_bins;
  float total = 0.0f;
  for (int64_t i = 0; i < n_bins; ++i) {
    total = total + w[i];
    p[i] = total;
  }
}

// grid-stride over the B * S samples
__global__ __launch_bounds__(kGroup) void sample_pdf_global_kernel(const float* __restrict__ bins, const float* __restrict__ weights,
                                                                   const float* __restrict__ partial, float* __restrict__ outputs,
                                                                   int64_t B, int64_t n_bins, int64_t S, float eps) {
  for (int64_t e = (int64_t)blockIdx.x * kGroup + threadIdx.x; e < B * S; e += (int64_t)gridDim.x * kGroup) {
    const int64_t row = e / S;
    const float* p = partial + row * n_bins;
    outputs[e] = sample_pdf_one(p, weights + row * n_bins, bins + row * (n_bins + 1), n_bins, p[n_bins - 1] + eps, eps, outputs[e]);
  }
}

// ---- raymarching --------------------------------------------------------------------------------------------------------------
int segment_lanes(int64_t P) {
  int g = 1;
  while (g < kWave && g < P) g <<= 1;
  return g;
}

// inclusive prefix product over the segment of G lanes (kseg: the lane's place in it), in Hillis-Steele rounds
__device__ __forceinline__ float seg_prefix_prod(float v, int kseg, int G) {
  for (int d = 1; d < G; d <<= 1) {
    const float t = __shfl_up(v, d, G);
    if (kseg >= d) v = v * t;
  }
  return v;
}

// inclusive suffix product
__device__ __forceinline__ float seg_suffix_prod(float v, int kseg, int G) {
  for (int d = 1; d < G; d <<= 1) {
    const float t = __shfl_down(v, d, G);
    if (kseg + d < G) v = v * t;
  }
  return v;
}

// inclusive suffix composition of the affine maps t -> b + m t: afterwards (m, b) of lane k maps the value BEHIND the segment to T_k
__device__ __forceinline__ void seg_suffix_affine(float& m, float& b, int kseg, int G) {
  for (int d = 1; d < G; d <<= 1) {
    const float m2 = __shfl_down(m, d, G), b2 = __shfl_down(b, d, G);
    if (kseg + d < G) {
      b = b + m * b2;
      m = m * m2;
    }
  }
}

// the sum of the segment in every lane of it: wave_sum's rounds (fixed_sum.h), the first log2 G of them
__device__ __forceinline__ float seg_sum(float x, int G) {
  for (int d = 1; d < G; d <<= 1) x += __shfl_xor(x, d);
  return x;
}

__device__ __forceinline__ float seg_prod(float x, int G) {
  for (int d = 1; d < G; d <<= 1) x = x * __shfl_xor(x, d);
  return x;
}

struct RayLane {
  int64_t ray;  // the lane's ray (may be >= N: then nothing is read or written, the lane only takes part in the shuffles)
  int kseg;     // its place in the segment
  bool live;
};

__device__ __forceinline__ RayLane ray_lane(int64_t N, int G) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t wave = (int64_t)blockIdx.x * (kGroup / kWave) + (threadIdx.x >> 6);
  RayLane r;
  r.ray = wave * (kWave / G) + lane / G;
  r.kseg = lane % G;
  r.live = r.ray < N;
  return r;
}

// the three prefix inputs of point k: y_k = x_{k-s} (absorption), z_k = x_{k-1} (L), e_k = 1 - d_{k-1} (Pre); 1 where there is none
__device__ __forceinline__ float shifted_x(const float* __restrict__ d, int64_t k, int64_t back, int64_t P, float one_eps, bool live) {
  return (live && k < P && k >= back) ? one_eps - d[k - back] : 1.0f;
}

// grid: ceil(N / (4 * 64 / G)) workgroups of 256.  C == 0: the opacity alone (features, weights unused).
__global__ __launch_bounds__(kGroup) void ea_forward_kernel(const float* __restrict__ densities, const float* __restrict__ features,
                                                            int64_t N, int64_t P, int C, int64_t s, float one_eps, int G,
                                                            float* __restrict__ out, float* __restrict__ weights) {
  const RayLane L = ray_lane(N, G);
  const float* d = densities + (L.live ? L.ray : 0) * P;
  const float* f = features + (L.live ? L.ray : 0) * P * C;
  const int64_t chunks = (P + G - 1) / G;
  int c0 = 0;
  do {  // channels in blocks of four accumulators; the opacity and the weights go with the first block
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float carry_a = 1.0f, transmission = 1.0f;
    for (int64_t c = 0; c < chunks; ++c) {
      const int64_t k = c * G + L.kseg;
      const bool in = L.live && k < P;
      const float dk = in ? d[k] : 0.0f;
      const float a = carry_a * seg_prefix_prod(shifted_x(d, k, s, P, one_eps, L.live), L.kseg, G);
      carry_a = __shfl(a, G - 1, G);
      const float w = dk * a;
      if (c0 == 0) {
        transmission = transmission * seg_prod(in ? 1.0f - dk : 1.0f, G);
        if (weights && in) weights[L.ray * P + k] = w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (in && c0 + j < C) acc[j] += w * f[k * C + c0 + j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (c0 + j < C) {  // (uniform over the wave)
        const float sum = seg_sum(acc[j], G);
        if (L.live && L.kseg == 0) out[L.ray * (C + 1) + c0 + j] = sum;
      }
    }
    if (c0 == 0 && L.live && L.kseg == 0) out[L.ray * (C + 1) + C] = 1.0f - transmission;
    c0 += 4;
  } while (c0 < C);
}

// grid as the forward's.  carries: (N, chunks, 3) floats when chunks > 1, else unused.
__global__ __launch_bounds__(kGroup) void ea_backward_kernel(const float* __restrict__ densities, const float* __restrict__ features,
                                                             const float* __restrict__ grad_out, const float* __restrict__ grad_weights,
                                                             int64_t N, int64_t P, int C, int64_t s, float one_eps, int G,
                                                             float* __restrict__ grad_densities, float* __restrict__ grad_features,
                                                             float* __restrict__ carries) {
  const RayLane L = ray_lane(N, G);
  const int64_t ray = L.live ? L.ray : 0;
  const float* d = densities + ray * P;
  const float* f = features + ray * P * C;
  const float* gF = grad_out + ray * (C + 1);
  const float* gW = grad_weights ? grad_weights + ray * P : nullptr;
  const float gO = L.live ? gF[C] : 0.0f;
  const int64_t chunks = (P + G - 1) / G;
  float* my_carries = chunks > 1 ? carries + ray * chunks * 3 : nullptr;  // (touched by the segment's first lane only)

  if (chunks > 1) {  // the prefix carries INTO every chunk
    float ca = 1.0f, cl = 1.0f, cp = 1.0f;
    for (int64_t c = 0; c < chunks; ++c) {
      if (L.live && L.kseg == 0) my_carries[3 * c] = ca, my_carries[3 * c + 1] = cl, my_carries[3 * c + 2] = cp;
      const int64_t k = c * G + L.kseg;
      const bool in = L.live && k < P;
      ca = __shfl(ca * seg_prefix_prod(shifted_x(d, k, s, P, one_eps, L.live), L.kseg, G), G - 1, G);
      cl = __shfl(cl * seg_prefix_prod(shifted_x(d, k, 1, P, one_eps, L.live), L.kseg, G), G - 1, G);
      cp = __shfl(cp * seg_prefix_prod((in && k >= 1) ? 1.0f - d[k - 1] : 1.0f, L.kseg, G), G - 1, G);
    }
  }

  float t_behind = 0.0f, suf_behind = 1.0f;  // T and the suffix product at the first point of the chunk behind
  for (int64_t c = chunks - 1; c >= 0; --c) {
    const int64_t k = c * G + L.kseg;
    const bool in = L.live && k < P;
    float ca = 1.0f, cl = 1.0f, cp = 1.0f;
    if (chunks > 1) {
      if (L.live && L.kseg == 0) ca = my_carries[3 * c], cl = my_carries[3 * c + 1], cp = my_carries[3 * c + 2];
      ca = __shfl(ca, 0, G), cl = __shfl(cl, 0, G), cp = __shfl(cp, 0, G);
    }
    const float dk = in ? d[k] : 0.0f;
    const float a = ca * seg_prefix_prod(shifted_x(d, k, s, P, one_eps, L.live), L.kseg, G);
    const float l = cl * seg_prefix_prod(shifted_x(d, k, 1, P, one_eps, L.live), L.kseg, G);
    const float pre = cp * seg_prefix_prod((in && k >= 1) ? 1.0f - d[k - 1] : 1.0f, L.kseg, G);
    const float suf = seg_suffix_prod((L.live && k + 1 < P) ? 1.0f - d[k + 1] : 1.0f, L.kseg, G) * suf_behind;

    // g_w of this point and of the point s on (the element of the reverse scan)
    float gw = (gW && in) ? gW[k] : 0.0f, gw_on = 0.0f, d_on = 0.0f;
    const bool on = L.live && k < P - s;  // (s >= 1: no overflow; P - s may be negative)
    if (on) {
      d_on = d[k + s];
      if (gW) gw_on = gW[k + s];
    }
    for (int ch = 0; ch < C; ++ch) {
      const float g = L.live ? gF[ch] : 0.0f;
      if (in) gw += g * f[k * C + ch];
      if (on) gw_on += g * f[(k + s) * C + ch];
    }
    float m = (L.live && k + 1 < P) ? one_eps - d[k + 1] : 1.0f, b = gw_on * d_on;
    seg_suffix_affine(m, b, L.kseg, G);
    const float T = b + m * t_behind;
    t_behind = __shfl(T, 0, G);
    suf_behind = __shfl(suf, 0, G);  // (the last lane of the chunk in front multiplies 1 - d of this chunk's first point in itself)

    if (in) {
      grad_densities[L.ray * P + k] = (a * gw - l * T) + gO * (pre * suf);
      const float w = dk * a;
      for (int ch = 0; ch < C; ++ch) grad_features[(L.ray * P + k) * C + ch] = w * gF[ch];
    }
  }
}

unsigned ray_groups(int64_t N, int G) { return (unsigned)ceil_div(N, (int64_t)(kGroup / kWave) * (kWave / G)); }
int64_t ray_chunks(int64_t P) { return ceil_div(P, kWave); }

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API size_t p3di_sample_pdf_workspace_bytes(int64_t B, int64_t n_bins) {
  if (B <= 0 || n_bins < 1 || pdf_in_lds(n_bins)) return 0;
  return align_up((size_t)B * (size_t)n_bins * sizeof(float), 256);
}

P3D_API int p3di_sample_pdf(const float* bins, const float* weights, float* outputs, int64_t B, int64_t n_bins, int64_t S, float eps,
                           void* workspace, size_t workspace_bytes, p3d_stream_t stream) {
  if (B < 0 || S < 0 || n_bins < 1) return P3D_ERR_INVALID_ARG;
  if (B == 0 || S == 0) return P3D_OK;
  if (!bins || !weights || !outputs) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (pdf_in_lds(n_bins)) {
    const int rows = pdf_rows(n_bins), stride = (int)pdf_stride(n_bins);
    const int64_t groups = ceil_div(B, rows);
    if (groups > INT32_MAX) return P3D_ERR_UNSUPPORTED;
    LaunchScope ls("sample_pdf_lds", s);
    sample_pdf_lds_kernel<<<(unsigned)groups, kGroup, (size_t)rows * stride * sizeof(float), s>>>(bins, weights, outputs, B, (int)n_bins, S,
                                                                                                  eps, rows, stride);
    return launch_status();
  }
  if (!workspace) return P3D_ERR_INVALID_ARG;
  if (workspace_bytes < p3di_sample_pdf_workspace_bytes(B, n_bins)) return P3D_ERR_WORKSPACE;
  if (ceil_div(B, kGroup) > INT32_MAX) return P3D_ERR_UNSUPPORTED;
  float* partial = static_cast<float*>(workspace);
  {
    LaunchScope ls("sample_pdf_sums", s);
    sample_pdf_sums_kernel<<<(unsigned)ceil_div(B, kGroup), kGroup, 0, s>>>(weights, partial, B, n_bins);
  }
  {
    LaunchScope ls("sample_pdf_global", s);
    sample_pdf_global_kernel<<<stream_blocks(B * S), kGroup, 0, s>>>(bins, weights, partial, outputs, B, n_bins, S, eps);
  }
  return launch_status();
}

P3D_API int p3di_sample_pdf_host(const float* bins, const float* weights, float* outputs, int64_t B, int64_t n_bins, int64_t S, float eps) {
  if (B < 0 || S < 0 || n_bins < 1) return P3D_ERR_INVALID_ARG;
  if (B == 0 || S == 0) return P3D_OK;
  if (!bins || !weights || !outputs) return P3D_ERR_INVALID_ARG;
  float* partial = new float[(size_t)n_bins];
  for (int64_t row = 0; row < B; ++row) {
    const float* w = weights + row * n_bins;
    float total = 0.0f;
    for (int64_t i = 0; i < n_bins; ++i) {
      total = total + w[i];
      partial[i] = total;
    }
    total = total + eps;
    for (int64_t j = 0; j < S; ++j)
      outputs[row * S + j] = sample_pdf_one(partial, w, bins + row * (n_bins + 1), n_bins, total, eps, outputs[row * S + j]);
  }
  delete[] partial;
  return P3D_OK;
}

P3D_API int p3di_ea_raymarch_forward(const float* densities, const float* features, int64_t N, int64_t P, int64_t C, int64_t shift,
                                    float one_plus_eps, float* out, float* weights, p3d_stream_t stream) {
  if (N < 0 || P < 1 || C < 0 || C > INT32_MAX / 2 || shift < 1) return P3D_ERR_INVALID_ARG;
  if (N == 0) return P3D_OK;
  if (!densities || !out || (C > 0 && !features)) return P3D_ERR_INVALID_ARG;
  const int G = segment_lanes(P);
  if (ceil_div(N, (kGroup / kWave) * (kWave / G)) > INT32_MAX) return P3D_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("ea_raymarch_forward", s);
  ea_forward_kernel<<<ray_groups(N, G), kGroup, 0, s>>>(densities, features, N, P, (int)C, shift, one_plus_eps, G, out, weights);
  return launch_status();
}

P3D_API size_t p3di_ea_raymarch_backward_workspace_bytes(int64_t N, int64_t P) {
  if (N <= 0 || P <= kWave) return 0;
  return align_up((size_t)N * (size_t)ray_chunks(P) * 3 * sizeof(float), 256);
}

P3D_API int p3di_ea_raymarch_backward(const float* densities, const float* features, const float* grad_out, const float* grad_weights,
                                     int64_t N, int64_t P, int64_t C, int64_t shift, float one_plus_eps, float* grad_densities,
                                     float* grad_features, void* workspace, size_t workspace_bytes, p3d_stream_t stream) {
  if (N < 0 || P < 1 || C < 0 || C > INT32_MAX / 2 || shift < 1) return P3D_ERR_INVALID_ARG;
  if (N == 0) return P3D_OK;
  if (!densities || !grad_out || !grad_densities || (C > 0 && (!features || !grad_features))) return P3D_ERR_INVALID_ARG;
  const size_t need = p3di_ea_raymarch_backward_workspace_bytes(N, P);
  if (need && !workspace) return P3D_ERR_INVALID_ARG;
  if (workspace_bytes < need) return P3D_ERR_WORKSPACE;
  const int G = segment_lanes(P);
  if (ceil_div(N, (kGroup / kWave) * (kWave / G)) > INT32_MAX) return P3D_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("ea_raymarch_backward", s);
  ea_backward_kernel<<<ray_groups(N, G), kGroup, 0, s>>>(densities, features, grad_out, grad_weights, N, P, (int)C, shift, one_plus_eps, G,
                                                         grad_densities, grad_features, static_cast<float*>(workspace));
  return launch_status();
}
