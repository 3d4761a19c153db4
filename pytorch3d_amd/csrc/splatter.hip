// splatter.hip -- SplatterBlender (pytorch3d/renderer/splatter_blend.py) for gfx950, forward and backward, after the
// camera transform (SURVEY 8(f) row 4 carried to SplatterPhongShader).
//
// The reference builds several (N,H,W,K,9,5) float tensors (splat colours and weights, their padded copy, two gathers,
// the permuted bmm operand) and an (N,H,W,K,9,3) occlusion mask; at 64 x 512^2 x K = 8 one of them is 24 GB.  Here one
// lane owns one output pixel q: it reads the K-layer records (screen xyz, RGB, background flag) of its 3 x 3
// neighbourhood through L1 / L2, classifies each splat into the three occlusion buffers, normalises and composites.
// Nothing of size 9 x K per pixel reaches memory.
//
// Direction bookkeeping (mirrored, not cleaned up): the occlusion test of slot d looks at the unfold neighbour
// (h + d/3 - 1, w + d%3 - 1) (_compute_occlusion_layers, F.unfold), while the splat delivered into slot d comes from
// the source (h + d%3 - 1, w + d/3 - 1) (_offset_splats, crop_ids_h / crop_ids_w) and was weighted with the offset
// offsets[d] = (d/3 - 1, d%3 - 1) on (x, y).  A splat from neighbour (dh, dw) is thus classified with the occlusion
// test of neighbour (dw, dh), exactly as in the reference.
//
// Backward, gather form, no atomics (two runs are bit-identical):
//   splatter_bwd_pre_kernel   per output pixel q: recompute the three buffers, back through the compositing and the
//                             normalisation -> 5 upstream terms per buffer (dL/dC_b RGBA, dL/dW_b) + the 9 occlusion
//                             offsets of q, 24 words into a scratch record.
//   splatter_bwd_kernel       per source (p, k): sum over the 9 pixels q it splats into.
// torch.maximum(W_b, 1) at equality passes half the gradient (torch's own rule for maximum, checked on its CPU build).
#include <math.h>

#include "p3d_common.h"

namespace p3d {
namespace {

constexpr int kTile = 16;       // 16 x 16 pixels per workgroup, 4 rows of 16 per wave
constexpr int kRecWords = 24;   // backward scratch record: 15 upstream terms, 9 occlusion offsets (int bits)

struct SplatArgs {
  const float* colors;    // (N,H,W,K,3)
  const float* coords;    // (N,H,W,K,3) screen xyz, not flipped
  const uint8_t* mask;    // (N,H,W,K) nonzero = background (pix_to_face < 0)
  const float* grad_out;  // (N,H,W,4)   backward
  float* out;             // (N,H,W,4)   forward
  float* rec;             // (N,H,W,24)  backward scratch
  float* g_colors;        // (N,H,W,K,3) backward
  float* g_coords;        // (N,H,W,K,3) backward
  int N, H, W, K;
  float two_s2;           // 2 sigma^2
  float norm;             // (1 + 0.05) / sum_d exp(-|offset_d|^2 / (2 sigma^2))
  float bg0, bg1, bg2;
};

template <int KT>
__device__ __forceinline__ int layers(const SplatArgs& a) {
  return KT ? KT : a.K;
}

__device__ __forceinline__ int64_t pixel(const SplatArgs& a, int n, int h, int w) {
  return ((int64_t)n * a.H + h) * a.W + w;
}

// depth of layer j of a pixel, background entries at 1.0 (_prepare_pixels_and_colors)
template <int KT>
__device__ __forceinline__ float depth(const SplatArgs& a, int64_t pix, int j) {
  const int64_t e = pix * layers<KT>(a) + j;
  return a.mask[e] ? 1.0f : a.coords[e * 3 + 2];
}

// _compute_occlusion_layers for one (q, d): neighbour (nh, nw) of q, depth 0 outside the image (F.unfold's zero padding).
// torch.min keeps the first index on ties: strict '<' in layer order.
template <int KT>
__device__ __forceinline__ int occlusion(const SplatArgs& a, int n, int64_t qpix, int nh, int nw) {
  const int K = layers<KT>(a);
  const bool inside = nh >= 0 && nh < a.H && nw >= 0 && nw < a.W;
  const int64_t npix = inside ? pixel(a, n, nh, nw) : 0;
  const float qtop = depth<KT>(a, qpix, 0);
  const float ptop = inside ? depth<KT>(a, npix, 0) : 0.0f;
  float best_qp = fabsf(ptop - qtop), best_pq = best_qp;
  int id_qp = 0, id_pq = 0;
  for (int j = 1; j < K; ++j) {
    const float pj = inside ? depth<KT>(a, npix, j) : 0.0f;
    const float v_qp = fabsf(pj - qtop);                      // qtop_to_p_zdist
    if (v_qp < best_qp) best_qp = v_qp, id_qp = j;
    const float v_pq = fabsf(ptop - depth<KT>(a, qpix, j));   // ptop_to_q_zdist
    if (v_pq < best_pq) best_pq = v_pq, id_pq = j;
  }
  return best_pq < best_qp ? -id_pq : id_qp;
}

// splat weight alpha * norm * exp(-|floor(xy) - xy + 0.5 + offset|^2 / 2 sigma^2) for a foreground entry (alpha = 1);
// u, v are returned for the backward (d weight / d x = weight * 2u / 2 sigma^2)
__device__ __forceinline__ float splat_weight(const SplatArgs& a, float x, float y, float ox, float oy, float& u, float& v) {
  u = floorf(x) - x + 0.5f + ox;
  v = floorf(y) - y + 0.5f + oy;
  return a.norm * expf(-(u * u + v * v) / a.two_s2);
}

// add the foreground layers [k0, k1) of source pixel spix into buffer acc (RGB, alpha = weight)
template <int KT>
__device__ __forceinline__ void add_layers(const SplatArgs& a, int64_t spix, int k0, int k1, float ox, float oy, float (&acc)[4]) {
  for (int k = k0; k < k1; ++k) {
    const int64_t e = spix * layers<KT>(a) + k;
    if (a.mask[e]) continue;  // alpha 0: weight 0
    const float* c = a.coords + e * 3;
    const float* col = a.colors + e * 3;
    float u, v;
    const float w = splat_weight(a, c[0], c[1], ox, oy, u, v);
    acc[0] += w * col[0];
    acc[1] += w * col[1];
    acc[2] += w * col[2];
    acc[3] += w;
  }
}

// the three occlusion buffers of pixel q (_compute_splatted_colors_and_weights): buffer 0 takes layers k < o, buffer 1
// k == o, buffer 2 k > o, where o is the occlusion offset of the slot.  The colour alpha and the weight are the same sum.
template <int KT>
__device__ __forceinline__ void accumulate(const SplatArgs& a, int n, int h, int w, float (&b0)[4], float (&b1)[4], float (&b2)[4],
                                           int (&occ)[9]) {
  const int K = layers<KT>(a);
  const int64_t qpix = pixel(a, n, h, w);
#pragma unroll
  for (int c = 0; c < 4; ++c) b0[c] = b1[c] = b2[c] = 0.0f;
#pragma unroll
  for (int d = 0; d < 9; ++d) {
    const int dr = d / 3 - 1, dc = d % 3 - 1;
    const int o = occlusion<KT>(a, n, qpix, h + dr, w + dc);
    occ[d] = o;
    const int sh = h + dc, sw = w + dr;
    if (sh < 0 || sh >= a.H || sw < 0 || sw >= a.W) continue;  // _offset_splats zero-pads
    const int64_t spix = pixel(a, n, sh, sw);
    const float ox = (float)dr, oy = (float)dc;
    const int k_eq = o < 0 ? 0 : (o < K ? o : K);
    add_layers<KT>(a, spix, 0, k_eq, ox, oy, b0);
    if (o >= 0 && o < K) add_layers<KT>(a, spix, o, o + 1, ox, oy, b1);
    add_layers<KT>(a, spix, o < 0 ? 0 : (o + 1 < K ? o + 1 : K), K, ox, oy, b2);
  }
}

__device__ __forceinline__ float inv_scale(float wsum) { return 1.0f / fmaxf(wsum, 1.0f); }

// _normalize_and_compose_all_layers, one over-step: out = N_b + (1 - N_b.a) * out
__device__ __forceinline__ void over(const float (&nb)[4], float (&o)[4]) {
  const float t = 1.0f - nb[3];
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = nb[c] + t * o[c];
}

template <int KT>
__global__ __launch_bounds__(kTile* kTile) void splatter_fwd_kernel(SplatArgs a) {
  const int w = blockIdx.x * kTile + threadIdx.x, h = blockIdx.y * kTile + threadIdx.y, n = blockIdx.z;
  if (w >= a.W || h >= a.H) return;
  float b0[4], b1[4], b2[4];
  int occ[9];
  accumulate<KT>(a, n, h, w, b0, b1, b2, occ);
  float n0[4], n1[4], n2[4];
  const float s0 = inv_scale(b0[3]), s1 = inv_scale(b1[3]), s2 = inv_scale(b2[3]);
#pragma unroll
  for (int c = 0; c < 4; ++c) n0[c] = b0[c] * s0, n1[c] = b1[c] * s1, n2[c] = b2[c] * s2;
  float o[4] = {a.bg0, a.bg1, a.bg2, 0.0f};
  over(n2, o);
  over(n1, o);
  over(n0, o);
  reinterpret_cast<float4*>(a.out)[pixel(a, n, h, w)] = make_float4(o[0], o[1], o[2], o[3]);
}

// d loss / d (C_b, W_b) for one buffer from d loss / d N_b (N_b = C_b * s_b, s_b = 1 / max(W_b, 1))
__device__ __forceinline__ void unnormalise(const float (&cb)[4], const float (&dn)[4], float* t) {
  const float m = fmaxf(cb[3], 1.0f), s = 1.0f / m;
  float ds = 0.0f;
#pragma unroll
  for (int c = 0; c < 4; ++c) t[c] = dn[c] * s, ds += dn[c] * cb[c];
  const float dm = -ds / (m * m);
  t[4] = cb[3] > 1.0f ? dm : (cb[3] == 1.0f ? 0.5f * dm : 0.0f);
}

template <int KT>
__global__ __launch_bounds__(kTile* kTile) void splatter_bwd_pre_kernel(SplatArgs a) {
  const int w = blockIdx.x * kTile + threadIdx.x, h = blockIdx.y * kTile + threadIdx.y, n = blockIdx.z;
  if (w >= a.W || h >= a.H) return;
  float b0[4], b1[4], b2[4];
  int occ[9];
  accumulate<KT>(a, n, h, w, b0, b1, b2, occ);
  float n0[4], n1[4], n2[4];
  const float s0 = inv_scale(b0[3]), s1 = inv_scale(b1[3]), s2 = inv_scale(b2[3]);
#pragma unroll
  for (int c = 0; c < 4; ++c) n0[c] = b0[c] * s0, n1[c] = b1[c] * s1, n2[c] = b2[c] * s2;
  float o0[4] = {a.bg0, a.bg1, a.bg2, 0.0f};
  float o1[4] = {o0[0], o0[1], o0[2], o0[3]};
  over(n2, o1);
  float o2[4] = {o1[0], o1[1], o1[2], o1[3]};
  over(n1, o2);
  const int64_t q = pixel(a, n, h, w);
  const float4 g4 = reinterpret_cast<const float4*>(a.grad_out)[q];
  float g[4] = {g4.x, g4.y, g4.z, g4.w};
  // back through out3 = N_0 + (1 - a_0) out2, out2 = N_1 + (1 - a_1) out1, out1 = N_2 + (1 - a_2) out0
  float dn0[4], dn1[4], dn2[4];
  float dot = 0.0f;
#pragma unroll
  for (int c = 0; c < 4; ++c) dn0[c] = g[c], dot += g[c] * o2[c];
  dn0[3] -= dot;
  const float t0 = 1.0f - n0[3];
  dot = 0.0f;
#pragma unroll
  for (int c = 0; c < 4; ++c) g[c] *= t0, dn1[c] = g[c], dot += g[c] * o1[c];
  dn1[3] -= dot;
  const float t1 = 1.0f - n1[3];
  dot = 0.0f;
#pragma unroll
  for (int c = 0; c < 4; ++c) g[c] *= t1, dn2[c] = g[c], dot += g[c] * o0[c];
  dn2[3] -= dot;
  float r[kRecWords];
  unnormalise(b0, dn0, r);
  unnormalise(b1, dn1, r + 5);
  unnormalise(b2, dn2, r + 10);
#pragma unroll
  for (int d = 0; d < 9; ++d) r[15 + d] = __int_as_float(occ[d]);
  float4* dst = reinterpret_cast<float4*>(a.rec + q * kRecWords);
#pragma unroll
  for (int i = 0; i < kRecWords / 4; ++i) dst[i] = make_float4(r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]);
}

// per source pixel p = (n, h, w), every layer k: the splat of slot d lands on q = (h - (d%3 - 1), w - (d/3 - 1))
template <int KT>
__global__ __launch_bounds__(kTile* kTile) void splatter_bwd_kernel(SplatArgs a) {
  const int w = blockIdx.x * kTile + threadIdx.x, h = blockIdx.y * kTile + threadIdx.y, n = blockIdx.z;
  if (w >= a.W || h >= a.H) return;
  const int K = layers<KT>(a);
  const int64_t p = pixel(a, n, h, w);
  const float dscale = 2.0f / a.two_s2;
  for (int k = 0; k < K; ++k) {
    const int64_t e = p * K + k;
    float* gc = a.g_colors + e * 3;
    float* gx = a.g_coords + e * 3;
    if (a.mask[e]) {  // background: colours and coordinates are overwritten by constants in the reference
      gc[0] = gc[1] = gc[2] = 0.0f;
      gx[0] = gx[1] = gx[2] = 0.0f;
      continue;
    }
    const float* c = a.coords + e * 3;
    const float* col = a.colors + e * 3;
    const float x = c[0], y = c[1], cr = col[0], cg = col[1], cb = col[2];
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sx = 0.0f, sy = 0.0f;
#pragma unroll
    for (int d = 0; d < 9; ++d) {
      const int dr = d / 3 - 1, dc = d % 3 - 1;
      const int qh = h - dc, qw = w - dr;
      if (qh < 0 || qh >= a.H || qw < 0 || qw >= a.W) continue;
      const float* rq = a.rec + pixel(a, n, qh, qw) * kRecWords;
      const int o = __float_as_int(rq[15 + d]);
      const float* t = rq + (o > k ? 0 : (o == k ? 5 : 10));
      float u, v;
      const float wt = splat_weight(a, x, y, (float)dr, (float)dc, u, v);
      sr += wt * t[0];
      sg += wt * t[1];
      sb += wt * t[2];
      const float dw = t[0] * cr + t[1] * cg + t[2] * cb + t[3] + t[4];
      sx += dw * wt * u;
      sy += dw * wt * v;
    }
    gc[0] = sr, gc[1] = sg, gc[2] = sb;
    gx[0] = sx * dscale, gx[1] = sy * dscale, gx[2] = 0.0f;  // depth only selects layers
  }
}

int fill(SplatArgs* a, const float* colors, const float* coords, const uint8_t* mask, float sigma, const float* background, int N,
         int H, int W, int K) {
  if (N < 0 || H < 0 || W < 0 || K < 1 || !background || !(sigma > 0.0f) || N > 65535) return P3D_ERR_INVALID_ARG;
  a->colors = colors;
  a->coords = coords;
  a->mask = mask;
  a->N = N, a->H = H, a->W = W, a->K = K;
  a->two_s2 = (float)(2.0 * (double)sigma * (double)sigma);
  // _get_splat_kernel_normalization, in float as the reference evaluates it
  float z = 0.0f;
  for (int d = 0; d < 9; ++d) {
    const int o2 = (d / 3 - 1) * (d / 3 - 1) + (d % 3 - 1) * (d % 3 - 1);
    z += expf(-(float)o2 / a->two_s2);
  }
  a->norm = 1.05f / z;
  a->bg0 = background[0], a->bg1 = background[1], a->bg2 = background[2];
  return P3D_OK;
}

#define P3D_SPLAT_K(KERNEL, ...)                                         \
  switch (K) {                                                           \
    case 1: KERNEL<1><<<grid, block, 0, s>>>(__VA_ARGS__); break;        \
    case 2: KERNEL<2><<<grid, block, 0, s>>>(__VA_ARGS__); break;        \
    case 4: KERNEL<4><<<grid, block, 0, s>>>(__VA_ARGS__); break;        \
    case 8: KERNEL<8><<<grid, block, 0, s>>>(__VA_ARGS__); break;        \
    default: KERNEL<0><<<grid, block, 0, s>>>(__VA_ARGS__); break;       \
  }

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API size_t p3d_splatter_blend_backward_workspace_bytes(int N, int H, int W) {
  if (N < 0 || H < 0 || W < 0) return 0;
  return (size_t)N * H * W * kRecWords * sizeof(float);
}

P3D_API int p3d_splatter_blend_forward(const float* colors, const float* coords, const uint8_t* background_mask, float sigma,
                                       const float background[3], int N, int H, int W, int K, float* out, p3d_stream_t stream) {
  SplatArgs a{};
  const int rc = fill(&a, colors, coords, background_mask, sigma, background, N, H, W, K);
  if (rc != P3D_OK) return rc;
  if ((int64_t)N * H * W == 0) return P3D_OK;
  if (!colors || !coords || !background_mask || !out || ((uintptr_t)out & 15) != 0) return P3D_ERR_INVALID_ARG;
  a.out = out;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)ceil_div(W, kTile), (unsigned)ceil_div(H, kTile), (unsigned)N), block(kTile, kTile);
  if (grid.y > 65535) return P3D_ERR_INVALID_ARG;
  LaunchScope ls("splatter_fwd", s);
  P3D_SPLAT_K(splatter_fwd_kernel, a);
  return launch_status();
}

P3D_API int p3d_splatter_blend_backward(const float* grad_out, const float* colors, const float* coords,
                                        const uint8_t* background_mask, float sigma, const float background[3], int N, int H,
                                        int W, int K, float* grad_colors, float* grad_coords, void* workspace,
                                        size_t workspace_bytes, p3d_stream_t stream) {
  SplatArgs a{};
  const int rc = fill(&a, colors, coords, background_mask, sigma, background, N, H, W, K);
  if (rc != P3D_OK) return rc;
  if ((int64_t)N * H * W == 0) return P3D_OK;
  if (!grad_out || !colors || !coords || !background_mask || !grad_colors || !grad_coords || !workspace) return P3D_ERR_INVALID_ARG;
  if (((uintptr_t)grad_out & 15) != 0 || ((uintptr_t)workspace & 15) != 0) return P3D_ERR_INVALID_ARG;  // float4 accesses
  if (workspace_bytes < p3d_splatter_blend_backward_workspace_bytes(N, H, W)) return P3D_ERR_WORKSPACE;
  a.grad_out = grad_out;
  a.rec = static_cast<float*>(workspace);
  a.g_colors = grad_colors;
  a.g_coords = grad_coords;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)ceil_div(W, kTile), (unsigned)ceil_div(H, kTile), (unsigned)N), block(kTile, kTile);
  if (grid.y > 65535) return P3D_ERR_INVALID_ARG;
  {
    LaunchScope ls("splatter_bwd_pre", s);
    P3D_SPLAT_K(splatter_bwd_pre_kernel, a);
    if (launch_status() != P3D_OK) return P3D_ERR_LAUNCH;
  }
  LaunchScope ls("splatter_bwd", s);
  P3D_SPLAT_K(splatter_bwd_kernel, a);
  return launch_status();
}
