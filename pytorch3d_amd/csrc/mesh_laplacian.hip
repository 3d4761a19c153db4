// mesh_laplacian.hip -- the cotangent Laplacian: mesh_laplacian_smoothing ("cot", "cotcurv") forward and backward, the entries of
// cot_laplacian (pytorch3d/ops/laplacian_matrices.py:73-141) and the half-step of taubin_smoothing (pytorch3d/ops/mesh_filtering.py).
//
// The reference builds an uncoalesced sparse V x V matrix on every call, takes torch.sparse.sum twice and an L.mm whose backward is a
// sparse scatter with float atomics.  Here the faces alone give a set of int32 tables built once (pytorch3d_amd/mesh_losses.py:
// cot_tables) and every step is a GATHER, as in mesh_losses.hip:
//   * face pass    one lane per face: the three cot / 4 of its corners and its area (Heron);
//   * edge pass    one lane per edge: w_e = the sum of face_cot over the corners opposite the edge, in list order -- L[i, j];
//   * vertex pass  one lane per vertex over its row of the adjacency CSR (adj_edge names the edge of every slot): L x, the row sum,
//                  for "cotcurv" the vertex area over its incidence row, the residual, its norm as the term; the terms go through
//                  block_sum_256 and segment_sum_kernel (fixed_sum.h), D(n) = 8 + ceil(ceil(n / 256) / 256) + 8 additions at most;
//   * backward     L is symmetric and a constant of the step (the reference builds it under no_grad): the same gather applied to
//                  y = scale * d.  One launch, one lane per vertex;
//   * taubin       one lane per vertex over its row: the weights 1 / (|x_v - x_j| + eps) of norm_laplacian, their sum, the blend.
// No float atomic anywhere: the same bits on every run, stream and process.  Forward values are one float32 operation per torch
// operation of the reference (-ffp-contract=off; IEEE sqrt and division); arithmetic that only a gradient sees may contract.
// The tables are the caller's: a vertex id outside [0, V), an edge id outside [0, E) or a mesh id outside [0, N) makes its term NaN,
// CSR offsets are clamped to the list and corners out of range skipped -- a table that breaks its contract gives wrong numbers,
// never an access outside the arrays.  Every kernel has one lane per item and no loop over the grid.
#include "csr_gather.h"
#include "fixed_sum.h"
#include "implicit_abi.h"

namespace p3d {
namespace {

__device__ __forceinline__ V3 vertex(const float* __restrict__ verts, int64_t id, int64_t V) {
  if (id < 0 || id >= V) return mk(quiet_nan(), quiet_nan(), quiet_nan());
  return load3(verts + id * 3);
}

__device__ __forceinline__ float edge_weight(const float* __restrict__ edge_w, int64_t e, int64_t E) {
  if (e < 0 || e >= E) return quiet_nan();
  return edge_w[e];
}

struct DivideByMeshes {
  int N;
  __device__ __forceinline__ float operator()(int64_t, float s) const { return s / (float)N; }
};

// laplacian_matrices.py:93-115 in its operation order.  A is the side opposite vertex 0, B opposite 1, C opposite 2.
__global__ __launch_bounds__(256) void cot_face_kernel(const float* __restrict__ verts, const int64_t* __restrict__ faces, int64_t V,
                                                       int64_t F, float eps, float* __restrict__ face_cot, float* __restrict__ face_area) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const V3 v0 = vertex(verts, faces[f * 3], V), v1 = vertex(verts, faces[f * 3 + 1], V), v2 = vertex(verts, faces[f * 3 + 2], V);
  const float A = norm3(v1 - v2), B = norm3(v0 - v2), C = norm3(v0 - v1);
  const float s = 0.5f * ((A + B) + C);
  const float prod = ((s * (s - A)) * (s - B)) * (s - C);
  // clamp(min=eps): a NaN stays a NaN
  const float area = sqrtf(prod < eps ? eps : prod);
  const float A2 = A * A, B2 = B * B, C2 = C * C;
  face_cot[f * 3 + 0] = (((B2 + C2) - A2) / area) / 4.0f;
  face_cot[f * 3 + 1] = (((A2 + C2) - B2) / area) / 4.0f;
  face_cot[f * 3 + 2] = (((A2 + B2) - C2) / area) / 4.0f;
  face_area[f] = area;
}

// w_e = +0 plus face_cot of the edge's corners in list order (corner 3 f + k lies opposite its edge)
__global__ __launch_bounds__(256) void cot_edge_kernel(const float* __restrict__ face_cot, const int32_t* __restrict__ offsets,
                                                       const int32_t* __restrict__ corners, int64_t E, int64_t n_corners,
                                                       float* __restrict__ edge_w) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  int64_t begin, end;
  csr_row(offsets, e, n_corners, begin, end);
  float w = 0.0f;
  for (int64_t i = begin; i < end; ++i) {
    const int64_t c = corners[i];
    if (c < 0 || c >= n_corners) continue;
    w += face_cot[c];
  }
  edge_w[e] = w;
}

// The sum of the areas of the faces round a vertex, in list order, and its reciprocal where it is positive
// (laplacian_matrices.py:133-138: the other sums stay as they are).
__device__ __forceinline__ float vertex_inv_area(const float* __restrict__ face_area, const int32_t* __restrict__ offsets,
                                                 const int32_t* __restrict__ corners, int64_t v, int64_t n_corners) {
  int64_t begin, end;
  csr_row(offsets, v, n_corners, begin, end);
  float a = 0.0f;
  for (int64_t i = begin; i < end; ++i) {
    const int64_t c = corners[i];
    if (c < 0 || c >= n_corners) continue;
    a += face_area[c / 3];
  }
  return a > 0.0f ? 1.0f / a : a;
}

__global__ __launch_bounds__(256) void cot_inv_area_kernel(const float* __restrict__ face_area, const int32_t* __restrict__ offsets,
                                                           const int32_t* __restrict__ corners, int64_t V, int64_t n_corners,
                                                           float* __restrict__ inv_areas) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < V) inv_areas[v] = vertex_inv_area(face_area, offsets, corners, v, n_corners);
}

// mesh_laplacian_smoothing.py:113-134.  "cot": r = (L x) nw - x with nw = 1 / rowsum where rowsum > 0, else rowsum;
// "cotcurv": r = (L x - rowsum x) (0.25 inv_area).  term = |r| weight; d = r weight / |r| (0 where the norm is 0), the scale
// and the row sum are kept for the backward.
template <bool CURV>
__global__ __launch_bounds__(256) void cot_vertex_fwd_kernel(const float* __restrict__ verts, const float* __restrict__ edge_w,
                                                             const float* __restrict__ face_area, const int32_t* __restrict__ adj_offsets,
                                                             const int32_t* __restrict__ adj, const int32_t* __restrict__ adj_edge,
                                                             const int32_t* __restrict__ inc_offsets, const int32_t* __restrict__ inc_corners,
                                                             const int32_t* __restrict__ vert_mesh, const int32_t* __restrict__ num_verts,
                                                             int64_t V, int64_t n_adj, int64_t E, int64_t n_corners, int N,
                                                             float* __restrict__ d, float* __restrict__ scale, float* __restrict__ rowsum,
                                                             float* __restrict__ partials) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float term = 0.0f;
  if (v < V) {
    int64_t begin, end;
    csr_row(adj_offsets, v, n_adj, begin, end);
    V3 lx = mk(0.f, 0.f, 0.f);
    float rs = 0.0f;
    for (int64_t i = begin; i < end; ++i) {
      const float w = edge_weight(edge_w, adj_edge[i], E);
      lx = lx + w * vertex(verts, adj[i], V);
      rs += w;
    }
    const V3 x = load3(verts + v * 3);
    float k;
    V3 r;
    if (CURV) {
      k = 0.25f * vertex_inv_area(face_area, inc_offsets, inc_corners, v, n_corners);
      r = (lx - rs * x) * k;
    } else {
      k = rs > 0.0f ? 1.0f / rs : rs;
      r = lx * k - x;
    }
    const float norm = norm3(r);
    const int32_t mesh = vert_mesh[v];
    const float w = (mesh < 0 || mesh >= N) ? quiet_nan() : 1.0f / (float)num_verts[mesh];
    term = norm * w;
    store3(d + v * 3, r * (norm == 0.0f ? 0.0f : w / norm));
    scale[v] = k;
    rowsum[v] = rs;
  }
  const float s = block_sum_256(term);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// With y = scale * d: "cot" g_u = (g / N) (sum_j w_e y_j - d_u), "cotcurv" g_u = (g / N) (sum_j w_e y_j - rowsum_u y_u).
template <bool CURV>
__global__ __launch_bounds__(256) void cot_vertex_bwd_kernel(const float* __restrict__ grad_loss, const float* __restrict__ d,
                                                             const float* __restrict__ scale, const float* __restrict__ rowsum,
                                                             const float* __restrict__ edge_w, const int32_t* __restrict__ adj_offsets,
                                                             const int32_t* __restrict__ adj, const int32_t* __restrict__ adj_edge,
                                                             int64_t V, int64_t n_adj, int64_t E, int N, float* __restrict__ grad_verts) {
#pragma clang fp contract(fast)
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const float g = grad_loss[0] / (float)N;
  int64_t begin, end;
  csr_row(adj_offsets, v, n_adj, begin, end);
  V3 s = mk(0.f, 0.f, 0.f);
  for (int64_t i = begin; i < end; ++i) {
    const int64_t u = adj[i];
    if (u < 0 || u >= V) continue;
    s = s + load3(d + u * 3) * (edge_weight(edge_w, adj_edge[i], E) * scale[u]);
  }
  const V3 own = CURV ? load3(d + v * 3) * (rowsum[v] * scale[v]) : load3(d + v * 3);
  store3(grad_verts + v * 3, (s - own) * g);
}

// mesh_filtering.py:50-52 with norm_laplacian (laplacian_matrices.py:159-172): w = 1 / (|x_v - x_j| + eps),
// out = c1 x_v + (c sum w x_j) / sum w.  A vertex without a neighbour gives 0 / 0 = NaN, as the reference returns it.
__global__ __launch_bounds__(256) void taubin_step_kernel(const float* __restrict__ verts, const int32_t* __restrict__ adj_offsets,
                                                          const int32_t* __restrict__ adj, int64_t V, int64_t n_adj, float c1, float c,
                                                          float eps, float* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  int64_t begin, end;
  csr_row(adj_offsets, v, n_adj, begin, end);
  const V3 x = load3(verts + v * 3);
  V3 lx = mk(0.f, 0.f, 0.f);
  float tw = 0.0f;
  for (int64_t i = begin; i < end; ++i) {
    const V3 xj = vertex(verts, adj[i], V);
    const float w = 1.0f / (norm3(x - xj) + eps);
    lx = lx + w * xj;
    tw += w;
  }
  store3(out + v * 3, c1 * x + (c * lx) / tw);
}

size_t partial_bytes(int64_t n) { return n <= 0 ? 0 : (size_t)ceil_div(n, 256) * sizeof(float); }

// V, the 2 E adjacency slots and the 3 F corners must fit an int32
bool sizes_ok(int64_t V, int64_t E, int64_t F) {
  return V >= 0 && E >= 0 && F >= 0 && V <= INT32_MAX && E <= INT32_MAX / 2 && F <= INT32_MAX / 3;
}

unsigned blocks(int64_t n) { return (unsigned)ceil_div(n, 256); }

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API size_t p3di_mesh_cot_laplacian_forward_workspace_bytes(int64_t V) { return partial_bytes(V); }

P3D_API int p3di_mesh_cot_weights(const float* verts, const int64_t* faces, const int32_t* edge_corner_offsets, const int32_t* edge_corners,
                                  int64_t V, int64_t F, int64_t E, float eps, float* face_cot, float* face_area, float* edge_w,
                                  p3d_stream_t stream) {
  if (!sizes_ok(V, E, F)) return P3D_ERR_INVALID_ARG;
  if (F > 0 && (!verts || !faces || !face_cot || !face_area)) return P3D_ERR_INVALID_ARG;
  if (E > 0 && (!edge_corner_offsets || !edge_w || (F > 0 && !edge_corners))) return P3D_ERR_INVALID_ARG;
  if (F == 0 && E == 0) return P3D_OK;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("mesh_cot_weights", s);
  if (F > 0) cot_face_kernel<<<blocks(F), 256, 0, s>>>(verts, faces, V, F, eps, face_cot, face_area);
  if (E > 0) cot_edge_kernel<<<blocks(E), 256, 0, s>>>(face_cot, edge_corner_offsets, edge_corners, E, F * 3, edge_w);
  return launch_status();
}

P3D_API int p3di_mesh_cot_inv_areas(const float* face_area, const int32_t* inc_offsets, const int32_t* inc_corners, int64_t V, int64_t F,
                                    float* inv_areas, p3d_stream_t stream) {
  if (!sizes_ok(V, 0, F)) return P3D_ERR_INVALID_ARG;
  if (V == 0) return P3D_OK;
  if (!inc_offsets || !inv_areas || (F > 0 && (!face_area || !inc_corners))) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("mesh_cot_inv_areas", s);
  cot_inv_area_kernel<<<blocks(V), 256, 0, s>>>(face_area, inc_offsets, inc_corners, V, F * 3, inv_areas);
  return launch_status();
}

P3D_API int p3di_mesh_cot_laplacian_forward(const float* verts, const float* edge_w, const float* face_area, const int32_t* adj_offsets,
                                            const int32_t* adj, const int32_t* adj_edge, const int32_t* inc_offsets,
                                            const int32_t* inc_corners, const int32_t* vert_mesh, const int32_t* num_verts, int64_t V,
                                            int64_t E, int64_t F, int N, int curvature, float* d, float* scale, float* rowsum,
                                            void* workspace, size_t workspace_bytes, float* loss, p3d_stream_t stream) {
  if (!sizes_ok(V, E, F) || N <= 0 || !loss) return P3D_ERR_INVALID_ARG;
  if (V > 0 && (!verts || !adj_offsets || !vert_mesh || !num_verts || !d || !scale || !rowsum)) return P3D_ERR_INVALID_ARG;
  if (V > 0 && E > 0 && (!adj || !adj_edge || !edge_w)) return P3D_ERR_INVALID_ARG;
  if (V > 0 && curvature && (!inc_offsets || (F > 0 && (!inc_corners || !face_area)))) return P3D_ERR_INVALID_ARG;
  if (V > 0 && (!workspace || workspace_bytes < partial_bytes(V))) return P3D_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* partials = static_cast<float*>(workspace);
  LaunchScope ls("mesh_cot_laplacian_forward", s);
  if (V > 0 && curvature)
    cot_vertex_fwd_kernel<true><<<blocks(V), 256, 0, s>>>(verts, edge_w, face_area, adj_offsets, adj, adj_edge, inc_offsets, inc_corners,
                                                          vert_mesh, num_verts, V, E * 2, E, F * 3, N, d, scale, rowsum, partials);
  else if (V > 0)
    cot_vertex_fwd_kernel<false><<<blocks(V), 256, 0, s>>>(verts, edge_w, face_area, adj_offsets, adj, adj_edge, inc_offsets, inc_corners,
                                                           vert_mesh, num_verts, V, E * 2, E, F * 3, N, d, scale, rowsum, partials);
  segment_sum_kernel<<<1, 256, 0, s>>>(partials, ceil_div(V, 256), DivideByMeshes{N}, loss);
  return launch_status();
}

P3D_API int p3di_mesh_cot_laplacian_backward(const float* grad_loss, const float* d, const float* scale, const float* rowsum,
                                             const float* edge_w, const int32_t* adj_offsets, const int32_t* adj, const int32_t* adj_edge,
                                             int64_t V, int64_t E, int N, int curvature, float* grad_verts, p3d_stream_t stream) {
  if (!sizes_ok(V, E, 0) || N <= 0) return P3D_ERR_INVALID_ARG;
  if (V == 0) return P3D_OK;
  if (!grad_loss || !d || !scale || !rowsum || !adj_offsets || !grad_verts || (E > 0 && (!adj || !adj_edge || !edge_w)))
    return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("mesh_cot_laplacian_backward", s);
  if (curvature)
    cot_vertex_bwd_kernel<true><<<blocks(V), 256, 0, s>>>(grad_loss, d, scale, rowsum, edge_w, adj_offsets, adj, adj_edge, V, E * 2, E, N,
                                                          grad_verts);
  else
    cot_vertex_bwd_kernel<false><<<blocks(V), 256, 0, s>>>(grad_loss, d, scale, rowsum, edge_w, adj_offsets, adj, adj_edge, V, E * 2, E, N,
                                                           grad_verts);
  return launch_status();
}

P3D_API int p3di_mesh_taubin_smoothing(const float* verts, const int32_t* adj_offsets, const int32_t* adj, int64_t V, int64_t E,
                                       float lambd_c1, float lambd_c, float mu_c1, float mu_c, float eps, int num_iter, float* scratch,
                                       float* out, p3d_stream_t stream) {
  if (!sizes_ok(V, E, 0) || num_iter < 0) return P3D_ERR_INVALID_ARG;
  if (V == 0) return P3D_OK;
  if (!verts || !adj_offsets || !out || (E > 0 && !adj) || (num_iter > 0 && !scratch)) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (num_iter == 0)
    return hipMemcpyAsync(out, verts, (size_t)V * 3 * sizeof(float), hipMemcpyDeviceToDevice, s) == hipSuccess ? P3D_OK : P3D_ERR_LAUNCH;
  LaunchScope ls("mesh_taubin_smoothing", s);
  const float* src = verts;
  for (int it = 0; it < num_iter; ++it) {
    taubin_step_kernel<<<blocks(V), 256, 0, s>>>(src, adj_offsets, adj, V, E * 2, lambd_c1, lambd_c, eps, scratch);
    taubin_step_kernel<<<blocks(V), 256, 0, s>>>(scratch, adj_offsets, adj, V, E * 2, mu_c1, mu_c, eps, out);
    src = out;
  }
  return launch_status();
}
