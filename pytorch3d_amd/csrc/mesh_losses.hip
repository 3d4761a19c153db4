// mesh_losses.hip -- the three mesh regularisers of a fitting loop, forward and backward: mesh_edge_loss, mesh_laplacian_smoothing
// ("uniform") and mesh_normal_consistency (pytorch3d/loss/mesh_*.py).
//
// The reference redoes the topology's work every step (sort + bincount + a host round trip for the wing pairs, a sparse V x V matrix
// for the Laplacian, gathers whose autograd ends in index_put / sparse mm with float atomics).  Here the topology is a set of int32
// tables built once (pytorch3d_amd/mesh_losses.py: mesh_loss_topology) and every step is a GATHER:
//   * forward: one lane per edge / vertex / wing pair computes its term, the terms are summed by the fixed tree of fixed_sum.h;
//   * backward of the edge loss and of the Laplacian: one lane per vertex walks its row of the adjacency CSR;
//   * backward of normal consistency: one lane per pair stores the gradients of its four vertices as rows (P, 4, 3), a second launch
//     sums, per vertex, the rows of its incidence list in list order (csr_gather.h, shared with normals.hip).
// No float atomic anywhere.  The sum of n terms is the tree of fixed_sum.h with a block of 256 terms at level 1 and the whole batch
// as the one segment of level 2, finished by the division by the number of meshes: a term passes through at most
// D(n) = 8 + ceil(ceil(n / 256) / 256) + 8  additions; the loss and the gradient have the same bits on every run, stream and process.
// Forward values follow the reference's Python one float32 operation per torch operation (the library is built with
// -ffp-contract=off; IEEE sqrt and division); arithmetic that only a gradient sees may contract.
// The tables are the caller's: a vertex id outside [0, V) or a mesh id outside [0, N) makes its term NaN, CSR offsets are clamped
// to the list and list entries out of range skipped -- a table that breaks its contract gives wrong numbers, never an access
// outside the arrays.
#include "csr_gather.h"
#include "fixed_sum.h"

namespace p3d {
namespace {

struct MeshLosses;  // this translation unit's instance of vert_gather_sum_kernel

// A vertex by a table's id: nothing outside `verts` is read, an id out of range gives NaN coordinates.
__device__ __forceinline__ V3 vertex(const float* __restrict__ verts, int64_t id, int64_t V) {
  if (id < 0 || id >= V) return mk(quiet_nan(), quiet_nan(), quiet_nan());
  return load3(verts + id * 3);
}

// 1.0 / count.float() of the element's mesh (mesh_edge_loss.py:44-45 and its likes): one float32 division.
__device__ __forceinline__ float mesh_weight(const int32_t* __restrict__ counts, int32_t mesh, int N) {
  if (mesh < 0 || mesh >= N) return quiet_nan();
  return 1.0f / (float)counts[mesh];
}

// the last step of segment_sum_kernel: loss.sum() / N
struct DivideByMeshes {
  int N;
  __device__ __forceinline__ float operator()(int64_t, float s) const { return s / (float)N; }
};

// ---- mesh_edge_loss ------------------------------------------------------------------------------------------------------------
// mesh_edge_loss.py:47-52: ((v0 - v1).norm(dim=1, p=2) - target) ** 2.0 * weights
__global__ __launch_bounds__(256) void edge_loss_fwd_kernel(const float* __restrict__ verts, const int32_t* __restrict__ edges,
                                                            const int32_t* __restrict__ edge_mesh, const int32_t* __restrict__ num_edges,
                                                            int64_t V, int64_t E, int N, float target, float* __restrict__ partials) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float term = 0.0f;
  if (e < E) {
    const V3 d = vertex(verts, edges[e * 2], V) - vertex(verts, edges[e * 2 + 1], V);
    const float len = norm3(d);
    const float t = len - target;
    term = (t * t) * mesh_weight(num_edges, edge_mesh[e], N);
  }
  const float s = block_sum_256(term);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// One lane per vertex over its row of the adjacency: g_v = (g / N) sum_u 2 (len - target) w / len (x_v - x_u), 0 where len == 0
// (torch's norm backward).  Every edge of a vertex lies in the vertex's mesh: one weight per vertex.
__global__ __launch_bounds__(256) void edge_loss_bwd_kernel(const float* __restrict__ grad_loss, const float* __restrict__ verts,
                                                            const int32_t* __restrict__ adj_offsets, const int32_t* __restrict__ adj,
                                                            const int32_t* __restrict__ vert_mesh, const int32_t* __restrict__ num_edges,
                                                            int64_t V, int64_t n_adj, int N, float target,
                                                            float* __restrict__ grad_verts) {
#pragma clang fp contract(fast)
  const float g = grad_loss[0] / (float)N;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    int64_t begin, end;
    csr_row(adj_offsets, v, n_adj, begin, end);
    const V3 x = load3(verts + v * 3);
    V3 s = mk(0.f, 0.f, 0.f);
    for (int64_t i = begin; i < end; ++i) {
      const int64_t u = adj[i];
      if (u < 0 || u >= V) continue;
      const V3 d = x - load3(verts + u * 3);
      const float len = sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
      const float k = len == 0.0f ? 0.0f : 2.0f * (len - target) / len;
      s = s + d * k;
    }
    // a vertex without an edge gets zeros, whatever its mesh's count is: a mesh of vertices alone has 0 edges, and 0 * (1 / 0) is NaN
    const float w = end > begin ? g * mesh_weight(num_edges, vert_mesh[v], N) : 0.0f;
    store3(grad_verts + v * 3, s * w);
  }
}

// ---- mesh_laplacian_smoothing, method "uniform" ---------------------------------------------------------------------------------
// r_v = (sum of the neighbours, ascending) / deg(v) - x_v (the sum term is 0 for deg = 0: laplacian_matrices.py:52-66);
// term = |r_v| * weight; q_v = r_v weight / |r_v| (0 where the norm is 0) is kept for the backward.
__global__ __launch_bounds__(256) void laplacian_fwd_kernel(const float* __restrict__ verts, const int32_t* __restrict__ adj_offsets,
                                                            const int32_t* __restrict__ adj, const int32_t* __restrict__ vert_mesh,
                                                            const int32_t* __restrict__ num_verts, int64_t V, int64_t n_adj, int N,
                                                            float* __restrict__ q, float* __restrict__ partials) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float term = 0.0f;
  if (v < V) {
    int64_t begin, end;
    csr_row(adj_offsets, v, n_adj, begin, end);
    V3 s = mk(0.f, 0.f, 0.f);
    for (int64_t i = begin; i < end; ++i) s = s + vertex(verts, adj[i], V);
    const float deg = (float)(end - begin);
    if (end > begin) s = s / deg;
    const V3 r = s - load3(verts + v * 3);
    const float norm = norm3(r);
    const float w = mesh_weight(num_verts, vert_mesh[v], N);
    term = norm * w;
    const float k = norm == 0.0f ? 0.0f : w / norm;
    store3(q + v * 3, r * k);
  }
  const float s = block_sum_256(term);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// g_v = (g / N) (sum_{u in adj(v)} q_u / deg(u) - q_v): the transposed Laplacian as a second gather (the adjacency is symmetric).
__global__ __launch_bounds__(256) void laplacian_bwd_kernel(const float* __restrict__ grad_loss, const float* __restrict__ q,
                                                            const int32_t* __restrict__ adj_offsets, const int32_t* __restrict__ adj,
                                                            int64_t V, int64_t n_adj, int N, float* __restrict__ grad_verts) {
#pragma clang fp contract(fast)
  const float g = grad_loss[0] / (float)N;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    int64_t begin, end;
    csr_row(adj_offsets, v, n_adj, begin, end);
    V3 s = mk(0.f, 0.f, 0.f);
    for (int64_t i = begin; i < end; ++i) {
      const int64_t u = adj[i];
      if (u < 0 || u >= V) continue;
      int64_t ub, ue;
      csr_row(adj_offsets, u, n_adj, ub, ue);
      if (ue > ub) s = s + load3(q + u * 3) * (1.0f / (float)(ue - ub));
    }
    store3(grad_verts + v * 3, (s - load3(q + v * 3)) * g);
  }
}

// ---- mesh_normal_consistency ---------------------------------------------------------------------------------------------------
// A wing pair (v0, v1, a, b): n0 = (x_v1 - x_v0) x (x_a - x_v0), n1 = -((x_v1 - x_v0) x (x_b - x_v0)) (mesh_normal_consistency.py:113-125).
struct Wing {
  V3 e, p, q, n0, n1;
};
__device__ __forceinline__ Wing wing(const float* __restrict__ verts, const int32_t* __restrict__ pairs, int64_t i, int64_t V) {
  const V3 x0 = vertex(verts, pairs[i * 4 + 0], V);
  Wing w;
  w.e = vertex(verts, pairs[i * 4 + 1], V) - x0;
  w.p = vertex(verts, pairs[i * 4 + 2], V) - x0;
  w.q = vertex(verts, pairs[i * 4 + 3], V) - x0;
  w.n0 = cross(w.e, w.p);
  w.n1 = -cross(w.e, w.q);
  return w;
}

constexpr float kCosEps = 1e-8f;  // cosine_similarity's default eps

// torch.cosine_similarity(n0, n1, dim=1) of torch 2.x (ATen/native/Distance.cpp): each vector is divided by its own norm,
// clamped from below at eps, and the quotients are multiplied and summed: ((x1 / max(|x1|, eps)) * (x2 / max(|x2|, eps))).sum().
__global__ __launch_bounds__(256) void normal_consistency_fwd_kernel(const float* __restrict__ verts, const int32_t* __restrict__ pairs,
                                                                     const int32_t* __restrict__ pair_mesh,
                                                                     const int32_t* __restrict__ num_pairs, int64_t V, int64_t P, int N,
                                                                     float* __restrict__ partials) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float term = 0.0f;
  if (i < P) {
    const Wing w = wing(verts, pairs, i, V);
    const float c0 = fmaxf(norm3(w.n0), kCosEps), c1 = fmaxf(norm3(w.n1), kCosEps);
    const V3 a = w.n0 / c0, b = w.n1 / c1;
    const float cosine = a.x * b.x + a.y * b.y + a.z * b.z;
    term = (1.0f - cosine) * mesh_weight(num_pairs, pair_mesh[i], N);
  }
  const float s = block_sum_256(term);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// The gradient of a = x / c, c = max(|x|, eps), as autograd takes it through cosine_similarity: the clamp is applied to the VALUE of
// the norm under no_grad, so d a = d x / c - x (x . d x) / (|x| c^2), and the second term is absent where |x| == 0 (the norm's
// backward is masked there).  Where |x| >= eps this is the derivative of x / |x|.
__device__ __forceinline__ V3 unit_grad(V3 x, V3 up) {
#pragma clang fp contract(fast)
  const float n = norm3(x);
  const float c = fmaxf(n, kCosEps);
  const V3 direct = up * (1.0f / c);
  if (n == 0.0f) return direct;
  return direct - x * (dot(up, x) / (c * c * n));
}

// rows (P, 4, 3): the gradient of pair i to v0, v1, a, b.  With G0 / G1 the gradients of n0 / n1: n0 = e x p gives d e = p x G0,
// d p = G0 x e; n1 = -(e x q) gives d e += q x (-G1), d q = (-G1) x e; v1, a, b get d e, d p, d q and v0 minus their sum.
__global__ __launch_bounds__(256) void normal_consistency_bwd_rows_kernel(const float* __restrict__ grad_loss, const float* __restrict__ verts,
                                                                          const int32_t* __restrict__ pairs,
                                                                          const int32_t* __restrict__ pair_mesh,
                                                                          const int32_t* __restrict__ num_pairs, int64_t V, int64_t P, int N,
                                                                          float* __restrict__ rows) {
#pragma clang fp contract(fast)
  const float g = grad_loss[0] / (float)N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 256) {
    const Wing w = wing(verts, pairs, i, V);
    const float c0 = fmaxf(norm3(w.n0), kCosEps), c1 = fmaxf(norm3(w.n1), kCosEps);
    const float gc = -(g * mesh_weight(num_pairs, pair_mesh[i], N));  // d loss / d cosine
    const V3 a = w.n0 * (1.0f / c0), b = w.n1 * (1.0f / c1);
    const V3 G0 = unit_grad(w.n0, b * gc), H = -unit_grad(w.n1, a * gc);
    const V3 de = cross(w.p, G0) + cross(w.q, H), dp = cross(G0, w.e), dq = cross(H, w.e);
    float* out = rows + i * 12;
    store3(out + 0, -(de + dp + dq));
    store3(out + 3, de);
    store3(out + 6, dp);
    store3(out + 9, dq);
  }
}

size_t partial_bytes(int64_t n) { return n <= 0 ? 0 : (size_t)ceil_div(n, 256) * sizeof(float); }

// V and `per_item` entries for each of the n items (2 E adjacency entries, 4 P slots) must fit an int32
bool sizes_ok(int64_t V, int64_t n, int per_item, int N) { return V >= 0 && n >= 0 && N > 0 && V <= INT32_MAX && n <= INT32_MAX / per_item; }

int zero_grad(float* grad_verts, int64_t V, hipStream_t s) {
  return hipMemsetAsync(grad_verts, 0, (size_t)V * 3 * sizeof(float), s) == hipSuccess ? P3D_OK : P3D_ERR_LAUNCH;
}

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API size_t p3d_mesh_edge_loss_forward_workspace_bytes(int64_t E) { return partial_bytes(E); }
P3D_API size_t p3d_mesh_laplacian_forward_workspace_bytes(int64_t V) { return partial_bytes(V); }
P3D_API size_t p3d_mesh_normal_consistency_forward_workspace_bytes(int64_t P) { return partial_bytes(P); }
P3D_API size_t p3d_mesh_normal_consistency_backward_workspace_bytes(int64_t P) { return P <= 0 ? 0 : (size_t)P * 12 * sizeof(float); }

P3D_API int p3d_mesh_edge_loss_forward(const float* verts, const int32_t* edges, const int32_t* edge_mesh, const int32_t* num_edges,
                                       int64_t V, int64_t E, int N, float target_length, void* workspace, size_t workspace_bytes,
                                       float* loss, p3d_stream_t stream) {
  if (!sizes_ok(V, E, 2, N) || !loss) return P3D_ERR_INVALID_ARG;
  if (E > 0 && (!verts || !edges || !edge_mesh || !num_edges)) return P3D_ERR_INVALID_ARG;
  if (E > 0 && (!workspace || workspace_bytes < partial_bytes(E))) return P3D_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* partials = static_cast<float*>(workspace);
  LaunchScope ls("mesh_edge_loss_forward", s);
  if (E > 0)
    edge_loss_fwd_kernel<<<(unsigned)ceil_div(E, 256), 256, 0, s>>>(verts, edges, edge_mesh, num_edges, V, E, N, target_length, partials);
  segment_sum_kernel<<<1, 256, 0, s>>>(partials, ceil_div(E, 256), DivideByMeshes{N}, loss);
  return launch_status();
}

P3D_API int p3d_mesh_edge_loss_backward(const float* grad_loss, const float* verts, const int32_t* adj_offsets, const int32_t* adj,
                                        const int32_t* vert_mesh, const int32_t* num_edges, int64_t V, int64_t E, int N,
                                        float target_length, float* grad_verts, p3d_stream_t stream) {
  if (!sizes_ok(V, E, 2, N)) return P3D_ERR_INVALID_ARG;
  if (V == 0) return P3D_OK;
  if (!grad_verts) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (E == 0) return zero_grad(grad_verts, V, s);
  if (!grad_loss || !verts || !adj_offsets || !adj || !vert_mesh || !num_edges) return P3D_ERR_INVALID_ARG;
  LaunchScope ls("mesh_edge_loss_backward", s);
  edge_loss_bwd_kernel<<<stream_blocks(V), 256, 0, s>>>(grad_loss, verts, adj_offsets, adj, vert_mesh, num_edges, V, E * 2, N,
                                                        target_length, grad_verts);
  return launch_status();
}

P3D_API int p3d_mesh_laplacian_forward(const float* verts, const int32_t* adj_offsets, const int32_t* adj, const int32_t* vert_mesh,
                                       const int32_t* num_verts, int64_t V, int64_t E, int N, float* q, void* workspace,
                                       size_t workspace_bytes, float* loss, p3d_stream_t stream) {
  if (!sizes_ok(V, E, 2, N) || !loss) return P3D_ERR_INVALID_ARG;
  if (V > 0 && (!verts || !adj_offsets || !vert_mesh || !num_verts || !q || (E > 0 && !adj))) return P3D_ERR_INVALID_ARG;
  if (V > 0 && (!workspace || workspace_bytes < partial_bytes(V))) return P3D_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* partials = static_cast<float*>(workspace);
  LaunchScope ls("mesh_laplacian_forward", s);
  if (V > 0)
    laplacian_fwd_kernel<<<(unsigned)ceil_div(V, 256), 256, 0, s>>>(verts, adj_offsets, adj, vert_mesh, num_verts, V, E * 2, N, q, partials);
  segment_sum_kernel<<<1, 256, 0, s>>>(partials, ceil_div(V, 256), DivideByMeshes{N}, loss);
  return launch_status();
}

P3D_API int p3d_mesh_laplacian_backward(const float* grad_loss, const float* q, const int32_t* adj_offsets, const int32_t* adj, int64_t V,
                                        int64_t E, int N, float* grad_verts, p3d_stream_t stream) {
  if (!sizes_ok(V, E, 2, N)) return P3D_ERR_INVALID_ARG;
  if (V == 0) return P3D_OK;
  if (!grad_loss || !q || !adj_offsets || !grad_verts || (E > 0 && !adj)) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("mesh_laplacian_backward", s);
  laplacian_bwd_kernel<<<stream_blocks(V), 256, 0, s>>>(grad_loss, q, adj_offsets, adj, V, E * 2, N, grad_verts);
  return launch_status();
}

P3D_API int p3d_mesh_normal_consistency_forward(const float* verts, const int32_t* pairs, const int32_t* pair_mesh, const int32_t* num_pairs,
                                                int64_t V, int64_t P, int N, void* workspace, size_t workspace_bytes, float* loss,
                                                p3d_stream_t stream) {
  if (!sizes_ok(V, P, 4, N) || !loss) return P3D_ERR_INVALID_ARG;
  if (P > 0 && (!verts || !pairs || !pair_mesh || !num_pairs)) return P3D_ERR_INVALID_ARG;
  if (P > 0 && (!workspace || workspace_bytes < partial_bytes(P))) return P3D_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* partials = static_cast<float*>(workspace);
  LaunchScope ls("mesh_normal_consistency_forward", s);
  if (P > 0)
    normal_consistency_fwd_kernel<<<(unsigned)ceil_div(P, 256), 256, 0, s>>>(verts, pairs, pair_mesh, num_pairs, V, P, N, partials);
  segment_sum_kernel<<<1, 256, 0, s>>>(partials, ceil_div(P, 256), DivideByMeshes{N}, loss);
  return launch_status();
}

P3D_API int p3d_mesh_normal_consistency_backward(const float* grad_loss, const float* verts, const int32_t* pairs, const int32_t* pair_mesh,
                                                 const int32_t* num_pairs, const int32_t* offsets, const int32_t* slots, int64_t V, int64_t P,
                                                 int N, void* workspace, size_t workspace_bytes, float* grad_verts, p3d_stream_t stream) {
  if (!sizes_ok(V, P, 4, N)) return P3D_ERR_INVALID_ARG;
  if (V == 0) return P3D_OK;
  if (!grad_verts) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (P == 0) return zero_grad(grad_verts, V, s);
  if (!grad_loss || !verts || !pairs || !pair_mesh || !num_pairs || !offsets || !slots) return P3D_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < (size_t)P * 12 * sizeof(float)) return P3D_ERR_WORKSPACE;
  float* rows = static_cast<float*>(workspace);
  LaunchScope ls("mesh_normal_consistency_backward", s);
  normal_consistency_bwd_rows_kernel<<<stream_blocks(P), 256, 0, s>>>(grad_loss, verts, pairs, pair_mesh, num_pairs, V, P, N, rows);
  // one lane per vertex: +0 plus the rows of its slots (4 pair + role) in list order
  vert_gather_sum_kernel<MeshLosses, false, false><<<stream_blocks(V), 256, 0, s>>>(rows, offsets, slots, V, P * 4, grad_verts, nullptr);
  return launch_status();
}
