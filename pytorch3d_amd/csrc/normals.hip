// normals.hip -- face areas / normals and area-weighted vertex normals of a packed mesh batch, forward and backward.
//
// The reference computes face areas and normals with a kernel pair of its own (csrc/face_areas_normals/face_areas_normals.cu)
// and vertex normals as a torch chain in Python (structures/meshes.py:884-926: gather, cross product, three index_add with float
// atomics, F.normalize; about twice that again in autograd, ending in index_put_(accumulate=True) -- a radix sort on ROCm, see
// gather.hip).  Here:
//   * face areas / normals: one thread per face each way; the backward writes the (F, 3, 3) per-corner gradients and the host
//     finishes with p3d_scatter_face_grads[_ordered] (gather.hip / ordered_bwd.hip): no scatter code in this file;
//   * vertex normals in GATHER form: the host sorts the corners by vertex once per topology (an incidence list: offsets (V + 1),
//     corners (<= 3 F)); a per-face kernel stores each face's contribution with plain stores and a per-vertex kernel sums the rows
//     of its list in list order.  No float atomic anywhere: the result is a pure function of verts, faces and the list, with the
//     same bits on every run, stream and process.  The backward has the same two-kernel shape.
// IEEE sqrt and division throughout (no rsqrt, no rcp): the forwards are compared with the reference at 1e-6 and below.
#include "csr_gather.h"

namespace p3d {
namespace {

struct Normals;  // this translation unit's instances of vert_gather_sum_kernel

__device__ __forceinline__ V3 unit(int d) { return mk(d == 0 ? 1.f : 0.f, d == 1 ? 1.f : 0.f, d == 2 ? 1.f : 0.f); }

// A vertex id as torch indexing reads it (a negative id wraps once); -1 when it is still outside [0, V).
__device__ __forceinline__ int64_t vertex_id(const int64_t* __restrict__ faces, int64_t corner, int64_t V) {
  int64_t v = faces[corner];
  if (v < 0) v += V;
  return (v >= 0 && v < V) ? v : -1;
}

// The vertex of a corner, as gather_faces_kernel (gather.hip) returns it: nothing outside `verts` is read, an id out of range
// gives NaN coordinates (visible downstream, never silent garbage).
__device__ __forceinline__ V3 corner_vertex(const float* __restrict__ verts, int64_t v) {
  if (v < 0) return mk(quiet_nan(), quiet_nan(), quiet_nan());
  return load3(verts + v * 3);
}

// ---- face areas and normals ----------------------------------------------------------------------------------------------------
// c = (v1 - v0) x (v2 - v0), area = |c| / 2, normal = c / max(|c|, 1e-6): the reference's expression order (face_areas_normals.cu:45-62).
__global__ __launch_bounds__(256) void face_areas_normals_fwd_kernel(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                                     int64_t V, int64_t F, float* __restrict__ areas,
                                                                     float* __restrict__ normals) {
  for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < F; f += (int64_t)gridDim.x * 256) {
    const V3 v0 = corner_vertex(verts, vertex_id(faces, f * 3 + 0, V));
    const V3 v1 = corner_vertex(verts, vertex_id(faces, f * 3 + 1, V));
    const V3 v2 = corner_vertex(verts, vertex_id(faces, f * 3 + 2, V));
    const V3 c = cross(v1 - v0, v2 - v0);
    float norm = norm3(c);
    areas[f] = norm / 2.0f;
    norm = norm < kNormEps ? kNormEps : norm;
    store3(normals + f * 3, c / norm);
  }
}

// With t = dc / d(vertex coordinate) and s = t . c (pytorch3d_amd/_aux_ops.py: face_areas_normals_backward):
//     grad = grad_area s / (2 |c|) + sum_j grad_normal_j (t_j - c_j s / |c|^2) / |c|                 (|c| clamped at 1e-6)
// t = e_d x b for v1, a x e_d for v2 and minus their sum for v0 (a = v1 - v0, b = v2 - v0).  ONE deviation from the derivative is kept
// because the reference has it: in d / d(v1.z) the j = y term multiplies by c_x (face_areas_normals.cu:183-184).
__global__ __launch_bounds__(256) void face_areas_normals_bwd_kernel(const float* __restrict__ grad_areas,
                                                                     const float* __restrict__ grad_normals,
                                                                     const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                                     int64_t V, int64_t F, float* __restrict__ grad_face_verts) {
  for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < F; f += (int64_t)gridDim.x * 256) {
    const V3 v0 = corner_vertex(verts, vertex_id(faces, f * 3 + 0, V));
    const V3 v1 = corner_vertex(verts, vertex_id(faces, f * 3 + 1, V));
    const V3 v2 = corner_vertex(verts, vertex_id(faces, f * 3 + 2, V));
    const V3 a = v1 - v0, b = v2 - v0;
    const V3 c = cross(a, b);
    float norm = norm3(c);
    norm = norm < kNormEps ? kNormEps : norm;
    const float inv = 1.0f / norm;
    const float inv2 = inv * inv;
    const float ga_half_inv = grad_areas[f] * (0.5f * inv);
    const V3 gn = load3(grad_normals + f * 3);
    float* out = grad_face_verts + f * 9;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const V3 t1 = cross(unit(d), b), t2 = cross(a, unit(d));
      const V3 t0 = -(t1 + t2);
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const V3 t = p == 0 ? t0 : p == 1 ? t1 : t2;
        const float s = dot(t, c);
        const float k = s * inv2;
        const float cy = (p == 1 && d == 2) ? c.x : c.y;  // the reference's c_x in place of c_y
        const V3 dn = mk((t.x - c.x * k) * inv, (t.y - cy * k) * inv, (t.z - c.z * k) * inv);
        out[p * 3 + d] = ga_half_inv * s + dot(dn, gn);
      }
    }
  }
}

// ---- vertex normals ------------------------------------------------------------------------------------------------------------
// (a) a face's contribution to each of its three vertices (structures/meshes.py:907-911): (v2 - v1) x (v0 - v1), once per face.
__global__ __launch_bounds__(256) void vert_normals_face_raw_kernel(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                                    int64_t V, int64_t F, float* __restrict__ face_raw) {
  for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < F; f += (int64_t)gridDim.x * 256) {
    const V3 v0 = corner_vertex(verts, vertex_id(faces, f * 3 + 0, V));
    const V3 v1 = corner_vertex(verts, vertex_id(faces, f * 3 + 1, V));
    const V3 v2 = corner_vertex(verts, vertex_id(faces, f * 3 + 2, V));
    store3(face_raw + f * 3, cross(v2 - v1, v0 - v1));
  }
}

// (b) / (d) one lane per vertex: vert_gather_sum_kernel (csr_gather.h) over the vertex's corners in list order.  Forward: PER_FACE
// (the row of a corner is its face's, face_raw (F, 3)) and NORMALIZE; backward: the corner's own row (face_rows (3 F, 3)).

// The gradient of n = s / max(|s|, 1e-6) at one vertex: g / 1e-6 where the clamp holds (what autograd gives for
// x / clamp_min(norm, eps) there), (g - n (n . g)) / |s| where it does not.  The clamp is tested as the forward tests it
// (norm < eps), so a NaN sum -- a vertex that shares a face with an id out of range -- takes the regular branch and stays NaN in
// every gradient it reaches.  A corner whose vertex is out of range is in no list: it contributes nothing.
__device__ __forceinline__ V3 normalize_grad(const float* __restrict__ sums, const float* __restrict__ grad_normals, int64_t v) {
  if (v < 0) return mk(0.f, 0.f, 0.f);
  const V3 s = load3(sums + v * 3), g = load3(grad_normals + v * 3);
  const float norm = norm3(s);
  if (norm < kNormEps) return g / kNormEps;
  const V3 n = s / norm;
  const float ng = dot(n, g);
  return (g - n * ng) / norm;
}

// (c) per face: G = the sum of its three vertices' sum-gradients in corner order (the face's contribution went to all three), then
// the cross product's backward with a = v2 - v1, b = v0 - v1: grad_v2 = b x G, grad_v0 = G x a, grad_v1 = -(grad_v0 + grad_v2).
__global__ __launch_bounds__(256) void vert_normals_face_rows_kernel(const float* __restrict__ grad_normals, const float* __restrict__ verts,
                                                                     const int64_t* __restrict__ faces, const float* __restrict__ sums,
                                                                     int64_t V, int64_t F, float* __restrict__ face_rows) {
  for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < F; f += (int64_t)gridDim.x * 256) {
    const int64_t i0 = vertex_id(faces, f * 3 + 0, V), i1 = vertex_id(faces, f * 3 + 1, V), i2 = vertex_id(faces, f * 3 + 2, V);
    const V3 v0 = corner_vertex(verts, i0), v1 = corner_vertex(verts, i1), v2 = corner_vertex(verts, i2);
    const V3 G = normalize_grad(sums, grad_normals, i0) + normalize_grad(sums, grad_normals, i1) + normalize_grad(sums, grad_normals, i2);
    const V3 a = v2 - v1, b = v0 - v1;
    const V3 g2 = cross(b, G), g0 = cross(G, a);
    float* out = face_rows + f * 9;
    store3(out + 0, g0);
    store3(out + 3, -(g0 + g2));
    store3(out + 6, g2);
  }
}

// V == 0 with faces: every id is out of range, every face NaN -- a fill, no kernel
int fill_nan(float* p, int64_t n, hipStream_t s) {
  return hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p), 0x7fc00000, (size_t)n, s) == hipSuccess ? P3D_OK : P3D_ERR_LAUNCH;
}

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API int p3d_face_areas_normals_forward(const float* verts, const int64_t* faces, int64_t V, int64_t F, float* areas, float* normals,
                                           p3d_stream_t stream) {
  if (V < 0 || F < 0) return P3D_ERR_INVALID_ARG;
  if (F == 0) return P3D_OK;
  if (!areas || !normals) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (V == 0) {
    const int st = fill_nan(areas, F, s);
    return st != P3D_OK ? st : fill_nan(normals, F * 3, s);
  }
  if (!verts || !faces) return P3D_ERR_INVALID_ARG;
  LaunchScope ls("face_areas_normals_forward", s);
  face_areas_normals_fwd_kernel<<<stream_blocks(F), 256, 0, s>>>(verts, faces, V, F, areas, normals);
  return launch_status();
}

P3D_API int p3d_face_areas_normals_backward(const float* grad_areas, const float* grad_normals, const float* verts, const int64_t* faces,
                                            int64_t V, int64_t F, float* grad_face_verts, p3d_stream_t stream) {
  if (V < 0 || F < 0) return P3D_ERR_INVALID_ARG;
  if (F == 0) return P3D_OK;
  if (!grad_face_verts) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (V == 0) return fill_nan(grad_face_verts, F * 9, s);
  if (!grad_areas || !grad_normals || !verts || !faces) return P3D_ERR_INVALID_ARG;
  LaunchScope ls("face_areas_normals_backward", s);
  face_areas_normals_bwd_kernel<<<stream_blocks(F), 256, 0, s>>>(grad_areas, grad_normals, verts, faces, V, F, grad_face_verts);
  return launch_status();
}

P3D_API size_t p3d_verts_normals_forward_workspace_bytes(int64_t F) { return F < 0 ? 0 : (size_t)F * 3 * sizeof(float); }
P3D_API size_t p3d_verts_normals_backward_workspace_bytes(int64_t F) { return F < 0 ? 0 : (size_t)F * 9 * sizeof(float); }

P3D_API int p3d_verts_normals_forward(const float* verts, const int64_t* faces, const int32_t* offsets, const int32_t* corners, int64_t V,
                                      int64_t F, float* face_raw, float* sums, float* normals, p3d_stream_t stream) {
  if (V < 0 || F < 0 || F * 3 > INT32_MAX) return P3D_ERR_INVALID_ARG;
  if (V == 0) return P3D_OK;
  if (!verts || !sums || !normals) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (F == 0) {  // every vertex is without a face: zeros
    if (hipMemsetAsync(sums, 0, (size_t)V * 3 * sizeof(float), s) != hipSuccess) return P3D_ERR_LAUNCH;
    return hipMemsetAsync(normals, 0, (size_t)V * 3 * sizeof(float), s) == hipSuccess ? P3D_OK : P3D_ERR_LAUNCH;
  }
  if (!faces || !offsets || !corners) return P3D_ERR_INVALID_ARG;
  if (!face_raw) return P3D_ERR_WORKSPACE;
  LaunchScope ls("verts_normals_forward", s);
  vert_normals_face_raw_kernel<<<stream_blocks(F), 256, 0, s>>>(verts, faces, V, F, face_raw);
  vert_gather_sum_kernel<Normals, true, true><<<stream_blocks(V), 256, 0, s>>>(face_raw, offsets, corners, V, F * 3, sums, normals);
  return launch_status();
}

P3D_API int p3d_verts_normals_backward(const float* grad_normals, const float* verts, const int64_t* faces, const float* sums,
                                       const int32_t* offsets, const int32_t* corners, int64_t V, int64_t F, float* face_rows,
                                       float* grad_verts, p3d_stream_t stream) {
  if (V < 0 || F < 0 || F * 3 > INT32_MAX) return P3D_ERR_INVALID_ARG;
  if (V == 0) return P3D_OK;
  if (!grad_verts) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (F == 0) return hipMemsetAsync(grad_verts, 0, (size_t)V * 3 * sizeof(float), s) == hipSuccess ? P3D_OK : P3D_ERR_LAUNCH;
  if (!grad_normals || !verts || !faces || !sums || !offsets || !corners) return P3D_ERR_INVALID_ARG;
  if (!face_rows) return P3D_ERR_WORKSPACE;
  LaunchScope ls("verts_normals_backward", s);
  vert_normals_face_rows_kernel<<<stream_blocks(F), 256, 0, s>>>(grad_normals, verts, faces, sums, V, F, face_rows);
  vert_gather_sum_kernel<Normals, false, false><<<stream_blocks(V), 256, 0, s>>>(face_rows, offsets, corners, V, F * 3, grad_verts, nullptr);
  return launch_status();
}
