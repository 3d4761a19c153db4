// transform.hip -- world -> NDC vertex transform fused into the passes either side of the rasterizer.
//
// The reference's MeshRasterizer.transform (pytorch3d/renderer/mesh/rasterizer.py:171-216) runs, as torch ops on the
// padded (N, Vmax, 3) vertices: verts_view = world_to_view.transform_points(verts_world); verts_ndc = (projection o
// to_ndc).transform_points(verts_view); verts_ndc.z = verts_view.z -- two batched 4x4 products with homogeneous
// divides (transforms/transform3d.py:325-360), a slice assignment, padded <-> packed conversions, and the autograd
// twins of all of them.  SURVEY.md 8(f) row 3: here the transform happens INSIDE the face gather
// (p3d_transform_gather_face_verts: world vertices + faces + two 4x4 matrices per mesh -> NDC face_verts (F,3,3), one
// launch, no NDC vertex tensor, no padded layout), and its backward is one per-vertex kernel applied to the NDC vertex
// gradient that p3d_rasterize_meshes_backward_ex (faces given) has already reduced per vertex.  Cameras that are being
// optimised take p3d_transform_backward_cameras instead: the same per-vertex pass plus a two-stage segmented sum of the
// gradient of both matrices (below: "camera gradients"; tree depth 12 + ceil(R / 64)).
//
// Matrices follow the reference's row-vector convention: out_j = sum_i in_i * M[i][j] with in = (x, y, z, 1), then
// xyz / w.  matrices: (N, 2, 4, 4) f32 row-major: [n][0] world -> view, [n][1] view -> NDC (projection composed with
// the NDC conversion).  Arithmetic is plain float (tolerance-gated against the reference's bmm: 1e-5 on NDC).
#include "p3d_common.h"

namespace p3d {
namespace {

struct Mat4 {
  float m[16];
};

__device__ __forceinline__ void load_mats(const float* __restrict__ mats, int n, Mat4* A, Mat4* B) {
  const float4* s = reinterpret_cast<const float4*>(mats + (int64_t)n * 32);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 a = s[i], b = s[4 + i];
    A->m[4 * i] = a.x;
    A->m[4 * i + 1] = a.y;
    A->m[4 * i + 2] = a.z;
    A->m[4 * i + 3] = a.w;
    B->m[4 * i] = b.x;
    B->m[4 * i + 1] = b.y;
    B->m[4 * i + 2] = b.z;
    B->m[4 * i + 3] = b.w;
  }
}

// (x, y, z, 1) @ M
__device__ __forceinline__ void mul4(const Mat4& M, float x, float y, float z, float (&o)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = x * M.m[j] + y * M.m[4 + j] + z * M.m[8 + j] + M.m[12 + j];
}

struct NdcPoint {
  float x, y, z;          // NDC x, y and view-space depth
  float vh[4], nh[4];     // homogeneous view / NDC coordinates (for the backward)
};

__device__ __forceinline__ NdcPoint to_ndc(const Mat4& A, const Mat4& B, float px, float py, float pz) {
  NdcPoint r;
  mul4(A, px, py, pz, r.vh);
  const float vx = r.vh[0] / r.vh[3], vy = r.vh[1] / r.vh[3], vz = r.vh[2] / r.vh[3];
  mul4(B, vx, vy, vz, r.nh);
  r.x = r.nh[0] / r.nh[3];
  r.y = r.nh[1] / r.nh[3];
  r.z = vz;
  return r;
}

// index of the segment that holds `i`: the last n with first[n] <= i (first ascending, first[0] == 0)
__device__ __forceinline__ int segment_of(const int64_t* __restrict__ first, int N, int64_t i) {
  int lo = 0, hi = N - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first[mid] <= i)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void transform_gather_kernel(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                               const int64_t* __restrict__ face_first, const float* __restrict__ mats,
                                                               int64_t V, int64_t n_corners, int N, int mats_n,
                                                               float* __restrict__ face_verts) {
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n_corners; c += (int64_t)gridDim.x * 256) {
    const int n = segment_of(face_first, N, c / 3);
    Mat4 A, B;
    load_mats(mats, mats_n == 1 ? 0 : n, &A, &B);
    int64_t v = faces[c];
    if (v < 0) v += V;
    const bool ok = v >= 0 && v < V;
    const float* s = verts + (ok ? v : 0) * 3;
    const NdcPoint p = to_ndc(A, B, s[0], s[1], s[2]);
    const float nan = __int_as_float(0x7fc00000);
    float* d = face_verts + c * 3;
    d[0] = ok ? p.x : nan;
    d[1] = ok ? p.y : nan;
    d[2] = ok ? p.z : nan;
  }
}

__global__ __launch_bounds__(256) void transform_verts_kernel(const float* __restrict__ verts, const int64_t* __restrict__ vert_first,
                                                              const float* __restrict__ mats, int64_t V, int N, int mats_n,
                                                              float* __restrict__ verts_ndc) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    const int n = segment_of(vert_first, N, v);
    Mat4 A, B;
    load_mats(mats, mats_n == 1 ? 0 : n, &A, &B);
    const NdcPoint p = to_ndc(A, B, verts[v * 3], verts[v * 3 + 1], verts[v * 3 + 2]);
    verts_ndc[v * 3] = p.x;
    verts_ndc[v * 3 + 1] = p.y;
    verts_ndc[v * 3 + 2] = p.z;
  }
}

// gn = dL/d((view, 1) @ B), gh = dL/d((p, 1) @ A) for out = (X/W, Y/W, vz) with (X, Y, ., W) = (view, 1) @ B,
// view = ((p, 1) @ A).xyz / w
__device__ __forceinline__ void homogeneous_grads(const Mat4& B, const NdcPoint& p, float gx, float gy, float gz, float (&gn)[4],
                                                  float (&gh)[4]) {
  const float iw = 1.0f / p.nh[3];
  // gradient wrt the homogeneous NDC coordinates (its z component has no consumer: the depth comes from the view)
  gn[0] = gx * iw;
  gn[1] = gy * iw;
  gn[2] = 0.0f;
  gn[3] = -(gx * p.nh[0] + gy * p.nh[1]) * iw * iw;
  float gv[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) gv[i] = gn[0] * B.m[4 * i] + gn[1] * B.m[4 * i + 1] + gn[2] * B.m[4 * i + 2] + gn[3] * B.m[4 * i + 3];
  gv[2] += gz;
  const float ia = 1.0f / p.vh[3];
  gh[0] = gv[0] * ia;
  gh[1] = gv[1] * ia;
  gh[2] = gv[2] * ia;
  gh[3] = -(gv[0] * p.vh[0] + gv[1] * p.vh[1] + gv[2] * p.vh[2]) * ia * ia;
}

// grad_world = J^T grad_ndc: row i of A against gh
__device__ __forceinline__ float world_grad(const Mat4& A, const float (&gh)[4], int i) {
  return gh[0] * A.m[4 * i] + gh[1] * A.m[4 * i + 1] + gh[2] * A.m[4 * i + 2] + gh[3] * A.m[4 * i + 3];
}

__global__ __launch_bounds__(256) void transform_verts_backward_kernel(const float* __restrict__ verts,
                                                                       const int64_t* __restrict__ vert_first,
                                                                       const float* __restrict__ mats,
                                                                       const float* __restrict__ grad_ndc, int64_t V, int N,
                                                                       int mats_n, float* __restrict__ grad_world) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    const int n = segment_of(vert_first, N, v);
    Mat4 A, B;
    load_mats(mats, mats_n == 1 ? 0 : n, &A, &B);
    const NdcPoint p = to_ndc(A, B, verts[v * 3], verts[v * 3 + 1], verts[v * 3 + 2]);
    float gn[4], gh[4];
    homogeneous_grads(B, p, grad_ndc[v * 3], grad_ndc[v * 3 + 1], grad_ndc[v * 3 + 2], gn, gh);
#pragma unroll
    for (int i = 0; i < 3; ++i) grad_world[v * 3 + i] = world_grad(A, gh, i);
  }
}

// ---- camera gradients -------------------------------------------------------------------------------
// grad_A[n][i][j] = sum_v p_i * gh[j], grad_B[n][i][j] = sum_v view_i * gn[j] over the vertices v that share matrix n (p = (x, y, z,
// 1), view = (vx, vy, vz, 1); gn[2] == 0, so column 2 of grad_B is exactly 0).  Segments are contiguous in the packed order; the
// sum is a tree that only (V, first_idx, num_matrices) decide -- no float atomic, the same bits on every run and stream:
//   stage 1  a wave owns 64 consecutive packed vertices; a segmented inclusive scan (six rounds of lane shifts, cut where the mesh
//            changes) leaves the sum of a segment's part inside the wave in that part's last lane, which stores it as one row of
//            kCamRow floats.  Wave w's part of segment n goes to row w + n (row w when all vertices share one matrix): w and n both
//            only grow along the packed order, so the rows are distinct, a segment's rows are CONSECUTIVE, and the row number
//            itself says which segment it belongs to (no id array).  At most ceil(V / 64) + N rows.
//   stage 2  one block per matrix: 64 slots of 8 lanes, a lane per float4 column of the row (a wave's load is 8 whole rows).  Slot
//            s adds rows s, s + 64, s + 128, ... of its segment in ascending order, then a fixed six-round tree over the slots:
//            three rounds of lane shifts inside each wave, three over the eight waves through LDS.  An empty segment adds
//            nothing and stores zeros.
// DEPTH of the tree (additions on the longest path from one vertex's product to the output): 6 (stage 1) + ceil(R / 64) (a slot's
// chain in stage 2) + 6 (slot tree), R <= ceil(count / 64) + 1 the rows of the segment: 13 up to 4032 vertices of one matrix, 257 at
// a cloud of one million points.  rasterize_meshes.camera_grad_tree_depth restates it for the tests' tolerance.
constexpr int kCamRow = 32;  // grad_A (4, 4) then grad_B (4, 4), the layout of one matrix pair of grad_matrices
constexpr int kCamSums = 28;  // what is scanned: column 2 of grad_B is stored as zeros

__global__ __launch_bounds__(256) void camera_grad_partial_kernel(const float* __restrict__ verts, const int64_t* __restrict__ vert_first,
                                                                  const float* __restrict__ mats, const float* __restrict__ grad_ndc,
                                                                  int64_t V, int N, int mats_n, int64_t nwaves,
                                                                  float* __restrict__ grad_world, float4* __restrict__ rows) {
  const int lane = threadIdx.x & 63;
  for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < nwaves; w += (int64_t)gridDim.x * 4) {  // wave-uniform
    const int64_t v = w * kWave + lane;
    const bool valid = v < V;  // lane 0 always is
    int n = -1;                // lanes past the array: a segment of zeros that nobody stores
    float r[kCamSums];
#pragma unroll
    for (int i = 0; i < kCamSums; ++i) r[i] = 0.0f;
    if (valid) {
      n = mats_n == 1 ? 0 : segment_of(vert_first, N, v);
      Mat4 A, B;
      load_mats(mats, n, &A, &B);
      const float pw[3] = {verts[v * 3], verts[v * 3 + 1], verts[v * 3 + 2]};
      const NdcPoint p = to_ndc(A, B, pw[0], pw[1], pw[2]);
      float gn[4], gh[4];
      homogeneous_grads(B, p, grad_ndc[v * 3], grad_ndc[v * 3 + 1], grad_ndc[v * 3 + 2], gn, gh);
      if (grad_world) {
#pragma unroll
        for (int i = 0; i < 3; ++i) grad_world[v * 3 + i] = world_grad(A, gh, i);
      }
      const float view[3] = {p.vh[0] / p.vh[3], p.vh[1] / p.vh[3], p.z};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) r[4 * i + j] = i < 3 ? pw[i] * gh[j] : gh[j];
        r[16 + 3 * i] = i < 3 ? view[i] * gn[0] : gn[0];
        r[16 + 3 * i + 1] = i < 3 ? view[i] * gn[1] : gn[1];
        r[16 + 3 * i + 2] = i < 3 ? view[i] * gn[3] : gn[3];
      }
    }
    // the lane where this lane's segment starts inside the wave (the scan of ordered_sum.h's pass1_kernel and knn.hip's
    // knn_bwd_scatter_kernel, written out in each on purpose: a shared helper compiled pass1_kernel to more instructions, see there)
    const int below = __shfl_up(n, 1), above = __shfl_down(n, 1);
    const unsigned long long starts = __ballot(lane == 0 || below != n);
    const int start = 63 - __clzll((long long)(starts & ((2ull << lane) - 1ull)));
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const bool take = lane - d >= start;
#pragma unroll
      for (int i = 0; i < kCamSums; ++i) {
        const float t = __shfl_up(r[i], d);
        if (take) r[i] += t;
      }
    }
    if (valid && (lane == 63 || above != n)) {  // last lane of the segment's part in this wave
      float4* dst = rows + (w + n) * (kCamRow / 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        dst[i] = make_float4(r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]);
        dst[4 + i] = make_float4(r[16 + 3 * i], r[16 + 3 * i + 1], 0.0f, r[16 + 3 * i + 2]);
      }
    }
  }
}

__global__ __launch_bounds__(512) void camera_grad_reduce_kernel(const int64_t* __restrict__ vert_first, int64_t V, int N, int mats_n,
                                                                 const float4* __restrict__ rows, float* __restrict__ grad_mats) {
  __shared__ float4 part[8][kCamRow / 4];  // [wave][column]
  // 64 slots of 8 lanes, a lane per float4 column: one load of a wave reads 8 whole rows (1 KB in a piece)
  const int n = blockIdx.x, col = threadIdx.x & 7, slot = threadIdx.x >> 3, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the segment's vertices [b, e): whatever first_idx holds, the rows read below lie inside the workspace
  int64_t b = 0, e = V;
  if (mats_n != 1) {
    b = vert_first[n] < 0 ? 0 : (vert_first[n] > V ? V : vert_first[n]);
    if (n + 1 < N) e = vert_first[n + 1] > V ? V : vert_first[n + 1];
    if (e < b) e = b;
  }
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (e > b) {
    const int64_t shift = mats_n == 1 ? 0 : n;
    const int64_t r1 = (e - 1) / kWave + shift;
#pragma unroll 4  // (the loads of four rounds in flight; the additions keep their order)
    for (int64_t r = b / kWave + shift + slot; r <= r1; r += 64) {
      const float4 t = rows[r * (kCamRow / 4) + col];
      acc.x += t.x;
      acc.y += t.y;
      acc.z += t.z;
      acc.w += t.w;
    }
  }
  // the six rounds over the 64 slots: three inside the wave (slots 4, 2, 1 apart) ...
#pragma unroll
  for (int d = 32; d >= 8; d >>= 1) {
    acc.x += __shfl_down(acc.x, d);
    acc.y += __shfl_down(acc.y, d);
    acc.z += __shfl_down(acc.z, d);
    acc.w += __shfl_down(acc.w, d);
  }
  if (lane < 8) part[wave][col] = acc;
  __syncthreads();  // (every thread of the block arrives: nothing above returns)
  // ... and three over the eight waves, pairwise
  if (threadIdx.x < 8) {
    float4 p[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = part[k][col];
#pragma unroll
    for (int d = 4; d > 0; d >>= 1) {
#pragma unroll
      for (int k = 0; k < d; ++k) {
        p[k].x += p[k + d].x;
        p[k].y += p[k + d].y;
        p[k].z += p[k + d].z;
        p[k].w += p[k + d].w;
      }
    }
    float* dst = grad_mats + (int64_t)n * kCamRow + col * 4;
    dst[0] = p[0].x;
    dst[1] = p[0].y;
    dst[2] = p[0].z;
    dst[3] = p[0].w;
  }
}

inline int64_t camera_grad_rows(int64_t V, int N, int num_matrices) { return ceil_div(V, kWave) + (num_matrices == 1 ? 0 : N); }

inline unsigned blocks_for(int64_t n) {
  int64_t b = ceil_div(n, 256);
  if (b > 256 * 16) b = 256 * 16;
  return (unsigned)(b > 0 ? b : 1);
}

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API int p3d_transform_gather_face_verts(const float* verts_world, const int64_t* faces, const int64_t* mesh_to_face_first_idx,
                                            const float* matrices, int64_t V, int64_t F, int N, int num_matrices,
                                            float* face_verts, p3d_stream_t stream) {
  if (V < 0 || F < 0 || N < 0 || (num_matrices != 1 && num_matrices != N)) return P3D_ERR_INVALID_ARG;
  if (F == 0) return P3D_OK;
  if (!verts_world || !faces || !mesh_to_face_first_idx || !matrices || !face_verts || N == 0) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("transform_gather_face_verts", s);
  transform_gather_kernel<<<blocks_for(F * 3), 256, 0, s>>>(verts_world, faces, mesh_to_face_first_idx, matrices, V, F * 3, N,
                                                          num_matrices, face_verts);
  return launch_status();
}

P3D_API int p3d_transform_verts_forward(const float* verts_world, const int64_t* mesh_to_vert_first_idx, const float* matrices,
                                        int64_t V, int N, int num_matrices, float* verts_ndc, p3d_stream_t stream) {
  if (V < 0 || N < 0 || (num_matrices != 1 && num_matrices != N)) return P3D_ERR_INVALID_ARG;
  if (V == 0) return P3D_OK;
  if (!verts_world || !mesh_to_vert_first_idx || !matrices || !verts_ndc || N == 0) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("transform_verts", s);
  transform_verts_kernel<<<blocks_for(V), 256, 0, s>>>(verts_world, mesh_to_vert_first_idx, matrices, V, N, num_matrices, verts_ndc);
  return launch_status();
}

P3D_API int p3d_transform_verts_backward(const float* verts_world, const int64_t* mesh_to_vert_first_idx, const float* matrices,
                                         const float* grad_verts_ndc, int64_t V, int N, int num_matrices,
                                         float* grad_verts_world, p3d_stream_t stream) {
  if (V < 0 || N < 0 || (num_matrices != 1 && num_matrices != N)) return P3D_ERR_INVALID_ARG;
  if (V == 0) return P3D_OK;
  if (!verts_world || !mesh_to_vert_first_idx || !matrices || !grad_verts_ndc || !grad_verts_world || N == 0) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("transform_verts_bwd", s);
  transform_verts_backward_kernel<<<blocks_for(V), 256, 0, s>>>(verts_world, mesh_to_vert_first_idx, matrices, grad_verts_ndc, V, N,
                                                                 num_matrices, grad_verts_world);
  return launch_status();
}

P3D_API size_t p3d_transform_backward_workspace_bytes(int64_t V, int N, int num_matrices) {
  if (V <= 0 || N <= 0 || (num_matrices != 1 && num_matrices != N)) return 0;
  return align_up((size_t)camera_grad_rows(V, N, num_matrices) * kCamRow * sizeof(float), 256);
}

P3D_API int p3d_transform_backward_cameras(const float* verts_world, const int64_t* mesh_to_vert_first_idx, const float* matrices,
                                           const float* grad_verts_ndc, int64_t V, int N, int num_matrices, float* grad_verts_world,
                                           float* grad_matrices, void* workspace, size_t workspace_bytes, p3d_stream_t stream) {
  if (V < 0 || N < 0 || (num_matrices != 1 && num_matrices != N)) return P3D_ERR_INVALID_ARG;
  if (!grad_matrices && num_matrices > 0) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (V == 0) {  // nothing to sum: zeros, without a launch
    if (num_matrices > 0 && hipMemsetAsync(grad_matrices, 0, (size_t)num_matrices * kCamRow * sizeof(float), s) != hipSuccess)
      return P3D_ERR_LAUNCH;
    return P3D_OK;
  }
  if (!verts_world || !mesh_to_vert_first_idx || !matrices || !grad_verts_ndc || N == 0) return P3D_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < p3d_transform_backward_workspace_bytes(V, N, num_matrices) || ((uintptr_t)workspace & 15) != 0)
    return P3D_ERR_INVALID_ARG;
  const int64_t nwaves = ceil_div(V, kWave);
  int64_t blocks = ceil_div(nwaves, 4);
  if (blocks > 256 * 16) blocks = 256 * 16;
  float4* rows = static_cast<float4*>(workspace);
  {
    LaunchScope ls("transform_cameras_bwd_partial", s);
    camera_grad_partial_kernel<<<(unsigned)blocks, 256, 0, s>>>(verts_world, mesh_to_vert_first_idx, matrices, grad_verts_ndc, V, N,
                                                               num_matrices, nwaves, grad_verts_world, rows);
  }
  const int st = launch_status();
  if (st != P3D_OK) return st;
  {
    LaunchScope ls("transform_cameras_bwd_reduce", s);
    camera_grad_reduce_kernel<<<(unsigned)num_matrices, 512, 0, s>>>(mesh_to_vert_first_idx, V, N, num_matrices, rows, grad_matrices);
  }
  return launch_status();
}
