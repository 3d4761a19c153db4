// gather.hip -- the packed-vertex <-> per-face-vertex indexing step either side of the rasterizer.
//
// The reference does `face_verts = verts_packed[faces_packed]` in Python
// (pytorch3d/renderer/mesh/rasterize_meshes.py:144-148) and lets torch autograd scatter
// grad_face_verts back with index_put_(accumulate=True): on ROCm that backward is a radix sort of
// the 3F indices plus a segmented sum (~0.5 ms for 321k faces, 10% of a whole fwd+bwd step).
// Here both directions are one streaming kernel each; the scatter merges the corners of one vertex
// in LDS before it touches memory with hardware f32 atomics.
// SURVEY section 8(f) row 3; optional entry points, `pytorch3d._C` is unchanged.
#include "p3d_common.h"
#include "p3d_geom.h"
#include "face_gather.h"
#include "wave_table.h"

namespace p3d {
namespace {

// Indices follow torch indexing: a negative id wraps once (v + V).  torch device-asserts on ids still out of range;
// here nothing outside `verts` is ever touched and the face gets NaN coordinates (visible downstream, never silent
// garbage); the scatters drop such corners.
__global__ __launch_bounds__(256) void gather_faces_kernel(const float* __restrict__ verts,
                                                           const int64_t* __restrict__ faces, int64_t V, int64_t n_corners,
                                                           float* __restrict__ face_verts) {
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n_corners; c += (int64_t)gridDim.x * 256) {
    int64_t v = faces[c];
    if (v < 0) v += V;
    const bool ok = v >= 0 && v < V;
    const float* s = verts + (ok ? v : 0) * 3;
    float* d = face_verts + c * 3;
    const float nan = __int_as_float(0x7fc00000);
    d[0] = ok ? s[0] : nan;
    d[1] = ok ? s[1] : nan;
    d[2] = ok ? s[2] : nan;
  }
}

// The same gather with a thread per FACE, which also writes what the rasterizer's backward needs of the face alone
// (p3d_geom.h: BwdFacePre -- 1 / area and 1 / |edge|^2 x 3, 16 bytes): p3d_gather_face_verts_pre.
__global__ __launch_bounds__(256) void gather_faces_pre_kernel(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                               int64_t V, int64_t F, float* __restrict__ face_verts,
                                                               float4* __restrict__ face_pre) {
  for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < F; f += (int64_t)gridDim.x * 256) {
    float c[9];
    gather_face_corners(verts, faces, V, f, c);
    store_face(c, f, face_verts, face_pre);
  }
}

// A vertex is shared by ~6 faces that sit close together in the face list, so consecutive corners
// are merged in a wave-private LDS table (wave_table.h) first: one global atomic per (wave span,
// vertex, component) instead of one per (corner, component).
using VertTable = WaveTable<3, 426>;  // 4 waves x 426 x 24 B = 40 KB

__global__ __launch_bounds__(256) void scatter_face_grads_kernel(const float* __restrict__ grad_face_verts,
                                                                 const int64_t* __restrict__ faces, int64_t V,
                                                                 int64_t n_corners, int64_t span,
                                                                 float* __restrict__ grad_verts) {
  __shared__ __align__(16) int s_table[4][VertTable::kLdsInts];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t begin = ((int64_t)blockIdx.x * 4 + w) * span;
  if (begin >= n_corners) return;  // wave-uniform; no workgroup barrier in this kernel
  const int64_t end = begin + span < n_corners ? begin + span : n_corners;
  VertTable tab;
  tab.init(s_table[w], lane);
  for (int64_t base = begin; base < end; base += 64) {
    const int64_t c = base + lane;
    int v = -1;
    float g[3] = {0.f, 0.f, 0.f};
    if (c < end) {
      int64_t vi = faces[c];
      if (vi < 0) vi += V;
      v = (vi >= 0 && vi < V) ? (int)vi : -1;
      const float* s = grad_face_verts + c * 3;
      g[0] = s[0];
      g[1] = s[1];
      g[2] = s[2];
    }
    tab.add(grad_verts, lane, v, g);
  }
  if (tab.used > 0) tab.flush(grad_verts, lane);
}

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API int p3d_gather_face_verts(const float* verts, const int64_t* faces, int64_t V, int64_t F, float* face_verts,
                                  p3d_stream_t stream) {
  if (V < 0 || F < 0) return P3D_ERR_INVALID_ARG;
  if (F == 0) return P3D_OK;
  if (!verts || !faces || !face_verts) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = F * 3;
  int64_t blocks = ceil_div(n, 256);
  if (blocks > 256 * 16) blocks = 256 * 16;
  LaunchScope ls("gather_face_verts", s);
  gather_faces_kernel<<<(unsigned)blocks, 256, 0, s>>>(verts, faces, V, n, face_verts);
  return launch_status();
}

P3D_API int p3d_gather_face_verts_pre(const float* verts, const int64_t* faces, int64_t V, int64_t F, float* face_verts,
                                      float* face_pre, p3d_stream_t stream) {
  if (V < 0 || F < 0) return P3D_ERR_INVALID_ARG;
  if (F == 0) return P3D_OK;
  if (!verts || !faces || !face_verts || !face_pre || ((uintptr_t)face_pre & 15u)) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  int64_t blocks = ceil_div(F, 256);
  if (blocks > 256 * 16) blocks = 256 * 16;
  LaunchScope ls("gather_face_verts", s);
  gather_faces_pre_kernel<<<(unsigned)blocks, 256, 0, s>>>(verts, faces, V, F, face_verts, reinterpret_cast<float4*>(face_pre));
  return launch_status();
}

P3D_API int p3d_scatter_face_grads(const float* grad_face_verts, const int64_t* faces, int64_t V, int64_t F,
                                   float* grad_verts, p3d_stream_t stream) {
  if (V < 0 || F < 0) return P3D_ERR_INVALID_ARG;
  if (V == 0) return P3D_OK;
  if (!grad_verts) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(grad_verts, 0, (size_t)V * 3 * sizeof(float), s) != hipSuccess) return P3D_ERR_LAUNCH;
  if (F == 0) return P3D_OK;
  if (!grad_face_verts || !faces) return P3D_ERR_INVALID_ARG;
  const int64_t n = F * 3;
  int64_t waves = ceil_div(n, 1024);  // >= 1024 corners per wave
  if (waves > 4 * 4096) waves = 4 * 4096;
  const int64_t blocks = ceil_div(waves, 4);
  const int64_t span = ceil_div(ceil_div(n, blocks * 4), 64) * 64;
  LaunchScope ls("scatter_face_grads", s);
  scatter_face_grads_kernel<<<(unsigned)blocks, 256, 0, s>>>(grad_face_verts, faces, V, n, span, grad_verts);
  return launch_status();
}
