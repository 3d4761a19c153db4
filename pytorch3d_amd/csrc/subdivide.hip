// subdivide.hip -- SubdivideMeshes (the reference's pytorch3d/ops/subdivide_meshes.py: argsorts, a scatter_add of an arange, bincounts,
// two gathers per tensor and an index_put backward there) over the tables of mesh_edges.hip.  Contract: implicit_abi.h (p3di_subdivide_*).
//
//   faces_kernel     a lane per OUTPUT face row: its mesh by a binary search over face_first, then block k and face f of the mesh; the
//                    argsorts of the reference's _create_verts_index / _create_faces_index are this arithmetic.
//   forward_kernel   memory bound.  A lane per output element in output order (scalar form: D = 3 fills a wave with 21 rows), or per
//                    16 bytes (D % 4 == 0, aligned base and strides), so a wave reads whole rows across its lanes.  blockIdx.y picks
//                    the tensor (vertices, features), blockIdx.z the batch entry of the homogeneous form.
//   backward_kernel  the same split over grad_x: every lane gathers its vertex's rows of g in ascending edge order.  No atomic.
#include "implicit_abi.h"
#include "p3d_common.h"

namespace p3d {
namespace {

constexpr int kLanes = 256;
constexpr int kMaxGroups = P3D_SUBDIVIDE_MAX_GROUPS;

// the mesh of item x: the largest n < N with first(n) <= x (empty meshes are stepped over)
template <typename First>
__device__ __forceinline__ int mesh_of(First first, int N, int x) {
  int lo = 0, hi = N;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first(mid) <= x) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kLanes) void faces_kernel(const int64_t* __restrict__ faces, const int* __restrict__ face_edges,
                                                       const int* __restrict__ vert_first, const int* __restrict__ face_first,
                                                       const int* __restrict__ edge_first, int rows, int N,
                                                       int64_t* __restrict__ faces_local, int64_t* __restrict__ faces_packed) {
  const int o = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (o >= rows) return;
  const int n = mesh_of([&](int m) { return face_first[m]; }, N, o >> 2);
  const int ff = face_first[n], Fn = face_first[n + 1] - ff;
  if (Fn <= 0) return;  // tables that break their contract
  const int local = o - 4 * ff, k = local / Fn, f = ff + local - k * Fn;
  if (k > 3) return;
  const int64_t vf = vert_first[n], ef = edge_first[n], Vn = vert_first[n + 1] - vf;
  const int64_t e0 = Vn + face_edges[3 * f] - ef, e1 = Vn + face_edges[3 * f + 1] - ef, e2 = Vn + face_edges[3 * f + 2] - ef;
  int64_t a, b, c;
  if (k == 3) {
    a = e0, b = e1, c = e2;
  } else {
    a = faces[3 * (int64_t)f + k] - vf;
    b = k == 0 ? e2 : k == 1 ? e0 : e1;
    c = k == 0 ? e1 : k == 1 ? e2 : e0;
  }
  if (faces_local) {
    int64_t* p = faces_local + 3 * (int64_t)o;
    p[0] = a, p[1] = b, p[2] = c;
  }
  if (faces_packed) {
    int64_t* p = faces_packed + 3 * (int64_t)o;
    const int64_t first = vf + ef;
    p[0] = a + first, p[1] = b + first, p[2] = c + first;
  }
}

struct Job {
  const float* x;  // forward: the input through (sb, sr, se); backward: g, contiguous
  float* out;
  int64_t sb, sr, se;
  int D, vec;
};
struct Jobs {
  Job job[2];
};

struct Tables {
  const int* edges;        // forward
  const int* row_offsets;  // backward
  const int* hi_edges;     // backward
  const int* vert_first;
  const int* edge_first;
  int V, E, N;
};

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : x; }

template <typename T>
__device__ __forceinline__ T half_sum(T a, T b);
template <>
__device__ __forceinline__ float half_sum(float a, float b) { return (a + b) * 0.5f; }
template <>
__device__ __forceinline__ float4 half_sum(float4 a, float4 b) {
  return make_float4((a.x + b.x) * 0.5f, (a.y + b.y) * 0.5f, (a.z + b.z) * 0.5f, (a.w + b.w) * 0.5f);
}

// T = float: W = D elements of a row; T = float4: W = D / 4
template <typename T>
__device__ __forceinline__ void forward_rows(const Job& j, const Tables& t, int64_t b) {
  constexpr int kPer = sizeof(T) / sizeof(float);
  const int W = j.D / kPer, rows = t.V + t.E;
  const int64_t total = (int64_t)rows * W;
  const float* x = j.x + b * j.sb;
  T* out = reinterpret_cast<T*>(j.out + b * (int64_t)rows * j.D);
  for (int64_t idx = (int64_t)blockIdx.x * kLanes + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kLanes) {
    const int r = (int)(idx / W), c = (int)(idx - (int64_t)r * W);
    const int n = mesh_of([&](int m) { return t.vert_first[m] + t.edge_first[m]; }, t.N, r);
    const int vf = t.vert_first[n], ef = t.edge_first[n], local = r - vf - ef, Vn = t.vert_first[n + 1] - vf;
    const int64_t col = (int64_t)c * kPer * j.se;
    T v;
    if (local < Vn || t.E == 0) {
      v = *reinterpret_cast<const T*>(x + (int64_t)clampi(vf + local, 0, t.V - 1) * j.sr + col);
    } else {
      const int e = clampi(ef + local - Vn, 0, t.E - 1);
      const int lo = clampi(t.edges[2 * e], 0, t.V - 1), hi = clampi(t.edges[2 * e + 1], 0, t.V - 1);
      v = half_sum(*reinterpret_cast<const T*>(x + (int64_t)lo * j.sr + col), *reinterpret_cast<const T*>(x + (int64_t)hi * j.sr + col));
    }
    out[idx] = v;
  }
}

__global__ __launch_bounds__(kLanes) void forward_kernel(Jobs jobs, Tables t) {
  const Job j = blockIdx.y ? jobs.job[1] : jobs.job[0];
  if (j.vec)
    forward_rows<float4>(j, t, blockIdx.z);
  else
    forward_rows<float>(j, t, blockIdx.z);
}

__device__ __forceinline__ void add_to(float& a, float b) { a += b; }
__device__ __forceinline__ void add_to(float4& a, float4 b) { a.x += b.x, a.y += b.y, a.z += b.z, a.w += b.w; }
__device__ __forceinline__ float own_plus_half(float g, float a) { return g + 0.5f * a; }
__device__ __forceinline__ float4 own_plus_half(float4 g, float4 a) {
  return make_float4(g.x + 0.5f * a.x, g.y + 0.5f * a.y, g.z + 0.5f * a.z, g.w + 0.5f * a.w);
}
template <typename T>
__device__ __forceinline__ T zero_of();
template <>
__device__ __forceinline__ float zero_of() { return 0.0f; }
template <>
__device__ __forceinline__ float4 zero_of() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

template <typename T>
__device__ __forceinline__ void backward_rows(const Job& j, const Tables& t, int64_t b) {
  constexpr int kPer = sizeof(T) / sizeof(float);
  const int W = j.D / kPer, rows = t.V + t.E;
  const int64_t total = (int64_t)t.V * W;
  const T* g = reinterpret_cast<const T*>(j.x + b * (int64_t)rows * j.D);
  T* out = reinterpret_cast<T*>(j.out + b * (int64_t)t.V * j.D);
  for (int64_t idx = (int64_t)blockIdx.x * kLanes + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kLanes) {
    const int v = (int)(idx / W), c = (int)(idx - (int64_t)v * W);
    const int n = mesh_of([&](int m) { return t.vert_first[m]; }, t.N, v);
    const int edge_rows = t.vert_first[n + 1];  // row(e) = e + vert_first[n + 1], row(v) = v + edge_first[n]
    T acc = zero_of<T>();
    const int h0 = clampi(t.row_offsets[t.V + v] - t.E, 0, t.E), h1 = clampi(t.row_offsets[t.V + v + 1] - t.E, h0, t.E);
    for (int p = h0; p < h1; ++p) add_to(acc, g[(int64_t)clampi(t.hi_edges[p] + edge_rows, 0, rows - 1) * W + c]);
    const int l0 = clampi(t.row_offsets[v], 0, t.E), l1 = clampi(t.row_offsets[v + 1], l0, t.E);
    for (int e = l0; e < l1; ++e) add_to(acc, g[(int64_t)clampi(e + edge_rows, 0, rows - 1) * W + c]);
    out[idx] = own_plus_half(g[(int64_t)clampi(v + t.edge_first[n], 0, rows - 1) * W + c], acc);
  }
}

__global__ __launch_bounds__(kLanes) void backward_kernel(Jobs jobs, Tables t) {
  const Job j = blockIdx.y ? jobs.job[1] : jobs.job[0];
  if (j.vec)
    backward_rows<float4>(j, t, blockIdx.z);
  else
    backward_rows<float>(j, t, blockIdx.z);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

unsigned groups_for(const Jobs& jobs, int njobs, int64_t rows) {
  int64_t most = 1;
  for (int i = 0; i < njobs; ++i) {
    const int64_t items = rows * (jobs.job[i].vec ? jobs.job[i].D / 4 : jobs.job[i].D);
    if (items > most) most = items;
  }
  const int64_t groups = ceil_div(most, kLanes);
  return (unsigned)(groups > kMaxGroups ? kMaxGroups : groups);
}

bool sizes_ok(int64_t V, int64_t E, int64_t N, int64_t B, int64_t D0, int64_t D1) {
  return V >= 0 && E >= 0 && N >= 1 && N < INT32_MAX && B >= 0 && B <= 65535 && V + E < INT32_MAX && D0 >= 0 && D1 >= 0 && D0 <= INT32_MAX &&
         D1 <= INT32_MAX;
}

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API int p3di_subdivide_faces(const int64_t* faces, const int32_t* face_edges, const int32_t* vert_first, const int32_t* face_first,
                                 const int32_t* edge_first, int64_t F, int64_t N, int64_t* faces_local, int64_t* faces_packed,
                                 p3d_stream_t stream) {
  if (F < 0 || N < 1 || N >= INT32_MAX || 4 * F > INT32_MAX / 3) return P3D_ERR_INVALID_ARG;
  if (F == 0 || (!faces_local && !faces_packed)) return P3D_OK;
  if (!faces || !face_edges || !vert_first || !face_first || !edge_first) return P3D_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  LaunchScope ls("subdivide_faces", st);
  faces_kernel<<<(unsigned)ceil_div(4 * F, kLanes), kLanes, 0, st>>>(faces, face_edges, vert_first, face_first, edge_first, (int)(4 * F),
                                                                     (int)N, faces_local, faces_packed);
  return launch_status();
}

P3D_API int p3di_subdivide_forward(const float* x0, const int64_t strides0[3], int64_t D0, float* out0, const float* x1,
                                   const int64_t strides1[3], int64_t D1, float* out1, const int32_t* edges, const int32_t* vert_first,
                                   const int32_t* edge_first, int64_t V, int64_t E, int64_t N, int64_t B, p3d_stream_t stream) {
  if (!sizes_ok(V, E, N, B, D0, D1) || !strides0 || (x1 && !strides1)) return P3D_ERR_INVALID_ARG;
  if (!x1) D1 = 0;
  if (B == 0 || V + E == 0 || (D0 == 0 && D1 == 0)) return P3D_OK;
  if (V == 0 || (D0 > 0 && (!x0 || !out0)) || (D1 > 0 && (!x1 || !out1)) || (E > 0 && !edges) || !vert_first || !edge_first)
    return P3D_ERR_INVALID_ARG;
  Jobs jobs;
  int njobs = 0;
  const float* xs[2] = {x0, x1};
  float* outs[2] = {out0, out1};
  const int64_t* strides[2] = {strides0, strides1};
  const int64_t Ds[2] = {D0, D1};
  for (int i = 0; i < 2; ++i) {
    if (Ds[i] == 0) continue;
    const int64_t* s = strides[i];
    if (s[0] < 0 || s[1] < 0 || s[2] < 0) return P3D_ERR_INVALID_ARG;
    Job& j = jobs.job[njobs++];
    j.x = xs[i], j.out = outs[i], j.sb = s[0], j.sr = s[1], j.se = s[2], j.D = (int)Ds[i];
    j.vec = Ds[i] % 4 == 0 && s[2] == 1 && s[1] % 4 == 0 && s[0] % 4 == 0 && aligned16(xs[i]) && aligned16(outs[i]);
  }
  const Tables t = {edges, nullptr, nullptr, vert_first, edge_first, (int)V, (int)E, (int)N};
  hipStream_t st = (hipStream_t)stream;
  LaunchScope ls("subdivide_forward", st);
  forward_kernel<<<dim3(groups_for(jobs, njobs, V + E), (unsigned)njobs, (unsigned)B), kLanes, 0, st>>>(jobs, t);
  return launch_status();
}

P3D_API int p3di_subdivide_backward(const float* g0, int64_t D0, float* grad_x0, const float* g1, int64_t D1, float* grad_x1,
                                    const int32_t* row_offsets, const int32_t* hi_edges, const int32_t* vert_first,
                                    const int32_t* edge_first, int64_t V, int64_t E, int64_t N, int64_t B, p3d_stream_t stream) {
  if (!sizes_ok(V, E, N, B, D0, D1)) return P3D_ERR_INVALID_ARG;
  if (!grad_x0) D0 = 0;
  if (!grad_x1) D1 = 0;
  if (B == 0 || V == 0 || (D0 == 0 && D1 == 0)) return P3D_OK;
  if ((D0 > 0 && !g0) || (D1 > 0 && !g1) || !row_offsets || (E > 0 && !hi_edges) || !vert_first || !edge_first) return P3D_ERR_INVALID_ARG;
  Jobs jobs;
  int njobs = 0;
  const float* gs[2] = {g0, g1};
  float* outs[2] = {grad_x0, grad_x1};
  const int64_t Ds[2] = {D0, D1};
  for (int i = 0; i < 2; ++i) {
    if (Ds[i] == 0) continue;
    Job& j = jobs.job[njobs++];
    j.x = gs[i], j.out = outs[i], j.sb = 0, j.sr = Ds[i], j.se = 1, j.D = (int)Ds[i];
    j.vec = Ds[i] % 4 == 0 && aligned16(gs[i]) && aligned16(outs[i]);
  }
  const Tables t = {nullptr, row_offsets, hi_edges, vert_first, edge_first, (int)V, (int)E, (int)N};
  hipStream_t st = (hipStream_t)stream;
  LaunchScope ls("subdivide_backward", st);
  backward_kernel<<<dim3(groups_for(jobs, njobs, V), (unsigned)njobs, (unsigned)B), kLanes, 0, st>>>(jobs, t);
  return launch_status();
}
