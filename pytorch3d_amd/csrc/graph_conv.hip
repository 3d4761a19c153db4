// graph_conv.hip -- per-vertex sums of neighbour rows through an inverted index (pytorch3d/ops/graph_conv.py: gather_scatter, the
// neighbour sum of GraphConv; the reference's gather_scatter.cu adds with one float atomic per edge and channel into a zero-filled
// output).  include/p3d_amd.h has the contract; DESIGN.md 8.19.
//
//   out[v, :] = (base ? base[v, :] : +0.0f) + (((+0.0f + rows[e_0, :]) + rows[e_1, :]) + ...)     e_i = entries[offsets[v] + i]
//
// The same kernel serves the forward (the table of a vertex's neighbours) and the backward (the transposed table; one table for an
// undirected graph).  No atomic, no zero fill, no workspace: every (v, d) is summed by one lane in list order, so the bits do not
// depend on the launch shape, the run or the stream.
//
// Lanes run along the feature dimension: a neighbour's row is one coalesced request.  lanes_per_row = min(64, next_pow2(units)),
// units = D / 4 float4s or D dwords; a wave serves 64 / lanes_per_row vertices, a row wider than one wave pass is walked in column
// blocks.  The loads of four neighbours are issued before the four adds; the adds stay in list order.  An entry outside [0, n_rows)
// is skipped (its load is redirected to row 0 and the sum keeps its value), offsets are clamped by csr_row: a broken table gives wrong
// sums, never a read outside the arrays.  A long row (the hub of a general graph) is summed by its lanes alone, sequentially.
#include "p3d_common.h"
#include "csr_gather.h"

namespace p3d {
namespace {

struct NeighborSum {
  const float* rows;
  const float* base;  // or nullptr
  const int32_t* offsets;
  const int32_t* entries;
  float* out;
  int64_t rows_stride, base_stride, out_stride;
  int64_t n_rows, V, n_entries;  // n_entries == 0: offsets and entries are not read
  int64_t units;                 // float4s (VEC) or dwords per row
  int lpr_log2;                  // log2(lanes per row)
};

template <bool VEC>
struct Cols;
template <>
struct Cols<true> {
  using T = float4;
  static constexpr int kWidth = 4;
  static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ T add(T a, T b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
  static __device__ __forceinline__ T load(const float* p) { return *reinterpret_cast<const float4*>(p); }
  static __device__ __forceinline__ void store(float* p, T v) { *reinterpret_cast<float4*>(p) = v; }
};
template <>
struct Cols<false> {
  using T = float;
  static constexpr int kWidth = 1;
  static __device__ __forceinline__ T zero() { return 0.f; }
  static __device__ __forceinline__ T add(T a, T b) { return a + b; }
  static __device__ __forceinline__ T load(const float* p) { return *p; }
  static __device__ __forceinline__ void store(float* p, T v) { *p = v; }
};

template <bool VEC>
__global__ __launch_bounds__(256) void neighbor_sum_kernel(NeighborSum p) {
  using C = Cols<VEC>;
  using T = typename C::T;
  const int lpr = 1 << p.lpr_log2;
  const int lane = threadIdx.x & (lpr - 1);
  const int64_t rows_per_group = 256 >> p.lpr_log2;
  const int64_t groups = (p.V + rows_per_group - 1) >> (8 - p.lpr_log2);
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t v = g * rows_per_group + (threadIdx.x >> p.lpr_log2);
    if (v >= p.V) continue;
    int64_t begin = 0, end = 0;
    if (p.n_entries > 0) csr_row(p.offsets, v, p.n_entries, begin, end);
    for (int64_t u = lane; u < p.units; u += lpr) {
      const int64_t col = u * C::kWidth;
      const float* src = p.rows + col;
      T acc = C::zero();
      int64_t i = begin;
      for (; i + 4 <= end; i += 4) {
        const int64_t c0 = p.entries[i], c1 = p.entries[i + 1], c2 = p.entries[i + 2], c3 = p.entries[i + 3];
        const bool k0 = c0 >= 0 && c0 < p.n_rows, k1 = c1 >= 0 && c1 < p.n_rows, k2 = c2 >= 0 && c2 < p.n_rows, k3 = c3 >= 0 && c3 < p.n_rows;
        const T x0 = C::load(src + (k0 ? c0 : 0) * p.rows_stride), x1 = C::load(src + (k1 ? c1 : 0) * p.rows_stride);
        const T x2 = C::load(src + (k2 ? c2 : 0) * p.rows_stride), x3 = C::load(src + (k3 ? c3 : 0) * p.rows_stride);
        acc = k0 ? C::add(acc, x0) : acc;
        acc = k1 ? C::add(acc, x1) : acc;
        acc = k2 ? C::add(acc, x2) : acc;
        acc = k3 ? C::add(acc, x3) : acc;
      }
      for (; i < end; ++i) {
        const int64_t c = p.entries[i];
        const bool k = c >= 0 && c < p.n_rows;
        const T x = C::load(src + (k ? c : 0) * p.rows_stride);
        acc = k ? C::add(acc, x) : acc;
      }
      if (p.base != nullptr) acc = C::add(C::load(p.base + v * p.base_stride + col), acc);
      C::store(p.out + v * p.out_stride + col, acc);
    }
  }
}

inline bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API int p3d_neighbor_sum(const float* rows, int64_t rows_stride, int64_t n_rows, const float* base, int64_t base_stride,
                             const int32_t* offsets, const int32_t* entries, int64_t V, int64_t n_entries, int64_t D, float* out,
                             int64_t out_stride, p3d_stream_t stream) {
  if (V < 0 || D < 0 || n_entries < 0 || n_rows < 0 || n_entries > INT32_MAX || D > INT32_MAX) return P3D_ERR_INVALID_ARG;
  if (V == 0 || D == 0) return P3D_OK;
  if (!out || out_stride < D || rows_stride < 0 || (base && base_stride < 0)) return P3D_ERR_INVALID_ARG;
  if (n_rows == 0) n_entries = 0;  // no row to gather from: every entry would be skipped
  if (n_entries > 0 && (!rows || !offsets || !entries)) return P3D_ERR_INVALID_ARG;
  NeighborSum p;
  p.rows = rows, p.base = base, p.offsets = offsets, p.entries = entries, p.out = out;
  p.rows_stride = rows_stride, p.base_stride = base_stride, p.out_stride = out_stride;
  p.n_rows = n_rows, p.V = V, p.n_entries = n_entries;
  const bool vec = D % 4 == 0 && out_stride % 4 == 0 && aligned16(out) && (n_entries == 0 || (rows_stride % 4 == 0 && aligned16(rows))) &&
                   (!base || (base_stride % 4 == 0 && aligned16(base)));
  p.units = vec ? D / 4 : D;
  p.lpr_log2 = 0;
  while (p.lpr_log2 < 6 && ((int64_t)1 << p.lpr_log2) < p.units) ++p.lpr_log2;
  int64_t groups = ceil_div(V, (int64_t)256 >> p.lpr_log2);
  if (groups > P3D_NEIGHBOR_SUM_MAX_GROUPS) groups = P3D_NEIGHBOR_SUM_MAX_GROUPS;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("neighbor_sum", s);
  if (vec)
    neighbor_sum_kernel<true><<<(unsigned)groups, 256, 0, s>>>(p);
  else
    neighbor_sum_kernel<false><<<(unsigned)groups, 256, 0, s>>>(p);
  return launch_status();
}
