// csr_gather.h -- one lane per vertex over its row of a CSR list: the row's bounds, and the per-vertex sum of the rows of a (., 3)
// array that the list names (vertex normals forward and backward in normals.hip, the normal-consistency backward in mesh_losses.hip).
#pragma once

#include "vec3.h"

namespace p3d {

constexpr float kNormEps = 1e-6f;  // face_areas_normals.cu:58 and F.normalize(eps=1e-6)

// Row v of a list of n entries: offsets outside [0, n] are clamped, so a list that breaks its contract gives wrong sums, never a
// read outside the list.
__device__ __forceinline__ void csr_row(const int32_t* __restrict__ offsets, int64_t v, int64_t n, int64_t& begin, int64_t& end) {
  begin = offsets[v], end = offsets[v + 1];
  begin = begin < 0 ? 0 : begin;
  end = end > n ? n : end;
}

// +0.0f plus the rows of the vertex's entries in list order; a vertex with no entry gets zeros, entries outside [0, n_entries) are
// skipped.  PER_FACE: the row of entry c is rows[c / 3] (a corner's face), else rows[c].  NORMALIZE: also s / max(|s|, 1e-6).
// Tag: any type of the including translation unit's unnamed namespace, so that each code object has a kernel of its own.
template <class Tag, bool PER_FACE, bool NORMALIZE>
__global__ __launch_bounds__(256) void vert_gather_sum_kernel(const float* __restrict__ rows, const int32_t* __restrict__ offsets,
                                                              const int32_t* __restrict__ entries, int64_t V, int64_t n_entries,
                                                              float* __restrict__ sums, float* __restrict__ normals) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    int64_t begin, end;
    csr_row(offsets, v, n_entries, begin, end);
    V3 s = mk(0.f, 0.f, 0.f);
    for (int64_t i = begin; i < end; ++i) {
      const int64_t c = entries[i];
      if (c < 0 || c >= n_entries) continue;
      s = s + load3(rows + (PER_FACE ? c / 3 : c) * 3);
    }
    store3(sums + v * 3, s);
    if (NORMALIZE) {
      float norm = norm3(s);
      norm = norm < kNormEps ? kNormEps : norm;
      store3(normals + v * 3, s / norm);
    }
  }
}

}  // namespace p3d
