// knn_queue.h -- the register queue of the one-lane-per-query scans (knn.hip, point_frames.hip): the KQ smallest (distance, index)
// pairs seen so far, ascending.  A candidate is offered only where `wants` holds in some lane of the wave; the insert is a fully
// unrolled, branch-free shift: slot s takes its left neighbour where that one is larger than the candidate, else the candidate where
// it itself is larger.  Strict comparisons and ascending j give the (dist, j) order: an equal distance met later never displaces or
// overtakes an earlier one.
#pragma once

#include "p3d_common.h"

namespace p3d {

__device__ __forceinline__ float pos_inf() { return __int_as_float(0x7f800000); }

// The KQ smallest (distance, index) pairs seen so far, ascending; +inf / -1 where nothing has arrived yet.
template <int KQ>
struct Queue {
  float d[KQ];
  int j[KQ];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int s = 0; s < KQ; ++s) d[s] = pos_inf(), j[s] = -1;
  }
  __device__ __forceinline__ bool wants(float dn) const { return dn < d[KQ - 1]; }
  // only lanes that want the candidate change anything: dn < d[KQ - 1] makes exactly one slot take it
  __device__ __forceinline__ void insert(float dn, int jn) {
#pragma unroll
    for (int s = KQ - 1; s >= 0; --s) {
      const bool shift = s > 0 && d[s > 0 ? s - 1 : 0] > dn;
      const bool here = !shift && d[s] > dn;
      const float dl = d[s > 0 ? s - 1 : 0];
      const int jl = j[s > 0 ? s - 1 : 0];
      d[s] = shift ? dl : (here ? dn : d[s]);
      j[s] = shift ? jl : (here ? jn : j[s]);
    }
  }
};

template <>
struct Queue<1> {
  float d[1];
  int j[1];
  __device__ __forceinline__ void init() { d[0] = pos_inf(), j[0] = -1; }
};

}  // namespace p3d
