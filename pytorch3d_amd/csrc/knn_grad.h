// knn_grad.h -- one hit of the nearest-neighbour backward (knn_cpu.cpp:101-126), shared by the atomic and gather kernels of
// knn.hip and by the ordered scatter of ordered_bwd.hip, so that the three sum the SAME float32 terms.
#pragma once

#include "p3d_common.h"

namespace p3d {
namespace knn {

// a cloud's length: NULL means full, anything else is clamped into [0, P]
__device__ __forceinline__ int64_t cloud_length(const int64_t* __restrict__ lengths, int64_t n, int64_t P) {
  if (!lengths) return P;
  const int64_t l = lengths[n];
  return l < 0 ? 0 : (l > P ? P : l);
}

// What p1[n,i]'s coordinate c receives from the hit with upstream gradient g (p2's coordinate gets the negative):
// norm 2: 2 g (x - y); norm 1: g where x > y, -g otherwise (x == y gives -g, as the reference does).
__device__ __forceinline__ float grad_term(float g, float x, float y, int norm) {
  if (norm == 2) return (2.0f * g) * (x - y);
  return x > y ? g : -g;
}

// The hits of the backward, by linear index e into (N, P1, K).
struct Hits {
  const float *p1, *p2;
  const int64_t *lengths1, *lengths2, *idx;
  const float *grad_dists, *cloud_scale;  // either may be NULL (1)
  int64_t N, P1, P2;
  int D, K, norm;

  // the p2 point of hit e as n * P2 + j, or -1 where e is padding (or its index lies outside p2)
  __device__ __forceinline__ int64_t target(int64_t e) const {
    const int k = (int)(e % K);
    const int64_t ni = e / K, n = ni / P1, i = ni % P1;
    if (i >= cloud_length(lengths1, n, P1) || k >= cloud_length(lengths2, n, P2)) return -1;
    const int64_t j = idx[e];
    return (j >= 0 && j < P2) ? n * P2 + j : -1;
  }
  __device__ __forceinline__ float upstream(int64_t e) const {
    const float g = grad_dists ? grad_dists[e] : 1.0f;
    return cloud_scale ? g * cloud_scale[e / ((int64_t)K * P1)] : g;
  }
  // coordinate c of what hit e (target t = target(e) >= 0) gives to its p1 point
  __device__ __forceinline__ float term(int64_t e, int64_t t, int c, float g) const {
    return grad_term(g, p1[(e / K) * D + c], p2[t * D + c], norm);
  }
};

}  // namespace knn
}  // namespace p3d
