// fixed_sum.h -- THE SUM OF n TERMS behind every fused loss (mesh_losses.hip, knn.hip: chamfer, point_mesh.hip): a tree whose shape
// depends on the counts alone, so that a loss has the same bits on every run, stream and process.  No float atomic.
//   level 1  the kernel that computes the terms sums them into PARTIALS, one per workgroup, a lane without a term holding +0:
//              a wave of 64 terms   wave_sum: six xor-butterfly rounds, i.e. six rounds of pairwise t[2 i] + t[2 i + 1]
//                                   (knn.hip, point_mesh.hip: one wave of queries per workgroup);
//              a block of 256 terms block_sum_256: wave_sum in each of the four waves, then (w0 + w1) + (w2 + w3) -- eight
//                                   pairwise rounds (mesh_losses.hip).
//   level 2  segment_sum_kernel, ONE block of 256 lanes per segment (the batch, a cloud, a batch element) over the segment's
//            `per_segment` consecutive partials: lane t adds the partials t, t + 256, ... in ascending order to +0, then
//            block_sum_256; thread 0 stores finish(segment, sum) -- the caller's last step (a division, or nothing).
// A term passes through at most  6 + ceil(ceil(n / 64) / 256) + 8  additions from a wave partial and
// 8 + ceil(ceil(n / 256) / 256) + 8  from a block partial, n the terms of the largest segment.
// tests/fixed_sum_case.py restates the tree in numpy; tests/test_gpu_loss_kernel_edges.py (section E) holds the kernels to its bits.
#pragma once

#include "p3d_common.h"

namespace p3d {

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) x += __shfl_xor(x, d);
  return x;
}

// every lane of the block calls it (no early return in front); lane 0 of the block holds the sum
__device__ __forceinline__ float block_sum_256(float x) {
  __shared__ float part[4];
  x = wave_sum(x);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

// grid: one block of 256 per segment.  Finish: __device__ float operator()(int64_t segment, float sum) const, a type of the
// including translation unit's unnamed namespace -- every translation unit instantiates a kernel of its own (as ordered_sum.h's).
template <class Finish>
__global__ __launch_bounds__(256) void segment_sum_kernel(const float* __restrict__ partials, int64_t per_segment, Finish finish,
                                                          float* __restrict__ sums) {
  const int64_t n = blockIdx.x;
  float acc = 0.0f;
  for (int64_t k = threadIdx.x; k < per_segment; k += 256) acc += partials[n * per_segment + k];
  const float s = block_sum_256(acc);
  if (threadIdx.x == 0) sums[n] = finish(n, s);
}

}  // namespace p3d
