// scan_blocks.h -- the scan pieces shared by the count -> scan -> fill operators that cut their items into SCAN BLOCKS of one mesh
// each (cubify.hip, marching_cubes.hip): a wave's inclusive scan, a workgroup's exclusive scan over its waves' totals, and the carry
// kernel that turns two tables of block totals into exclusive scans and the per-mesh (V_n, F_n).  Integers only, no atomic.
#pragma once

#include "p3d_common.h"

namespace p3d {
namespace {  // per translation unit, as the kernels that use them are

// The exclusive scan of x over the workgroup's WAVES waves, and its total.  wsum: WAVES ints of LDS, free again on return.
template <int WAVES>
__device__ __forceinline__ int block_exclusive(int wave_exclusive, int wave_total, int* wsum, int* total) {
  const int wave = (int)threadIdx.x / kWave;
  if (lane_id() == 0) wsum[wave] = wave_total;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < WAVES; ++i) {
    const int t = wsum[i];
    before += i < wave ? t : 0;
    all += t;
  }
  __syncthreads();
  *total = all;
  return before + wave_exclusive;
}

// inclusive Hillis-Steele scan over the wave
__device__ __forceinline__ int wave_inclusive(int x) {
  const int lane = lane_id();
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  return x;
}

// grid: 2 blocks of LANES.  Block 0 scans the face table (column 1 of counts), block 1 the vertex table (column 0): the exclusive scan
// of the nb block totals in rounds of LANES, in place, the grand total behind the last block; then counts[n] = the difference of the
// carries around mesh n's bpm blocks.
template <int LANES>
__global__ __launch_bounds__(LANES) void carry_kernel(int* carry_f, int nb_f, int bpm_f, int* carry_v, int nb_v, int bpm_v, int N,
                                                      int64_t* __restrict__ counts) {
  __shared__ int wsum[LANES / kWave];
  int* a = blockIdx.x ? carry_v : carry_f;
  const int nb = blockIdx.x ? nb_v : nb_f, bpm = blockIdx.x ? bpm_v : bpm_f, col = blockIdx.x ? 0 : 1;
  int running = 0;
  for (int base = 0; base < nb; base += LANES) {
    const int i = base + (int)threadIdx.x;
    const int x = i < nb ? a[i] : 0;
    const int incl = wave_inclusive(x);
    int total;
    const int ex = running + block_exclusive<LANES / kWave>(incl - x, __shfl(incl, kWave - 1), wsum, &total);
    if (i < nb) a[i] = ex;
    running += total;
  }
  if (threadIdx.x == 0) a[nb] = running;
  __syncthreads();  // the table was written by this workgroup: visible to it behind the barrier
  for (int n = (int)threadIdx.x; n < N; n += LANES) counts[2 * n + col] = (int64_t)(a[(n + 1) * bpm] - a[n * bpm]);
}

}  // namespace
}  // namespace p3d
