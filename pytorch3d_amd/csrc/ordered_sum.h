// ordered_sum.h -- the segmented sum behind the deterministic backwards (ordered_bwd.hip).
//
// The atomic backwards add a sample's partials to the row of its primitive in whatever order the hardware serves them.  Here
// the caller hands over the samples that hold a primitive SORTED by primitive (stable: ascending sample index inside one
// primitive), a lane owns one position of that array, recomputes its row of R partials, and the rows of one primitive are
// summed by a tree that only the positions in the sorted array decide:
//   pass 1  a wave owns 64 consecutive positions.  A segmented inclusive scan (six rounds of lane shifts, a lane adds the value
//           d lanes below while that lane is still inside its segment) leaves the sum of a segment's part inside the wave in its
//           last lane.  A segment that begins and ends inside the wave is stored to its output row; a part that is cut by
//           the wave's border goes to the workspace: slot A = the part that came in over lane 0, slot B = the part that leaves
//           over lane 63 and began in this wave (a wave inside one long segment has only A).
//   pass 2  one thread per wave that holds a slot B: B + A(next wave) + A(the one after) ... in ascending wave order until
//           a slot A says that the segment ended there.
// No float atomic anywhere, no dependence on launch timing; rows nobody hits are zero-filled by a kernel in front.
#pragma once

#include <string>

#include "p3d_common.h"

namespace p3d {
namespace ordered {

constexpr int kNone = -1;            // a sample without a (valid) primitive: forms segments that are never stored
constexpr int kOutside = -2147483647 - 1;  // "key" of the positions in front of and behind the array

// An Op names the samples' primitives and their rows:
//   static constexpr int R                 floats of a row (per chunk)
//   int64_t nsamples; int64_t nkeys;
//   __device__ int64_t key(int64_t s)      primitive of sample s (any value: checked against nkeys here)
//   __device__ void row(int64_t s, int key, int chunk, float (&r)[R])
//   __device__ void store(int key, int chunk, const float (&r)[R])
template <class Op>
__device__ __forceinline__ int checked_key(const Op& op, int64_t s) {
  if (s < 0 || s >= op.nsamples) return kNone;
  const int64_t k = op.key(s);
  return (k >= 0 && k < op.nkeys) ? (int)k : kNone;
}

// rows: [chunk][wave][slot A, B][R] floats; meta: [chunk][wave]{has B, A closes its segment}
inline size_t partial_bytes(int64_t S, int R, int chunks) {
  const size_t waves = (size_t)ceil_div(S, kWave);
  return align_up(waves * (size_t)chunks * 2 * R * sizeof(float), 256) + align_up(waves * (size_t)chunks * 2 * sizeof(int), 256);
}

// (static: the header is included by more than one translation unit)
static __global__ __launch_bounds__(256) void fill_zero_kernel(float* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0.0f;
}

template <class Op>
__global__ __launch_bounds__(256) void pass1_kernel(Op op, const int64_t* __restrict__ sorted, int64_t S, float* __restrict__ prow,
                                                    int* __restrict__ pmeta, int64_t nwaves) {
  constexpr int R = Op::R;
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int chunk = blockIdx.y;
  if (wave >= nwaves) return;  // wave-uniform; no workgroup barrier in this kernel
  const int64_t pos = wave * kWave + lane;
  const bool valid = pos < S;  // lane 0 always is
  int64_t s = -1;
  int key = kNone;
  if (valid) {
    s = sorted[pos];
    key = checked_key(op, s);
  }
  int kp = __shfl_up(key, 1), kn = __shfl_down(key, 1);
  if (lane == 0) kp = pos > 0 ? checked_key(op, sorted[pos - 1]) : kOutside;
  if (lane == 63) kn = pos + 1 < S ? checked_key(op, sorted[pos + 1]) : kOutside;
  const bool head = valid && (pos == 0 || kp != key);       // the segment BEGINS here (in the whole array)
  const bool tail = valid && (pos == S - 1 || kn != key);   // ... ENDS here
  float r[R];
#pragma unroll
  for (int i = 0; i < R; ++i) r[i] = 0.0f;
  if (key >= 0) op.row(s, key, chunk, r);

  // the lane where this lane's segment starts inside the wave (lanes past the array are segments of their own).  This scan is
  // written out three times on purpose -- here, transform.hip (camera_grad) and knn.hip (knn_bwd_scatter_kernel): hoisted into one
  // helper it compiled this kernel to more instructions for gfx950 (MeshOp 1353 -> 1391, PointMeshOp<0, 2> 1651 -> 1700,
  // SplatOp<4> 977 -> 999: compare / select pairs in their _e64 forms, more waits), and these are the measured backwards of
  // DESIGN section 8.8.
  const unsigned long long true_heads = __ballot(head);
  const unsigned long long starts = __ballot(head || !valid || lane == 0);
  const int start = 63 - __clzll((long long)(starts & ((2ull << lane) - 1ull)));
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const bool take = lane - d >= start;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const float t = __shfl_up(r[i], d);
      if (take) r[i] += t;
    }
  }

  const bool last = valid && (tail || lane == 63);  // last lane of the segment's part in this wave
  const bool began_here = ((true_heads >> start) & 1ull) != 0;
  const bool slot_a = last && !began_here;            // came in over lane 0 (start == 0)
  const bool slot_b = last && began_here && !tail;    // leaves over lane 63
  const int64_t cell = (int64_t)chunk * nwaves + wave;
  if (last && began_here && tail) {
    if (key >= 0) op.store(key, chunk, r);
  } else if (slot_a || slot_b) {
    float* dst = prow + (cell * 2 + (slot_b ? 1 : 0)) * R;
#pragma unroll
    for (int i = 0; i < R; ++i) dst[i] = r[i];
    if (slot_a) pmeta[cell * 2 + 1] = tail ? 1 : 0;
  }
  const bool has_b = __ballot(slot_b) != 0;
  if (lane == 0) pmeta[cell * 2] = has_b ? 1 : 0;
}

template <class Op>
__global__ __launch_bounds__(256) void pass2_kernel(Op op, const int64_t* __restrict__ sorted, int64_t S, const float* __restrict__ prow,
                                                    const int* __restrict__ pmeta, int64_t nwaves) {
  constexpr int R = Op::R;
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int chunk = blockIdx.y;
  if (w >= nwaves) return;
  const int64_t cell = (int64_t)chunk * nwaves + w;
  if (pmeta[cell * 2] == 0) return;
  float acc[R];
  const float* b = prow + (cell * 2 + 1) * R;
#pragma unroll
  for (int i = 0; i < R; ++i) acc[i] = b[i];
  // (a slot B means that lane 63 did not end its segment: the next wave exists and has a slot A)
  for (int64_t w2 = w + 1; w2 < nwaves; ++w2) {
    const int64_t c2 = (int64_t)chunk * nwaves + w2;
    const float* a = prow + c2 * 2 * R;
#pragma unroll
    for (int i = 0; i < R; ++i) acc[i] += a[i];
    if (pmeta[c2 * 2 + 1] != 0) break;
  }
  const int key = checked_key(op, sorted[w * kWave + 63]);
  if (key >= 0) op.store(key, chunk, acc);
}

inline int fill_zero(float* p, int64_t n, hipStream_t s) {
  if (n <= 0) return P3D_OK;
  LaunchScope ls("ordered_fill_zero", s);
  int64_t blocks = ceil_div(n, 256);
  if (blocks > 16384) blocks = 16384;
  fill_zero_kernel<<<(unsigned)blocks, 256, 0, s>>>(p, n);
  return launch_status();
}

// The two passes over `sorted` (S entries); `partials` holds partial_bytes(S, Op::R, chunks).  The output rows were zero-filled.
// `what` names the two launches for the built-in timing (p3d_profile_*): <what>_pass1, <what>_pass2.
template <class Op>
int run(const Op& op, const int64_t* sorted, int64_t S, int chunks, void* partials, hipStream_t s, const char* what) {
  if (S <= 0 || chunks <= 0) return P3D_OK;
  const int64_t nwaves = ceil_div(S, kWave);
  const int64_t b1 = ceil_div(nwaves, 4), b2 = ceil_div(nwaves, 256);
  if (b1 > 0x7fffffffll || chunks > 65535) return P3D_ERR_INVALID_ARG;
  float* prow = static_cast<float*>(partials);
  int* pmeta = reinterpret_cast<int*>(static_cast<char*>(partials) + align_up((size_t)nwaves * chunks * 2 * Op::R * sizeof(float), 256));
  {
    LaunchScope ls(profile_enabled() ? (std::string(what) + "_pass1").c_str() : what, s);
    pass1_kernel<Op><<<dim3((unsigned)b1, (unsigned)chunks), 256, 0, s>>>(op, sorted, S, prow, pmeta, nwaves);
  }
  const int st = launch_status();
  if (st != P3D_OK) return st;
  {
    LaunchScope ls(profile_enabled() ? (std::string(what) + "_pass2").c_str() : what, s);
    pass2_kernel<Op><<<dim3((unsigned)b2, (unsigned)chunks), 256, 0, s>>>(op, sorted, S, prow, pmeta, nwaves);
  }
  return launch_status();
}

}  // namespace ordered
}  // namespace p3d
