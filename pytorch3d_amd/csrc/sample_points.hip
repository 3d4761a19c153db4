// sample_points.hip -- sample_points_from_meshes (pytorch3d/ops/sample_points_from_meshes.py), forward and backward.
// include/p3d_amd.h has the contract.  The randomness is an INPUT: uniforms (N, S, 3) in [0, 1); everything here is a pure function of
// it.
//
// Forward, (1) the table: cdf (F,) f32, per mesh the inclusive prefix sum of the face areas |(v1 - v0) x (v2 - v0)| / 2 over the mesh's
// range of packed faces, restarting at every mesh's first face.  A face is a segment head when its index is one of
// mesh_to_faces_packed_first_idx.  The table is DEFINED as
//     cdf[f] = max { T[j] : j <= f in f's mesh, area[j] > 0 }      (0 when there is no such j)
// with T the two-level segmented tree sum below.  The running maximum is exact in any order, so the table is non-decreasing inside
// a mesh BY CONSTRUCTION, a face of zero area repeats its predecessor's value (it adds nothing to the maximum), and the bits depend on
// the face counts alone -- a tree sum's own prefixes may step down by an ulp where two of them round differently.  No float atomic, no
// host round trip, the grids are sized from F:
//   level 1  cdf_local_kernel, a block of kScanBlock = 256 consecutive faces, a face per lane: a segmented Kogge-Stone scan in each wave
//            (six rounds, a lane adds the value d lanes below while that lane is inside its segment), then the waves' totals chained
//            in wave order ((w0 + w1) + w2) and added to the lanes in front of the wave's first head: at most 6 + 3 additions.  The
//            same shape again with max over the faces of non-zero area.  A block leaves its last lane's sum and maximum (the part of
//            the segment that runs into the next block) and the position of its first head.
//   level 2  cdf_carry_kernel, ONE block of 256 lanes over the blocks' records in rounds of 256, the same scan (6 + 3 additions)
//            after the carry of the round before: carry[b], what block b's lanes in front of its first head
//            add to their sums, and runmax[b], the table's value at the end of block b - 1.
//   finish   cdf_finish_kernel: T = carry[b] + local (one addition), the maximum with runmax[b], 0 where no face of non-zero area
//            came before.
// A term passes through at most (6 + 3) additions at level 1, (6 + 3) in its round of level 2, 4 in every later round (the carry
// joins the round's three wave totals and the lane) and one in the finish.  With rounds = ceil(ceil(F / 256) / 256) that is
// 19 + 4 (rounds - 1); the depth the header states and the tests gate with is
//     D(F) = 19 + 4 rounds                                  23 for every F up to 65 536 faces, 27 up to 131 072
// which carries one spare round, so a table entry is within D(F) 2^-24 total of the
// exact prefix sum of the same float32 areas.  A NaN area stays NaN in every later entry
// of its mesh (the maximum passes NaN on), so a mesh with a NaN or infinite total is recognised by its last entry.
//
// (2) sampling, one lane per sample (n, s): t = u0 * total_n, the face is the first f of mesh n with cdf[f] > t (a plain binary search:
// the table of a 5 000-face mesh is 20 KB and stays in L2), t clamped below total_n so that a product that rounds up to the total lands
// on the last face of non-zero area; then r = sqrt(u1), w0 = 1 - r, w1 = r (1 - u2), w2 = r u2, sample = (w0 a + w1 b) + w2 c -- the
// reference's _rand_barycentric_coords and its line 112 in their operation order (IEEE sqrt, nothing fused) -- and the sampler's normal
// (v1 - v0) x (v2 - v1) / max(|.|, DBL_EPSILON).  Every entry of every output is written; an empty mesh, or one whose total is zero or
// not finite, gets zero rows and face index -1.
//
// Backward: one lane per sample adds w_k grad_sample to corner k of its face (9 values) and grad_normal to the face's normal sum (3
// more, only when that gradient is live) in a row per face -- merged in wave-private LDS tables (wave_table.h), flushed with float
// atomics; the ordered form is ordered_bwd.hip's SampleOp.  One lane per face then folds the summed normal gradient through the
// Jacobian of c / max(|c|, eps), ONCE per face, into the nine corner gradients, and the host finishes with p3d_scatter_face_grads.
#include <float.h>

#include "vec3.h"
#include "wave_table.h"

namespace p3d {

// ordered_bwd.hip: the per-face rows as an ordered segmented sum over the samples sorted by face
size_t sample_points_ordered_bytes(int64_t num_sorted);
int sample_points_ordered_rows(const int64_t* face_idxs, const float* bary, const float* grad_samples, const float* grad_normals,
                               const int64_t* sorted, int64_t num_sorted, int64_t num_samples, int64_t F, int nv, float* rows,
                               void* workspace, hipStream_t s);

namespace {

constexpr int kScanBlock = 256;                   // faces per block of level 1, block records per round of level 2
constexpr float kNone = -1.0f;                    // "no face of non-zero area so far": sums of areas are never negative
constexpr float kSamplerEps = (float)DBL_EPSILON;  // sys.float_info.epsilon, as the float32 clamp of the reference reads it

// A vertex id as torch indexing reads it (a negative id wraps once); -1 when it is still outside [0, V).
__device__ __forceinline__ int64_t vertex_id(const int64_t* __restrict__ faces, int64_t corner, int64_t V) {
  int64_t v = faces[corner];
  if (v < 0) v += V;
  return (v >= 0 && v < V) ? v : -1;
}

// nothing outside `verts` is read; an id out of range gives NaN coordinates
__device__ __forceinline__ V3 corner_vertex(const float* __restrict__ verts, int64_t v) {
  if (v < 0) return mk(quiet_nan(), quiet_nan(), quiet_nan());
  return load3(verts + v * 3);
}

// the maximum that passes a NaN on (associative and commutative, NaN included)
__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// f is a segment head when some mesh begins there.  first_idx is ascending (a packed batch); whatever it holds, only its N entries
// are read.
__device__ __forceinline__ bool is_head(const int64_t* __restrict__ first_idx, int64_t N, int64_t f) {
  int64_t lo = 0, hi = N;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (first_idx[mid] <= f) lo = mid + 1; else hi = mid;
  }
  return lo > 0 && first_idx[lo - 1] == f;
}

// The segmented inclusive scan of a block of 256 lanes under `op` (a sum, or nan_max).  x: the lane's term; head: a segment begins at
// this lane; carry: what comes in over lane 0 of the block.  Kogge-Stone in each wave (six rounds: a lane takes the value d lanes below
// while that lane is inside its segment), then the waves' last values chained in wave order, restarting at a wave that holds a head,
// and joined to the lanes in front of the wave's first head.  Every lane of the block calls it.
template <class Op>
__device__ __forceinline__ float block_seg_scan(float x, bool head, float carry, Op op) {
  __shared__ float s_last[4];
  __shared__ int s_has_head[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long heads = __ballot(head);
  const unsigned long long below = heads & ((2ull << lane) - 1ull);  // heads at or below this lane
  const int start = below ? 63 - __clzll((long long)below) : 0;     // where this lane's segment starts inside the wave
  float v = x;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const float t = __shfl_up(v, d);
    if (lane - d >= start) v = op(t, v);
  }
  __syncthreads();  // the tables of the call before are free
  if (lane == 63) s_last[w] = v, s_has_head[w] = heads != 0;
  __syncthreads();
  float c = carry;
  for (int k = 0; k < w; ++k) c = s_has_head[k] ? s_last[k] : op(c, s_last[k]);
  return below == 0 ? op(c, v) : v;  // no head at or below this lane inside the wave: it continues what came in
}

// the value of the lane before (`first` for lane 0 of the block); every lane of the block calls it
__device__ __forceinline__ float block_shift_up(float v, float first) {
  __shared__ float s_v[kScanBlock];
  __syncthreads();
  s_v[threadIdx.x] = v;
  __syncthreads();
  return threadIdx.x > 0 ? s_v[threadIdx.x - 1] : first;
}

struct AddOp {
  __device__ float operator()(float a, float b) const { return a + b; }
};
struct MaxOp {
  __device__ float operator()(float a, float b) const { return nan_max(a, b); }
};

// what level 1 leaves per block and level 2 makes of it
struct BlockRec {
  float* sum;        // level 1: the last lane's sum -- the part of its segment inside the block
  float* cm;         // level 1: the last lane's running maximum of the block's own sums (kNone: no face of non-zero area in that part)
  int* first_head;   // level 1: position of the block's first head, kScanBlock for none
  float* carry;      // level 2: what the lanes in front of the first head add to their sums
  float* runmax;     // level 2: the table's value at the end of the block before (kNone for nothing)
};

// ---- (1) the table ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cdf_local_kernel(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                        const int64_t* __restrict__ first_idx, int64_t V, int64_t F, int64_t N,
                                                        float* __restrict__ cdf, BlockRec rec) {
  __shared__ unsigned long long s_heads[4];
  const int64_t f = (int64_t)blockIdx.x * kScanBlock + threadIdx.x;
  float area = 0.0f;
  bool head = false;
  if (f < F) {
    const V3 v0 = corner_vertex(verts, vertex_id(faces, f * 3 + 0, V));
    const V3 v1 = corner_vertex(verts, vertex_id(faces, f * 3 + 1, V));
    const V3 v2 = corner_vertex(verts, vertex_id(faces, f * 3 + 2, V));
    area = norm3(cross(v1 - v0, v2 - v0)) / 2.0f;  // p3d_face_areas_normals_forward's arithmetic
    head = is_head(first_idx, N, f);
  }
  // (a lane past F holds a zero area and no head: it repeats what came before, which the block's record then carries)
  const unsigned long long heads = __ballot(head);
  if ((threadIdx.x & 63) == 0) s_heads[threadIdx.x >> 6] = heads;
  const float sum = block_seg_scan(area, head, 0.0f, AddOp());
  const float cm = block_seg_scan((area > 0.0f || area != area) ? sum : kNone, head, kNone, MaxOp());
  if (f < F) cdf[f] = cm;
  if (threadIdx.x == kScanBlock - 1) {
    int first_head = kScanBlock;
    for (int k = 3; k >= 0; --k)
      if (s_heads[k]) first_head = k * 64 + __builtin_ctzll(s_heads[k]);
    rec.sum[blockIdx.x] = sum;
    rec.cm[blockIdx.x] = cm;
    rec.first_head[blockIdx.x] = first_head;
  }
}

// one block; the rounds chain through the inclusive values of a round's last lane
__global__ __launch_bounds__(256) void cdf_carry_kernel(int64_t nblocks, BlockRec rec) {
  __shared__ float s_round[2];
  float round_sum = 0.0f, round_max = kNone;
  for (int64_t base = 0; base < nblocks; base += kScanBlock) {
    const int64_t b = base + threadIdx.x;
    const bool valid = b < nblocks;
    const float part = valid ? rec.sum[b] : 0.0f;
    const float cm = valid ? rec.cm[b] : kNone;
    const bool head = valid && rec.first_head[b] < kScanBlock;
    const float incl = block_seg_scan(part, head, round_sum, AddOp());
    const float carry = block_shift_up(incl, round_sum);
    // the table's value at the end of block b: its own maximum, lifted by the carry where the block holds no head
    const float t_end = cm < 0.0f ? kNone : (head ? cm : carry + cm);
    const float run = block_seg_scan(t_end, head, round_max, MaxOp());
    const float runmax = block_shift_up(run, round_max);
    if (valid) rec.carry[b] = carry, rec.runmax[b] = runmax;
    if (threadIdx.x == kScanBlock - 1) s_round[0] = incl, s_round[1] = run;
    __syncthreads();
    round_sum = s_round[0], round_max = s_round[1];
  }
}

__global__ __launch_bounds__(256) void cdf_finish_kernel(int64_t F, float* __restrict__ cdf, BlockRec rec) {
  for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < F; f += (int64_t)gridDim.x * 256) {
    const int64_t b = f / kScanBlock;
    float v = cdf[f];
    if ((int)(f - b * kScanBlock) < rec.first_head[b]) {  // in front of the block's first head: the segment came in from block b - 1
      const float t = v < 0.0f ? kNone : rec.carry[b] + v;
      v = nan_max(t, rec.runmax[b]);
    }
    cdf[f] = v < 0.0f ? 0.0f : v;
  }
}

// ---- (2) sampling ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_kernel(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                     const int64_t* __restrict__ first_idx, const int64_t* __restrict__ num_faces,
                                                     const float* __restrict__ uniforms, const float* __restrict__ cdf, int64_t V,
                                                     int64_t F, int64_t N, int64_t S, float* __restrict__ samples,
                                                     float* __restrict__ normals, int64_t* __restrict__ face_idxs,
                                                     float* __restrict__ bary) {
  const int64_t total_samples = N * S;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total_samples; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / S;
    // the mesh's range, clamped into the table
    int64_t first = first_idx[n], count = num_faces[n];
    first = first < 0 ? 0 : (first > F ? F : first);
    count = count < 0 ? 0 : (count > F - first ? F - first : count);
    const float total = count > 0 ? cdf[first + count - 1] : 0.0f;
    int64_t face = -1;
    V3 w = mk(0.f, 0.f, 0.f), p = mk(0.f, 0.f, 0.f), nrm = mk(0.f, 0.f, 0.f);
    if (total > 0.0f && total <= FLT_MAX) {  // (false for NaN)
      const float u0 = uniforms[i * 3], u1 = uniforms[i * 3 + 1], u2 = uniforms[i * 3 + 2];
      float t = u0 * total;
      // inside [0, total): a product that rounds up to the total takes the last face of non-zero area, the first one that reaches it
      if (!(t < total)) t = __int_as_float(__float_as_int(total) - 1);
      if (!(t >= 0.0f)) t = 0.0f;
      int64_t lo = 0, hi = count - 1;  // cdf[first + count - 1] = total > t: the answer exists
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (cdf[first + mid] > t) hi = mid; else lo = mid + 1;
      }
      face = first + lo;
      const V3 a = corner_vertex(verts, vertex_id(faces, face * 3 + 0, V));
      const V3 b = corner_vertex(verts, vertex_id(faces, face * 3 + 1, V));
      const V3 c = corner_vertex(verts, vertex_id(faces, face * 3 + 2, V));
      const float r = sqrtf(u1);
      w = mk(1.0f - r, r * (1.0f - u2), r * u2);
      p = (w.x * a + w.y * b) + w.z * c;
      if (normals) {
        const V3 cr = cross(b - a, c - b);
        float norm = norm3(cr);
        norm = norm < kSamplerEps ? kSamplerEps : norm;
        nrm = cr / norm;
      }
    }
    store3(samples + i * 3, p);
    if (normals) store3(normals + i * 3, nrm);
    face_idxs[i] = face;
    store3(bary + i * 3, w);
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
// NV = 9: w_k grad_sample per corner; NV = 12: and grad_normal.  4 waves x 192 slots x 56 B = 42 KB.
template <int NV>
using FaceTable = WaveTable<NV, 192>;

template <int NV>
__global__ __launch_bounds__(256) void face_sums_kernel(const int64_t* __restrict__ face_idxs, const float* __restrict__ bary,
                                                        const float* __restrict__ grad_samples,
                                                        const float* __restrict__ grad_normals, int64_t num_samples, int64_t F,
                                                        int64_t span, float* __restrict__ rows) {
  __shared__ __align__(16) int s_table[4][FaceTable<NV>::kLdsInts];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t begin = ((int64_t)blockIdx.x * 4 + w) * span;
  if (begin >= num_samples) return;  // wave-uniform; no workgroup barrier in this kernel
  const int64_t end = begin + span < num_samples ? begin + span : num_samples;
  FaceTable<NV> tab;
  tab.init(s_table[w], lane);
  for (int64_t base = begin; base < end; base += 64) {
    const int64_t i = base + lane;
    int f = -1;
    float g[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) g[j] = 0.0f;
    if (i < end) {
      const int64_t fi = face_idxs[i];
      if (fi >= 0 && fi < F) {
        f = (int)fi;
        const V3 gs = load3(grad_samples + i * 3);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float wk = bary[i * 3 + k];
          g[3 * k] = wk * gs.x, g[3 * k + 1] = wk * gs.y, g[3 * k + 2] = wk * gs.z;
        }
        if constexpr (NV == 12) {
          g[9] = grad_normals[i * 3], g[10] = grad_normals[i * 3 + 1], g[11] = grad_normals[i * 3 + 2];
        }
      }
    }
    tab.add(rows, lane, f, g);
  }
  if (tab.used > 0) tab.flush(rows, lane);
}

// One lane per face: the nine corner gradients, and the normal sum G through n = c / max(|c|, eps), c = a x b, a = v1 - v0,
// b = v2 - v1:  dL/dc = (G - n (n . G)) / |c|, or G / eps where the clamp holds (what autograd gives for x / clamp(norm, min = eps)
// there: the clamp passes no gradient to the norm); then grad_a = b x dL/dc, grad_b = dL/dc x a, v0 -= grad_a, v1 += grad_a - grad_b,
// v2 += grad_b.  The clamp is tested as the forward tests it.
template <int NV>
__global__ __launch_bounds__(256) void face_finish_kernel(const float* __restrict__ rows, const float* __restrict__ verts,
                                                          const int64_t* __restrict__ faces, int64_t V, int64_t F,
                                                          float* __restrict__ grad_face_verts) {
  for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < F; f += (int64_t)gridDim.x * 256) {
    const float* r = rows + f * NV;
    V3 g0 = load3(r), g1 = load3(r + 3), g2 = load3(r + 6);
    if constexpr (NV == 12) {
      const V3 G = load3(r + 9);
      const V3 v0 = corner_vertex(verts, vertex_id(faces, f * 3 + 0, V));
      const V3 v1 = corner_vertex(verts, vertex_id(faces, f * 3 + 1, V));
      const V3 v2 = corner_vertex(verts, vertex_id(faces, f * 3 + 2, V));
      const V3 a = v1 - v0, b = v2 - v1;
      const V3 c = cross(a, b);
      const float norm = norm3(c);
      V3 gc;
      if (norm < kSamplerEps) {
        gc = G / kSamplerEps;
      } else {
        const V3 n = c / norm;
        gc = (G - n * dot(n, G)) / norm;
      }
      const V3 ga = cross(b, gc), gb = cross(gc, a);
      g0 = g0 - ga, g1 = g1 + (ga - gb), g2 = g2 + gb;
    }
    float* out = grad_face_verts + f * 9;
    store3(out, g0);
    store3(out + 3, g1);
    store3(out + 6, g2);
  }
}

struct Workspace {
  float* cdf;
  BlockRec rec;
  size_t bytes;
};

Workspace carve(void* workspace, int64_t F) {
  const int64_t nb = ceil_div(F, kScanBlock);
  Arena a(workspace, ~(size_t)0);
  Workspace w;
  w.cdf = a.take<float>((size_t)F);  // first: the table is what tests read back
  w.rec.sum = a.take<float>((size_t)nb);
  w.rec.cm = a.take<float>((size_t)nb);
  w.rec.first_head = a.take<int>((size_t)nb);
  w.rec.carry = a.take<float>((size_t)nb);
  w.rec.runmax = a.take<float>((size_t)nb);
  w.bytes = a.off;
  return w;
}

template <int NV>
int backward_rows_atomic(const int64_t* face_idxs, const float* bary, const float* gs, const float* gn, int64_t num_samples, int64_t F,
                         float* rows, hipStream_t s) {
  if (hipMemsetAsync(rows, 0, (size_t)F * NV * sizeof(float), s) != hipSuccess) return P3D_ERR_LAUNCH;
  if (num_samples == 0) return P3D_OK;
  // A wave's samples: enough waves to cover the chip's 1024 SIMDs twice before a wave takes more than one step of 64 -- one cow x
  // 10 000 samples is 157 waves of one step, not 10 waves of 16 dependent steps -- then up to 1024 samples per wave, then more.
  int64_t waves = ceil_div(num_samples, 64);
  if (waves > 2048) waves = ceil_div(num_samples, 1024) > 2048 ? ceil_div(num_samples, 1024) : 2048;
  if (waves > 4 * 4096) waves = 4 * 4096;
  const int64_t blocks = ceil_div(waves, 4);
  const int64_t span = ceil_div(ceil_div(num_samples, blocks * 4), 64) * 64;
  LaunchScope ls("sample_points_face_sums", s);
  face_sums_kernel<NV><<<(unsigned)blocks, 256, 0, s>>>(face_idxs, bary, gs, gn, num_samples, F, span, rows);
  return launch_status();
}

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API size_t p3d_sample_points_forward_workspace_bytes(int64_t F) { return F < 0 ? 0 : carve(nullptr, F).bytes; }

P3D_API int p3d_sample_points_forward(const float* verts, const int64_t* faces, const int64_t* mesh_to_faces_first_idx,
                                      const int64_t* num_faces_per_mesh, const float* uniforms, int64_t V, int64_t F, int64_t N,
                                      int64_t S, float* samples, float* normals, int64_t* face_idxs, float* bary, void* workspace,
                                      size_t workspace_bytes, p3d_stream_t stream) {
  if (V < 0 || F < 0 || N < 0 || S < 0 || F > INT32_MAX) return P3D_ERR_INVALID_ARG;
  if (N > 0 && S > INT64_MAX / 3 / N) return P3D_ERR_INVALID_ARG;
  if (N * S == 0) return P3D_OK;
  if (!mesh_to_faces_first_idx || !num_faces_per_mesh || !uniforms || !samples || !face_idxs || !bary) return P3D_ERR_INVALID_ARG;
  if (F > 0 && (!faces || (V > 0 && !verts))) return P3D_ERR_INVALID_ARG;
  if (F > 0 && (!workspace || workspace_bytes < p3d_sample_points_forward_workspace_bytes(F))) return P3D_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const Workspace w = carve(workspace, F);
  if (F > 0) {
    const int64_t nb = ceil_div(F, kScanBlock);
    LaunchScope ls("sample_points_cdf", s);
    cdf_local_kernel<<<(unsigned)nb, 256, 0, s>>>(verts, faces, mesh_to_faces_first_idx, V, F, N, w.cdf, w.rec);
    cdf_carry_kernel<<<1, 256, 0, s>>>(nb, w.rec);
    cdf_finish_kernel<<<stream_blocks(F), 256, 0, s>>>(F, w.cdf, w.rec);
    const int st = launch_status();
    if (st != P3D_OK) return st;
  }
  LaunchScope ls("sample_points_forward", s);
  sample_kernel<<<stream_blocks(N * S), 256, 0, s>>>(verts, faces, mesh_to_faces_first_idx, num_faces_per_mesh, uniforms, w.cdf, V, F, N,
                                                     S, samples, normals, face_idxs, bary);
  return launch_status();
}

P3D_API size_t p3d_sample_points_backward_workspace_bytes(int64_t F, int with_normals, int64_t num_sorted) {
  if (F < 0 || num_sorted < 0) return 0;
  return align_up((size_t)F * (with_normals ? 12 : 9) * sizeof(float), 256) + sample_points_ordered_bytes(num_sorted);
}

P3D_API int p3d_sample_points_backward(const float* grad_samples, const float* grad_normals, const float* verts, const int64_t* faces,
                                       const int64_t* face_idxs, const float* bary, const int64_t* sorted_samples, int64_t num_sorted,
                                       int64_t V, int64_t F, int64_t num_samples, float* grad_face_verts, void* workspace,
                                       size_t workspace_bytes, p3d_stream_t stream) {
  if (V < 0 || F < 0 || num_samples < 0 || num_sorted < 0 || num_sorted > num_samples || F > INT32_MAX) return P3D_ERR_INVALID_ARG;
  if (F == 0) return P3D_OK;
  if (!grad_face_verts || !faces || (V > 0 && !verts)) return P3D_ERR_INVALID_ARG;
  if (num_samples > 0 && (!grad_samples || !face_idxs || !bary)) return P3D_ERR_INVALID_ARG;
  const int nv = grad_normals ? 12 : 9;
  if (!workspace || workspace_bytes < p3d_sample_points_backward_workspace_bytes(F, grad_normals != nullptr, sorted_samples ? num_sorted : 0))
    return P3D_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* rows = static_cast<float*>(workspace);
  void* partials = static_cast<char*>(workspace) + align_up((size_t)F * nv * sizeof(float), 256);
  int st;
  if (sorted_samples)
    st = sample_points_ordered_rows(face_idxs, bary, grad_samples, grad_normals, sorted_samples, num_sorted, num_samples, F, nv, rows,
                                    partials, s);
  else
    st = grad_normals ? backward_rows_atomic<12>(face_idxs, bary, grad_samples, grad_normals, num_samples, F, rows, s)
                      : backward_rows_atomic<9>(face_idxs, bary, grad_samples, grad_normals, num_samples, F, rows, s);
  if (st != P3D_OK) return st;
  LaunchScope ls("sample_points_backward_finish", s);
  if (grad_normals)
    face_finish_kernel<12><<<stream_blocks(F), 256, 0, s>>>(rows, verts, faces, V, F, grad_face_verts);
  else
    face_finish_kernel<9><<<stream_blocks(F), 256, 0, s>>>(rows, verts, faces, V, F, grad_face_verts);
  return launch_status();
}
