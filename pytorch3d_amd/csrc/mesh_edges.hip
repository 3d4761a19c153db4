// mesh_edges.hip -- the unique edges of a packed face list, every face's three edge ids, and per vertex the edges that name it
// (the reference's Meshes._compute_edges_packed: two global sorts of 3 F keys, a unique and a scatter_add there).
// Contract: implicit_abi.h (p3di_mesh_edges_build).  Count -> scan -> fill -> sort the rows -> scan -> emit; integers only.
//
// The key order lo V + hi is lexicographic in (lo, hi), so no global sort is needed: bucket by lo, order inside the bucket.  The
// table the subdivision's backward needs -- the edges that name a vertex as hi -- is the same problem with lo and hi swapped, so both
// go through the same kernels as ONE set of R = 2 V rows: row v holds (hi, corner) of the corners with lo == v, row V + v holds
// (lo, corner) of the corners with hi == v.  A slot is one 64-bit key, other << 32 | corner; the corners of a row are distinct, so
// the keys are, and the sorted row does not depend on the order the fill's tickets came in.
//
//   zero_kernel      the counters
//   count_kernel     a lane per corner: ids checked (a bad one sets the flag; its corner is skipped here and in fill), two counts
//   scan_*           exclusive scan over the R counts: block totals, one workgroup over the totals, apply.  The apply pass of the
//                    first scan lists the rows longer than kRowRegs
//   fill_kernel      a lane per corner: two tickets, two keys
//   rows_short       a lane per row of up to kRowRegs entries: a bitonic network over registers (static indices)
//   rows_long        kLongGroups workgroups take the listed rows in turns: up to kRowLds entries a bitonic sort in LDS, beyond that
//                    a rank sort over the row's own slots (every lane counts the keys below its own: O(len^2), rare, only right)
//                    both kernels store, per slot, the index of its run of equal first halves, and per row the number of runs
//   scan_*           exclusive scan over the R run counts: row_offsets
//   emit_kernel<0>   a lane per slot of the lo rows: face_edges, and the first slot of a run its edge and the edge's mesh
//   emit_kernel<1>   a lane per slot of the hi rows: the first slot of a run stores the id of its edge (face_edges of its corner);
//                    and edge_first and the record the host reads
#include "implicit_abi.h"
#include "p3d_common.h"
#include "scan_blocks.h"

namespace p3d {
namespace {

constexpr int kLanes = P3D_MESH_EDGES_BLOCK;
constexpr int kItems = P3D_MESH_EDGES_ITEMS;
constexpr int kCarryLanes = P3D_MESH_EDGES_CARRY_BLOCK;
constexpr int kRowRegs = P3D_MESH_EDGES_ROW_REGISTERS;
constexpr int kRowLds = P3D_MESH_EDGES_ROW_LDS;
constexpr int kLongGroups = P3D_MESH_EDGES_LONG_GROUPS;
static_assert(kLanes == 256 && kItems % kLanes == 0 && kCarryLanes % kWave == 0 && kCarryLanes <= 1024, "launch constants");
static_assert(kRowRegs == 16, "the register network is written for 16 keys");
static_assert((kRowLds & (kRowLds - 1)) == 0 && kRowLds >= kLanes && kRowLds * 8 <= 32768, "the LDS rung sorts a power of two");

typedef unsigned long long key_t;

struct Workspace {
  int* counts;     // R + 1: the rows' lengths, then their exclusive scan
  int* cursor;     // R: the fill's tickets
  int* misc;       // 4: invalid flag, rows > kRowRegs, rows > kRowLds, unused  (counts, cursor and misc are one zeroed range)
  int* totals;     // blocks + 1: the scans' block totals
  int* runs;       // R + 1: runs per row (its scan goes to row_offsets)
  int* slot_row;   // S
  int* slot_run;   // S
  int* long_rows;  // S / (kRowRegs + 1) + 1
  key_t* keys;     // S
  key_t* keys2;    // S: the rank sort's copy
  size_t zero_ints, bytes;
};

bool sizes_ok(int64_t V, int64_t F) { return V >= 1 && F >= 1 && 6 * F <= INT32_MAX && 2 * V + 1 <= INT32_MAX; }

Workspace carve(void* workspace, int64_t V, int64_t F) {
  const size_t R = (size_t)(2 * V), S = (size_t)(6 * F);
  Arena a(workspace, ~(size_t)0);
  Workspace w;
  w.zero_ints = R + 1 + R + 4;
  w.counts = a.take<int>(w.zero_ints);
  w.cursor = w.counts ? w.counts + R + 1 : nullptr;
  w.misc = w.counts ? w.cursor + R : nullptr;
  w.totals = a.take<int>((size_t)ceil_div((int64_t)R, kItems) + 1);
  w.runs = a.take<int>(R + 1);
  w.slot_row = a.take<int>(S);
  w.slot_run = a.take<int>(S);
  w.long_rows = a.take<int>(S / (kRowRegs + 1) + 1);
  w.keys = a.take<key_t>(S);
  w.keys2 = a.take<key_t>(S);
  w.bytes = a.off;
  return w;
}

__global__ __launch_bounds__(kLanes) void zero_kernel(int* p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x; i < n; i += (int64_t)gridDim.x * kLanes) p[i] = 0;
}

// (lo, hi) of the edge opposite corner c; false where one of its ids is outside [0, V)
__device__ __forceinline__ bool corner_edge(const int64_t* __restrict__ faces, int c, int64_t V, int* lo, int* hi) {
  const int f = c / 3, k = c - 3 * f;
  const int64_t a = faces[3 * (int64_t)f + (k == 2 ? 0 : k + 1)], b = faces[3 * (int64_t)f + (k == 0 ? 2 : k - 1)];
  if (a < 0 || a >= V || b < 0 || b >= V) return false;
  *lo = (int)(a < b ? a : b);
  *hi = (int)(a < b ? b : a);
  return true;
}

__global__ __launch_bounds__(kLanes) void count_kernel(const int64_t* __restrict__ faces, int corners, int64_t V, int* counts, int* misc) {
  const int c = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (c >= corners) return;
  const int64_t own = faces[c];
  int lo, hi;
  const bool ok = corner_edge(faces, c, V, &lo, &hi);
  if (!ok || own < 0 || own >= V) misc[0] = 1;  // every writer stores the same value
  if (!ok) return;
  atomicAdd(&counts[lo], 1);
  atomicAdd(&counts[(int)V + hi], 1);
}

__global__ __launch_bounds__(kLanes) void fill_kernel(const int64_t* __restrict__ faces, int corners, int64_t V,
                                                      const int* __restrict__ offsets, int* cursor, key_t* __restrict__ keys,
                                                      int* __restrict__ slot_row) {
  const int c = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (c >= corners) return;
  int lo, hi;
  if (!corner_edge(faces, c, V, &lo, &hi)) return;
  const int rows[2] = {lo, (int)V + hi}, others[2] = {hi, lo};
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int slot = offsets[rows[s]] + atomicAdd(&cursor[rows[s]], 1);
    keys[slot] = ((key_t)(unsigned)others[s] << 32) | (unsigned)c;
    slot_row[slot] = rows[s];
  }
}

// ---- the exclusive scan of a[0..n) in place, a[n] = the total: three launches -------------------------------------------------------
__global__ __launch_bounds__(kLanes) void scan_totals_kernel(const int* __restrict__ a, int n, int* __restrict__ totals) {
  __shared__ int wsum[kLanes / kWave];
  int sum = 0;
  for (int r = 0; r < kItems / kLanes; ++r) {
    const int i = (int)blockIdx.x * kItems + r * kLanes + (int)threadIdx.x;
    sum += i < n ? a[i] : 0;
  }
  const int incl = wave_inclusive(sum);
  int total;
  block_exclusive<kLanes / kWave>(0, __shfl(incl, kWave - 1), wsum, &total);
  if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// one workgroup: the exclusive scan of totals[0..nb) in rounds, in place, the grand total behind the last
__global__ __launch_bounds__(kCarryLanes) void scan_carry_kernel(int* totals, int nb) {
  __shared__ int wsum[kCarryLanes / kWave];
  int running = 0;
  for (int base = 0; base < nb; base += kCarryLanes) {
    const int i = base + (int)threadIdx.x;
    const int x = i < nb ? totals[i] : 0;
    const int incl = wave_inclusive(x);
    int total;
    const int ex = running + block_exclusive<kCarryLanes / kWave>(incl - x, __shfl(incl, kWave - 1), wsum, &total);
    if (i < nb) totals[i] = ex;
    running += total;
  }
  if (threadIdx.x == 0) totals[nb] = running;
}

// LIST: a holds row lengths; the rows longer than kRowRegs are appended to long_rows (the order of the list decides nothing: every
// listed row is sorted on its own) and counted in misc[1], those longer than kRowLds in misc[2]
template <bool LIST>
__global__ __launch_bounds__(kLanes) void scan_apply_kernel(int* a, int n, const int* __restrict__ totals, int nb, int* out,
                                                            int* misc, int* __restrict__ long_rows) {
  __shared__ int wsum[kLanes / kWave];
  int running = totals[blockIdx.x];
  for (int r = 0; r < kItems / kLanes; ++r) {  // every lane stays for the barriers
    const int i = (int)blockIdx.x * kItems + r * kLanes + (int)threadIdx.x;
    const int x = i < n ? a[i] : 0;
    const int incl = wave_inclusive(x);
    int total;
    const int ex = running + block_exclusive<kLanes / kWave>(incl - x, __shfl(incl, kWave - 1), wsum, &total);
    if (i < n) out[i] = ex;
    running += total;
    if (LIST && x > kRowRegs) {
      long_rows[atomicAdd(&misc[1], 1)] = i;
      if (x > kRowLds) atomicAdd(&misc[2], 1);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = totals[nb];
}

void scan(int* a, int n, int* totals, int* out, int* misc, int* long_rows, hipStream_t st) {
  const int nb = (int)ceil_div(n, kItems);
  scan_totals_kernel<<<nb, kLanes, 0, st>>>(a, n, totals);
  scan_carry_kernel<<<1, kCarryLanes, 0, st>>>(totals, nb);
  if (long_rows)
    scan_apply_kernel<true><<<nb, kLanes, 0, st>>>(a, n, totals, nb, out, misc, long_rows);
  else
    scan_apply_kernel<false><<<nb, kLanes, 0, st>>>(a, n, totals, nb, out, misc, long_rows);
}

// ---- the rows -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned first_half(key_t k) { return (unsigned)(k >> 32); }

// a lane per row of up to kRowRegs entries
__global__ __launch_bounds__(kLanes) void rows_short_kernel(const int* __restrict__ offsets, int R, key_t* __restrict__ keys,
                                                            int* __restrict__ slot_run, int* __restrict__ runs) {
  const int row = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  if (row >= R) return;
  const int base = offsets[row], len = offsets[row + 1] - base;
  if (len > kRowRegs) return;  // rows_long_kernel's
  if (len == 0) {
    runs[row] = 0;
    return;
  }
  key_t k[kRowRegs];
#pragma unroll
  for (int i = 0; i < kRowRegs; ++i) k[i] = i < len ? keys[base + i] : ~(key_t)0;
#pragma unroll
  for (int size = 2; size <= kRowRegs; size <<= 1) {
#pragma unroll
    for (int j = size >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int i = 0; i < kRowRegs; ++i) {
        const int l = i ^ j;
        if (l > i) {
          const key_t a = k[i], b = k[l];
          const bool swap = (i & size) == 0 ? a > b : a < b;
          k[i] = swap ? b : a;
          k[l] = swap ? a : b;
        }
      }
    }
  }
  int run = 0;
#pragma unroll
  for (int i = 0; i < kRowRegs; ++i) {
    if (i < len) {
      if (i > 0 && first_half(k[i]) != first_half(k[i - 1])) ++run;
      keys[base + i] = k[i];
      slot_run[base + i] = run;
    }
  }
  runs[row] = run + 1;
}

// kLongGroups workgroups over the listed rows.  The row's slots are written and read again by this workgroup alone, with a barrier
// in between.
__global__ __launch_bounds__(kLanes) void rows_long_kernel(const int* __restrict__ offsets, const int* __restrict__ misc,
                                                           const int* __restrict__ long_rows, key_t* keys, key_t* keys2, int* slot_run,
                                                           int* __restrict__ runs) {
  __shared__ key_t lds[kRowLds];
  __shared__ int wsum[kLanes / kWave];
  const int listed = misc[1], tid = (int)threadIdx.x;
  for (int q = (int)blockIdx.x; q < listed; q += (int)gridDim.x) {
    const int row = long_rows[q], base = offsets[row], len = offsets[row + 1] - base;
    key_t* mine = keys + base;
    if (len <= kRowLds) {
      int P = kLanes;
      while (P < len) P <<= 1;
      for (int i = tid; i < P; i += kLanes) lds[i] = i < len ? mine[i] : ~(key_t)0;
      __syncthreads();
      for (int size = 2; size <= P; size <<= 1) {
        for (int j = size >> 1; j > 0; j >>= 1) {
          for (int i = tid; i < P; i += kLanes) {
            const int l = i ^ j;
            if (l > i) {
              const key_t a = lds[i], b = lds[l];
              if ((i & size) == 0 ? a > b : a < b) {
                lds[i] = b;
                lds[l] = a;
              }
            }
          }
          __syncthreads();
        }
      }
      for (int i = tid; i < len; i += kLanes) mine[i] = lds[i];
    } else {
      key_t* copy = keys2 + base;
      for (int i = tid; i < len; i += kLanes) copy[i] = mine[i];
      __syncthreads();
      for (int i = tid; i < len; i += kLanes) {
        const key_t k = copy[i];
        int rank = 0;
        for (int j = 0; j < len; ++j) rank += copy[j] < k ? 1 : 0;
        mine[rank] = k;  // the keys of a row are distinct: the ranks are a permutation
      }
    }
    __syncthreads();
    int running = 0;
    for (int c0 = 0; c0 < len; c0 += kLanes) {  // every lane stays for the barriers
      const int i = c0 + tid;
      const bool first = i < len && (i == 0 || first_half(mine[i]) != first_half(mine[i - 1]));
      const unsigned long long ballot = __ballot(first);
      int total;
      const int before = running + block_exclusive<kLanes / kWave>(mask_rank(ballot), __popcll(ballot), wsum, &total);
      if (i < len) slot_run[base + i] = before + (first ? 1 : 0) - 1;
      running += total;
    }
    if (tid == 0) runs[row] = running;
    __syncthreads();
  }
}

// the mesh of item x: the largest n < N with first[n] <= x (empty meshes are stepped over)
__device__ __forceinline__ int mesh_of(const int* __restrict__ first, int N, int x) {
  int lo = 0, hi = N;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int clamp_row(int v, int V) { return v < 0 ? 0 : v > V ? V : v; }

// PHASE 0: the slots of the lo rows.  PHASE 1: the slots of the hi rows (reads the face_edges of phase 0), edge_first and the record.
template <int PHASE>
__global__ __launch_bounds__(kLanes) void emit_kernel(const int* __restrict__ offsets, const int* __restrict__ row_offsets,
                                                      const key_t* __restrict__ keys, const int* __restrict__ slot_row,
                                                      const int* __restrict__ slot_run, const int* __restrict__ vert_first, int V, int N,
                                                      const int* __restrict__ misc, int* edges, int* face_edges, int* __restrict__ edge_mesh,
                                                      int* __restrict__ edge_first, int* __restrict__ hi_edges, int64_t* __restrict__ record) {
  const int i = (int)blockIdx.x * kLanes + (int)threadIdx.x;
  const int E = row_offsets[V];
  if (PHASE == 1) {
    if (i <= N) edge_first[i] = row_offsets[clamp_row(vert_first[i], V)];
    if (i < N) record[4 + i] = (int64_t)(row_offsets[clamp_row(vert_first[i + 1], V)] - row_offsets[clamp_row(vert_first[i], V)]);
    if (i == 0) {
      record[0] = E;
      record[1] = misc[0];
      record[2] = misc[1];
      record[3] = misc[2];
    }
  }
  const int lo_slots = offsets[V];
  if (PHASE == 0 ? i >= lo_slots : (i < lo_slots || i >= offsets[2 * V])) return;
  const int row = slot_row[i];
  const key_t k = keys[i];
  const int other = (int)first_half(k), corner = (int)(unsigned)k;
  const bool first = i == offsets[row] || first_half(keys[i - 1]) != (unsigned)other;
  const int id = row_offsets[row] + slot_run[i];
  if (PHASE == 0) {
    face_edges[corner] = id;
    if (first) {
      edges[2 * id] = row;
      edges[2 * id + 1] = other;
      edge_mesh[id] = mesh_of(vert_first, N, row);
    }
  } else if (first) {
    hi_edges[id - E] = face_edges[corner];
  }
}

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API size_t p3di_mesh_edges_workspace_bytes(int64_t V, int64_t F) { return sizes_ok(V, F) ? carve(nullptr, V, F).bytes : 0; }

P3D_API int p3di_mesh_edges_build(const int64_t* faces, const int32_t* vert_first, int64_t V, int64_t F, int64_t N, void* workspace,
                                  size_t workspace_bytes, int32_t* edges, int32_t* face_edges, int32_t* edge_mesh, int32_t* edge_first,
                                  int32_t* row_offsets, int32_t* hi_edges, int64_t* record, p3d_stream_t stream) {
  if (!sizes_ok(V, F) || N < 1 || N >= INT32_MAX || !faces || !vert_first || !edges || !face_edges || !edge_mesh || !edge_first ||
      !row_offsets || !hi_edges || !record)
    return P3D_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < carve(nullptr, V, F).bytes) return P3D_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const Workspace w = carve(workspace, V, F);
  const int R = (int)(2 * V), corners = (int)(3 * F), S = (int)(6 * F);
  const unsigned corner_blocks = (unsigned)ceil_div(corners, kLanes);
  const int64_t tail = S > N + 1 ? S : N + 1;
  LaunchScope ls("mesh_edges_build", st);
  zero_kernel<<<stream_blocks((int64_t)w.zero_ints), kLanes, 0, st>>>(w.counts, (int64_t)w.zero_ints);
  count_kernel<<<corner_blocks, kLanes, 0, st>>>(faces, corners, V, w.counts, w.misc);
  scan(w.counts, R, w.totals, w.counts, w.misc, w.long_rows, st);
  fill_kernel<<<corner_blocks, kLanes, 0, st>>>(faces, corners, V, w.counts, w.cursor, w.keys, w.slot_row);
  rows_short_kernel<<<(unsigned)ceil_div(R, kLanes), kLanes, 0, st>>>(w.counts, R, w.keys, w.slot_run, w.runs);
  rows_long_kernel<<<kLongGroups, kLanes, 0, st>>>(w.counts, w.misc, w.long_rows, w.keys, w.keys2, w.slot_run, w.runs);
  scan(w.runs, R, w.totals, row_offsets, w.misc, nullptr, st);
  emit_kernel<0><<<(unsigned)ceil_div(S, kLanes), kLanes, 0, st>>>(w.counts, row_offsets, w.keys, w.slot_row, w.slot_run, vert_first,
                                                                   (int)V, (int)N, w.misc, edges, face_edges, edge_mesh, edge_first,
                                                                   hi_edges, record);
  emit_kernel<1><<<(unsigned)ceil_div(tail, kLanes), kLanes, 0, st>>>(w.counts, row_offsets, w.keys, w.slot_row, w.slot_run, vert_first,
                                                                      (int)V, (int)N, w.misc, edges, face_edges, edge_mesh, edge_first,
                                                                      hi_edges, record);
  return launch_status();
}
