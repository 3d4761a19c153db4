// point_mesh_grid.hip -- the two point-query directions of p3d_point_mesh_forward (point -> nearest triangle, point -> nearest segment
// of its batch element) through a uniform grid per element: the same dists and idxs, bit for bit, without looking at most pairs.
// implicit_abi.h has the contract; DESIGN 8.32 the figures.
//
// The search is EXACT.  A pair's distance is point_mesh_geom.h's tri_dist / seg_dist from the record make_tri / make_seg builds, as
// in point_mesh.hip; the winner is the minimum under the total order (distance, -index), which is idempotent and independent of the
// order and the number of offers; the grid only decides which pairs are never evaluated, and a lane stops only where a proven lower
// bound (stop_bound below) says that no target it has not seen could win.
//
// Triangles and segments have extent.  A target is REGISTERED in every cell its axis-aligned box overlaps -- at most kMaxSpan cells
// along an axis and P3D_POINT_MESH_GRID_MAX_REFS in all.  A target beyond that (a ground plane, a sliver across the mesh), one with a
// coordinate that is not finite, and a triangle whose inside branch is ill-conditioned (grid_target below; the bound's proof needs
// the condition) goes to the element's LARGE LIST instead, which every wave of the element scans first.  So a target has a bounded
// number of references and the workspace is a function of (N, Q, T) alone.
//
// Launches, no host read, no float atomic, no memset:
//   bounds   per element 1..kBoundsBlocks workgroups: min / max of the finite vertex coordinates of its targets (fminf / fmaxf trees:
//            any order gives the same bits); the same launch clears the cell counts and the large lists' lengths.
//   header   per element one wave: the box, the cell side from the box volume, the target count and the occupancy (knn_grid.hip's
//            choice); at most max(targets of the element, 1) cells, so all elements' cells fit a pool of T + N ints: element n's
//            cells start at t0 + n, its cap + 1 scan entries at t0 + 2 n.
//   count    per element: a lane per target adds 1 to every cell of its box, a lane per query to its own cell (integer atomics).
//   scan     per (element, table) one workgroup: the exclusive scan of the counts (scan_blocks.h).
//   fill     the count pass again: a reference's place is its cell's start + a ticket (atomicSub on the count, which ends at 0); a
//            large target takes a ticket of its element's list; a query writes (x, y, z, row) at its place, so that a wave owns 64
//            neighbouring queries.  The order inside a cell and inside the large list differs from run to run; the result does not.
//   search   one wave per 64 ordered queries.  The large list first, then the box of cells the wave's queries occupy, grown ring by
//            ring; x runs fastest, so a row of cells is one span of the references, a ring a list of spans (knn_grid.hip's walk).
//            A tile is kTile references: lane l builds the record of reference l ONCE (make_tri: edges, normal, the barycentric
//            constants), every lane then reads the 64 records by broadcast ds_read_b128, as point_mesh.hip does.  A reference that
//            two cells share is offered twice: harmless.  When a wave has staged as many references as its element has targets and
//            a lane still cannot stop (a NaN query, a query far outside the box, a cloud far from the origin, cells below the
//            slack), it scans the element's targets in index order once -- all pairs -- and is done: never more than that.
//   sums     (only with `sums`) per 64 consecutive queries IN THE ORIGINAL ORDER the wave sum of dists[q] * weights[n], then
//            fixed_sum.h's segment sum: the tree, and so the bits, of p3d_point_mesh_forward's fused loss.
//
// Every loop has a bound known before it starts: rings <= the largest grid dimension + 1, span batches <= ceil(2 dim_y dim_z / 64),
// tiles <= ceil(references / kTile); no workgroup waits for another.  Every index read from a table is checked against its range
// before it is used: first-index arrays that are not ascending give wrong numbers, never an access outside the buffers.
#include "fixed_sum.h"
#include "implicit_abi.h"
#include "point_mesh_geom.h"
#include "scan_blocks.h"

namespace p3d {
namespace {

using namespace pm;

constexpr int kTile = kWave;  // lane l builds the record of reference l of a tile
constexpr int kMaxRefs = P3D_POINT_MESH_GRID_MAX_REFS;
constexpr int kMaxSpan = 3;  // cells along one axis of a registered target's box: stop_bound's L rests on it
constexpr int kBoundsBlocks = 64, kBoundsRows = 4096;
constexpr int kScanLanes = 1024, kScanItems = 8;
constexpr int kItemBlocks = 64;  // workgroups per element of count / fill at most

struct Header {
  float lo[3];   // the box's minimum corner
  float inv_h;   // 1 / cell side; 0 where the grid is a single cell
  float hs;      // a float BELOW the real 1 / inv_h
  float hup;     // a float ABOVE it
  float mbox;    // the largest |coordinate| of the box
  int dim[3];
  int cells;
  int pad[5];
};
static_assert(sizeof(Header) == 64, "one header per 64 bytes");

struct Range {
  int64_t q0, q1, t0, t1;
};
__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
// p3d_point_mesh_forward's reading of the first-index arrays
__device__ __forceinline__ Range elem_range(const int64_t* qfirst, const int64_t* tfirst, int64_t n, int64_t N, int64_t Q, int64_t T) {
  Range r;
  r.q0 = clamp64(qfirst[n], 0, Q), r.q1 = n + 1 < N ? clamp64(qfirst[n + 1], r.q0, Q) : Q;
  r.t0 = clamp64(tfirst[n], 0, T), r.t1 = n + 1 < N ? clamp64(tfirst[n + 1], r.t0, T) : T;
  return r;
}

__device__ __forceinline__ float pos_inf() { return __int_as_float(0x7f800000); }
__device__ __forceinline__ float neg_inf() { return __int_as_float(0xff800000); }
__device__ __forceinline__ float wave_fmin(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fminf(x, __shfl_xor(x, o));
  return x;
}
__device__ __forceinline__ float wave_fmax(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
  return x;
}
__device__ __forceinline__ int wave_imin(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int y = __shfl_xor(x, o);
    x = y < x ? y : x;
  }
  return x;
}
__device__ __forceinline__ int wave_imax(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int y = __shfl_xor(x, o);
    x = y > x ? y : x;
  }
  return x;
}

// the cell coordinate, before the clamp: two float32 operations, THE SAME in count, fill and search; monotone in x
__device__ __forceinline__ float cell_coord(float x, float lo, float inv_h) { return (x - lo) * inv_h; }
// clamp(floor(t), 0, dim - 1); NaN goes to 0
__device__ __forceinline__ int cell_clamp(float t, int dim) { return (int)fminf(fmaxf(t, 0.0f), (float)(dim - 1)); }

// the workspace: element n's tables lie at offsets that its first indices give
struct Tables {
  float* partials;  // N kBoundsBlocks 6
  Header* headers;  // N
  int* counts;      // table 0 (targets) T + N, table 1 (queries) T + N, then N large-list lengths: cleared by bounds
  int* starts;      // per table T + 2 N
  int* refs;        // kMaxRefs T: element n's from kMaxRefs t0
  int* large;       // T: element n's from t0
  float4* qrec;     // Q: element n's from q0, in cell order
  float* sums;      // N ceil(Q / 64) wave partials of the fused loss
  int64_t N, Q, T;
  size_t bytes;
  Tables(void* ws, int64_t N_, int64_t Q_, int64_t T_) : N(N_), Q(Q_), T(T_) {
    Arena a(ws, ~(size_t)0);
    partials = a.take<float>((size_t)N * kBoundsBlocks * 6);
    headers = a.take<Header>((size_t)N);
    counts = a.take<int>(2 * (size_t)(T + N) + (size_t)N);
    starts = a.take<int>(2 * (size_t)(T + 2 * N));
    refs = a.take<int>((size_t)kMaxRefs * (size_t)T);
    large = a.take<int>((size_t)T);
    qrec = a.take<float4>((size_t)Q);
    sums = a.take<float>((size_t)N * (size_t)ceil_div(Q, kWave));
    bytes = a.off;
  }
  __host__ __device__ int64_t ncleared() const { return 2 * (T + N) + N; }
  __device__ __forceinline__ int* cell_counts(int table, int64_t n, int64_t t0) const { return counts + table * (T + N) + t0 + n; }
  __device__ __forceinline__ int* cell_starts(int table, int64_t n, int64_t t0) const { return starts + table * (T + 2 * N) + t0 + 2 * n; }
  __device__ __forceinline__ int* large_count(int64_t n) const { return counts + 2 * (T + N) + n; }
};

struct Args {
  const float *queries, *targets;
  const int64_t *qfirst, *tfirst;
  int64_t N, Q, T;
  double min_area;
};

// grid: N * bpc workgroups of 256.  partials[(n * kBoundsBlocks + b) * 6 + {0..2: min, 3..5: max}] for b < bpc.
__global__ __launch_bounds__(256) void pmg_bounds_kernel(Args A, int tf, int bpc, Tables W) {
  __shared__ float part[4][6];
  const int64_t ncl = W.ncleared();
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < ncl; v += (int64_t)gridDim.x * 256) W.counts[v] = 0;
  const int64_t n = blockIdx.x / bpc;
  const int b = (int)(blockIdx.x % bpc);
  const Range r = elem_range(A.qfirst, A.tfirst, n, A.N, A.Q, A.T);
  float lo[3] = {pos_inf(), pos_inf(), pos_inf()}, hi[3] = {neg_inf(), neg_inf(), neg_inf()};
  const int64_t corners = (r.t1 - r.t0) * (tf / 3);
  for (int64_t i = (int64_t)b * 256 + threadIdx.x; i < corners; i += (int64_t)bpc * 256) {
    const float* p = A.targets + r.t0 * tf + i * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float v = p[a];
      if (fabsf(v) < pos_inf()) lo[a] = fminf(lo[a], v), hi[a] = fmaxf(hi[a], v);
    }
  }
  const int wave = (int)threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float l = wave_fmin(lo[a]), h = wave_fmax(hi[a]);
    if (lane_id() == 0) part[wave][a] = l, part[wave][3 + a] = h;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = (int)threadIdx.x;
    float v = part[0][a];
    for (int w = 1; w < 4; ++w) v = a < 3 ? fminf(v, part[w][a]) : fmaxf(v, part[w][a]);
    W.partials[(n * kBoundsBlocks + b) * 6 + a] = v;
  }
}

// grid: N workgroups of one wave.  Lane 0 chooses the grid in double (knn_grid.hip's choice): nothing here is on the hot path.
__global__ __launch_bounds__(64) void pmg_header_kernel(Args A, int bpc, int occupancy, Tables W) {
  const int64_t n = blockIdx.x;
  const int lane = (int)threadIdx.x;
  float lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = wave_fmin(lane < bpc ? W.partials[(n * kBoundsBlocks + lane) * 6 + a] : pos_inf());
    hi[a] = wave_fmax(lane < bpc ? W.partials[(n * kBoundsBlocks + lane) * 6 + 3 + a] : neg_inf());
  }
  if (lane != 0) return;
  const Range r = elem_range(A.qfirst, A.tfirst, n, A.N, A.Q, A.T);
  const int64_t tcount = r.t1 - r.t0;
  const int64_t cap = tcount < 1 ? 1 : (tcount > P3D_POINT_MESH_GRID_MAX_CELLS ? P3D_POINT_MESH_GRID_MAX_CELLS : tcount);
  Header H;
  for (int a = 0; a < 5; ++a) H.pad[a] = 0;
  H.inv_h = 0.0f, H.hs = 0.0f, H.hup = 0.0f, H.mbox = 0.0f, H.cells = 1;
  double ext[3];
  bool finite = tcount > 0;
  for (int a = 0; a < 3; ++a) {
    H.dim[a] = 1;
    ext[a] = (double)hi[a] - (double)lo[a];
    finite = finite && fabsf(lo[a]) < pos_inf() && fabsf(hi[a]) < pos_inf();  // false too where no coordinate was finite
  }
  for (int a = 0; a < 3; ++a) {
    H.lo[a] = finite ? lo[a] : 0.0f;
    if (finite) H.mbox = fmaxf(H.mbox, fmaxf(fabsf(lo[a]), fabsf(hi[a])));
  }
  if (finite) {
    int64_t target = (tcount + occupancy - 1) / occupancy;
    target = target < 1 ? 1 : (target > cap ? cap : target);
    // the side that gives `target` cells over the axes longer than a cell: an axis shorter than the side leaves the product
    bool active[3] = {ext[0] > 0.0, ext[1] > 0.0, ext[2] > 0.0};
    double h = 0.0;
    for (int it = 0; it < 4; ++it) {
      int m = 0;
      double vol = 1.0;
      for (int a = 0; a < 3; ++a) {
        if (active[a]) vol *= ext[a], ++m;
      }
      if (m == 0) {
        h = 0.0;
        break;
      }
      h = m == 1 ? vol / (double)target : (m == 2 ? sqrt(vol / (double)target) : cbrt(vol / (double)target));
      if (it < 3) {
        for (int a = 0; a < 3; ++a) active[a] = active[a] && ext[a] >= h;
      }
    }
    // dims = ceil(ext / h), at least 1; a product above the cap lengthens the side (at most 8 times, then a single cell)
    int64_t dim[3] = {1, 1, 1};
    bool fits = false;
    for (int it = 0; it < 8 && h > 0.0 && !fits; ++it) {
      double prod = 1.0;
      for (int a = 0; a < 3; ++a) {
        double d = ceil(ext[a] / h);
        d = d >= 1.0 ? (d <= (double)cap ? d : (double)cap) : 1.0;  // NaN: 1
        dim[a] = (int64_t)d;
        prod *= d;
      }
      fits = prod <= (double)cap;
      if (!fits) h *= cbrt(prod / (double)cap) * 1.02;
    }
    const float inv_h = h > 0.0 ? (float)(1.0 / h) : 0.0f;
    if (fits && inv_h > 0.0f && inv_h < pos_inf() && dim[0] * dim[1] * dim[2] <= cap) {
      H.inv_h = inv_h;
      H.hs = (1.0f / inv_h) * (1.0f - 0x1p-18f);
      H.hup = (1.0f / inv_h) * (1.0f + 0x1p-18f);
      if (!(H.hup < pos_inf())) H.hs = 0.0f, H.hup = pos_inf();
      for (int a = 0; a < 3; ++a) H.dim[a] = (int)dim[a];
      H.cells = (int)(dim[0] * dim[1] * dim[2]);
    }
  }
  W.headers[n] = H;
}

// Whether target j of an element is registered in cells (then its box of cells c0..c1), or goes to the large list.  Registered:
// every coordinate finite, at most kMaxSpan cells along each axis and kMaxRefs in all, and for a triangle whose inside branch is
// possible (ok == 1) the CONDITION  norm >= max(d00, d11, l12) / 4  and  norm >= 2^-7  that stop_bound's proof uses.  The same
// instructions in count and fill: the two passes decide alike.
template <int TK>
__device__ __forceinline__ bool grid_target(const Header& H, const float* src, double min_area, int (&c0)[3], int (&c1)[3]) {
  constexpr int TF = kind_floats(TK);
  float v[TF];
#pragma unroll
  for (int c = 0; c < TF; ++c) v[c] = src[c];
  bool fine = true;
  int refs = 1;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float lo = v[a], hi = v[a];
#pragma unroll
    for (int c = 3; c < TF; c += 3) lo = fminf(lo, v[c + a]), hi = fmaxf(hi, v[c + a]);
#pragma unroll
    for (int c = 0; c < TF; c += 3) fine = fine && fabsf(v[c + a]) < pos_inf();
    c0[a] = cell_clamp(cell_coord(lo, H.lo[a], H.inv_h), H.dim[a]);
    c1[a] = cell_clamp(cell_coord(hi, H.lo[a], H.inv_h), H.dim[a]);
    fine = fine && c1[a] >= c0[a] && c1[a] - c0[a] < kMaxSpan;
    refs *= c1[a] - c0[a] + 1;
  }
  fine = fine && refs <= kMaxRefs;
  if constexpr (TK == kTri) {
    const Tri f = make_tri(load3(v), load3(v + 3), load3(v + 6), min_area);
    const float l2 = fmaxf(f.d00, fmaxf(f.d11, f.l12));
    fine = fine && (f.ok == 0.0f || (f.norm >= 0.25f * l2 && f.norm >= 0x1p-7f));
  }
  return fine;
}

// grid: N * ipb workgroups of 256; workgroup b of an element takes its items b * 256 + thread, + ipb * 256, ...
template <int TK, bool FILL>
__global__ __launch_bounds__(256) void pmg_place_kernel(Args A, int ipb, Tables W) {
  constexpr int TF = kind_floats(TK);
  const int64_t n = blockIdx.x / ipb;
  const int64_t first = (int64_t)(blockIdx.x % ipb) * 256 + threadIdx.x, step = (int64_t)ipb * 256;
  const Range r = elem_range(A.qfirst, A.tfirst, n, A.N, A.Q, A.T);
  const int64_t tcount = r.t1 - r.t0, qcount = r.q1 - r.q0;
  const Header H = W.headers[n];
  int* const tc = W.cell_counts(0, n, r.t0);
  int* const qc = W.cell_counts(1, n, r.t0);
  const int* const ts = W.cell_starts(0, n, r.t0);
  const int* const qs = W.cell_starts(1, n, r.t0);
  for (int64_t j = first; j < tcount; j += step) {
    int c0[3], c1[3];
    if (grid_target<TK>(H, A.targets + (r.t0 + j) * TF, A.min_area, c0, c1)) {
      for (int z = c0[2]; z <= c1[2]; ++z)
        for (int y = c0[1]; y <= c1[1]; ++y)
          for (int x = c0[0]; x <= c1[0]; ++x) {
            const int c = (z * H.dim[1] + y) * H.dim[0] + x;
            if constexpr (FILL) {
              const int ticket = atomicSub(tc + c, 1) - 1;  // count - 1 .. 0: every place of the cell once
              const int64_t place = (int64_t)ts[c] + ticket;
              if (ticket >= 0 && place >= 0 && place < kMaxRefs * tcount) W.refs[kMaxRefs * r.t0 + place] = (int)j;
            } else {
              atomicAdd(tc + c, 1);
            }
          }
    } else if constexpr (FILL) {
      const int k = atomicAdd(W.large_count(n), 1);
      if (k >= 0 && k < tcount) W.large[r.t0 + k] = (int)j;
    }
  }
  for (int64_t i = first; i < qcount; i += step) {
    const float* p = A.queries + (r.q0 + i) * 3;
    const float x = p[0], y = p[1], z = p[2];
    const int c = (cell_clamp(cell_coord(z, H.lo[2], H.inv_h), H.dim[2]) * H.dim[1] + cell_clamp(cell_coord(y, H.lo[1], H.inv_h), H.dim[1])) * H.dim[0] +
                  cell_clamp(cell_coord(x, H.lo[0], H.inv_h), H.dim[0]);
    if constexpr (FILL) {
      const int ticket = atomicSub(qc + c, 1) - 1;
      const int64_t place = (int64_t)qs[c] + ticket;
      if (ticket >= 0 && place >= 0 && place < qcount) W.qrec[r.q0 + place] = make_float4(x, y, z, __int_as_float((int)i));
    } else {
      atomicAdd(qc + c, 1);
    }
  }
}

// grid: 2 N workgroups of kScanLanes, block = table * N + n: the exclusive scan of the element's `cells` counts, their total behind
__global__ __launch_bounds__(kScanLanes) void pmg_scan_kernel(Args A, Tables W) {
  __shared__ int wsum[kScanLanes / kWave];
  const int64_t n = blockIdx.x % A.N;
  const int table = (int)(blockIdx.x / A.N);
  const Range r = elem_range(A.qfirst, A.tfirst, n, A.N, A.Q, A.T);
  const int cells = W.headers[n].cells;  // <= max(tcount, 1), written by the launch before
  const int* c = W.cell_counts(table, n, r.t0);
  int* s = W.cell_starts(table, n, r.t0);
  int running = 0;
  for (int base = 0; base < cells; base += kScanLanes * kScanItems) {
    const int first = base + (int)threadIdx.x * kScanItems;
    int x[kScanItems], mine = 0;
#pragma unroll
    for (int u = 0; u < kScanItems; ++u) x[u] = first + u < cells ? c[first + u] : 0, mine += x[u];
    const int incl = wave_inclusive(mine);
    int total;
    int at = running + block_exclusive<kScanLanes / kWave>(incl - mine, __shfl(incl, kWave - 1), wsum, &total);
#pragma unroll
    for (int u = 0; u < kScanItems; ++u) {
      if (first + u < cells) s[first + u] = at;
      at += x[u];
    }
    running += total;
  }
  if (threadIdx.x == 0) s[cells] = running;
}

// THE STOPPING RULE.  stop_bound returns a float32 B2 such that every REGISTERED target of the element whose box of cells misses the
// box of cells [b0, b1] has a computed distance to the lane's query q that is NaN or >= B2.  A lane whose best distance is STRICTLY
// below B2 is done: an unseen target with an equal distance and a larger index would have to win, hence strict; the large list was
// scanned before.  u = 2^-24; "fl" is one float32 rounding.
//   The gap.  Two boxes of cells miss each other along some axis a.  The target's cells along a are clamp(floor(T(min_a))) ..
//     clamp(floor(T(max_a))) with T = cell_coord, monotone, the same instructions for q; min_a / max_a are exact (fminf / fmaxf of
//     finite floats) and H.lo[a] is the exact minimum of the element's finite coordinates.  So knn_grid.hip's proof at stop_bound
//     holds with p_a := min_a on the side above and p_a := max_a on the side below: the b computed below -- its g, hs and factors
//     1 - 2^-18 -- is <= |x_a - q_a| for EVERY point x of the target's convex hull, a NaN from a query that is not finite giving
//     the bound 0.  With d the real distance from q to the target: b <= d.  Every vertex coordinate and q_a have magnitude <= Mq :=
//     max(mbox, |q_0|, |q_1|, |q_2|).
//   A segment distance (seg_dist_parts: all of seg_dist, and the three edges of tri_dist).  l2 <= 1e-8: the result is
//     fl-sum of fl(q_a - v1_a)^2 >= |q_a - v1_a|^2 (1 - 4 u) for the axis a of the gap (a sum of non-negative terms rounded to
//     nearest is never below one of them).  Else it is the same sum for x = fl(v0 + fl(tt d)), d = fl(v1 - v0), tt in [0, 1] (the
//     clamp; a NaN quotient gives tt = 0): |fl(tt d_a)| <= |d_a| because d_a is a float, and rounding is monotone, so x_a lies
//     between v0_a and fl(v0_a + d_a), which is within 2 u Mq of v1_a: |q_a - x_a| >= b - 2 u Mq whatever the quotient was.
//     So a segment distance is >= (b - 2 u Mq)^2 (1 - 4 u), or NaN, or the gap's square underflows (below).
//   The inside branch of tri_dist (ok == 1, all three computed barycentric coordinates in [0, 1]; result fl(t t)).  The CONDITION of
//     grid_target holds: norm >= L2 / 4, L2 the largest computed squared edge length, and norm >= 2^-7.  L := sqrt(L2) is at most
//     sqrt(3) kMaxSpan cells (1 + 8 u) <= 6 hup =: Lb, because the box of a registered target spans at most kMaxSpan cells an axis.
//     (i) the normal.  raw = cross(e02, e01) from edges with relative error u a component: each component errs by <= 6 u L^2, the
//       vector by <= 11 u L^2 <= 44 u norm.  n = raw / (norm + 1e-8) with 1e-8 <= 2^-19 norm: n = N (1 + r1) + r2 with N the real
//       unit normal, |r1|, |r2| <= 2^-17.  t = fl-dot(fl(v0 - q), n) = h + E, h = (v0 - q) . N the real signed distance to the
//       plane, |E| <= |v0 - q| 2^-16 <= (d + L) 2^-16.
//     (ii) the barycentric coordinates.  p0 = fl(q + fl(t n)), p2 = fl(p0 - v0): coordinates <= 5 Mq, absolute error <= 16 u Mq a
//       component.  d20, d21 err by <= 4 u |p2| L + 28 u Mq L; the numerators d11 d20 - d01 d21 by <= 14 u (|p2| + 4 Mq) L^3; the
//       denominator is |raw|^2 + 1e-8 >= L^4 / 16 up to 64 u of itself, and the added 1e-8 is <= 2^-12.5 of norm^2 >= 2^-14.  The
//       real coordinates W of q's projection have |W| <= (d + L) / (L / 4).  So a computed w in [0, 1] means a real
//       W >= -beta, beta <= 2^-12.5 4 (d + L) / L + 224 u (d + L + 4 Mq) / L + 2^-16 (d + L) / L (from E) <= 2^-10.3 (d + L) / L +
//       2^-14 Mq / L, twice that for w0 = 1 - w1 - w2.  A point of the plane with all W >= -2 beta lies within 12 beta L of the
//       triangle (move the negative weight to the others: the weights change by <= 12 beta in all, the vertices are <= L apart):
//       the projection of q is at r <= 2^-6.7 (d + L) + 2^-10.4 Mq from the triangle, and d^2 = h^2 + r^2.
//     (iii) |t| >= |h| - |E| >= d - r - |E| >= d (1 - 2^-6) - 2^-6 L - 2^-10 Mq >= b (1 - 2^-5) - 2^-5 Lb - 2^-9 Mq + (what the
//       float evaluation of that expression below can lose: a few u (b + Lb + Mq), inside the halved constants).
//   Both kinds: computed distance >= lb^2 (1 - 4 u) with lb = b (1 - 2^-5) - (2^-5 Lb + 2^-9 Mq) where lb > 0 (the segment
//   bound is the larger one), and B2 = fl(fl(lb lb) (1 - 2^-18)) is below that.  For segment targets the constants 2^-18, 0, 2^-20
//   serve.  Underflow: a B2 < 2^-100 is returned as 0 -- nothing is strictly below it -- and above it no square underflows.
struct Box {
  int b0[3], b1[3];
};
template <int TK>
__device__ __forceinline__ float stop_bound(const Header& H, const Box& box, const float (&t)[3], float mq) {
  constexpr float kSlack = 0x1p-18f;
  constexpr float kRel = TK == kTri ? 0x1p-5f : 0x1p-18f, kLen = TK == kTri ? 0x1p-5f : 0.0f, kAbs = TK == kTri ? 0x1p-9f : 0x1p-20f;
  float g = pos_inf();
  bool nan = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float m = kSlack * fabsf(t[a]);
    if (box.b1[a] < H.dim[a] - 1) {
      const float B = (float)(box.b1[a] + 1);
      const float r = (B - t[a]) - (kSlack * B + m);
      nan = nan || !(r == r);
      g = r < g ? r : g;
    }
    if (box.b0[a] > 0) {
      const float B = (float)box.b0[a];
      const float r = (t[a] - B) - (kSlack * B + m);
      nan = nan || !(r == r);
      g = r < g ? r : g;
    }
  }
  const float b = fmaxf(g, 0.0f) * H.hs * (1.0f - kSlack);
  const float lb = b * (1.0f - kRel) - (kLen * (6.0f * H.hup) + kAbs * mq);
  const float b2 = (lb * lb) * (1.0f - kSlack);
  return !nan && lb > 0.0f && b2 >= 0x1p-100f && b2 < pos_inf() ? b2 : 0.0f;
}

__host__ __device__ constexpr int rec4(int kind) { return kind == kSeg ? 3 : 7; }  // float4 per staged record (point_mesh.hip's layout)
__device__ __forceinline__ void put(float4* dst, const Seg& s) {
  dst[0] = make_float4(s.v0.x, s.v0.y, s.v0.z, s.v1.x);
  dst[1] = make_float4(s.v1.y, s.v1.z, s.d.x, s.d.y);
  dst[2] = make_float4(s.d.z, s.l2, 0.0f, 0.0f);
}
__device__ __forceinline__ void get(const float4* src, Seg& s) {
  const float4 a = src[0], b = src[1], c = src[2];
  s.v0 = mk(a.x, a.y, a.z), s.v1 = mk(a.w, b.x, b.y), s.d = mk(b.z, b.w, c.x), s.l2 = c.y;
}
__device__ __forceinline__ void put(float4* dst, const Tri& f) {
  dst[0] = make_float4(f.v0.x, f.v0.y, f.v0.z, f.v1.x);
  dst[1] = make_float4(f.v1.y, f.v1.z, f.v2.x, f.v2.y);
  dst[2] = make_float4(f.v2.z, f.e01.x, f.e01.y, f.e01.z);
  dst[3] = make_float4(f.e02.x, f.e02.y, f.e02.z, f.e12.x);
  dst[4] = make_float4(f.e12.y, f.e12.z, f.n.x, f.n.y);
  dst[5] = make_float4(f.n.z, f.d00, f.d01, f.d11);
  dst[6] = make_float4(f.l12, f.denom, f.norm, f.ok);
}
__device__ __forceinline__ void get(const float4* src, Tri& f) {
  const float4 a = src[0], b = src[1], c = src[2], d = src[3], e = src[4], g = src[5], h = src[6];
  f.v0 = mk(a.x, a.y, a.z), f.v1 = mk(a.w, b.x, b.y), f.v2 = mk(b.z, b.w, c.x);
  f.e01 = mk(c.y, c.z, c.w), f.e02 = mk(d.x, d.y, d.z), f.e12 = mk(d.w, e.x, e.y), f.n = mk(e.z, e.w, g.x);
  f.d00 = g.y, f.d01 = g.z, f.d11 = g.w, f.l12 = h.x, f.denom = h.y, f.norm = h.z, f.ok = h.w;
}
template <int TK>
struct Rec;
template <>
struct Rec<kSeg> {
  Seg r;
  __device__ __forceinline__ void make(const float* v, double) { r = make_seg(load3(v), load3(v + 3)); }
  __device__ __forceinline__ float dist(V3 p) const { return seg_dist(p, r); }
};
template <>
struct Rec<kTri> {
  Tri r;
  __device__ __forceinline__ void make(const float* v, double min_area) { r = make_tri(load3(v), load3(v + 3), load3(v + 6), min_area); }
  __device__ __forceinline__ float dist(V3 p) const { return tri_dist(p, r); }
};

// One tile: lane l holds target j (an index into the element's targets, or -1: a NaN record, which no lane selects) of the tile's
// tn <= kTile references, builds its record, and every lane offers all of them to its query.  Wave-uniform control flow.
template <int TK>
__device__ __forceinline__ void offer_tile(const float* __restrict__ elem_targets, int j, int tn, double min_area, V3 q, float4* tile,
                                           int* tile_j, float& best_d, int& best_j) {
  constexpr int TF = kind_floats(TK);
  const int lane = (int)threadIdx.x, tn4 = (tn + 3) & ~3;
  __syncthreads();  // the wave is done with the tile before
  if (lane < tn4) {
    float v[TF];
    const float* src = elem_targets + (int64_t)(j < 0 ? 0 : j) * TF;
#pragma unroll
    for (int c = 0; c < TF; ++c) v[c] = j >= 0 && lane < tn ? src[c] : quiet_nan();
    Rec<TK> rec;
    rec.make(v, min_area);
    put(tile + lane * rec4(TK), rec.r);
    tile_j[lane] = j;
  }
  __syncthreads();
  for (int t = 0; t < tn4; t += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      Rec<TK> rec;
      get(tile + (t + u) * rec4(TK), rec.r);
      const int jn = tile_j[t + u];
      const float dn = rec.dist(q);
      const bool better = dn < best_d || (dn == best_d && jn > best_j);  // the order (distance, -index); NaN: never
      best_d = better ? dn : best_d;
      best_j = better ? jn : best_j;
    }
  }
}

// grid: N * bpe workgroups of one wave: the 64 ordered queries b * 64 .. of element n
template <int TK>
__global__ __launch_bounds__(64) void pmg_search_kernel(Args A, int64_t bpe, Tables W, float* __restrict__ dists, int64_t* __restrict__ idxs) {
  constexpr int TF = kind_floats(TK);
  __shared__ float4 tile[kTile * rec4(TK)];
  __shared__ int tile_j[kTile];
  __shared__ int span_at[kWave], span_start[kWave];
  const int lane = (int)threadIdx.x;
  const int64_t n = blockIdx.x / bpe, b = blockIdx.x % bpe;
  const Range r = elem_range(A.qfirst, A.tfirst, n, A.N, A.Q, A.T);
  const int64_t qcount = r.q1 - r.q0;
  if (b * kWave >= qcount) return;  // wave-uniform
  const int tcount = (int)(r.t1 - r.t0);
  const int64_t slot = b * kWave + lane;
  const bool live = slot < qcount;
  const Header H = W.headers[n];
  const int* const starts = W.cell_starts(0, n, r.t0);
  const int* const refs = W.refs + kMaxRefs * r.t0;
  const int64_t nrefs = (int64_t)kMaxRefs * tcount;
  const float* const elem_targets = A.targets + r.t0 * TF;

  float qv[3] = {0.0f, 0.0f, 0.0f}, t[3];
  int64_t row = -1;
  if (live) {
    const float4 rec = W.qrec[r.q0 + slot];
    qv[0] = rec.x, qv[1] = rec.y, qv[2] = rec.z;
    const int64_t own = (int64_t)__float_as_int(rec.w);
    row = own >= 0 && own < qcount ? own : -1;
  }
  const V3 q = mk(qv[0], qv[1], qv[2]);
  const float mq = fmaxf(fmaxf(H.mbox, fabsf(qv[0])), fmaxf(fabsf(qv[1]), fabsf(qv[2])));
  float best_d = FLT_MAX;
  int best_j = -1;

  // ---- the large list
  int nlarge = *W.large_count(n);
  nlarge = __builtin_amdgcn_readfirstlane(nlarge < 0 ? 0 : (nlarge > tcount ? tcount : nlarge));
  for (int k0 = 0; k0 < nlarge; k0 += kTile) {
    const int tn = nlarge - k0 < kTile ? nlarge - k0 : kTile;
    int j = lane < tn ? W.large[r.t0 + k0 + lane] : -1;
    j = j >= 0 && j < tcount ? j : -1;
    offer_tile<TK>(elem_targets, j, tn, A.min_area, q, tile, tile_j, best_d, best_j);
  }

  // ---- the cells, ring by ring
  Box box, old;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    t[a] = cell_coord(qv[a], H.lo[a], H.inv_h);
    const int c = cell_clamp(t[a], H.dim[a]);
    box.b0[a] = __builtin_amdgcn_readfirstlane(wave_imin(live ? c : 0x7fffffff));
    box.b1[a] = __builtin_amdgcn_readfirstlane(wave_imax(live ? c : -1));
    old.b0[a] = 0, old.b1[a] = -1;
  }
  bool done = !live;
  const int max_dim = H.dim[0] > H.dim[1] ? (H.dim[0] > H.dim[2] ? H.dim[0] : H.dim[2]) : (H.dim[1] > H.dim[2] ? H.dim[1] : H.dim[2]);
  int64_t staged = 0;
  bool all_pairs = false;

  for (int ring = 0; ring <= max_dim; ++ring) {
    if (ring > 0) {
      old = box;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        box.b0[a] = box.b0[a] > 0 ? box.b0[a] - 1 : 0;
        box.b1[a] = box.b1[a] < H.dim[a] - 1 ? box.b1[a] + 1 : H.dim[a] - 1;
      }
    }
    const int ny = box.b1[1] - box.b0[1] + 1, nz = box.b1[2] - box.b0[2] + 1;
    const int nslots = 2 * ny * nz;  // two span slots per (y, z) row
    for (int s0 = 0; s0 < nslots; s0 += kWave) {
      const int sl = s0 + lane, rw = sl >> 1, piece = sl & 1;
      const int y = box.b0[1] + rw % ny, z = box.b0[2] + rw / ny;
      const bool covered = ring > 0 && y >= old.b0[1] && y <= old.b1[1] && z >= old.b0[2] && z <= old.b1[2];
      // the old box covered the middle of the row: the piece below it and the piece above it; a new row: all of it, once
      const int x0 = covered && piece ? old.b1[0] + 1 : box.b0[0];
      const int x1 = covered ? (piece ? box.b1[0] : old.b0[0] - 1) : (piece ? box.b0[0] - 1 : box.b1[0]);
      int start = 0, count = 0;
      if (sl < nslots && x0 <= x1) {
        const int at = (z * H.dim[1] + y) * H.dim[0];
        start = starts[at + x0];
        count = starts[at + x1 + 1] - start;
        if (start < 0 || count < 0 || (int64_t)start + count > nrefs) count = 0;  // never read outside the element's references
      }
      const int incl = wave_inclusive(count);
      const int total = __builtin_amdgcn_readfirstlane(__shfl(incl, kWave - 1));
      __syncthreads();  // the wave is done with the tables of the batch before
      span_at[lane] = incl - count;
      span_start[lane] = start;
      __syncthreads();
      staged += total;
      for (int e0 = 0; e0 < total; e0 += kTile) {
        const int tn = total - e0 < kTile ? total - e0 : kTile;
        int j = -1;
        if (lane < tn) {
          // the last span that begins at or before reference e0 + lane: empty spans share their successor's offset and lose to it
          const int g = e0 + lane;
          int s = 0;
#pragma unroll
          for (int step = kWave / 2; step > 0; step >>= 1) s += span_at[s + step] <= g ? step : 0;
          j = refs[span_start[s] + (g - span_at[s])];
          j = j >= 0 && j < tcount ? j : -1;
        }
        offer_tile<TK>(elem_targets, j, tn, A.min_area, q, tile, tile_j, best_d, best_j);
      }
    }
    bool covers = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) covers = covers && box.b0[a] == 0 && box.b1[a] == H.dim[a] - 1;
    if (covers) break;  // every registered target was offered
    done = done || best_d < stop_bound<TK>(H, box, t, mq);
    if (__ballot(!done) == 0ull) break;
    if (staged >= tcount) {  // the walk has cost a scan of all pairs and a lane still cannot stop: that scan, once
      all_pairs = true;
      break;
    }
  }
  if (all_pairs) {
    for (int j0 = 0; j0 < tcount; j0 += kTile) {
      const int tn = tcount - j0 < kTile ? tcount - j0 : kTile;
      offer_tile<TK>(elem_targets, lane < tn ? j0 + lane : -1, tn, A.min_area, q, tile, tile_j, best_d, best_j);
    }
  }
  if (live && row >= 0) {
    dists[r.q0 + row] = best_d;
    idxs[r.q0 + row] = best_j >= 0 ? r.t0 + best_j : 0;
  }
}

// grid: N * bpe workgroups of one wave: partials[n * bpe + b] = the wave sum of dists * weights[n] over the 64 consecutive queries
// b * 64 .. of element n in the ORIGINAL order -- what pm_forward_kernel of point_mesh.hip leaves for the element sum
__global__ __launch_bounds__(64) void pmg_partials_kernel(Args A, int64_t bpe, const float* __restrict__ weights,
                                                          const float* __restrict__ dists, float* __restrict__ partials) {
  const int64_t n = blockIdx.x / bpe, b = blockIdx.x % bpe;
  const Range r = elem_range(A.qfirst, A.tfirst, n, A.N, A.Q, A.T);
  const int64_t i = b * kWave + threadIdx.x;
  float term = i < r.q1 - r.q0 ? dists[r.q0 + i] * (weights ? weights[n] : 1.0f) : 0.0f;
  term = wave_sum(term);
  if (threadIdx.x == 0) partials[blockIdx.x] = term;
}

struct ElementSum {
  __device__ __forceinline__ float operator()(int64_t, float s) const { return s; }
};

bool sizes_ok(int64_t N, int64_t Q, int64_t T) {
  return N >= 0 && Q >= 0 && T >= 0 && N <= INT32_MAX && Q <= INT32_MAX && T <= INT32_MAX / (2 * kMaxRefs);
}

template <int TK>
int launch_all(const Args& A, const Tables& W, int occupancy, int64_t bpe, const float* weights, float* dists, int64_t* idxs, float* sums,
               hipStream_t s) {
  const int64_t N = A.N;
  int bpc = (int)ceil_div(A.T, kBoundsRows);
  bpc = bpc < 1 ? 1 : (bpc > kBoundsBlocks ? kBoundsBlocks : bpc);
  int ipb = (int)ceil_div(A.T > A.Q ? A.T : A.Q, 256 * 4);
  ipb = ipb < 1 ? 1 : (ipb > kItemBlocks ? kItemBlocks : ipb);
  {
    LaunchScope ls(TK == kTri ? "point_face_grid_build" : "point_edge_grid_build", s);
    pmg_bounds_kernel<<<(unsigned)(N * bpc), 256, 0, s>>>(A, kind_floats(TK), bpc, W);
    pmg_header_kernel<<<(unsigned)N, 64, 0, s>>>(A, bpc, occupancy, W);
    pmg_place_kernel<TK, false><<<(unsigned)(N * ipb), 256, 0, s>>>(A, ipb, W);
    pmg_scan_kernel<<<(unsigned)(2 * N), kScanLanes, 0, s>>>(A, W);
    pmg_place_kernel<TK, true><<<(unsigned)(N * ipb), 256, 0, s>>>(A, ipb, W);
    const int rc = launch_status();
    if (rc != P3D_OK) return rc;
  }
  if (bpe > 0) {
    LaunchScope ls(TK == kTri ? "point_face_grid_search" : "point_edge_grid_search", s);
    pmg_search_kernel<TK><<<(unsigned)(N * bpe), 64, 0, s>>>(A, bpe, W, dists, idxs);
    const int rc = launch_status();
    if (rc != P3D_OK) return rc;
  }
  if (sums) {
    LaunchScope ls("point_mesh_grid_element_sum", s);
    if (bpe > 0) pmg_partials_kernel<<<(unsigned)(N * bpe), 64, 0, s>>>(A, bpe, weights, dists, W.sums);
    segment_sum_kernel<<<(unsigned)N, 256, 0, s>>>(W.sums, bpe, ElementSum{}, sums);
    return launch_status();
  }
  return P3D_OK;
}

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API size_t p3di_point_mesh_grid_forward_workspace_bytes(int64_t N, int64_t Q, int64_t T) {
  if (N <= 0 || !sizes_ok(N, Q, T)) return 0;
  return Tables(nullptr, N, Q, T).bytes;
}

P3D_API int p3di_point_mesh_grid_forward(int query_kind, int target_kind, const float* queries, const float* targets,
                                         const int64_t* query_first_idx, const int64_t* target_first_idx, int64_t N, int64_t Q, int64_t T,
                                         int64_t max_queries, double min_triangle_area, int occupancy, const float* weights, float* dists,
                                         int64_t* idxs, float* sums, void* workspace, size_t workspace_bytes, p3d_stream_t stream) {
  const bool point_query = query_kind == kPoint && (target_kind == kSeg || target_kind == kTri);
  const bool target_query = target_kind == kPoint && (query_kind == kSeg || query_kind == kTri);
  if (!point_query && !target_query) return P3D_ERR_INVALID_ARG;
  if (!sizes_ok(N, Q, T) || max_queries < 0 || occupancy < 0) return P3D_ERR_INVALID_ARG;
  if (!point_query) return P3D_ERR_UNSUPPORTED;  // face_point / edge_point: p3d_point_mesh_forward
  if (max_queries > Q) max_queries = Q;
  if (N > 0 && (!query_first_idx || !target_first_idx)) return P3D_ERR_INVALID_ARG;
  if (Q > 0 && (!queries || !dists || !idxs || (T > 0 && !targets))) return P3D_ERR_INVALID_ARG;
  if (Q > 0 && (N == 0 || max_queries == 0)) return P3D_ERR_INVALID_ARG;  // rows nobody would write
  if (N == 0) return P3D_OK;
  if (!workspace || workspace_bytes < p3di_point_mesh_grid_forward_workspace_bytes(N, Q, T)) return P3D_ERR_WORKSPACE;
  const int64_t bpe = ceil_div(max_queries, kWave);
  if (N * bpe > 0x7fffffffll || N * (int64_t)kBoundsBlocks > 0x7fffffffll) return P3D_ERR_INVALID_ARG;
  Args A;
  A.queries = queries, A.targets = targets, A.qfirst = query_first_idx, A.tfirst = target_first_idx;
  A.N = N, A.Q = Q, A.T = T, A.min_area = min_triangle_area;
  const Tables W(workspace, N, Q, T);
  const int occ = occupancy > 0 ? occupancy : P3D_POINT_MESH_GRID_OCCUPANCY;
  hipStream_t s = (hipStream_t)stream;
  return target_kind == kTri ? launch_all<kTri>(A, W, occ, bpe, weights, dists, idxs, sums, s)
                             : launch_all<kSeg>(A, W, occ, bpe, weights, dists, idxs, sums, s);
}
