// knn_grid.hip -- K nearest neighbours between large 3D clouds through a uniform grid: p3d_knn_points_forward's result at D = 3,
// norm 2, bit for bit, without looking at most pairs.  implicit_abi.h has the contract; DESIGN 8.30 the figures.
//
// The search is EXACT.  Distances are knn.hip's pair_dist (unfused, coordinate order); the queue orders by (dist, j) whatever the
// order of the offers (knn_queue.h: LexQueue); the grid only decides which pairs are never looked at, and a lane stops only where a
// proven lower bound (stop_bound below) says that no pair it has not seen could enter its queue.
//
// Six launches, no host read, no float atomic:
//   bounds   per cloud, 1..kBoundsBlocks workgroups: min / max of the valid rows of p2[n] (fminf / fmaxf trees: any order gives the
//            same bits) into partials; the same launch clears the two tables of cell counts (no memset node in a captured graph).
//   header   per cloud one wave: the box, then the cell side from the box volume, lengths2[n] and the target occupancy; axes
//            shorter than a cell drop out of the volume (a flat, linear or single-point cloud has dimension 1 there).  Cells per
//            cloud <= cap = min(max(P2, 1), P3D_KNN_GRID_MAX_CELLS): a function of the padded P2, the workspace is sized from shapes.
//   count    one lane per point of p2 and of p1: cell = clamp(floor((x - lo) * inv_h), 0, dim - 1) per axis, x fastest; integer
//            atomics.  The queries are binned by the grid of p2[n]: one outside the box lands in a border cell.
//   scan     per (cloud, table) one workgroup: exclusive scan of the counts in rounds of kScanLanes * kScanItems cells
//            (scan_blocks.h).
//   fill     one lane per point: its place is the cell's start + a ticket (atomicSub on the count, which ends at 0); writes the
//            16-byte record (x, y, z, j) -- j the row in p2 or p1.  The order inside a cell differs from run to run; the result
//            does not, by LexQueue.
//   search   one wave per 64 consecutive ordered queries, one wave per workgroup, control flow uniform across the wave.  The wave
//            takes the box of cells its queries occupy and grows it ring by ring, clamped to the grid.  With x fastest a run of
//            cells along x is one contiguous span of the ordered records, so a ring is a list of spans: per (y, z) row of the new
//            box either the whole row (the row is new) or the two end pieces (the old box covered the middle).  Lane l takes span
//            slot l of a batch of 64 (two slots per row), a wave scan gives every span its offset, and the points of the batch are
//            copied into LDS tiles of kTile points (each lane finds the span of its point by a 6-step search of the offsets) and
//            read by broadcast, four points per ds_read_b128 and coordinate, as knn.hip does.  A point is offered ONCE: only the
//            shell a ring adds is staged.  Results go to the query's original row.
//
// Every loop has a bound known before it starts; none depends on data written in the same launch, none spins, no workgroup
// talks to another:
//   rings   <= the largest grid dimension + 1: the loop ends when the box covers the grid, and every ring before that grows the box
//              by at least one cell along some axis;
//   batches <= ceil(2 * rows / 64), rows = the box's y x z extent <= dim_y dim_z;
//   tiles   <= ceil(points of the batch / kTile) <= ceil(lengths2[n] / kTile);
//   scan    <= ceil(cells / (kScanLanes * kScanItems)) rounds, cells read from the header of the launch before.
// A search that cannot end early (a NaN query, a cloud shorter than K, one giant cell) offers every point of its cloud once: the
// brute-force scan, never anything else.
#include "implicit_abi.h"
#include "knn_grad.h"
#include "knn_queue.h"
#include "scan_blocks.h"

namespace p3d {
namespace {

constexpr int kTile = P3D_KNN_GRID_TILE;
static_assert(kTile % 4 == 0 && kTile % kWave == 0, "a tile is read four points at a time and copied a wave at a time");
constexpr int kBoundsBlocks = 64;  // partial boxes per cloud: one wave reduces them
constexpr int kBoundsRows = 4096;  // rows per partial box before a cloud gets the next workgroup
constexpr int kScanLanes = 1024, kScanItems = 8;

// per cloud, written by header_kernel
struct Header {
  float lo[3];  // the box's minimum corner
  float inv_h;  // 1 / cell side; 0 where the grid is a single cell
  float hs;     // a float BELOW the real 1 / inv_h (see stop_bound)
  int dim[3];
  int cells;  // dim[0] dim[1] dim[2] <= cap
  int pad[7];
};
static_assert(sizeof(Header) == 64, "one header per 64 bytes");

__device__ __forceinline__ float quiet_nan() { return __int_as_float(0x7fc00000); }
__device__ __forceinline__ float neg_inf() { return __int_as_float(0xff800000); }

// the cell coordinate, before the clamp, of coordinate x: two float32 operations, THE SAME in count, fill and search
__device__ __forceinline__ float cell_coord(float x, float lo, float inv_h) { return (x - lo) * inv_h; }
// clamp(floor(t), 0, dim - 1); NaN goes to 0
__device__ __forceinline__ int cell_clamp(float t, int dim) { return (int)fminf(fmaxf(t, 0.0f), (float)(dim - 1)); }
__device__ __forceinline__ int cell_of(const Header& H, float x, float y, float z) {
  const int cx = cell_clamp(cell_coord(x, H.lo[0], H.inv_h), H.dim[0]);
  const int cy = cell_clamp(cell_coord(y, H.lo[1], H.inv_h), H.dim[1]);
  const int cz = cell_clamp(cell_coord(z, H.lo[2], H.inv_h), H.dim[2]);
  return (cz * H.dim[1] + cy) * H.dim[0] + cx;
}

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

// grid: N * bpc workgroups of 256.  partials[(n * kBoundsBlocks + b) * 6 + {0..2: min, 3..5: max}] for b < bpc; counts cleared.
__global__ __launch_bounds__(256) void knn_grid_bounds_kernel(const float* __restrict__ p2, const int64_t* __restrict__ lengths2, int64_t P2,
                                                              int bpc, float* __restrict__ partials, int* __restrict__ counts,
                                                              int64_t ncounts) {
  __shared__ float part[4][6];
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < ncounts; v += (int64_t)gridDim.x * 256) counts[v] = 0;
  const int64_t n = blockIdx.x / bpc;
  const int b = (int)(blockIdx.x % bpc);
  const int64_t len2 = knn::cloud_length(lengths2, n, P2);
  float lo[3] = {pos_inf(), pos_inf(), pos_inf()}, hi[3] = {neg_inf(), neg_inf(), neg_inf()};
  for (int64_t i = (int64_t)b * 256 + threadIdx.x; i < len2; i += (int64_t)bpc * 256) {
    const float* p = p2 + (n * P2 + i) * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) lo[a] = fminf(lo[a], p[a]), hi[a] = fmaxf(hi[a], p[a]);
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
    float r = part[0][a];
    for (int w = 1; w < 4; ++w) r = a < 3 ? fminf(r, part[w][a]) : fmaxf(r, part[w][a]);
    partials[(n * kBoundsBlocks + b) * 6 + a] = r;
  }
}

// grid: N workgroups of one wave.  Lane 0 chooses the grid in double: nothing here is on the hot path.
__global__ __launch_bounds__(64) void knn_grid_header_kernel(const float* __restrict__ partials, const int64_t* __restrict__ lengths2,
                                                             int64_t P2, int bpc, int occupancy, int cap, Header* __restrict__ headers) {
  const int64_t n = blockIdx.x;
  const int lane = (int)threadIdx.x;
  float lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = wave_fmin(lane < bpc ? partials[(n * kBoundsBlocks + lane) * 6 + a] : pos_inf());
    hi[a] = wave_fmax(lane < bpc ? partials[(n * kBoundsBlocks + lane) * 6 + 3 + a] : neg_inf());
  }
  if (lane != 0) return;
  const int64_t len2 = knn::cloud_length(lengths2, n, P2);
  Header H;
  for (int a = 0; a < 7; ++a) H.pad[a] = 0;
  H.inv_h = 0.0f, H.hs = 0.0f, H.cells = 1;
  double ext[3];
  bool finite = len2 > 0;
  for (int a = 0; a < 3; ++a) {
    H.dim[a] = 1;
    ext[a] = (double)hi[a] - (double)lo[a];
    finite = finite && fabsf(lo[a]) < pos_inf() && fabsf(hi[a]) < pos_inf();
    H.lo[a] = finite ? lo[a] : 0.0f;
  }
  if (finite) {
    int64_t target = (len2 + occupancy - 1) / occupancy;
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
    if (fits && inv_h > 0.0f && inv_h < pos_inf() && dim[0] * dim[1] * dim[2] <= (int64_t)cap) {
      H.inv_h = inv_h;
      H.hs = (1.0f / inv_h) * (1.0f - 0x1p-18f);
      if (!(H.hs < pos_inf())) H.hs = 0.0f;
      for (int a = 0; a < 3; ++a) H.dim[a] = (int)dim[a];
      H.cells = (int)(dim[0] * dim[1] * dim[2]);
    }
  }
  headers[n] = H;
}

// item v of the point launches: v < N * P2 a row of p2, else a row of p1
struct Points {
  const float *p1, *p2;
  const int64_t *lengths1, *lengths2;
  int64_t N, P1, P2;
  // (n, row, table) of item v, or false where the row is padding
  __device__ __forceinline__ bool item(int64_t v, int64_t* n, int64_t* i, int* table, const float** p) const {
    const bool target = v < N * P2;
    const int64_t u = target ? v : v - N * P2, P = target ? P2 : P1;
    *n = u / P, *i = u % P, *table = target ? 0 : 1;
    *p = (target ? p2 : p1) + u * 3;
    return *i < knn::cloud_length(target ? lengths2 : lengths1, *n, P);
  }
};

// counts: table 0 (p2) N * cap ints, then table 1 (p1) N * cap ints
__global__ __launch_bounds__(256) void knn_grid_count_kernel(Points pts, const Header* __restrict__ headers, int cap, int* __restrict__ counts) {
  const int64_t items = pts.N * (pts.P1 + pts.P2);
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < items; v += (int64_t)gridDim.x * 256) {
    int64_t n, i;
    int table;
    const float* p;
    if (!pts.item(v, &n, &i, &table, &p)) continue;
    const int c = cell_of(headers[n], p[0], p[1], p[2]);
    atomicAdd(counts + ((int64_t)table * pts.N + n) * cap + c, 1);
  }
}

// grid: 2 N workgroups of kScanLanes, block = table * N + n.  starts: per (table, cloud) cap + 1 ints, the exclusive scan of the
// cloud's `cells` counts and their total behind it.
__global__ __launch_bounds__(kScanLanes) void knn_grid_scan_kernel(const Header* __restrict__ headers, int64_t N, int cap,
                                                                    const int* __restrict__ counts, int* __restrict__ starts) {
  __shared__ int wsum[kScanLanes / kWave];
  const int64_t n = blockIdx.x % N;
  const int cells = headers[n].cells;  // <= cap, written by the launch before
  const int* c = counts + (int64_t)blockIdx.x * cap;
  int* s = starts + (int64_t)blockIdx.x * (cap + 1);
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

// records: table 0 N * P2 float4, then table 1 N * P1 float4; a cloud's first `length` records are written
__global__ __launch_bounds__(256) void knn_grid_fill_kernel(Points pts, const Header* __restrict__ headers, int cap, int* __restrict__ counts,
                                                            const int* __restrict__ starts, float4* __restrict__ records) {
  const int64_t items = pts.N * (pts.P1 + pts.P2);
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < items; v += (int64_t)gridDim.x * 256) {
    int64_t n, i;
    int table;
    const float* p;
    if (!pts.item(v, &n, &i, &table, &p)) continue;
    const float x = p[0], y = p[1], z = p[2];
    const int c = cell_of(headers[n], x, y, z);
    const int64_t tn = (int64_t)table * pts.N + n;
    const int ticket = atomicSub(counts + tn * cap + c, 1) - 1;  // count - 1 .. 0: every place of the cell once
    const int64_t place = (int64_t)starts[tn * (cap + 1) + c] + ticket;
    const int64_t P = table ? pts.P1 : pts.P2;
    if (ticket < 0 || place >= P) continue;  // cannot happen with the counts of the same grid: never write outside the cloud
    records[(table ? pts.N * pts.P2 : 0) + n * P + place] = make_float4(x, y, z, __int_as_float((int)i));
  }
}

// THE STOPPING RULE.  stop_bound returns a float32 B2 such that every point p of p2[n] whose cell lies OUTSIDE the box of cells
// [b0, b1] has a contract distance dist(q, p) >= B2; a lane whose queue is full with its worst distance STRICTLY below B2 is done
// (an equal distance with a smaller j outside the box would have to displace the worst entry, hence strict).  u = 2^-24.
//   Cells.  T(x) = fl(fl(x - lo) * inv_h) is the float cell_coord, the same instructions for p in count / fill and for q here; its
//     real counterpart X = (x - lo) inv_h has |T(x) - X| <= 3 u |X| (two roundings; a product flushed towards 0 errs by < 2^-149,
//     which the slack below covers because every B in it is >= 1).  The cell is clamp(floor(T), 0, dim - 1).  This assumes that
//     fl(x - lo) is finite.  In a box wider than FLT_MAX (lo near -3.4e38, points near +1e37) it overflows and T = +inf puts points
//     of interior cells into the last one; the results stand all the same: such an x is above 2^102, so its difference to any
//     other float on that axis squares to +inf, no distance to a misplaced point is ever strictly below a bound, and a query
//     whose own t is not finite gets the bound 0 (below).
//   A cell outside the box differs from it along some axis a, on one of two sides:
//     above, c_a(p) >= B := b1_a + 1 (only if b1_a < dim_a - 1): the clamp from above only lowers, so T(p_a) >= B >= 1, hence
//       P >= B (1 - 4 u), and Q <= T(q_a) + 4 u |T(q_a)|:       (p_a - q_a) inv_h >= B - t - 4 u (B + |t|),  t = T(q_a) unclamped;
//     below, c_a(p) <= b0_a - 1, B := b0_a >= 1: max(T(p_a), 0) < B, and P >= 0 because lo_a is the exact minimum over the valid
//       rows, so P <= B (1 + 4 u), and Q >= t - 4 u |t|:         (q_a - p_a) inv_h >= t - B - 4 u (B + |t|).
//     This holds for a query OUTSIDE the bounding box too (t < 0 or t >= dim): nothing above used 0 <= t < dim.  Towards a side
//     where the box has reached the grid's border there is no outside cell and no term.
//   Arithmetic.  s = fl(+-(B - t)), e = fl(2^-18 B + 2^-18 |t|) (the two products are exact), r = fl(s - e): three roundings of
//     values <= B + |t|, together below 4 u (B + |t|); with the 4 u above that is 8 u against the 64 u (1 - u) subtracted.  So
//     r <= the real (p_a - q_a) inv_h or its mirror.  g = max(0, min over the sides of r); a NaN r, from a non-finite t, gives
//     the bound 0.  hs = fl(fl(1 / inv_h) (1 - 2^-18)) <= (1 / inv_h) (1 + 3 u) (1 - 64 u) (1 + u) < the real 1 / inv_h whether
//     or not the division rounds correctly, so b = fl(fl(g hs) (1 - 2^-18)) <= |p_a - q_a| (1 - 62 u) and
//     B2 = fl(fl(b b) (1 - 2^-18)) <= |p_a - q_a|^2 (1 - 180 u).
//   Distance.  The contract's dist is >= its term fl(fl(q_a - p_a)^2) >= |p_a - q_a|^2 (1 - 4 u) when nothing underflows (adding
//     the other non-negative terms and rounding to nearest never goes below a term): B2 <= dist.  Underflow: B2 < 2^-100 is
//     returned as 0 -- nothing is strictly below it -- and above that |p_a - q_a|^2 is far from the subnormals.
struct Box {
  int b0[3], b1[3];
};
__device__ __forceinline__ float stop_bound(const Header& H, const Box& box, const float (&t)[3]) {
  constexpr float kSlack = 0x1p-18f;
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
  const float b2 = (b * b) * (1.0f - kSlack);
  return !nan && b2 >= 0x1p-100f ? b2 : 0.0f;
}

// grid: N * blocks_per_cloud workgroups of one wave; K <= KQ
template <int KQ>
__global__ __launch_bounds__(64) void knn_grid_search_kernel(const Header* __restrict__ headers, const int* __restrict__ starts2, int cap,
                                                             const float4* __restrict__ rec2, const float4* __restrict__ rec1,
                                                             const int64_t* __restrict__ lengths1, const int64_t* __restrict__ lengths2,
                                                             int64_t P1, int64_t P2, int K, int64_t blocks_per_cloud,
                                                             int64_t* __restrict__ idx, float* __restrict__ dists) {
  __shared__ __align__(16) float tile[3][kTile];
  __shared__ __align__(16) int tile_j[kTile];
  __shared__ int span_at[kWave], span_start[kWave];
  const int lane = (int)threadIdx.x;
  const int64_t n = blockIdx.x / blocks_per_cloud, b = blockIdx.x % blocks_per_cloud;
  const int64_t slot = b * kWave + lane;
  const int64_t len1 = knn::cloud_length(lengths1, n, P1), len2 = knn::cloud_length(lengths2, n, P2);
  const bool live = slot < len1;
  const int found = (int)(len2 < K ? len2 : K);
  LexQueue<KQ> best;
  best.init();
  int64_t row = slot;  // a padding slot zeroes the padding row of its own number: the live slots are a permutation of the live rows

  if (b * kWave < len1 && found > 0) {  // wave-uniform
    const Header H = headers[n];
    const int* const starts = starts2 + n * (int64_t)(cap + 1);
    const float4* const points = rec2 + n * P2;
    float q[3] = {0.0f, 0.0f, 0.0f}, t[3];
    if (live) {
      const float4 r = rec1[n * P1 + slot];
      q[0] = r.x, q[1] = r.y, q[2] = r.z;
      const int64_t own = (int64_t)__float_as_int(r.w);
      row = own >= 0 && own < len1 ? own : slot;
    }
    Box box, old;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      t[a] = cell_coord(q[a], H.lo[a], H.inv_h);
      const int c = cell_clamp(t[a], H.dim[a]);
      box.b0[a] = __builtin_amdgcn_readfirstlane(wave_imin(live ? c : 0x7fffffff));
      box.b1[a] = __builtin_amdgcn_readfirstlane(wave_imax(live ? c : -1));
      old.b0[a] = 0, old.b1[a] = -1;
    }
    bool done = !live;
    const int max_dim = H.dim[0] > H.dim[1] ? (H.dim[0] > H.dim[2] ? H.dim[0] : H.dim[2]) : (H.dim[1] > H.dim[2] ? H.dim[1] : H.dim[2]);

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
      const int nslots = 2 * ny * nz;  // <= 2 cap; two span slots per (y, z) row
      for (int s0 = 0; s0 < nslots; s0 += kWave) {
        // ---- lane l: span slot s0 + l
        const int sl = s0 + lane, r = sl >> 1, piece = sl & 1;
        const int y = box.b0[1] + r % ny, z = box.b0[2] + r / ny;
        const bool covered = ring > 0 && y >= old.b0[1] && y <= old.b1[1] && z >= old.b0[2] && z <= old.b1[2];
        // the old box covered the middle of the row: the piece below it and the piece above it; a new row: all of it, once
        const int x0 = covered && piece ? old.b1[0] + 1 : box.b0[0];
        const int x1 = covered ? (piece ? box.b1[0] : old.b0[0] - 1) : (piece ? box.b0[0] - 1 : box.b1[0]);
        int start = 0, count = 0;
        if (sl < nslots && x0 <= x1) {
          const int at = (z * H.dim[1] + y) * H.dim[0];
          start = starts[at + x0];
          count = starts[at + x1 + 1] - start;
          // what the scan of this cloud's own counts cannot give: never read outside the cloud's records
          if (start < 0 || count < 0 || (int64_t)start + count > len2) count = 0;
        }
        const int incl = wave_inclusive(count);
        const int total = __builtin_amdgcn_readfirstlane(__shfl(incl, kWave - 1));
        __syncthreads();  // the wave is done with the tables and the tile of the batch before
        span_at[lane] = incl - count;
        span_start[lane] = start;
        for (int e0 = 0; e0 < total; e0 += kTile) {
          const int tn = total - e0 < kTile ? total - e0 : kTile, tn4 = (tn + 3) & ~3;
          __syncthreads();  // the tables are in place; the wave is done with the tile before
          for (int e = lane; e < tn; e += kWave) {
            // the last span that begins at or before point e0 + e: empty spans share their successor's offset and lose to it
            const int g = e0 + e;
            int s = 0;
#pragma unroll
            for (int step = kWave / 2; step > 0; step >>= 1) s += span_at[s + step] <= g ? step : 0;
            const float4 v = points[span_start[s] + (g - span_at[s])];
            tile[0][e] = v.x, tile[1][e] = v.y, tile[2][e] = v.z, tile_j[e] = __float_as_int(v.w);
          }
          if (lane < tn4 - tn) tile[0][tn + lane] = tile[1][tn + lane] = tile[2][tn + lane] = quiet_nan(), tile_j[tn + lane] = 0;
          __syncthreads();
          for (int e = 0; e < tn4; e += 4) {
            const float4 vx = *reinterpret_cast<const float4*>(&tile[0][e]);
            const float4 vy = *reinterpret_cast<const float4*>(&tile[1][e]);
            const float4 vz = *reinterpret_cast<const float4*>(&tile[2][e]);
            const int4 vj = *reinterpret_cast<const int4*>(&tile_j[e]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const float px = u == 0 ? vx.x : (u == 1 ? vx.y : (u == 2 ? vx.z : vx.w));
              const float py = u == 0 ? vy.x : (u == 1 ? vy.y : (u == 2 ? vy.z : vy.w));
              const float pz = u == 0 ? vz.x : (u == 1 ? vz.y : (u == 2 ? vz.z : vz.w));
              const int jn = u == 0 ? vj.x : (u == 1 ? vj.y : (u == 2 ? vj.z : vj.w));
              // knn.hip's pair_dist<3, 2>: unfused, coordinate order
              const float dx = q[0] - px, dy = q[1] - py, dz = q[2] - pz;
              float dn = dx * dx;
              dn = dn + dy * dy;
              dn = dn + dz * dz;
              if constexpr (KQ == 1) {
                best.insert(dn, jn);
              } else {
                if (__ballot(best.wants(dn, jn)) != 0ull) best.insert(dn, jn);
              }
            }
          }
        }
      }
      // ---- who is done: the queue's entry found - 1 strictly below the bound
      bool covers = true;
#pragma unroll
      for (int a = 0; a < 3; ++a) covers = covers && box.b0[a] == 0 && box.b1[a] == H.dim[a] - 1;
      if (covers) break;
      float worst = best.d[0];
#pragma unroll
      for (int s = 1; s < KQ; ++s) worst = s == found - 1 ? best.d[s] : worst;
      done = done || worst < stop_bound(H, box, t);
      if (__ballot(!done) == 0ull) break;
    }
  }

  if (slot < P1) {
    const int64_t out = (n * P1 + row) * K;
#pragma unroll
    for (int k = 0; k < KQ; ++k) {
      if (k < K) {
        const bool has = live && k < found;
        idx[out + k] = has && best.j[k] >= 0 ? (int64_t)best.j[k] : 0;
        dists[out + k] = has ? best.d[k] : 0.0f;
      }
    }
  }
}

// every index the kernels form fits an int64 comfortably, a row an int32
bool sizes_ok(int64_t N, int64_t P1, int64_t P2, int K) {
  if (N < 0 || P1 < 0 || P2 < 0 || P2 > INT32_MAX || P1 > INT32_MAX) return false;
  const int64_t per_cloud = (P1 > P2 ? P1 : P2) * (int64_t)(K > 0 ? K : 1) * 16;
  return N == 0 || per_cloud <= INT64_MAX / 4 / N;
}

int cell_cap(int64_t P2) { return (int)(P2 < 1 ? 1 : (P2 > P3D_KNN_GRID_MAX_CELLS ? P3D_KNN_GRID_MAX_CELLS : P2)); }

struct Workspace {
  float* partials;
  Header* headers;
  int *counts, *starts;
  float4* records;
  size_t bytes;
  Workspace(void* ws, int64_t N, int64_t P1, int64_t P2) {
    const size_t cap = (size_t)cell_cap(P2);
    Arena a(ws, ~(size_t)0);
    partials = a.take<float>((size_t)N * kBoundsBlocks * 6);
    headers = a.take<Header>((size_t)N);
    counts = a.take<int>(2 * (size_t)N * cap);
    starts = a.take<int>(2 * (size_t)N * (cap + 1));
    records = a.take<float4>((size_t)N * (size_t)(P1 + P2));
    bytes = a.off;
  }
};

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API size_t p3di_knn_grid_forward_workspace_bytes(int64_t N, int64_t P1, int64_t P2) {
  if (N <= 0 || P1 <= 0 || P2 < 0 || !sizes_ok(N, P1, P2, 1)) return 0;
  return Workspace(nullptr, N, P1, P2).bytes;
}

P3D_API int p3di_knn_grid_forward(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2, int64_t N, int64_t P1,
                                 int64_t P2, int D, int K, int occupancy, int64_t* idx, float* dists, void* workspace,
                                 size_t workspace_bytes, p3d_stream_t stream) {
  if (!sizes_ok(N, P1, P2, K) || K < 1 || D < 1 || occupancy < 0) return P3D_ERR_INVALID_ARG;
  if (D != 3 || K > P3D_KNN_MAX_K) return P3D_ERR_UNSUPPORTED;
  if (N * P1 == 0) return P3D_OK;
  if (!p1 || !idx || !dists || (P2 > 0 && !p2)) return P3D_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < p3di_knn_grid_forward_workspace_bytes(N, P1, P2)) return P3D_ERR_WORKSPACE;
  const int64_t bpc = ceil_div(P1, kWave), blocks = N * bpc;
  if (blocks > 0x7fffffffll || N * kBoundsBlocks > 0x7fffffffll) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const Workspace w(workspace, N, P1, P2);
  const int cap = cell_cap(P2);
  const int occ = occupancy > 0 ? occupancy : P3D_KNN_GRID_OCCUPANCY;
  int bounds_blocks = (int)ceil_div(P2, kBoundsRows);
  bounds_blocks = bounds_blocks < 1 ? 1 : (bounds_blocks > kBoundsBlocks ? kBoundsBlocks : bounds_blocks);
  Points pts;
  pts.p1 = p1, pts.p2 = p2, pts.lengths1 = lengths1, pts.lengths2 = lengths2, pts.N = N, pts.P1 = P1, pts.P2 = P2;
  const float4* rec2 = w.records;
  const float4* rec1 = w.records + N * P2;
  {
    LaunchScope ls("knn_grid_build", s);
    knn_grid_bounds_kernel<<<(unsigned)(N * bounds_blocks), 256, 0, s>>>(p2, lengths2, P2, bounds_blocks, w.partials, w.counts, 2 * N * (int64_t)cap);
    knn_grid_header_kernel<<<(unsigned)N, 64, 0, s>>>(w.partials, lengths2, P2, bounds_blocks, occ, cap, w.headers);
    knn_grid_count_kernel<<<stream_blocks(N * (P1 + P2)), 256, 0, s>>>(pts, w.headers, cap, w.counts);
    knn_grid_scan_kernel<<<(unsigned)(2 * N), kScanLanes, 0, s>>>(w.headers, N, cap, w.counts, w.starts);
    knn_grid_fill_kernel<<<stream_blocks(N * (P1 + P2)), 256, 0, s>>>(pts, w.headers, cap, w.counts, w.starts, w.records);
    const int rc = launch_status();
    if (rc != P3D_OK) return rc;
  }
  LaunchScope ls("knn_grid_search", s);
#define P3D_KNN_GRID_LAUNCH(KQ) \
  knn_grid_search_kernel<KQ><<<(unsigned)blocks, 64, 0, s>>>(w.headers, w.starts, cap, rec2, rec1, lengths1, lengths2, P1, P2, K, bpc, idx, dists)
  if (K == 1) P3D_KNN_GRID_LAUNCH(1);
  else if (K <= 2) P3D_KNN_GRID_LAUNCH(2);
  else if (K <= 4) P3D_KNN_GRID_LAUNCH(4);
  else if (K <= 8) P3D_KNN_GRID_LAUNCH(8);
  else if (K <= 16) P3D_KNN_GRID_LAUNCH(16);
  else P3D_KNN_GRID_LAUNCH(32);
#undef P3D_KNN_GRID_LAUNCH
  return launch_status();
}
