// knn_tree.hip -- K nearest neighbours between large 3D clouds through a tree of boxes built on the device: p3d_knn_points_forward's
// result at D = 3, norm 2, bit for bit, at a cost that follows the density of the data.  implicit_abi.h has the contract; DESIGN 8.33
// the figures.
//
// The search is EXACT.  Distances are knn.hip's pair_dist (unfused, coordinate order); the queue orders by (dist, j) whatever the
// order of the offers (knn_queue.h: LexQueue); the tree only decides which pairs are never looked at, and a node is skipped only
// where a proven lower bound (box_bound below) says that no point inside could enter the queue of any lane of the wave.  The ORDER of
// the points (the Morton keys, the sort) decides the time alone: a leaf's box is the exact minimum and maximum of whatever points it
// holds, so the result is the same for every permutation.
//
// The tree is implicit: the records of cloud n in key order, a leaf per kLeaf consecutive records, an inner node per kFan
// consecutive nodes of the level below; node i of level l covers the records [i * kLeaf * kFan^l, (i + 1) * kLeaf * kFan^l) and has
// ceil(lengths2[n] / (kLeaf * kFan^l)) siblings: no pointers, no atomics, the last node of a level may be partial.
//
// Launches, no host read, no atomic of any kind:
//   bounds   per cloud, 1..kBoundsBlocks workgroups: min / max of the FINITE coordinates of the valid rows of p2[n] into partials.
//   header   per cloud one wave: the box's corner and 2^21 / its longest side (0 where there is no side: every key is 0 then).
//   keys     one workgroup per kSortTile elements of the padded key tables (p2's, then p1's): the 63-bit Morton key of the row, 21
//            bits per axis, by the box of p2[n] -- a query outside it is clamped --, ~0 for padding; then the bitonic network up to
//            k = kSortTile in LDS.  An element is the pair (key, row), compared lexicographically: nothing is ever equal.
//   step     the network's steps with a partner kSortTile or more apart, one launch each; merge: the steps below that of one k, in LDS.
//            Every cloud is padded to the same power of two >= kSortTile, so the network never crosses a cloud and a launch sorts all
//            of them (and both tables at once where they are padded alike).
//   leaves   one wave per leaf: the records (x, y, z, j) in key order and the leaf's box by fminf / fmaxf trees.
//   inner    one workgroup per cloud, level after level behind a barrier: the union of the children's boxes.
//   search   one wave per 64 consecutive queries in key order, one wave per workgroup, control flow uniform across the wave: see
//            the kernel.
//
// Every loop has a bound known before it starts: the network's steps come from the padded sizes, the levels from P2, the stack never
// holds more than (kFan - 1) * levels + 1 nodes (a pop of an inner node pushes at most kFan), and a node is pushed once by its one
// parent, so a wave visits every node at most once: a search that cannot prune (a NaN query, a cloud shorter than K, all points
// identical) offers every point of its cloud once -- the brute-force scan, never anything else.
#include "implicit_abi.h"
#include "knn_grad.h"
#include "knn_queue.h"

namespace p3d {
namespace {

constexpr int kLeaf = P3D_KNN_TREE_LEAF, kFan = P3D_KNN_TREE_FANOUT;
static_assert(kLeaf == kWave, "one lane per point of a leaf");
static_assert(kFan == 8, "a level is three bits of the record's position");
constexpr int kLeafBits = 6, kFanBits = 3;
constexpr int kMaxLevels = 10;  // P2 <= 2^31: 2^25 leaves, nine levels of eight above them
constexpr int kStack = 96;      // >= (kFan - 1) * kMaxLevels + 1
constexpr int kSortTile = 2048, kSortLanes = kSortTile / 2;
constexpr int kBoundsBlocks = 64;  // partial boxes per cloud: one wave reduces them
constexpr int kBoundsRows = 4096;  // rows per partial box before a cloud gets the next workgroup
constexpr float kCells = 2097151.0f;  // 2^21 - 1: the largest cell coordinate along an axis
using u64 = unsigned long long;

__device__ __forceinline__ float quiet_nan() { return __int_as_float(0x7fc00000); }
__device__ __forceinline__ float neg_inf() { return __int_as_float(0xff800000); }
__device__ __forceinline__ bool is_finite(float x) { return fabsf(x) < pos_inf(); }
// a value every lane holds, in scalar registers: what is indexed by it is read by scalar loads
__device__ __forceinline__ int64_t uniform64(int64_t x) {
  return (int64_t)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(x >> 32)) << 32) |
                   (unsigned)__builtin_amdgcn_readfirstlane((int)x));
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

// nodes of level l over `len` records: ceil(len / (kLeaf * kFan^l)) -- nested ceilings of positive integers compose
__host__ __device__ __forceinline__ int64_t level_nodes(int64_t len, int l) {
  const int s = kLeafBits + kFanBits * l;
  return (len + ((int64_t)1 << s) - 1) >> s;
}

// grid: N * bpc workgroups of 256.  partials[(n * kBoundsBlocks + b) * 6 + {0..2: min, 3..5: max}] for b < bpc
__global__ __launch_bounds__(256) void knn_tree_bounds_kernel(const float* __restrict__ p2, const int64_t* __restrict__ lengths2, int64_t P2,
                                                              int bpc, float* __restrict__ partials) {
  __shared__ float part[4][6];
  const int64_t n = blockIdx.x / bpc;
  const int b = (int)(blockIdx.x % bpc);
  const int64_t len2 = knn::cloud_length(lengths2, n, P2);
  float lo[3] = {pos_inf(), pos_inf(), pos_inf()}, hi[3] = {neg_inf(), neg_inf(), neg_inf()};
  for (int64_t i = (int64_t)b * 256 + threadIdx.x; i < len2; i += (int64_t)bpc * 256) {
    const float* p = p2 + (n * P2 + i) * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float x = p[a];
      if (is_finite(x)) lo[a] = fminf(lo[a], x), hi[a] = fmaxf(hi[a], x);
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
    float r = part[0][a];
    for (int w = 1; w < 4; ++w) r = a < 3 ? fminf(r, part[w][a]) : fmaxf(r, part[w][a]);
    partials[(n * kBoundsBlocks + b) * 6 + a] = r;
  }
}

// grid: N workgroups of one wave.  headers[n] = (lo.x, lo.y, lo.z, cells per unit length); all 0 where the cloud has no finite extent
__global__ __launch_bounds__(64) void knn_tree_header_kernel(const float* __restrict__ partials, int bpc, float4* __restrict__ headers) {
  const int64_t n = blockIdx.x;
  const int lane = (int)threadIdx.x;
  float lo[3], ext = 0.0f;
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = wave_fmin(lane < bpc ? partials[(n * kBoundsBlocks + lane) * 6 + a] : pos_inf());
    const float hi = wave_fmax(lane < bpc ? partials[(n * kBoundsBlocks + lane) * 6 + 3 + a] : neg_inf());
    ok = ok && is_finite(lo[a]) && is_finite(hi);
    ext = fmaxf(ext, hi - lo[a]);  // +inf where the side is wider than FLT_MAX: the scale is 0 then
  }
  if (lane != 0) return;
  const float scale = ok && ext > 0.0f ? kCells / ext : 0.0f;
  const bool use = ok && is_finite(scale);
  headers[n] = use ? make_float4(lo[0], lo[1], lo[2], scale) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// 21 bits -> every third bit of 63
__device__ __forceinline__ u64 spread3(u64 x) {
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}
// the key of a point by the header of its cloud: a coordinate outside the box is clamped, NaN goes to cell 0.  Below 2^63.
__device__ __forceinline__ u64 morton_key(const float4 H, const float* __restrict__ p) {
  const u64 cx = (u64)fminf(fmaxf((p[0] - H.x) * H.w, 0.0f), kCells);
  const u64 cy = (u64)fminf(fmaxf((p[1] - H.y) * H.w, 0.0f), kCells);
  const u64 cz = (u64)fminf(fmaxf((p[2] - H.z) * H.w, 0.0f), kCells);
  return spread3(cx) | spread3(cy) << 1 | spread3(cz) << 2;
}

// ---- the sort: a bitonic network over elements (key, row), every cloud padded to `pad` elements (a power of two >= kSortTile)
__device__ __forceinline__ bool elem_after(u64 ka, int va, u64 kb, int vb) { return ka > kb || (ka == kb && va > vb); }

// steps j = j_from, j_from / 2, .. 1 of stage k on the tile in LDS; i0: the tile's first position inside its cloud
__device__ __forceinline__ void tile_steps(u64* key, int* val, int k, int j_from, int i0) {
  const int t = (int)threadIdx.x;
  for (int j = j_from; j > 0; j >>= 1) {
    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
    const bool ascending = ((i0 + i) & k) == 0;
    const u64 ka = key[i], kb = key[l];
    const int va = val[i], vb = val[l];
    if (elem_after(ka, va, kb, vb) == ascending) key[i] = kb, key[l] = ka, val[i] = vb, val[l] = va;
    __syncthreads();
  }
}

// grid: N * (pad2 + pad1) / kSortTile workgroups of kSortLanes.  Tiles of p2's table first, then p1's; both keyed by p2's box.
__global__ __launch_bounds__(kSortLanes) void knn_tree_keys_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                                                                    const int64_t* __restrict__ lengths1, const int64_t* __restrict__ lengths2,
                                                                    int64_t N, int64_t P1, int64_t P2, int pad1, int pad2,
                                                                    const float4* __restrict__ headers, u64* __restrict__ keys,
                                                                    int* __restrict__ vals) {
  __shared__ u64 key[kSortTile];
  __shared__ int val[kSortTile];
  const int64_t tiles2 = N * (pad2 / kSortTile);
  const bool target = (int64_t)blockIdx.x < tiles2;
  const int64_t tile = target ? (int64_t)blockIdx.x : (int64_t)blockIdx.x - tiles2;
  const int pad = target ? pad2 : pad1;
  const int64_t P = target ? P2 : P1;
  const int64_t n = tile / (pad / kSortTile);
  const int i0 = (int)(tile % (pad / kSortTile)) * kSortTile;
  const int64_t len = knn::cloud_length(target ? lengths2 : lengths1, n, P);
  const float* const src = (target ? p2 : p1) + n * P * 3;
  const float4 H = headers[n];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = (int)threadIdx.x + u * kSortLanes, i = i0 + e;
    key[e] = i < len ? morton_key(H, src + (int64_t)i * 3) : ~0ull;
    val[e] = i;
  }
  __syncthreads();
  for (int k = 2; k <= kSortTile; k <<= 1) tile_steps(key, val, k, k >> 1, i0);
  const int64_t out = (int64_t)blockIdx.x * kSortTile;  // the two tables lie behind one another
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = (int)threadIdx.x + u * kSortLanes;
    keys[out + e] = key[e], vals[out + e] = val[e];
  }
}

// one step (k, j), j >= kSortTile, over `total` elements (a multiple of pad): a lane per pair
__global__ __launch_bounds__(256) void knn_tree_sort_step_kernel(u64* __restrict__ keys, int* __restrict__ vals, int64_t total, int pad, int k,
                                                                 int j) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total / 2; t += (int64_t)gridDim.x * 256) {
    const int64_t i = ((t & ~(int64_t)(j - 1)) << 1) | (t & (j - 1)), l = i | j;
    const bool ascending = ((int)(i & (pad - 1)) & k) == 0;
    const u64 ka = keys[i], kb = keys[l];
    const int va = vals[i], vb = vals[l];
    if (elem_after(ka, va, kb, vb) == ascending) keys[i] = kb, keys[l] = ka, vals[i] = vb, vals[l] = va;
  }
}

// the steps j < kSortTile of stage k: a workgroup per tile
__global__ __launch_bounds__(kSortLanes) void knn_tree_sort_merge_kernel(u64* __restrict__ keys, int* __restrict__ vals, int pad, int k) {
  __shared__ u64 key[kSortTile];
  __shared__ int val[kSortTile];
  const int64_t at = (int64_t)blockIdx.x * kSortTile;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = (int)threadIdx.x + u * kSortLanes;
    key[e] = keys[at + e], val[e] = vals[at + e];
  }
  __syncthreads();
  tile_steps(key, val, k, kSortTile >> 1, (int)(at & (pad - 1)));
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = (int)threadIdx.x + u * kSortLanes;
    keys[at + e] = key[e], vals[at + e] = val[e];
  }
}

// ---- the tree.  A node's box is two float4: (lo, 0), (hi, 0).  Level l of cloud n begins at node base(l) + n * cap(l), where
// cap(l) = level_nodes(P2, l) and base(l) = N * (cap(0) + .. + cap(l - 1)): functions of the shapes.
struct Levels {
  int64_t base[kMaxLevels];
  int count;  // levels whose cap is >= 1, the last one with cap 1
};

// grid: ceil(N * cap0 / 4) workgroups of 256, a wave per leaf.  records: N * P2 float4, (x, y, z, row) in key order.
__global__ __launch_bounds__(256) void knn_tree_leaves_kernel(const float* __restrict__ p2, const int64_t* __restrict__ lengths2, int64_t N,
                                                              int64_t P2, int pad2, const int* __restrict__ vals2, int64_t cap0,
                                                              float4* __restrict__ records, float4* __restrict__ boxes) {
  const int64_t w = (int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (w >= N * cap0) return;
  const int64_t n = w / cap0, leaf = w % cap0;
  const int64_t len2 = knn::cloud_length(lengths2, n, P2);
  if (leaf >= level_nodes(len2, 0)) return;
  const int lane = lane_id();
  const int64_t s = leaf * kLeaf + lane;
  float lo[3] = {pos_inf(), pos_inf(), pos_inf()}, hi[3] = {neg_inf(), neg_inf(), neg_inf()};
  if (s < len2) {
    int64_t j = vals2[n * pad2 + s];
    j = j >= 0 && j < len2 ? j : s;  // what a sort of this cloud's own rows cannot give: never read outside the cloud
    const float* p = p2 + (n * P2 + j) * 3;
    records[n * P2 + s] = make_float4(p[0], p[1], p[2], __int_as_float((int)j));
#pragma unroll
    for (int a = 0; a < 3; ++a) lo[a] = hi[a] = p[a];
  }
  // fminf / fmaxf pass over a NaN: a point with one lies outside its leaf's box, and its distance to anything is NaN -- never taken
#pragma unroll
  for (int a = 0; a < 3; ++a) lo[a] = wave_fmin(lo[a]), hi[a] = wave_fmax(hi[a]);
  if (lane == 0) {
    boxes[2 * w] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    boxes[2 * w + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
  }
}

// grid: N workgroups of 256.  Level l reads what the same workgroup wrote for level l - 1 in front of the barrier.
__global__ __launch_bounds__(256) void knn_tree_inner_kernel(const int64_t* __restrict__ lengths2, int64_t P2, Levels L, float4* boxes) {
  const int64_t n = blockIdx.x;
  const int64_t len2 = knn::cloud_length(lengths2, n, P2);
#pragma unroll 1
  for (int l = 1; l < kMaxLevels; ++l) {
    if (l >= L.count) break;
    const int64_t below = level_nodes(len2, l - 1), here = level_nodes(len2, l);
    const float4* const from = boxes + 2 * (L.base[l - 1] + n * level_nodes(P2, l - 1));
    float4* const to = boxes + 2 * (L.base[l] + n * level_nodes(P2, l));
    for (int64_t i = threadIdx.x; i < here; i += 256) {
      float4 lo = from[2 * (i * kFan)], hi = from[2 * (i * kFan) + 1];
      for (int64_t c = i * kFan + 1; c < (i + 1) * kFan && c < below; ++c) {
        const float4 a = from[2 * c], b = from[2 * c + 1];
        lo.x = fminf(lo.x, a.x), lo.y = fminf(lo.y, a.y), lo.z = fminf(lo.z, a.z);
        hi.x = fmaxf(hi.x, b.x), hi.y = fmaxf(hi.y, b.y), hi.z = fmaxf(hi.z, b.z);
      }
      to[2 * i] = lo, to[2 * i + 1] = hi;
    }
    __threadfence();
    __syncthreads();
  }
}

// THE LOWER BOUND.  box_bound(q, lo, hi) is the contract's distance between q and c = clamp(q, lo, hi), the nearest point of the box:
// the same unfused float32 subtract, square and add in coordinate order as pair_dist.  For every point p with lo_a <= p_a <= hi_a on
// every axis -- every point of the node whose coordinates are numbers, lo and hi being the exact float minimum and maximum --
// box_bound <= dist(q, p) as FLOATS, with no slack term, because every operation is monotone under round-to-nearest:
//   the gap.  Where q_a < lo_a, c_a = lo_a <= p_a: the reals q_a - p_a <= q_a - c_a <= 0, and rounding is monotone, so
//     fl(q_a - p_a) <= fl(q_a - c_a) <= 0: |fl(q_a - p_a)| >= |fl(q_a - c_a)|.  Where q_a > hi_a the mirror image.  Where q_a lies
//     inside, c_a = q_a and the gap is 0 <= anything's magnitude.  (A zero of either sign is the same number: -0 for +0 in lo or c
//     changes no magnitude.)
//   the square.  |x| >= |y| gives x^2 >= y^2 in the reals, hence fl(x x) >= fl(y y): overflow to +inf and underflow to 0 are
//     monotone too.
//   the sums.  fl(s + t) is monotone in s and in t: the two additions, in the same order, keep the inequality.
// What is not a number: a NaN or infinite q_a makes a gap of NaN (+inf - +inf) or +inf; a NaN bound fails every comparison, so such
// a lane never prunes, and a lane whose bound is +inf has an empty queue only when its distances are +inf or NaN as well -- and then
// its worst distance is +inf, which nothing is strictly above.  An infinite lo_a or hi_a (an infinite target inside) gives a gap of
// 0, +inf or NaN by the same arithmetic the distance to that target uses.  A box nothing is inside of (lo = +inf, hi = -inf: only
// NaN points) gives +inf: skipped by full queues, and nothing in it could be taken.
// THE RULE.  A node is skipped only if bound > worst holds in EVERY live lane, worst being the lane's min(K, lengths2[n])-th
// distance so far, +inf while the queue is short of that.  Strictly: a point at exactly the worst distance with a smaller j would
// have to displace the worst entry.  A lane that skipped has dist(q, p) >= bound > worst >= every later worst: p could never enter.
__device__ __forceinline__ float box_bound(const float (&q)[3], const float4 lo, const float4 hi) {
  const float dx = q[0] - fminf(fmaxf(q[0], lo.x), hi.x);
  const float dy = q[1] - fminf(fmaxf(q[1], lo.y), hi.y);
  const float dz = q[2] - fminf(fmaxf(q[2], lo.z), hi.z);
  float dn = dx * dx;
  dn = dn + dy * dy;
  dn = dn + dz * dz;
  return dn;
}

// grid: N * blocks_per_cloud workgroups of one wave; K <= KQ.
// The wave's 64 queries are neighbours in key order.  It first walks down by keys -- at each level the last child whose first key
// is at or below the key of the wave's middle query, the eight first keys read by eight lanes at once -- and offers that leaf, so
// that the queues fill before anything is tested.  Then it walks the tree from the root with one stack in LDS: pop a node, test it
// again (the queues have shrunk since it was pushed), and either offer the leaf or test the children, each against every lane, and
// push those that some lane needs, the farthest first by the wave's smallest bound, so that the nearest is popped next.  A leaf's
// records are staged in LDS once per wave and read by broadcast, four points per ds_read_b128 and coordinate; while they are
// offered, the records of the node on top of the stack, if that is a leaf, are already on their way into registers.  A lane whose
// own bound fails needs no mask: every distance into that box is >= its bound > its worst, which the queue refuses by itself.
template <int KQ>
__global__ __launch_bounds__(64) void knn_tree_search_kernel(const float* __restrict__ p1, const int* __restrict__ vals1,
                                                             const u64* __restrict__ keys1, const u64* __restrict__ keys2,
                                                             const float4* __restrict__ rec2, const float4* __restrict__ boxes, Levels L,
                                                             const int64_t* __restrict__ lengths1, const int64_t* __restrict__ lengths2,
                                                             int64_t P1, int64_t P2, int pad1, int pad2, int K, int64_t blocks_per_cloud,
                                                             int64_t* __restrict__ idx, float* __restrict__ dists) {
  __shared__ __align__(16) float tile[3][kLeaf];
  __shared__ __align__(16) int tile_j[kLeaf];
  __shared__ unsigned stack[kStack];
  __shared__ int64_t level_at[kMaxLevels];  // of this cloud: the first node of each level
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
    float q[3] = {0.0f, 0.0f, 0.0f};
    if (live) {
      const int64_t own = vals1[n * pad1 + slot];
      row = own >= 0 && own < len1 ? own : slot;
      const float* p = p1 + (n * P1 + row) * 3;
      q[0] = p[0], q[1] = p[1], q[2] = p[2];
    }
    if (lane < kMaxLevels) level_at[lane] = lane < L.count ? L.base[lane < L.count ? lane : 0] + n * level_nodes(P2, lane) : 0;
    __syncthreads();
    const float4* const points = rec2 + n * P2;
    int root = 0;  // the lowest level with one node
    while (root < L.count - 1 && level_nodes(len2, root) > 1) ++root;
    float worst = pos_inf();

    float4 ahead = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // the records of leaf `ahead_leaf`, one per lane
    int ahead_leaf = -1;
    auto fetch = [&](int leaf) {
      const int64_t at = (int64_t)leaf * kLeaf + lane;
      return at < len2 ? points[at] : make_float4(quiet_nan(), quiet_nan(), quiet_nan(), 0.0f);
    };
    // ---- down by keys to the leaf at the wave's own place
    int first_leaf = 0;
    {
      const int64_t mid = b * kWave + kWave / 2;
      const u64 qkey = keys1[n * pad1 + (mid < len1 ? mid : len1 - 1)];
      const u64* const k2 = keys2 + n * pad2;
      for (int l = root; l > 0; --l) {
        const int64_t c = (int64_t)first_leaf * kFan + lane;
        const bool at_or_below = lane < kFan && c < level_nodes(len2, l - 1) && k2[c << (kLeafBits + kFanBits * (l - 1))] <= qkey;
        const unsigned m = (unsigned)__ballot(at_or_below) & 0xffu;
        first_leaf = first_leaf * kFan + (m ? 31 - __builtin_clz(m) : 0);
      }
      first_leaf = __builtin_amdgcn_readfirstlane(first_leaf);
    }

    // ---- the walk.  A stack entry is level << 28 | node; a node index is below 2^25.  Level kFirst: the leaf found above, offered
    // untested; the walk passes over it where it meets it again: a point is offered once.
    constexpr unsigned kFirst = 15u;
    int top = 2;
    if (lane == 0) stack[0] = (unsigned)root << 28, stack[1] = kFirst << 28 | (unsigned)first_leaf;
    while (top > 0) {
      __syncthreads();  // the pushes are in place
      const unsigned entry = (unsigned)__builtin_amdgcn_readfirstlane((int)stack[top - 1]);
      --top;
      const bool first = entry >> 28 == kFirst;
      const int level = first ? 0 : (int)(entry >> 28), node = (int)(entry & 0x0fffffffu);
      if (!first) {
        if (level == 0 && node == first_leaf) continue;
        const int64_t at = uniform64(level_at[level]);
        const float bound = box_bound(q, boxes[2 * (at + node)], boxes[2 * (at + node) + 1]);
        if (__ballot(live && !(bound > worst)) == 0ull) continue;
      }
      if (level == 0) {
        const float4 v = node == ahead_leaf ? ahead : fetch(node);
        __syncthreads();  // the wave is done with the tile before
        tile[0][lane] = v.x, tile[1][lane] = v.y, tile[2][lane] = v.z, tile_j[lane] = __float_as_int(v.w);
        __syncthreads();
        if (top > 0) {  // the node that is popped next: a leaf's records set out now
          const unsigned next = (unsigned)__builtin_amdgcn_readfirstlane((int)stack[top - 1]);
          if (next >> 28 == 0u) ahead_leaf = (int)next, ahead = fetch((int)next);
        }
#pragma unroll 4
        for (int e = 0; e < kLeaf; e += 4) {
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
        worst = best.d[0];
#pragma unroll
        for (int s = 1; s < KQ; ++s) worst = s == found - 1 ? best.d[s] : worst;
        continue;
      }
      // lane c < kFan keeps child c's verdict and the wave's smallest bound to it
      const int64_t below = level_nodes(len2, level - 1);
      const int64_t cat = uniform64(level_at[level - 1]);
      float near = pos_inf();
      bool keep = false;
#pragma unroll
      for (int c = 0; c < kFan; ++c) {
        const int64_t child = (int64_t)node * kFan + c;
        if (child >= below) break;  // uniform
        if (level == 1 && child == first_leaf) continue;
        const float cb = box_bound(q, boxes[2 * (cat + child)], boxes[2 * (cat + child) + 1]);
        const bool some = __ballot(live && !(cb > worst)) != 0ull;
        // It only orders.  fminf passes over a NaN next to a number, but where EVERY live lane has a NaN bound (64 NaN queries,
        // which share key 0 and so a wave; +inf queries against a box that reaches +inf) the minimum is NaN itself: +inf then,
        // so that `near` is never NaN and the order below is total.
        const float m = wave_fmin(live ? cb : pos_inf());
        if (lane == c) near = m == m ? m : pos_inf(), keep = some;
      }
      // the farthest kept child first: rank = the kept children that are nearer (or as near with a smaller number).  No `near`
      // is NaN, so (near, c) is a total order and the kept children get the distinct ranks 0 .. kept - 1: every slot is written
      int rank = 0;
#pragma unroll
      for (int c = 0; c < kFan; ++c) {
        const float m = __shfl(near, c);
        const bool k = __shfl((int)keep, c) != 0;
        rank += k && (m < near || (m == near && c < lane)) ? 1 : 0;
      }
      const int kept = __popcll(__ballot(keep));
      if (keep && top + kept <= kStack) stack[top + kept - 1 - rank] = (unsigned)(level - 1) << 28 | (unsigned)(node * kFan + lane);
      top += top + kept <= kStack ? kept : 0;  // cannot overflow: at most (kFan - 1) * levels + 1 entries
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
  if (N < 0 || P1 < 0 || P2 < 0 || P2 > (1ll << 30) || P1 > (1ll << 30)) return false;  // the padded tables stay below 2^31 rows
  const int64_t per_cloud = (P1 > P2 ? P1 : P2) * (int64_t)(K > 0 ? K : 1) * 64;
  return N == 0 || per_cloud <= INT64_MAX / 4 / N;
}

// a cloud's rows in the key tables: the power of two >= max(P, kSortTile)
int padded(int64_t P) {
  int64_t pad = kSortTile;
  while (pad < P) pad <<= 1;
  return (int)pad;
}

struct Workspace {
  float* partials;
  float4* headers;
  u64* keys;  // p2's table, N * pad2, then p1's, N * pad1
  int* vals;
  float4 *records, *boxes;
  Levels levels;
  int pad1, pad2;
  size_t bytes;
  Workspace(void* ws, int64_t N, int64_t P1, int64_t P2) : pad1(padded(P1)), pad2(padded(P2)) {
    int64_t nodes = 0;
    levels.count = 0;
    for (int l = 0; l < kMaxLevels; ++l) {
      const int64_t cap = level_nodes(P2, l);
      levels.base[l] = nodes;
      if (cap >= 1 && (l == 0 || level_nodes(P2, l - 1) > 1)) nodes += N * cap, levels.count = l + 1;
    }
    Arena a(ws, ~(size_t)0);
    partials = a.take<float>((size_t)N * kBoundsBlocks * 6);
    headers = a.take<float4>((size_t)N);
    keys = a.take<u64>((size_t)N * ((size_t)pad1 + (size_t)pad2));
    vals = a.take<int>((size_t)N * ((size_t)pad1 + (size_t)pad2));
    records = a.take<float4>((size_t)N * (size_t)P2);
    boxes = a.take<float4>(2 * (size_t)nodes);
    bytes = a.off;
  }
};

// the rest of the network behind the keys kernel: stages k = 2 kSortTile .. pad over `clouds` clouds of `pad` elements
void sort_rest(u64* keys, int* vals, int64_t clouds, int pad, hipStream_t s) {
  const int64_t total = clouds * pad;
  for (int64_t k = 2 * (int64_t)kSortTile; k <= pad; k <<= 1) {
    for (int64_t j = k >> 1; j >= kSortTile; j >>= 1) knn_tree_sort_step_kernel<<<stream_blocks(total / 2), 256, 0, s>>>(keys, vals, total, pad, (int)k, (int)j);
    knn_tree_sort_merge_kernel<<<(unsigned)(total / kSortTile), kSortLanes, 0, s>>>(keys, vals, pad, (int)k);
  }
}

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API size_t p3di_knn_tree_forward_workspace_bytes(int64_t N, int64_t P1, int64_t P2) {
  if (N <= 0 || P1 <= 0 || P2 < 0 || !sizes_ok(N, P1, P2, 1)) return 0;
  return Workspace(nullptr, N, P1, P2).bytes;
}

P3D_API int p3di_knn_tree_forward(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2, int64_t N, int64_t P1,
                                 int64_t P2, int D, int K, int64_t* idx, float* dists, void* workspace, size_t workspace_bytes,
                                 p3d_stream_t stream) {
  if (!sizes_ok(N, P1, P2, K) || K < 1 || D < 1) return P3D_ERR_INVALID_ARG;
  if (D != 3 || K > P3D_KNN_MAX_K) return P3D_ERR_UNSUPPORTED;
  if (N * P1 == 0) return P3D_OK;
  if (!p1 || !idx || !dists || (P2 > 0 && !p2)) return P3D_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < p3di_knn_tree_forward_workspace_bytes(N, P1, P2)) return P3D_ERR_WORKSPACE;
  const Workspace w(workspace, N, P1, P2);
  const int64_t bpc = ceil_div(P1, kWave), blocks = N * bpc, cap0 = level_nodes(P2, 0);
  const int64_t tiles = N * ((int64_t)(w.pad1 + w.pad2) / kSortTile);
  if (blocks > 0x7fffffffll || N * kBoundsBlocks > 0x7fffffffll || tiles > 0x7fffffffll || ceil_div(N * cap0, 4) > 0x7fffffffll) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  u64* const keys1 = w.keys + N * (int64_t)w.pad2;
  int* const vals1 = w.vals + N * (int64_t)w.pad2;
  if (P2 > 0) {  // an empty p2 finds nothing: the search writes its zeros without a tree
    LaunchScope ls("knn_tree_build", s);
    int bounds_blocks = (int)ceil_div(P2, kBoundsRows);
    bounds_blocks = bounds_blocks < 1 ? 1 : (bounds_blocks > kBoundsBlocks ? kBoundsBlocks : bounds_blocks);
    knn_tree_bounds_kernel<<<(unsigned)(N * bounds_blocks), 256, 0, s>>>(p2, lengths2, P2, bounds_blocks, w.partials);
    knn_tree_header_kernel<<<(unsigned)N, 64, 0, s>>>(w.partials, bounds_blocks, w.headers);
    knn_tree_keys_kernel<<<(unsigned)tiles, kSortLanes, 0, s>>>(p1, p2, lengths1, lengths2, N, P1, P2, w.pad1, w.pad2, w.headers, w.keys, w.vals);
    if (w.pad1 == w.pad2) {
      sort_rest(w.keys, w.vals, 2 * N, w.pad2, s);
    } else {
      sort_rest(w.keys, w.vals, N, w.pad2, s);
      sort_rest(keys1, vals1, N, w.pad1, s);
    }
    knn_tree_leaves_kernel<<<(unsigned)ceil_div(N * cap0, 4), 256, 0, s>>>(p2, lengths2, N, P2, w.pad2, w.vals, cap0, w.records, w.boxes);
    if (w.levels.count > 1) knn_tree_inner_kernel<<<(unsigned)N, 256, 0, s>>>(lengths2, P2, w.levels, w.boxes);
    const int rc = launch_status();
    if (rc != P3D_OK) return rc;
  }
  LaunchScope ls("knn_tree_search", s);
#define P3D_KNN_TREE_LAUNCH(KQ)                                                                                                          \
  knn_tree_search_kernel<KQ><<<(unsigned)blocks, 64, 0, s>>>(p1, vals1, keys1, w.keys, w.records, w.boxes, w.levels, lengths1, lengths2, P1, \
                                                             P2, w.pad1, w.pad2, K, bpc, idx, dists)
  if (K == 1) P3D_KNN_TREE_LAUNCH(1);
  else if (K <= 2) P3D_KNN_TREE_LAUNCH(2);
  else if (K <= 4) P3D_KNN_TREE_LAUNCH(4);
  else if (K <= 8) P3D_KNN_TREE_LAUNCH(8);
  else if (K <= 16) P3D_KNN_TREE_LAUNCH(16);
  else P3D_KNN_TREE_LAUNCH(32);
#undef P3D_KNN_TREE_LAUNCH
  return launch_status();
}
