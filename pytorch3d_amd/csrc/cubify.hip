// cubify.hip -- voxel occupancy grids to merged cube meshes (the reference's pytorch3d/ops/cubify.py, a torch chain there).
// Contract: implicit_abi.h (p3di_cubify_*).  Count -> scan -> fill, as binning.hip and clip.hip do; integers and gathered floats only:
// no atomic anywhere, so every run, stream and launch shape writes the same bits.
//
// Work is cut into SCAN BLOCKS of P3D_CUBIFY_ITEMS consecutive items of ONE mesh (voxels in output order (h, w, d), lattice points in
// g order), P3D_CUBIFY_BLOCK lanes going over them in rounds.  A scan block never spans two meshes: mesh n owns the blocks
// [n * bpm, (n + 1) * bpm), bpm = ceil(items per mesh / P3D_CUBIFY_ITEMS), so per-mesh totals and the per-mesh restart of the vertex
// ranks are differences of block carries and need no segmented scan.
//
//   count   classify_kernel   a lane per voxel: 7 strided occupancy reads -> the 6-bit exposure mask, one byte, in output order; the
//                             block's face total (2 popcount) goes to the face carry table.
//           vertex_kernel     a lane per lattice point: kept iff one of the 8 voxels around it exposes a side that meets at this corner
//                             (a gather over the masks).  The kept flags are scanned by ballot / mbcnt within a wave and 4 wave sums
//                             in LDS; the lane's rank INSIDE its block is stored (kept: rank, dropped: ~rank), the block's total goes to
//                             the vertex carry table.
//           carry_kernel      two workgroups of P3D_CUBIFY_CARRY_BLOCK lanes, one per carry table: the exclusive scan of the block
//                             totals in rounds, in place, the grand total behind the last block; then (V_n, F_n) per mesh.
//   emit    emit_faces_kernel a lane per voxel again: the masks' block scan is redone (a byte read) instead of kept as a table, so a
//                             voxel's faces start at carry[block] + its prefix; the rank of a corner is its block-local rank plus its
//                             block's carry minus the carry of the mesh's first block.
//           emit_verts_kernel a lane per lattice point: the kept ones write their float32 row at carry[block] + rank.
// Blocks whose carry does not move (nothing to emit) leave at once: a ball-shaped occupancy emits from its shell's blocks only.
// The host reads the (N, 2) counts between the two entries, sizes the outputs and calls emit: the one sync of a call.
#include "implicit_abi.h"
#include "p3d_common.h"
#include "scan_blocks.h"

namespace p3d {
namespace {

constexpr int kLanes = P3D_CUBIFY_BLOCK;
constexpr int kItems = P3D_CUBIFY_ITEMS;
constexpr int kCarryLanes = P3D_CUBIFY_CARRY_BLOCK;
static_assert(kLanes == 256 && kItems % kLanes == 0 && kCarryLanes % kWave == 0 && kCarryLanes <= 1024, "launch constants");

struct Sizes {
  int64_t M, L;        // voxels and lattice points of one mesh
  int64_t bpm_f, bpm_v;  // scan blocks of one mesh: over its voxels, over its lattice points
};

// false: a size the kernels' int32 indices do not cover (the Python layer takes its torch formulation there)
bool sizes_of(int64_t N, int64_t D, int64_t H, int64_t W, Sizes* s) {
  if (N < 0 || D < 1 || H < 1 || W < 1 || D >= INT32_MAX || H >= INT32_MAX || W >= INT32_MAX) return false;
  int64_t M = D * H, L = (D + 1) * (H + 1);
  if (L > INT32_MAX) return false;
  M *= W;
  L *= W + 1;
  if (L > INT32_MAX) return false;
  if (N > 0 && (L > INT32_MAX / N || 12 * M > INT32_MAX / N)) return false;
  s->M = M;
  s->L = L;
  s->bpm_f = ceil_div(M, kItems);
  s->bpm_v = ceil_div(L, kItems);
  return N * s->bpm_v < INT32_MAX;
}

struct Workspace {
  uint8_t* masks;  // N * M, order (n, h, w, d)
  int* local;      // N * L block-local vertex ranks (dropped: ~rank)
  int* carry_f;    // N * bpm_f + 1
  int* carry_v;    // N * bpm_v + 1
  size_t bytes;
};

Workspace carve(void* workspace, int64_t N, const Sizes& s) {
  Arena a(workspace, ~(size_t)0);
  Workspace w;
  w.masks = a.take<uint8_t>((size_t)(N * s.M));
  w.local = a.take<int>((size_t)(N * s.L));
  w.carry_f = a.take<int>((size_t)(N * s.bpm_f + 1));
  w.carry_v = a.take<int>((size_t)(N * s.bpm_v + 1));
  w.bytes = a.off;
  return w;
}

__device__ __forceinline__ bool occupied(const float* p, float thresh) { return *p >= thresh; }  // NaN: false

// grid: N * bpm blocks.  sums[block] = the faces of the block's voxels.
__global__ __launch_bounds__(kLanes) void classify_kernel(const float* __restrict__ voxels, int64_t sn, int64_t sd, int64_t sh, int64_t sw,
                                                          int D, int H, int W, int M, int bpm, float thresh,
                                                          uint8_t* __restrict__ masks, int* __restrict__ sums) {
  __shared__ int wsum[kLanes / kWave];
  const int n = (int)blockIdx.x / bpm, j = (int)blockIdx.x % bpm;
  const float* grid = voxels + (int64_t)n * sn;
  int faces = 0;
  for (int r = 0; r < kItems / kLanes; ++r) {
    const int i = j * kItems + r * kLanes + (int)threadIdx.x;
    if (i >= M) break;
    const int d = i % D, t = i / D, w = t % W, h = t / W;
    const float* p = grid + d * sd + h * sh + w * sw;
    unsigned m = 0;
    if (occupied(p, thresh)) {
      m |= (w > 0 && occupied(p - sw, thresh)) ? 0u : 1u;       // -x
      m |= (h + 1 < H && occupied(p + sh, thresh)) ? 0u : 2u;   // +y
      m |= (d > 0 && occupied(p - sd, thresh)) ? 0u : 4u;       // -z
      m |= (h > 0 && occupied(p - sh, thresh)) ? 0u : 8u;       // -y
      m |= (w + 1 < W && occupied(p + sw, thresh)) ? 0u : 16u;  // +x
      m |= (d + 1 < D && occupied(p + sd, thresh)) ? 0u : 32u;  // +z
    }
    masks[(int64_t)n * M + i] = (uint8_t)m;
    faces += 2 * __popc(m);
  }
  const int incl = wave_inclusive(faces);
  int total;
  block_exclusive<kLanes / kWave>(0, __shfl(incl, kWave - 1), wsum, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// grid: N * bpm blocks.  local[n * L + g] = the rank of g among the kept points of its block (~rank where g is dropped).
__global__ __launch_bounds__(kLanes) void vertex_kernel(const uint8_t* __restrict__ masks, int D, int H, int W, int M, int L, int bpm,
                                                        int* __restrict__ local, int* __restrict__ sums) {
  __shared__ int wsum[kLanes / kWave];
  const int n = (int)blockIdx.x / bpm, j = (int)blockIdx.x % bpm;
  const uint8_t* mesh = masks + (int64_t)n * M;
  int running = 0;
  for (int r = 0; r < kItems / kLanes; ++r) {  // every lane stays for the barriers of block_exclusive
    const int g = j * kItems + r * kLanes + (int)threadIdx.x;
    unsigned hit = 0;
    if (g < L) {
      const int z = g % (D + 1), t = g / (D + 1), x = t % (W + 1), y = t / (W + 1);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int a = (c >> 1) & 1, b = (c >> 2) & 1, e = c & 1;  // this point is corner (x = b, y = a, z = e) of voxel (y-a, x-b, z-e)
        const int h = y - a, w = x - b, d = z - e;
        if (h >= 0 && h < H && w >= 0 && w < W && d >= 0 && d < D)
          hit |= mesh[(h * W + w) * D + d] & ((b ? 16u : 1u) | (a ? 2u : 8u) | (e ? 32u : 4u));
      }
    }
    const unsigned long long ballot = __ballot(hit != 0);
    int total;
    const int rank = running + block_exclusive<kLanes / kWave>(mask_rank(ballot), __popcll(ballot), wsum, &total);
    if (g < L) local[(int64_t)n * L + g] = hit ? rank : ~rank;
    running += total;
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = running;
}

// corners of the twelve triangles, two per direction in the mask's bit order
__device__ constexpr int kTri[12][3] = {{0, 1, 2}, {1, 3, 2}, {2, 3, 6}, {3, 7, 6}, {0, 2, 6}, {0, 6, 4},
                                        {0, 5, 1}, {0, 4, 5}, {6, 7, 5}, {6, 5, 4}, {1, 7, 3}, {1, 5, 7}};

// grid: N * bpm_f blocks
__global__ __launch_bounds__(kLanes) void emit_faces_kernel(const uint8_t* __restrict__ masks, const int* __restrict__ local,
                                                            const int* __restrict__ carry_f, const int* __restrict__ carry_v, int D,
                                                            int H, int W, int M, int L, int bpm_f, int bpm_v,
                                                            int64_t* __restrict__ faces, const float* __restrict__ feats, int64_t fn,
                                                            int64_t fk, int64_t fd, int64_t fh, int64_t fw, int K,
                                                            float* __restrict__ face_feats) {
  __shared__ int wsum[kLanes / kWave];
  int running = carry_f[blockIdx.x];
  if (carry_f[blockIdx.x + 1] == running) return;  // the whole workgroup: nothing exposed in this block
  const int n = (int)blockIdx.x / bpm_f, j = (int)blockIdx.x % bpm_f;
  const int* vcarry = carry_v + (int64_t)n * bpm_v;
  const int* vlocal = local + (int64_t)n * L;
  const int first = vcarry[0];
  for (int r = 0; r < kItems / kLanes; ++r) {
    const int i = j * kItems + r * kLanes + (int)threadIdx.x;
    const unsigned m = i < M ? masks[(int64_t)n * M + i] : 0u;
    const int cnt = 2 * __popc(m);
    const int incl = wave_inclusive(cnt);
    int total;
    int64_t row = running + block_exclusive<kLanes / kWave>(incl - cnt, __shfl(incl, kWave - 1), wsum, &total);
    running += total;
    if (m == 0) continue;
    const int d = i % D, t = i / D, w = t % W, h = t / W;
    int64_t rank[8];  // of the corners that an exposed side uses; the others are never stored
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int g = ((h + ((c >> 1) & 1)) * (W + 1) + w + ((c >> 2) & 1)) * (D + 1) + d + (c & 1);
      rank[c] = (int64_t)(vlocal[g] + vcarry[g / kItems] - first);
    }
    const float* f = feats ? feats + n * fn + d * fd + h * fh + w * fw : nullptr;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      if (!((m >> k) & 1u)) continue;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        int64_t* o = faces + (row + u) * 3;
        o[0] = rank[kTri[2 * k + u][0]];
        o[1] = rank[kTri[2 * k + u][1]];
        o[2] = rank[kTri[2 * k + u][2]];
      }
      if (f) {
        for (int c = 0; c < K; ++c) {
          const float v = f[c * fk];
          face_feats[row * K + c] = v;
          face_feats[(row + 1) * K + c] = v;
        }
      }
      row += 2;
    }
  }
}

// grid: N * bpm blocks.  coords: the x values (W + 1), then the y values (H + 1), then the z values (D + 1).
__global__ __launch_bounds__(kLanes) void emit_verts_kernel(const int* __restrict__ local, const int* __restrict__ carry_v, int D, int H,
                                                            int W, int L, int bpm, const float* __restrict__ coords,
                                                            float* __restrict__ verts) {
  const int base = carry_v[blockIdx.x];
  if (carry_v[blockIdx.x + 1] == base) return;
  const int n = (int)blockIdx.x / bpm, j = (int)blockIdx.x % bpm;
  for (int r = 0; r < kItems / kLanes; ++r) {
    const int g = j * kItems + r * kLanes + (int)threadIdx.x;
    if (g >= L) break;
    const int rank = local[(int64_t)n * L + g];
    if (rank < 0) continue;
    const int z = g % (D + 1), t = g / (D + 1), x = t % (W + 1), y = t / (W + 1);
    float* o = verts + (int64_t)(base + rank) * 3;
    o[0] = coords[x];
    o[1] = coords[W + 1 + y];
    o[2] = coords[W + 1 + H + 1 + z];
  }
}

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API size_t p3di_cubify_workspace_bytes(int64_t N, int64_t D, int64_t H, int64_t W) {
  Sizes s;
  return sizes_of(N, D, H, W, &s) ? carve(nullptr, N, s).bytes : 0;
}

P3D_API int p3di_cubify_count(const float* voxels, const int64_t voxel_strides[4], int64_t N, int64_t D, int64_t H, int64_t W,
                              float thresh, void* workspace, size_t workspace_bytes, int64_t* counts, p3d_stream_t stream) {
  Sizes s;
  if (!sizes_of(N, D, H, W, &s) || !voxel_strides) return P3D_ERR_INVALID_ARG;
  if (N == 0) return P3D_OK;
  if (!voxels || !counts) return P3D_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < carve(nullptr, N, s).bytes) return P3D_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const Workspace w = carve(workspace, N, s);
  LaunchScope ls("cubify_count", st);
  classify_kernel<<<(unsigned)(N * s.bpm_f), kLanes, 0, st>>>(voxels, voxel_strides[0], voxel_strides[1], voxel_strides[2],
                                                              voxel_strides[3], (int)D, (int)H, (int)W, (int)s.M, (int)s.bpm_f, thresh,
                                                              w.masks, w.carry_f);
  vertex_kernel<<<(unsigned)(N * s.bpm_v), kLanes, 0, st>>>(w.masks, (int)D, (int)H, (int)W, (int)s.M, (int)s.L, (int)s.bpm_v, w.local,
                                                            w.carry_v);
  carry_kernel<kCarryLanes><<<2, kCarryLanes, 0, st>>>(w.carry_f, (int)(N * s.bpm_f), (int)s.bpm_f, w.carry_v, (int)(N * s.bpm_v), (int)s.bpm_v, (int)N,
                                          counts);
  return launch_status();
}

P3D_API int p3di_cubify_emit(const float* coords, const float* feats, const int64_t feat_strides[5], int64_t K, int64_t N, int64_t D,
                             int64_t H, int64_t W, int64_t total_verts, int64_t total_faces, const void* workspace, size_t workspace_bytes,
                             float* verts, int64_t* faces, float* face_feats, p3d_stream_t stream) {
  Sizes s;
  if (!sizes_of(N, D, H, W, &s) || K < 0 || K > INT32_MAX || total_verts < 0 || total_faces < 0 || total_verts > N * s.L ||
      total_faces > 12 * N * s.M || (feats && !feat_strides))
    return P3D_ERR_INVALID_ARG;
  if (total_faces == 0) return P3D_OK;  // no face, so no kept vertex either
  if (!coords || !verts || !faces || total_verts == 0 || (feats && K > 0 && !face_feats)) return P3D_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < carve(nullptr, N, s).bytes) return P3D_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const Workspace w = carve(const_cast<void*>(workspace), N, s);
  const bool with_feats = feats && K > 0;
  LaunchScope ls("cubify_emit", st);
  emit_faces_kernel<<<(unsigned)(N * s.bpm_f), kLanes, 0, st>>>(
      w.masks, w.local, w.carry_f, w.carry_v, (int)D, (int)H, (int)W, (int)s.M, (int)s.L, (int)s.bpm_f, (int)s.bpm_v, faces,
      with_feats ? feats : nullptr, with_feats ? feat_strides[0] : 0, with_feats ? feat_strides[1] : 0, with_feats ? feat_strides[2] : 0,
      with_feats ? feat_strides[3] : 0, with_feats ? feat_strides[4] : 0, (int)K, face_feats);
  emit_verts_kernel<<<(unsigned)(N * s.bpm_v), kLanes, 0, st>>>(w.local, w.carry_v, (int)D, (int)H, (int)W, (int)s.L, (int)s.bpm_v, coords,
                                                                verts);
  return launch_status();
}
