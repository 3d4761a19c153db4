// marching_cubes.hip -- scalar fields to isosurface meshes (the reference's csrc/marching_cubes: three kernels, two host reads, a table
// upload per volume and a torch.unique over 3 F keys behind them).  Contract: implicit_abi.h (p3di_marching_cubes_*).
// Count -> scan -> fill on cubify.hip's skeleton (scan_blocks.h), with one idea that removes the sort: a mesh vertex belongs to a lattice
// EDGE, the edge to its low lattice point, and (lattice point, axis) order is the order of the reference's sorted edge ids.  So the
// vertices are counted and ranked per lattice point without the table -- an edge carries a vertex iff its ends differ in the inside
// test --, each is computed and written once, and a face entry (cube, edge) finds its vertex as the rank stored at the owning point.
//
// Work is cut into SCAN BLOCKS of P3D_MARCHING_CUBES_ITEMS consecutive lattice points of ONE volume, P3D_MARCHING_CUBES_BLOCK lanes
// going over them in rounds; a lattice point is also the low corner of at most one cube, so the one item space serves vertices and
// faces.  Volume n owns the blocks [n bpm, (n + 1) bpm): per-volume totals and the per-volume restart of the ranks are differences of
// block carries.
//
//   count   classify_kernel    a lane per lattice point: the inside test of the up to 8 corners above it (strided reads) -> its three
//                              edge flags and, where it is a cube's low corner, the configuration byte.  The vertex counts (0..3)
//                              are scanned by two ballots within a wave and the wave sums in LDS; the word (rank inside the block,
//                              flags, configuration) is stored.  The block's vertex and triangle totals go to the two carry tables.
//           carry_kernel       scan_blocks.h: both tables to exclusive scans, and (V_n, F_n).
//   emit    emit_verts_kernel  a lane per lattice point: up to three vertices by marching_cubes_geom.h at carry[block] + rank, with
//                              the int64 edge id.
//           emit_faces_kernel  a lane per lattice point: the triangle counts are scanned again (three ballots); an entry (axis, corner)
//                              reads the word of the owning point: its rank + the carries + the flags below `axis`.  The 4 KB triangle
//                              table and the 256 counts are staged in LDS once per workgroup: the lanes index them by configuration,
//                              64 different addresses a wave.
// Blocks whose carry does not move leave at once.  The host reads the (N, 2) counts between the two entries: the one sync of a call.
#include "implicit_abi.h"
#include "p3d_common.h"
#include "scan_blocks.h"
// (behind p3d_common.h: the two headers spell __host__ __device__ where the HIP runtime header has been seen)
#include "marching_cubes_geom.h"
#include "marching_cubes_tables.h"

namespace p3d {
namespace {

constexpr int kLanes = P3D_MARCHING_CUBES_BLOCK;
constexpr int kItems = P3D_MARCHING_CUBES_ITEMS;
constexpr int kCarryLanes = P3D_MARCHING_CUBES_CARRY_BLOCK;
constexpr int kWaves = kLanes / kWave;
// the word of a lattice point: configuration byte | edge flags << 8 | rank of its first vertex inside its scan block << 11
constexpr int kFlagShift = 8, kRankShift = 11;
static_assert(kLanes == 256 && kItems % kLanes == 0 && kCarryLanes % kWave == 0 && kCarryLanes <= 1024 && 3 * kItems < (1 << (31 - kRankShift)),
              "launch constants");

struct Sizes {
  int64_t L;    // lattice points of one volume
  int64_t bpm;  // scan blocks of one volume
};

// false: a size the kernels' int32 indices do not cover (the Python layer takes its torch formulation there)
bool sizes_of(int64_t N, int64_t D, int64_t H, int64_t W, Sizes* s) {
  if (N < 0 || D < 1 || H < 1 || W < 1 || D >= INT32_MAX || H >= INT32_MAX || W >= INT32_MAX) return false;
  int64_t L = D * H;
  if (L > INT32_MAX) return false;
  L *= W;
  if (L > INT32_MAX / 15 || (N > 0 && L > INT32_MAX / 15 / N)) return false;  // 3 L vertices, 5 L triangles of 3 entries
  s->L = L;
  s->bpm = ceil_div(L, kItems);
  return true;
}

struct Workspace {
  unsigned* words;  // N * L
  int* carry_v;     // N * bpm + 1
  int* carry_f;     // N * bpm + 1
  size_t bytes;
};

Workspace carve(void* workspace, int64_t N, const Sizes& s) {
  Arena a(workspace, ~(size_t)0);
  Workspace w;
  w.words = a.take<unsigned>((size_t)(N * s.L));
  w.carry_v = a.take<int>((size_t)(N * s.bpm + 1));
  w.carry_f = a.take<int>((size_t)(N * s.bpm + 1));
  w.bytes = a.off;
  return w;
}

struct Grid {
  const float* vol;
  int64_t sn, sd, sh, sw;
  int D, H, W, L, bpm;
};

// grid: N * bpm blocks
__global__ __launch_bounds__(kLanes) void classify_kernel(Grid q, const float* __restrict__ isolevels, unsigned* __restrict__ words,
                                                          int* __restrict__ sums_v, int* __restrict__ sums_f) {
  __shared__ int wsum[kWaves];
  __shared__ uint8_t counts[256];
  counts[threadIdx.x] = mc_triangle_count((int)threadIdx.x);
  __syncthreads();
  const int n = (int)blockIdx.x / q.bpm, j = (int)blockIdx.x % q.bpm;
  const float* grid = q.vol + (int64_t)n * q.sn;
  const float iso = isolevels[n];
  int running = 0, triangles = 0;
  for (int r = 0; r < kItems / kLanes; ++r) {  // every lane stays for the barriers of block_exclusive
    const int g = j * kItems + r * kLanes + (int)threadIdx.x;
    unsigned flags = 0, config = 0;
    if (g < q.L) {
      const int x = g % q.W, t = g / q.W, y = t % q.H, z = t / q.H;
      const bool mx = x + 1 < q.W, my = y + 1 < q.H, mz = z + 1 < q.D;
      const float* p = grid + z * q.sd + y * q.sh + x * q.sw;
      unsigned in = 0;  // bit i: corner i exists and is inside
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const bool there = (!(i & 1) || mx) && (!(i & 2) || my) && (!(i & 4) || mz);
        if (there && mc_inside(p[(i & 1) * q.sw + (i >> 1 & 1) * q.sh + (i >> 2 & 1) * q.sd], iso)) in |= 1u << i;
      }
      const unsigned low = in & 1u;
      flags = (mx && (in >> 1 & 1u) != low ? 1u : 0u) | (my && (in >> 2 & 1u) != low ? 2u : 0u) | (mz && (in >> 4 & 1u) != low ? 4u : 0u);
      config = mx && my && mz ? in : 0u;
    }
    const int nv = __popc(flags);
    const unsigned long long b0 = __ballot(nv & 1), b1 = __ballot(nv & 2);
    int total;
    const int rank = running + block_exclusive<kWaves>(mask_rank(b0) + 2 * mask_rank(b1), __popcll(b0) + 2 * __popcll(b1), wsum, &total);
    if (g < q.L) words[(int64_t)n * q.L + g] = config | flags << kFlagShift | (unsigned)rank << kRankShift;
    running += total;
    triangles += counts[config];
  }
  const int incl = wave_inclusive(triangles);
  int total;
  block_exclusive<kWaves>(0, __shfl(incl, kWave - 1), wsum, &total);
  if (threadIdx.x == 0) {
    sums_v[blockIdx.x] = running;
    sums_f[blockIdx.x] = total;
  }
}

// grid: N * bpm blocks
__global__ __launch_bounds__(kLanes) void emit_verts_kernel(Grid q, const float* __restrict__ isolevels, const unsigned* __restrict__ words,
                                                            const int* __restrict__ carry_v, int local, float* __restrict__ verts,
                                                            int64_t* __restrict__ ids) {
  const int base = carry_v[blockIdx.x];
  if (carry_v[blockIdx.x + 1] == base) return;
  const int n = (int)blockIdx.x / q.bpm, j = (int)blockIdx.x % q.bpm;
  const float* grid = q.vol + (int64_t)n * q.sn;
  const float iso = isolevels[n];
  const int64_t id_scale = (int64_t)q.W + (int64_t)q.W * q.H + (int64_t)q.L;
  for (int r = 0; r < kItems / kLanes; ++r) {
    const int g = j * kItems + r * kLanes + (int)threadIdx.x;
    if (g >= q.L) break;
    const unsigned word = words[(int64_t)n * q.L + g], flags = word >> kFlagShift & 7u;
    if (!flags) continue;
    const int x = g % q.W, t = g / q.W, y = t % q.H, z = t / q.H;
    const float* p = grid + z * q.sd + y * q.sh + x * q.sw;
    const float v1 = *p;
    int64_t row = base + (int)(word >> kRankShift);
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
      if (!(flags >> axis & 1u)) continue;
      float out[3];
      mc_edge_vertex(iso, v1, p[axis == 0 ? q.sw : axis == 1 ? q.sh : q.sd], x, y, z, axis, out);
      if (local) {
        out[0] = mc_local(out[0], q.W);
        out[1] = mc_local(out[1], q.H);
        out[2] = mc_local(out[2], q.D);
      }
      float* o = verts + row * 3;
      o[0] = out[0];
      o[1] = out[1];
      o[2] = out[2];
      ids[row] = (int64_t)g * id_scale + g + (axis == 0 ? 1 : axis == 1 ? q.W : q.W * q.H);
      ++row;
    }
  }
}

// grid: N * bpm blocks
__global__ __launch_bounds__(kLanes) void emit_faces_kernel(Grid q, const unsigned* __restrict__ words, const int* __restrict__ carry_v,
                                                            const int* __restrict__ carry_f, int64_t* __restrict__ faces) {
  __shared__ int wsum[kWaves];
  __shared__ uint8_t counts[256];
  __shared__ uint8_t table[256][16];
  int running = carry_f[blockIdx.x];
  if (carry_f[blockIdx.x + 1] == running) return;  // the whole workgroup: no cube of this block emits
  counts[threadIdx.x] = mc_triangle_count((int)threadIdx.x);
#pragma unroll
  for (int k = 0; k < 16; ++k) table[threadIdx.x][k] = mc_table_entry((int)threadIdx.x, k);
  __syncthreads();
  const int n = (int)blockIdx.x / q.bpm, j = (int)blockIdx.x % q.bpm;
  const int* vcarry = carry_v + (int64_t)n * q.bpm;
  const unsigned* vwords = words + (int64_t)n * q.L;
  const int first = vcarry[0];
  for (int r = 0; r < kItems / kLanes; ++r) {
    const int g = j * kItems + r * kLanes + (int)threadIdx.x;
    const unsigned config = g < q.L ? vwords[g] & 255u : 0u;
    const int cnt = counts[config];  // 0..5
    const unsigned long long b0 = __ballot(cnt & 1), b1 = __ballot(cnt & 2), b2 = __ballot(cnt & 4);
    int total;
    int64_t entry = 3 * (int64_t)(running + block_exclusive<kWaves>(mask_rank(b0) + 2 * mask_rank(b1) + 4 * mask_rank(b2),
                                                                    __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2), wsum, &total));
    running += total;
    for (int k = 0; k < 3 * cnt; ++k) {
      const unsigned e = table[config][k], axis = e >> 3;
      const int owner = g + (int)(e & 1u) + (e & 2u ? q.W : 0) + (e & 4u ? q.W * q.H : 0);
      const unsigned word = vwords[owner];
      faces[entry + k] = (int64_t)((int)(word >> kRankShift) + vcarry[owner / kItems] - first + __popc(word >> kFlagShift & ((1u << axis) - 1u)));
    }
  }
}

Grid grid_of(const float* vol, const int64_t strides[4], int64_t D, int64_t H, int64_t W, const Sizes& s) {
  return Grid{vol, strides[0], strides[1], strides[2], strides[3], (int)D, (int)H, (int)W, (int)s.L, (int)s.bpm};
}

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API size_t p3di_marching_cubes_workspace_bytes(int64_t N, int64_t D, int64_t H, int64_t W) {
  Sizes s;
  return sizes_of(N, D, H, W, &s) ? carve(nullptr, N, s).bytes : 0;
}

P3D_API int p3di_marching_cubes_count(const float* vol, const int64_t vol_strides[4], int64_t N, int64_t D, int64_t H, int64_t W,
                                      const float* isolevels, void* workspace, size_t workspace_bytes, int64_t* counts,
                                      p3d_stream_t stream) {
  Sizes s;
  if (!sizes_of(N, D, H, W, &s) || !vol_strides) return P3D_ERR_INVALID_ARG;
  if (N == 0) return P3D_OK;
  if (!vol || !isolevels || !counts) return P3D_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (D == 1 || H == 1 || W == 1)  // no cube: no face, and the reference returns nothing then
    return hipMemsetAsync(counts, 0, (size_t)N * 2 * sizeof(int64_t), st) == hipSuccess ? P3D_OK : P3D_ERR_LAUNCH;
  if (!workspace || workspace_bytes < carve(nullptr, N, s).bytes) return P3D_ERR_WORKSPACE;
  const Workspace w = carve(workspace, N, s);
  const int blocks = (int)(N * s.bpm);
  LaunchScope ls("marching_cubes_count", st);
  classify_kernel<<<(unsigned)blocks, kLanes, 0, st>>>(grid_of(vol, vol_strides, D, H, W, s), isolevels, w.words, w.carry_v, w.carry_f);
  carry_kernel<kCarryLanes><<<2, kCarryLanes, 0, st>>>(w.carry_f, blocks, (int)s.bpm, w.carry_v, blocks, (int)s.bpm, (int)N, counts);
  return launch_status();
}

P3D_API int p3di_marching_cubes_emit(const float* vol, const int64_t vol_strides[4], int64_t N, int64_t D, int64_t H, int64_t W,
                                     const float* isolevels, int64_t local, int64_t total_verts, int64_t total_faces,
                                     const void* workspace, size_t workspace_bytes, float* verts, int64_t* ids, int64_t* faces,
                                     p3d_stream_t stream) {
  Sizes s;
  if (!sizes_of(N, D, H, W, &s) || !vol_strides || total_verts < 0 || total_faces < 0 || total_verts > 3 * N * s.L ||
      total_faces > 5 * N * s.L)
    return P3D_ERR_INVALID_ARG;
  if (total_faces == 0) return P3D_OK;  // no face, so nothing is returned for any volume
  if (D == 1 || H == 1 || W == 1 || !vol || !isolevels || !verts || !ids || !faces || total_verts == 0) return P3D_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < carve(nullptr, N, s).bytes) return P3D_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const Workspace w = carve(const_cast<void*>(workspace), N, s);
  const Grid q = grid_of(vol, vol_strides, D, H, W, s);
  const unsigned blocks = (unsigned)(N * s.bpm);
  LaunchScope ls("marching_cubes_emit", st);
  emit_verts_kernel<<<blocks, kLanes, 0, st>>>(q, isolevels, w.words, w.carry_v, local != 0, verts, ids);
  emit_faces_kernel<<<blocks, kLanes, 0, st>>>(q, w.words, w.carry_v, w.carry_f, faces);
  return launch_status();
}

P3D_API int p3di_marching_cubes_host(const float* vol, const int64_t vol_strides[3], int64_t D, int64_t H, int64_t W, float isolevel,
                                     int64_t* edge_rank, float* verts, int64_t cap_verts, int64_t* faces, int64_t cap_faces,
                                     int64_t* counts) {
  if (D < 1 || H < 1 || W < 1 || !vol_strides || !counts || cap_verts < 0 || cap_faces < 0 || (cap_verts && !verts) || (cap_faces && !faces))
    return P3D_ERR_INVALID_ARG;
  counts[0] = counts[1] = 0;
  if (D == 1 || H == 1 || W == 1) return P3D_OK;
  if (!vol || !edge_rank) return P3D_ERR_INVALID_ARG;
  const int64_t sd = vol_strides[0], sh = vol_strides[1], sw = vol_strides[2];
  int64_t n_verts = 0, n_faces = 0;
  for (int64_t z = 0; z + 1 < D; ++z)
    for (int64_t y = 0; y + 1 < H; ++y)
      for (int64_t x = 0; x + 1 < W; ++x) {
        const float* p = vol + z * sd + y * sh + x * sw;
        int config = 0;
        for (int i = 0; i < 8; ++i)
          if (mc_inside(p[(i & 1) * sw + (i >> 1 & 1) * sh + (i >> 2 & 1) * sd], isolevel)) config |= 1 << i;
        const int cnt = mc_triangle_count(config);
        for (int t = 0; t < cnt; ++t) {
          float ps[3][3];
          int64_t edge[3];
          for (int k = 0; k < 3; ++k) {
            const int e = mc_table_entry(config, 3 * t + k), axis = e >> 3;
            const int64_t px = x + (e & 1), py = y + (e >> 1 & 1), pz = z + (e >> 2 & 1);
            const float* p1 = vol + pz * sd + py * sh + px * sw;
            mc_edge_vertex(isolevel, *p1, p1[axis == 0 ? sw : axis == 1 ? sh : sd], (int)px, (int)py, (int)pz, axis, ps[k]);
            edge[k] = 3 * ((pz * H + py) * W + px) + axis;
          }
          // the reference keeps the rejected triangle in front of its test: every later triangle of this cube fails with it
          if (!(mc_differ(ps[0], ps[1]) && mc_differ(ps[1], ps[2]) && mc_differ(ps[2], ps[0]))) break;
          for (int k = 0; k < 3; ++k) {
            if (edge_rank[edge[k]] < 0) {
              edge_rank[edge[k]] = n_verts;
              if (n_verts < cap_verts) verts[3 * n_verts] = ps[k][0], verts[3 * n_verts + 1] = ps[k][1], verts[3 * n_verts + 2] = ps[k][2];
              ++n_verts;
            }
            if (n_faces < cap_faces) faces[3 * n_faces + k] = edge_rank[edge[k]];
          }
          ++n_faces;
        }
      }
  counts[0] = n_verts;
  counts[1] = n_faces;
  return P3D_OK;
}
