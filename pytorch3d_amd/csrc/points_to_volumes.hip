// points_to_volumes.hip -- a batch of point clouds added to a batch of voxel grids (pytorch3d/ops/points_to_volumes.py over the
// contract of csrc/points_to_volumes/points_to_volumes_cpu.cpp and .cu).  include/p3d_amd.h has the contract; DESIGN.md 8.16.
//
// A point's location on an axis is (p + 1) * 0.5 * (grid - (align_corners ? 1 : 0)) - (align_corners ? 0 : 0.5): the sum p + 1 in
// float32, everything behind it in float64, as the reference's expression evaluates (0.5 is a double literal).
//   nearest    the voxel is that float64 location rounded half AWAY from zero (lround); one corner of weight 1.
//   trilinear  the location is rounded once to float32 and split by modf, which truncates TOWARD ZERO: x = trunc, rx = loc - x.
//              Corner (x + ux, y + uy, z + uz) gets (ux ? rx : 1 - rx) (uy ? ry : 1 - ry) (uz ? rz : 1 - rz), a float32 product
//              from the left.  For a location in (-1, 0) x is 0 and rx NEGATIVE: voxel 0 gets 1 - rx > 1 and voxel 1 gets rx < 0,
//              an extrapolation the reference's compiled operator has and its Python twin (floor) has not.  Kept: a drop-in.
// A corner outside [0, grid) on any axis is skipped; so is a point with mask == 0, and one whose location is not finite or does
// not fit an int64 (undefined behaviour in the reference).  A cloud's grid may be smaller than the tensor; one that is LARGER is
// cut at the tensor's extent (the reference would write out of bounds).
//
// Forward, atomic form: EIGHT LANES PER POINT for trilinear, lane bit 0 the x corner, so the two voxels of an x pair -- adjacent
// addresses for an x stride of 1 -- leave the wave from adjacent lanes; every lane then walks the 1 + C channels of its corner,
// which lie a whole volume apart.  Nearest: one lane per point.  No return value is used: global_atomic_add_f32 without return.
// Forward, ordered form (torch.use_deterministic_algorithms(True)): the samples are the (point, corner) pairs in the reference's
// corner order, the key of a sample is its voxel n * D*H*W + (z * H + y) * W + x or -1 (keys kernel); the caller sorts the samples
// stably by key and ordered_sum.h adds the rows (1 + C floats, in chunks of 4) of one voxel in a tree that only the positions
// in the sorted array decide.  A voxel's total is added to what the volume held, ONCE, by the one lane that ends up with it: no
// float atomic, the same bits on every run and stream.
// Backward: a gather, one lane per point, no atomics.  Channels go through registers four at a time; for each of them the eight
// corners are added in the reference's corner order, and the eight float64 `source` sums (the density gradient plus
// sum_c feature * feature gradient, channels ascending) fill up along the way, so every gradient voxel is read once.
#include "ordered_sum.h"

namespace p3d {
namespace {

constexpr float kTooLargeF = 9.0e18f;  // below 2^63: a location under it converts to int64 without overflow
constexpr double kTooLarge = 9.0e18;

struct Vol {
  float* p;
  int64_t sn, sc, sz, sy, sx;  // element strides of (N, C, D, H, W)
};

struct Cloud {
  const float* points;   // (N,P,3)
  const float* feats;    // (N,P,C)
  const int64_t* grid;   // (N,3): depth, height, width
  const float* mask;     // element (n, p) at n * mask_sn + p * mask_sp, or nullptr: every point counts
  int64_t mask_sn, mask_sp;
  int64_t N, P;
  int C;
  int64_t D, H, W;  // the tensors' extents
  float pw;
  int so;         // scale offset: align_corners ? 1 : 0
  float offset;   // align_corners ? 0 : 0.5
};

struct PointGrid {
  int64_t gx, gy, gz;  // the cloud's grid: the location arithmetic
  int64_t bx, by, bz;  // min(grid, tensor extent): the bounds
};

__device__ __forceinline__ bool masked_out(const Cloud& c, int64_t n, int64_t p) {
  return c.mask != nullptr && c.mask[n * c.mask_sn + p * c.mask_sp] == 0.0f;
}

__device__ __forceinline__ PointGrid point_grid(const Cloud& c, int64_t n) {
  PointGrid g;
  g.gz = c.grid[n * 3 + 0];
  g.gy = c.grid[n * 3 + 1];
  g.gx = c.grid[n * 3 + 2];
  g.bx = g.gx < c.W ? g.gx : c.W;
  g.by = g.gy < c.H ? g.gy : c.H;
  g.bz = g.gz < c.D ? g.gz : c.D;
  return g;
}

// the sum in float32, the rest in float64 (exact products: 24 bits x 1 bit x an integer)
__device__ __forceinline__ double location(const Cloud& c, float p, int64_t grid) {
  return (double)(p + 1.0f) * 0.5 * (double)(grid - c.so) - (double)c.offset;
}

// nearest: the voxel of point `pt`, or false (outside, not finite)
__device__ __forceinline__ bool nearest_voxel(const Cloud& c, const PointGrid& g, int64_t pt, int64_t& x, int64_t& y, int64_t& z) {
  const float* q = c.points + pt * 3;
  const double lx = location(c, q[0], g.gx), ly = location(c, q[1], g.gy), lz = location(c, q[2], g.gz);
  if (!(fabs(lx) < kTooLarge && fabs(ly) < kTooLarge && fabs(lz) < kTooLarge)) return false;  // NaN fails too
  x = (int64_t)round(lx);  // half away from zero, as lround
  y = (int64_t)round(ly);
  z = (int64_t)round(lz);
  return x >= 0 && y >= 0 && z >= 0 && x < g.bx && y < g.by && z < g.bz;
}

struct Splat {
  float x, y, z;     // the truncated location, still a float: the reference adds the corner bit in float32
  float rx, ry, rz;  // what modf leaves: the sign of the location
  bool ok;
};

__device__ __forceinline__ Splat splat_of(const Cloud& c, const PointGrid& g, int64_t pt) {
  const float* q = c.points + pt * 3;
  const float lx = (float)location(c, q[0], g.gx), ly = (float)location(c, q[1], g.gy), lz = (float)location(c, q[2], g.gz);
  Splat s;
  s.ok = fabsf(lx) < kTooLargeF && fabsf(ly) < kTooLargeF && fabsf(lz) < kTooLargeF;
  s.x = truncf(lx);
  s.y = truncf(ly);
  s.z = truncf(lz);
  s.rx = lx - s.x;
  s.ry = ly - s.y;
  s.rz = lz - s.z;
  return s;
}

// corner (ux, uy, uz) of a splat: its voxel and the three axis weights; false when it lies outside
__device__ __forceinline__ bool splat_corner(const Splat& s, const PointGrid& g, int ux, int uy, int uz, int64_t& x, int64_t& y,
                                             int64_t& z, float& wx, float& wy, float& wz) {
  x = (int64_t)(s.x + (float)ux);
  y = (int64_t)(s.y + (float)uy);
  z = (int64_t)(s.z + (float)uz);
  wx = ux ? s.rx : 1.0f - s.rx;
  wy = uy ? s.ry : 1.0f - s.ry;
  wz = uz ? s.rz : 1.0f - s.rz;
  return x >= 0 && y >= 0 && z >= 0 && x < g.bx && y < g.by && z < g.bz;
}

__device__ __forceinline__ int64_t voxel_offset(const Vol& v, int64_t n, int64_t x, int64_t y, int64_t z) {
  return n * v.sn + z * v.sz + y * v.sy + x * v.sx;
}

// ---- forward, atomic ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void add_corner(const Cloud& c, const Vol& dens, const Vol& feat, int64_t n, int64_t pt, int64_t x, int64_t y,
                                           int64_t z, float weight) {
  atomicAdd(dens.p + voxel_offset(dens, n, x, y, z), weight * c.pw);
  float* v = feat.p + voxel_offset(feat, n, x, y, z);
  const float* f = c.feats + pt * c.C;
  for (int ch = 0; ch < c.C; ++ch) atomicAdd(v + ch * feat.sc, f[ch] * weight * c.pw);
}

__global__ __launch_bounds__(256) void p2v_forward_splat_kernel(Cloud c, Vol dens, Vol feat) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t pt = i >> 3;
  if (pt >= c.N * c.P) return;
  const int j = (int)(i & 7);  // bit 0: x, bit 1: y, bit 2: z -- the x pair in adjacent lanes
  const int64_t n = pt / c.P;
  if (masked_out(c, n, pt - n * c.P)) return;
  const PointGrid g = point_grid(c, n);
  const Splat s = splat_of(c, g, pt);
  if (!s.ok) return;
  int64_t x, y, z;
  float wx, wy, wz;
  if (!splat_corner(s, g, j & 1, (j >> 1) & 1, j >> 2, x, y, z, wx, wy, wz)) return;
  add_corner(c, dens, feat, n, pt, x, y, z, wx * wy * wz);
}

__global__ __launch_bounds__(256) void p2v_forward_nearest_kernel(Cloud c, Vol dens, Vol feat) {
  const int64_t pt = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pt >= c.N * c.P) return;
  const int64_t n = pt / c.P;
  if (masked_out(c, n, pt - n * c.P)) return;
  const PointGrid g = point_grid(c, n);
  int64_t x, y, z;
  if (!nearest_voxel(c, g, pt, x, y, z)) return;
  add_corner(c, dens, feat, n, pt, x, y, z, 1.0f);
}

// ---- forward, ordered -----------------------------------------------------------------------------------------------------------
// sample s = point * corners + corner, corner in the reference's order: (ux, uy, uz) = (bit 2, bit 1, bit 0)
template <bool SPLAT>
__device__ __forceinline__ bool sample_voxel(const Cloud& c, int64_t s, int64_t& n, int64_t& pt, int64_t& x, int64_t& y, int64_t& z,
                                             float& weight) {
  pt = SPLAT ? s >> 3 : s;
  n = pt / c.P;
  if (masked_out(c, n, pt - n * c.P)) return false;
  const PointGrid g = point_grid(c, n);
  if (SPLAT) {
    const int j = (int)(s & 7);
    const Splat sp = splat_of(c, g, pt);
    float wx, wy, wz;
    if (!sp.ok || !splat_corner(sp, g, j >> 2, (j >> 1) & 1, j & 1, x, y, z, wx, wy, wz)) return false;
    weight = wx * wy * wz;
    return true;
  }
  weight = 1.0f;
  return nearest_voxel(c, g, pt, x, y, z);
}

template <bool SPLAT>
__global__ __launch_bounds__(256) void p2v_keys_kernel(Cloud c, int64_t nsamples, int* __restrict__ keys) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= nsamples) return;
  int64_t n, pt, x, y, z;
  float weight;
  keys[s] = sample_voxel<SPLAT>(c, s, n, pt, x, y, z, weight) ? (int)(((n * c.D + z) * c.H + y) * c.W + x) : ordered::kNone;
}

template <bool SPLAT>
struct VolumeOp {
  static constexpr int R = 4;
  Cloud c;
  Vol dens, feat;
  const int* keys;
  int64_t nsamples, nkeys;
  __device__ int64_t key(int64_t s) const { return keys[s]; }
  // channel 0 of a row is the density, channel 1 + k feature k
  __device__ void row(int64_t s, int, int chunk, float (&r)[R]) const {
    int64_t n, pt, x, y, z;
    float weight;
    if (!sample_voxel<SPLAT>(c, s, n, pt, x, y, z, weight)) return;  // (its key said otherwise)
    const float* f = c.feats + pt * c.C;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int ch = chunk * R + i;
      if (ch == 0) r[i] = weight * c.pw;
      else if (ch <= c.C) r[i] = f[ch - 1] * weight * c.pw;
    }
  }
  __device__ void store(int k, int chunk, const float (&r)[R]) const {
    int64_t v = k;
    const int64_t x = v % c.W;
    v /= c.W;
    const int64_t y = v % c.H;
    v /= c.H;
    const int64_t z = v % c.D, n = v / c.D;
    float* d = dens.p + voxel_offset(dens, n, x, y, z);
    float* q = feat.p + voxel_offset(feat, n, x, y, z);
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int ch = chunk * R + i;
      if (ch == 0) *d = *d + r[i];
      else if (ch <= c.C) q[(ch - 1) * feat.sc] = q[(ch - 1) * feat.sc] + r[i];
    }
  }
};

// ---- backward -------------------------------------------------------------------------------------------------------------------
template <bool SPLAT>
__global__ __launch_bounds__(256) void p2v_backward_kernel(Cloud c, Vol gdens, Vol gfeat, float* __restrict__ grad_points,
                                                           float* __restrict__ grad_feats) {
  constexpr int NC = SPLAT ? 8 : 1;
  constexpr int T = 4;  // channels in registers at a time
  const int64_t pt = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pt >= c.N * c.P) return;
  const int64_t n = pt / c.P;
  if (masked_out(c, n, pt - n * c.P)) return;
  const PointGrid g = point_grid(c, n);

  int64_t off[NC];    // the corner's voxel in the feature gradient
  float w[NC];        // its weight
  double src[NC];     // SPLAT: grad_density + sum_c feature * grad_feature at the corner
  float wx[2], wy[2], wz[2];
  unsigned inside = 0;
  if (SPLAT) {
    const Splat s = splat_of(c, g, pt);
    if (!s.ok) return;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int ux = j >> 2, uy = (j >> 1) & 1, uz = j & 1;  // the reference's corner order
      int64_t x, y, z;
      const bool in = splat_corner(s, g, ux, uy, uz, x, y, z, wx[ux], wy[uy], wz[uz]);
      w[j] = wx[ux] * wy[uy] * wz[uz];
      off[j] = in ? voxel_offset(gfeat, n, x, y, z) : 0;
      src[j] = in ? (double)gdens.p[voxel_offset(gdens, n, x, y, z)] : 0.0;
      inside |= (in ? 1u : 0u) << j;
    }
  } else {
    int64_t x, y, z;
    if (!nearest_voxel(c, g, pt, x, y, z)) return;
    off[0] = voxel_offset(gfeat, n, x, y, z);
    w[0] = 1.0f;
    inside = 1u;
  }
  if (inside == 0) return;

  const float* f = c.feats + pt * c.C;
  float* gf = grad_feats + pt * c.C;
  for (int c0 = 0; c0 < c.C; c0 += T) {
    float acc[T], fv[T];
#pragma unroll
    for (int i = 0; i < T; ++i) {
      const bool live = c0 + i < c.C;
      acc[i] = live ? gf[c0 + i] : 0.0f;
      fv[i] = (SPLAT && live) ? f[c0 + i] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      if (!((inside >> j) & 1u)) continue;
#pragma unroll
      for (int i = 0; i < T; ++i) {
        if (c0 + i >= c.C) continue;
        const float gv = gfeat.p[off[j] + (c0 + i) * gfeat.sc];
        acc[i] = acc[i] + gv * w[j] * c.pw;
        if (SPLAT) src[j] = src[j] + (double)(fv[i] * gv);
      }
    }
#pragma unroll
    for (int i = 0; i < T; ++i)
      if (c0 + i < c.C) gf[c0 + i] = acc[i];
  }

  if (SPLAT) {
    float* gp = grad_points + pt * 3;
    float gx = gp[0], gy = gp[1], gz = gp[2];
    const double sx = (double)(g.gx - c.so), sy = (double)(g.gy - c.so), sz = (double)(g.gz - c.so), pw = (double)c.pw;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      if (!((inside >> j) & 1u)) continue;
      const int ux = j >> 2, uy = (j >> 1) & 1, uz = j & 1;
      // float += double: the sum in float64, rounded to float32 once per corner
      gx = (float)((double)gx + src[j] * (ux ? 1.0 : -1.0) * (double)wy[uy] * (double)wz[uz] * 0.5 * sx * pw);
      gy = (float)((double)gy + src[j] * (uy ? 1.0 : -1.0) * (double)wx[ux] * (double)wz[uz] * 0.5 * sy * pw);
      gz = (float)((double)gz + src[j] * (uz ? 1.0 : -1.0) * (double)wx[ux] * (double)wy[uy] * 0.5 * sz * pw);
    }
    gp[0] = gx;
    gp[1] = gy;
    gp[2] = gz;
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
Vol make_vol(const float* p, const int64_t* strides) {
  return Vol{const_cast<float*>(p), strides[0], strides[1], strides[2], strides[3], strides[4]};
}

// the arguments every entry shares; P3D_OK with `empty` set: nothing to launch
int make_cloud(const float* points, const float* feats, const int64_t* grid_sizes, const float* mask, int64_t mask_stride_n,
               int64_t mask_stride_p, int64_t N, int64_t P, int64_t C, int64_t D, int64_t H, int64_t W, float point_weight,
               int align_corners, bool reads_feats, Cloud& c, bool& empty) {
  empty = true;
  if (N < 0 || P < 0 || C < 0 || D < 0 || H < 0 || W < 0 || C > 0x7fffffffll) return P3D_ERR_INVALID_ARG;
  if (N > 0 && P > 0 && (P > INT64_MAX / 64 / N || (C > 0 && N * P > INT64_MAX / 64 / C))) return P3D_ERR_INVALID_ARG;
  if (N == 0 || P == 0) return P3D_OK;
  if (!points || !grid_sizes || (C > 0 && reads_feats && !feats)) return P3D_ERR_INVALID_ARG;
  empty = D == 0 || H == 0 || W == 0;  // no voxel: every corner is outside
  c = Cloud{points, feats, grid_sizes, mask, mask_stride_n, mask_stride_p, N, P, (int)C, D, H, W, point_weight,
            align_corners ? 1 : 0, align_corners ? 0.0f : 0.5f};
  return P3D_OK;
}

bool grid_for(int64_t items, unsigned& blocks) {
  const int64_t b = ceil_div(items, 256);
  blocks = (unsigned)b;
  return b <= 0x7fffffffll;
}

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API size_t p3d_points_to_volumes_workspace_bytes(int64_t N, int64_t P, int64_t C, int splat) {
  if (N <= 0 || P <= 0 || C < 0) return 0;
  return ordered::partial_bytes(N * P * (splat ? 8 : 1), 4, (int)ceil_div(1 + C, 4));
}

P3D_API int p3d_points_to_volumes_keys(const float* points, const int64_t* grid_sizes, const float* mask, int64_t mask_stride_n,
                                       int64_t mask_stride_p, int64_t N, int64_t P, int64_t D, int64_t H, int64_t W, int align_corners,
                                       int splat, int32_t* keys, p3d_stream_t stream) {
  Cloud c;
  bool empty;
  const int rc = make_cloud(points, nullptr, grid_sizes, mask, mask_stride_n, mask_stride_p, N, P, 0, D, H, W, 1.0f, align_corners, false, c, empty);
  if (rc != P3D_OK) return rc;
  if (N == 0 || P == 0) return P3D_OK;
  if (!keys) return P3D_ERR_INVALID_ARG;
  if (!empty && N > (int64_t)INT32_MAX / D / H / W) return P3D_ERR_UNSUPPORTED;  // a key is an int32
  const int64_t S = N * P * (splat ? 8 : 1);
  unsigned blocks;
  if (!grid_for(S, blocks)) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("points_to_volumes_keys", s);
  if (splat) p2v_keys_kernel<true><<<blocks, 256, 0, s>>>(c, S, keys);
  else p2v_keys_kernel<false><<<blocks, 256, 0, s>>>(c, S, keys);
  return launch_status();
}

P3D_API int p3d_points_to_volumes_forward(const float* points, const float* feats, const int64_t* grid_sizes, const float* mask,
                                          int64_t mask_stride_n, int64_t mask_stride_p, int64_t N, int64_t P, int64_t C, int64_t D,
                                          int64_t H, int64_t W, float* densities, const int64_t* densities_strides, float* features,
                                          const int64_t* features_strides, float point_weight, int align_corners, int splat,
                                          const int32_t* keys, const int64_t* sorted_samples, void* workspace, size_t workspace_bytes,
                                          p3d_stream_t stream) {
  Cloud c;
  bool empty;
  const int rc = make_cloud(points, feats, grid_sizes, mask, mask_stride_n, mask_stride_p, N, P, C, D, H, W, point_weight, align_corners, true,
                            c, empty);
  if (rc != P3D_OK) return rc;
  if ((keys == nullptr) != (sorted_samples == nullptr)) return P3D_ERR_INVALID_ARG;
  if (N == 0 || P == 0 || empty) return P3D_OK;
  if (!densities || !densities_strides || (C > 0 && (!features || !features_strides))) return P3D_ERR_INVALID_ARG;
  static const int64_t no_strides[5] = {0, 0, 0, 0, 0};
  const Vol dens = make_vol(densities, densities_strides), feat = make_vol(features, C > 0 ? features_strides : no_strides);
  hipStream_t s = (hipStream_t)stream;
  if (sorted_samples) {
    if (N > (int64_t)INT32_MAX / D / H / W) return P3D_ERR_UNSUPPORTED;
    const int64_t S = N * P * (splat ? 8 : 1);
    const int chunks = (int)ceil_div(1 + C, 4);
    if (!workspace || workspace_bytes < p3d_points_to_volumes_workspace_bytes(N, P, C, splat)) return P3D_ERR_WORKSPACE;
    if (splat) return ordered::run(VolumeOp<true>{c, dens, feat, keys, S, N * D * H * W}, sorted_samples, S, chunks, workspace, s,
                                   "points_to_volumes_ordered");
    return ordered::run(VolumeOp<false>{c, dens, feat, keys, S, N * D * H * W}, sorted_samples, S, chunks, workspace, s,
                        "points_to_volumes_ordered");
  }
  unsigned blocks;
  if (!grid_for(N * P * (splat ? 8 : 1), blocks)) return P3D_ERR_INVALID_ARG;
  LaunchScope ls("points_to_volumes_forward", s);
  if (splat) p2v_forward_splat_kernel<<<blocks, 256, 0, s>>>(c, dens, feat);
  else p2v_forward_nearest_kernel<<<blocks, 256, 0, s>>>(c, dens, feat);
  return launch_status();
}

P3D_API int p3d_points_to_volumes_backward(const float* points, const float* feats, const int64_t* grid_sizes, const float* mask,
                                           int64_t mask_stride_n, int64_t mask_stride_p, int64_t N, int64_t P, int64_t C, int64_t D,
                                           int64_t H, int64_t W, const float* grad_densities, const int64_t* grad_densities_strides,
                                           const float* grad_features, const int64_t* grad_features_strides, float point_weight,
                                           int align_corners, int splat, float* grad_points, float* grad_feats, p3d_stream_t stream) {
  Cloud c;
  bool empty;
  const int rc = make_cloud(points, feats, grid_sizes, mask, mask_stride_n, mask_stride_p, N, P, C, D, H, W, point_weight, align_corners,
                            splat != 0, c, empty);
  if (rc != P3D_OK) return rc;
  if (N == 0 || P == 0 || empty) return P3D_OK;
  if ((splat && (!grad_points || !grad_densities || !grad_densities_strides)) ||
      (C > 0 && (!grad_feats || !grad_features || !grad_features_strides)))
    return P3D_ERR_INVALID_ARG;
  static const int64_t no_strides[5] = {0, 0, 0, 0, 0};
  const Vol gdens = make_vol(grad_densities, splat ? grad_densities_strides : no_strides);
  const Vol gfeat = make_vol(grad_features, C > 0 ? grad_features_strides : no_strides);
  unsigned blocks;
  if (!grid_for(N * P, blocks)) return P3D_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("points_to_volumes_backward", s);
  if (splat) p2v_backward_kernel<true><<<blocks, 256, 0, s>>>(c, gdens, gfeat, grad_points, grad_feats);
  else p2v_backward_kernel<false><<<blocks, 256, 0, s>>>(c, gdens, gfeat, grad_points, grad_feats);
  return launch_status();
}
