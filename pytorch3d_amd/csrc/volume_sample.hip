// volume_sample.hip -- voxel grids sampled at the points of rays: steps 2 and 3 of the reference's VolumeSampler.forward
// (pytorch3d/renderer/implicit/renderer.py: ray_bundle_variables_to_ray_points, two F.grid_sample calls on 5-D inputs, permute and
// view), forward and backward.  Contract: implicit_abi.h; DESIGN.md 8.23.
//
// The point of sample k of a ray is o + l_k * d, one float32 multiply and one add (no FMA); it lives in registers only.  The sampling
// is ATen's grid_sampler_3d restated in float32 (x indexes W, y indexes H, z indexes D): the source index of uvm_sample.h /
// vert_align.hip per axis, the corners tnw tne tsw tse bnw bne bsw bse = (x0 + kx, y0 + ky, z0 + kz) for k = kx + 2 ky + 4 kz with the
// weights (wx wy) wz, the in-range ones summed in that order from +0; nearest rounds half to even.  Under zeros padding a source
// coordinate that is not finite or does not fit an int32 makes the whole sample empty, as in vert_align.hip.
//
// Forward: one lane per point, consecutive lanes consecutive points of a ray; corners and weights once per point, then the Cd + Cf
// channels of both grids, each through its own five strides.
// Backward: lanes run ALONG the ray, TWO lanes per point: lane bit 0 is the x corner, so the two voxels of an x pair -- adjacent
// addresses at an x stride of 1 -- leave the wave from adjacent lanes, as in points_to_volumes.hip; each lane walks the four (y, z)
// corners of its x side.  The volume gradients are float atomics without return value.  The coordinate gradient g_k of a point is
// the pair's two halves added, times d index / d coordinate; grad_lengths_k = g_k . d is written per point, grad_origins = sum_k g_k
// and grad_directions = sum_k l_k g_k are xor butterflies over the ray's segment of lanes (a ray of P <= 32 points owns
// 2 next_pow2(P) lanes, a longer one the whole wave and goes through chunks of 32 points, each chunk's sum added to a carry in chunk
// order): no atomic, the same bits on every run.  Without ray gradients the kernel is compiled without any read of the volumes.
// Ordered form: sample 8 pt + k has the key of its voxel (no batch index for a shared grid) or -1; the caller sorts the samples that
// have a voxel stably by it and ordered_sum.h adds the rows (Cd + Cf channels in chunks of 4).  (The samples without a voxel -- half
// of a ray that crosses the grid and goes on -- stay out of the sorted list: as one run of keys -1 in front of it they were one
// segment that a single lane of pass 2 walked, 186 ms at 24.6 million points.)
#include "implicit_abi.h"
#include "ordered_sum.h"

namespace p3d {
namespace {

constexpr float kTooLargeF = 2.0e9f;  // below 2^31: a source coordinate under it (and its + 1) converts to int32 without overflow
constexpr int kGroup = 256;
constexpr int kPointsPerWave = P3D_VOLUME_SAMPLE_CHUNK;  // backward: two lanes per point
static_assert(kPointsPerWave * 2 == kWave, "two lanes per point");

struct Grid {
  const float* p;
  int64_t sn, sc, sz, sy, sx;  // element strides of (N, C, D, H, W); sn == 0: one grid for every ray batch
};

struct GradGrid {
  float* p;
  int64_t sn, sc, sz, sy, sx;
};

struct Rays {
  const float* o;  // (N, R, 3)
  const float* d;  // (N, R, 3)
  const float* l;  // (N, R, P), or nullptr: P == 1 and the point is the origin
  int64_t N, R, P;
};

struct Dims {
  int D, H, W;
  int Cd, Cf;
  unsigned flags;
};

struct Axis {
  int i0;        // floor (bilinear) or the rounded index (nearest); -2 for an empty sample
  float w0, w1;  // weights of i0 and i0 + 1
  float mult;    // d index / d coordinate; 0 where border clipped, for nearest and for an empty sample
  bool ok;
};

__device__ __forceinline__ Axis axis_of(float c, int S, unsigned flags) {
  const float size = (float)S;
  float i, mult;
  if (flags & P3D_VOLUME_SAMPLE_CORNERS) {
    i = ((c + 1.0f) / 2.0f) * (size - 1.0f);
    mult = (size - 1.0f) / 2.0f;
  } else {
    i = ((c + 1.0f) * size - 1.0f) / 2.0f;
    mult = size / 2.0f;
  }
  Axis a;
  a.ok = true;
  if (flags & P3D_VOLUME_SAMPLE_BORDER) {
    if (!(i > 0.0f)) i = 0.0f, mult = 0.0f;  // NaN too
    else if (i >= size - 1.0f) i = size - 1.0f, mult = 0.0f;
  } else {
    a.ok = fabsf(i) < kTooLargeF;  // NaN fails
  }
  if (!a.ok) {
    a.i0 = -2, a.w0 = a.w1 = a.mult = 0.0f;
  } else if (flags & P3D_VOLUME_SAMPLE_NEAREST) {
    a.i0 = (int)rintf(i);  // half to even
    a.w0 = 1.0f, a.w1 = 0.0f, a.mult = 0.0f;
  } else {
    const float f = floorf(i);
    a.i0 = (int)f;
    a.w1 = i - f;
    a.w0 = (f + 1.0f) - i;
    a.mult = mult;
  }
  return a;
}

struct Sample {
  Axis x, y, z;
  bool ok;  // false: empty (every corner out of range)
};

__device__ __forceinline__ Sample sample_of(float px, float py, float pz, const Dims& dm) {
  Sample s;
  s.x = axis_of(px, dm.W, dm.flags);
  s.y = axis_of(py, dm.H, dm.flags);
  s.z = axis_of(pz, dm.D, dm.flags);
  s.ok = s.x.ok && s.y.ok && s.z.ok;
  if (!s.ok) s.x.i0 = s.y.i0 = s.z.i0 = -2, s.x.mult = s.y.mult = s.z.mult = 0.0f;
  return s;
}

// corner (kx, ky, kz): its voxel, whether it lies in the grid, and its weight
__device__ __forceinline__ bool corner_of(const Sample& s, const Dims& dm, int kx, int ky, int kz, int& x, int& y, int& z, float& w) {
  x = s.x.i0 + kx, y = s.y.i0 + ky, z = s.z.i0 + kz;
  w = ((kx ? s.x.w1 : s.x.w0) * (ky ? s.y.w1 : s.y.w0)) * (kz ? s.z.w1 : s.z.w0);
  return x >= 0 && y >= 0 && z >= 0 && x < dm.W && y < dm.H && z < dm.D;
}

__device__ __forceinline__ int corners_of(const Dims& dm) { return (dm.flags & P3D_VOLUME_SAMPLE_NEAREST) ? 1 : 8; }

// point pt = (n, r, k) flattened: its ray and its batch element.  small: N R P fits an unsigned, and the two divisions are 32-bit ones
// (a 64-bit division is a long instruction sequence, paid per point)
__device__ __forceinline__ void ray_of(const Rays& ry, int64_t pt, bool small, int64_t& ray, int64_t& n) {
  if (small) {
    const unsigned r = (unsigned)pt / (unsigned)ry.P;
    ray = r;
    n = r / (unsigned)ry.R;
  } else {
    ray = pt / ry.P;
    n = ray / ry.R;
  }
}

// the coordinates of point pt of ray `ray`
__device__ __forceinline__ void point_of(const Rays& ry, int64_t ray, int64_t pt, float& px, float& py, float& pz) {
  const float* o = ry.o + ray * 3;
  if (ry.l == nullptr) {
    px = o[0], py = o[1], pz = o[2];
    return;
  }
  const float* d = ry.d + ray * 3;
  const float t = ry.l[pt];
  px = o[0] + t * d[0];
  py = o[1] + t * d[1];
  pz = o[2] + t * d[2];
}

// ---- forward --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sample_grid(const Grid& g, int64_t n, int C, const Sample& s, const Dims& dm, float* __restrict__ out) {
  int64_t off[8];
  float w[8];
  unsigned mask = 0;
  const int nc = corners_of(dm);
  const int64_t base = s.z.i0 * g.sz + s.y.i0 * g.sy + s.x.i0 * g.sx;  // (of corner 0; only in-range corners are read)
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    int x, y, z;
    off[k] = 0, w[k] = 0.0f;
    if (k < nc && corner_of(s, dm, k & 1, (k >> 1) & 1, k >> 2, x, y, z, w[k])) {
      mask |= 1u << k;
      off[k] = base + ((k & 1) ? g.sx : 0) + ((k & 2) ? g.sy : 0) + ((k & 4) ? g.sz : 0);
    }
  }
  const float* src = g.p + n * g.sn;
  for (int c = 0; c < C; ++c) {
    const float* q = src + c * g.sc;
    float v[8], acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = k < nc ? q[off[k]] : 0.0f;  // (unconditional: the loads leave together; offset 0 where out of range)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc = (mask >> k & 1u) ? acc + v[k] * w[k] : acc;
    out[c] = acc;
  }
}

// grid-stride over the N R P points
__global__ __launch_bounds__(kGroup) void volume_sample_fwd_kernel(Rays ry, Grid gd, Grid gf, Dims dm, float* __restrict__ out_d,
                                                                   float* __restrict__ out_f, int64_t total) {
  const bool small = total <= 0xffffffffll;
  for (int64_t pt = (int64_t)blockIdx.x * kGroup + threadIdx.x; pt < total; pt += (int64_t)gridDim.x * kGroup) {
    int64_t ray, n;
    float px, py, pz;
    ray_of(ry, pt, small, ray, n);
    point_of(ry, ray, pt, px, py, pz);
    const Sample s = sample_of(px, py, pz, dm);
    sample_grid(gd, n, dm.Cd, s, dm, out_d + pt * dm.Cd);
    if (dm.Cf > 0) sample_grid(gf, n, dm.Cf, s, dm, out_f + pt * dm.Cf);
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
int segment_points(int64_t P) {
  int g = 1;
  while (g < kPointsPerWave && g < P) g <<= 1;
  return g;
}

// the four (y, z) corners of this lane's x side over the C channels of one grid: the atomics (VOL) and the three sums of
// value x d weight / d index x grad (RAY)
template <bool VOL, bool RAY>
__device__ __forceinline__ void grid_backward(const Grid& g, const GradGrid& gg, int64_t n, int C, const Sample& s, const Dims& dm, int kx,
                                              const float* __restrict__ go, float& gix, float& giy, float& giz) {
  if (go == nullptr || C == 0) return;
  const int nc = corners_of(dm);
  if (kx >= nc) return;  // nearest: the x side 1 has no corner
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ky = j & 1, kz = j >> 1;
    if (kx + 2 * ky + 4 * kz >= nc) continue;
    int x, y, z;
    float w;
    if (!corner_of(s, dm, kx, ky, kz, x, y, z, w)) continue;
    const float wx = kx ? s.x.w1 : s.x.w0, wy = ky ? s.y.w1 : s.y.w0, wz = kz ? s.z.w1 : s.z.w0;
    const float dx = (kx ? wy : -wy) * wz, dy = (ky ? wx : -wx) * wz, dz = (kz ? wx : -wx) * wy;
    for (int c = 0; c < C; ++c) {
      const float gc = go[c];
      if (VOL && gg.p != nullptr) atomicAdd(gg.p + n * gg.sn + c * gg.sc + z * gg.sz + y * gg.sy + x * gg.sx, w * gc);
      if (RAY) {
        const float val = g.p[n * g.sn + c * g.sc + z * g.sz + y * g.sy + x * g.sx];
        gix += val * dx * gc;
        giy += val * dy * gc;
        giz += val * dz * gc;
      }
    }
  }
}

// a wave takes 32 / G rays (G = segment_points(P)) per round and walks their chunks of G points; grid-stride over the rounds
template <bool VOL, bool RAY>
__global__ __launch_bounds__(kGroup) void volume_sample_bwd_kernel(Rays ry, Grid gd, Grid gf, Dims dm, const float* __restrict__ go_d,
                                                                   const float* __restrict__ go_f, GradGrid ggd, GradGrid ggf,
                                                                   float* __restrict__ grad_o, float* __restrict__ grad_dir,
                                                                   float* __restrict__ grad_l, int G, int64_t rounds) {
  const int lane = (int)(threadIdx.x & 63);
  const int kx = lane & 1;
  const int seg = lane / (2 * G), kseg = (lane % (2 * G)) >> 1;
  const int rays_per_wave = kPointsPerWave / G;
  const int64_t n_rays = ry.N * ry.R;
  const int64_t chunks = (ry.P + G - 1) / G;
  for (int64_t u = (int64_t)blockIdx.x * (kGroup / kWave) + (threadIdx.x >> 6); u < rounds; u += (int64_t)gridDim.x * (kGroup / kWave)) {
    const int64_t ray = u * rays_per_wave + seg;
    const bool live = ray < n_rays;  // (wave-uniform loop bounds: every lane takes part in the shuffles)
    const int64_t n = live ? ray / ry.R : 0;
    float dx = 0.0f, dy = 0.0f, dz = 0.0f;
    if (RAY && live && ry.l != nullptr) dx = ry.d[ray * 3], dy = ry.d[ray * 3 + 1], dz = ry.d[ray * 3 + 2];
    float so[3] = {0.0f, 0.0f, 0.0f}, sd[3] = {0.0f, 0.0f, 0.0f};
    for (int64_t c = 0; c < chunks; ++c) {
      const int64_t k = c * G + kseg;
      const bool in = live && k < ry.P;
      float g[3] = {0.0f, 0.0f, 0.0f}, t = 0.0f;
      if (in) {
        const int64_t pt = ray * ry.P + k;
        float px, py, pz;
        point_of(ry, ray, pt, px, py, pz);
        const Sample s = sample_of(px, py, pz, dm);
        grid_backward<VOL, RAY>(gd, ggd, n, dm.Cd, s, dm, kx, go_d ? go_d + pt * dm.Cd : nullptr, g[0], g[1], g[2]);
        grid_backward<VOL, RAY>(gf, ggf, n, dm.Cf, s, dm, kx, go_f ? go_f + pt * dm.Cf : nullptr, g[0], g[1], g[2]);
        if (RAY) {
          if (ry.l != nullptr) t = ry.l[pt];
          g[0] *= s.x.mult, g[1] *= s.y.mult, g[2] *= s.z.mult;  // (each half times the multiplier, then the pair's sum below)
        }
      }
      if (RAY) {
#pragma unroll
        for (int a = 0; a < 3; ++a) g[a] += __shfl_xor(g[a], 1);  // the x pair: both lanes hold the point's gradient
        if (in && kx == 0 && grad_l != nullptr) grad_l[ray * ry.P + k] = (g[0] * dx + g[1] * dy) + g[2] * dz;
        if (grad_o != nullptr || grad_dir != nullptr) {
          float vo[3], vd[3];
#pragma unroll
          for (int a = 0; a < 3; ++a) vo[a] = g[a], vd[a] = t * g[a];
          for (int d = 2; d < 2 * G; d <<= 1) {
#pragma unroll
            for (int a = 0; a < 3; ++a) vo[a] += __shfl_xor(vo[a], d), vd[a] += __shfl_xor(vd[a], d);
          }
#pragma unroll
          for (int a = 0; a < 3; ++a) so[a] += vo[a], sd[a] += vd[a];
        }
      }
    }
    if (RAY && live && kseg == 0 && kx == 0) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (grad_o != nullptr) grad_o[ray * 3 + a] = so[a];
        if (grad_dir != nullptr) grad_dir[ray * 3 + a] = sd[a];
      }
    }
  }
}

// ---- ordered form ---------------------------------------------------------------------------------------------------------------
// sample 8 pt + k: the voxel of corner k of point pt and its weight, or false
__device__ __forceinline__ bool sample_voxel(const Rays& ry, const Dims& dm, int64_t s, int64_t& n, int& x, int& y, int& z, float& w) {
  const int64_t pt = s >> 3;
  const int k = (int)(s & 7);
  if (k >= corners_of(dm)) return false;
  float px, py, pz;
  int64_t ray;
  ray_of(ry, pt, false, ray, n);
  point_of(ry, ray, pt, px, py, pz);
  const Sample sm = sample_of(px, py, pz, dm);
  return corner_of(sm, dm, k & 1, (k >> 1) & 1, k >> 2, x, y, z, w);
}

__global__ __launch_bounds__(kGroup) void volume_sample_keys_kernel(Rays ry, Dims dm, int shared, int64_t nsamples, int* __restrict__ keys) {
  const int64_t s = (int64_t)blockIdx.x * kGroup + threadIdx.x;
  if (s >= nsamples) return;
  int64_t n;
  int x, y, z;
  float w;
  const bool ok = sample_voxel(ry, dm, s, n, x, y, z, w);
  keys[s] = ok ? (int)((((shared ? 0 : n) * dm.D + z) * dm.H + y) * dm.W + x) : ordered::kNone;
}

struct VoxelOp {
  static constexpr int R = 4;
  Rays ry;
  Dims dm;
  const float* go_d;
  const float* go_f;
  GradGrid ggd, ggf;
  const int* keys;
  int64_t nsamples, nkeys;
  __device__ int64_t key(int64_t s) const { return keys[s]; }
  // channel c < Cd is density c, channel Cd + c feature c
  __device__ void row(int64_t s, int, int chunk, float (&r)[R]) const {
    int64_t n;
    int x, y, z;
    float w;
    if (!sample_voxel(ry, dm, s, n, x, y, z, w)) return;
    const int64_t pt = s >> 3;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int c = chunk * R + i;
      if (c < dm.Cd) r[i] = go_d ? w * go_d[pt * dm.Cd + c] : 0.0f;
      else if (c < dm.Cd + dm.Cf) r[i] = go_f ? w * go_f[pt * dm.Cf + (c - dm.Cd)] : 0.0f;
    }
  }
  __device__ void store(int k, int chunk, const float (&r)[R]) const {
    int64_t p = k;
    const int64_t x = p % dm.W;
    p /= dm.W;
    const int64_t y = p % dm.H;
    p /= dm.H;
    const int64_t z = p % dm.D, n = p / dm.D;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int c = chunk * R + i;
      if (c < dm.Cd) {
        if (ggd.p) ggd.p[n * ggd.sn + c * ggd.sc + z * ggd.sz + y * ggd.sy + x * ggd.sx] = r[i];
      } else if (c < dm.Cd + dm.Cf) {
        if (ggf.p) ggf.p[n * ggf.sn + (c - dm.Cd) * ggf.sc + z * ggf.sz + y * ggf.sy + x * ggf.sx] = r[i];
      }
    }
  }
};

// ---- host -----------------------------------------------------------------------------------------------------------------------
Grid grid_of(const float* p, const int64_t st[5]) { return Grid{p, st[0], st[1], st[2], st[3], st[4]}; }
GradGrid grad_grid_of(float* p, const int64_t st[5]) { return GradGrid{p, st[0], st[1], st[2], st[3], st[4]}; }

bool bad_sizes(int64_t Cd, int64_t Cf, int64_t D, int64_t H, int64_t W, int64_t N, int64_t R, int64_t P, unsigned flags) {
  return Cd < 1 || Cf < 0 || Cd > INT32_MAX / 2 || Cf > INT32_MAX / 2 || D < 1 || H < 1 || W < 1 || D > INT32_MAX || H > INT32_MAX ||
         W > INT32_MAX || N < 0 || R < 0 || P < 0 || (flags & ~7u);
}

bool bad_strides(const int64_t st[5]) {
  if (!st) return true;
  for (int i = 0; i < 5; ++i)
    if (st[i] < 0) return true;
  return false;
}

// the keys hold a voxel (with its batch element unless the grid is shared) and a sample index must fit the sort's int32 keys' count
bool beyond_keys(int64_t D, int64_t H, int64_t W, int64_t shared, int64_t N, int64_t R, int64_t P) {
  const double voxels = (shared ? 1.0 : (double)N) * (double)D * (double)H * (double)W;
  return voxels >= 2147483648.0 || (double)N * (double)R * (double)P > (double)(INT32_MAX / 8);
}

unsigned capped(int64_t groups) { return (unsigned)(groups > P3D_VOLUME_SAMPLE_MAX_GROUPS ? P3D_VOLUME_SAMPLE_MAX_GROUPS : groups); }

}  // namespace
}  // namespace p3d

using namespace p3d;

P3D_API int p3di_volume_sample_forward(const float* densities, const int64_t d_strides[5], const float* features,
                                       const int64_t f_strides[5], int64_t Cd, int64_t Cf, int64_t D, int64_t H, int64_t W,
                                       const float* origins, const float* directions, const float* lengths, int64_t N, int64_t R,
                                       int64_t P, unsigned flags, float* rays_densities, float* rays_features, p3d_stream_t stream) {
  if (bad_sizes(Cd, Cf, D, H, W, N, R, P, flags) || (!lengths && P > 1)) return P3D_ERR_INVALID_ARG;
  if (N == 0 || R == 0 || P == 0) return P3D_OK;
  if (!densities || bad_strides(d_strides) || !origins || (lengths && !directions) || !rays_densities) return P3D_ERR_INVALID_ARG;
  if (Cf > 0 && (!features || bad_strides(f_strides) || !rays_features)) return P3D_ERR_INVALID_ARG;
  const Rays ry{origins, directions, lengths, N, R, P};
  const Dims dm{(int)D, (int)H, (int)W, (int)Cd, (int)Cf, flags};
  const Grid gd = grid_of(densities, d_strides);
  const Grid gf = Cf > 0 ? grid_of(features, f_strides) : Grid{nullptr, 0, 0, 0, 0, 0};
  const int64_t total = N * R * P;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("volume_sample_forward", s);
  volume_sample_fwd_kernel<<<capped(ceil_div(total, kGroup)), kGroup, 0, s>>>(ry, gd, gf, dm, rays_densities, rays_features, total);
  return launch_status();
}

P3D_API int p3di_volume_sample_backward(const float* grad_rays_densities, const float* grad_rays_features, const float* densities,
                                        const int64_t d_strides[5], const float* features, const int64_t f_strides[5], int64_t Cd,
                                        int64_t Cf, int64_t D, int64_t H, int64_t W, const float* origins, const float* directions,
                                        const float* lengths, int64_t N, int64_t R, int64_t P, unsigned flags, float* grad_densities,
                                        const int64_t gd_strides[5], float* grad_features, const int64_t gf_strides[5],
                                        float* grad_origins, float* grad_directions, float* grad_lengths, p3d_stream_t stream) {
  if (bad_sizes(Cd, Cf, D, H, W, N, R, P, flags) || (!lengths && P > 1)) return P3D_ERR_INVALID_ARG;
  if (N == 0 || R == 0 || P == 0) return P3D_OK;
  const bool vol = grad_densities || grad_features, ray = grad_origins || grad_directions || grad_lengths;
  if (!origins || (lengths && !directions)) return P3D_ERR_INVALID_ARG;
  if ((grad_densities && bad_strides(gd_strides)) || (grad_features && (Cf == 0 || bad_strides(gf_strides)))) return P3D_ERR_INVALID_ARG;
  if (ray && (!densities || bad_strides(d_strides) || (Cf > 0 && (!features || bad_strides(f_strides))))) return P3D_ERR_INVALID_ARG;
  if (!vol && !ray) return P3D_OK;
  if (!grad_rays_densities && !(Cf > 0 && grad_rays_features)) return P3D_ERR_INVALID_ARG;
  if (Cf == 0) grad_rays_features = nullptr;
  const Rays ry{origins, directions, lengths, N, R, P};
  const Dims dm{(int)D, (int)H, (int)W, (int)Cd, (int)Cf, flags};
  const Grid none{nullptr, 0, 0, 0, 0, 0};
  const Grid gd = ray ? grid_of(densities, d_strides) : none;
  const Grid gf = ray && Cf > 0 ? grid_of(features, f_strides) : none;
  const GradGrid gnone{nullptr, 0, 0, 0, 0, 0};
  const GradGrid ggd = grad_densities ? grad_grid_of(grad_densities, gd_strides) : gnone;
  const GradGrid ggf = grad_features ? grad_grid_of(grad_features, gf_strides) : gnone;
  const int G = segment_points(P);
  const int64_t rounds = ceil_div(N * R, kPointsPerWave / G);
  const unsigned blocks = capped(ceil_div(rounds, kGroup / kWave));
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("volume_sample_backward", s);
#define P3D_VS_LAUNCH(VOL, RAY)                                                                                                         \
  volume_sample_bwd_kernel<VOL, RAY><<<blocks, kGroup, 0, s>>>(ry, gd, gf, dm, grad_rays_densities, grad_rays_features, ggd, ggf,    \
                                                               grad_origins, grad_directions, grad_lengths, G, rounds)
  if (vol && ray) P3D_VS_LAUNCH(true, true);
  else if (vol) P3D_VS_LAUNCH(true, false);
  else P3D_VS_LAUNCH(false, true);
#undef P3D_VS_LAUNCH
  return launch_status();
}

P3D_API size_t p3di_volume_sample_workspace_bytes(int64_t N, int64_t R, int64_t P, int64_t Cd, int64_t Cf) {
  if (N <= 0 || R <= 0 || P <= 0 || Cd < 1 || Cf < 0 || (double)N * (double)R * (double)P > (double)(INT32_MAX / 8)) return 0;
  return ordered::partial_bytes(N * R * P * 8, VoxelOp::R, (int)ceil_div(Cd + Cf, VoxelOp::R));
}

P3D_API int p3di_volume_sample_keys(int64_t D, int64_t H, int64_t W, int64_t shared, const float* origins, const float* directions,
                                    const float* lengths, int64_t N, int64_t R, int64_t P, unsigned flags, int32_t* keys,
                                    p3d_stream_t stream) {
  if (bad_sizes(1, 0, D, H, W, N, R, P, flags) || (!lengths && P > 1)) return P3D_ERR_INVALID_ARG;
  if (beyond_keys(D, H, W, shared, N, R, P)) return P3D_ERR_UNSUPPORTED;
  if (N == 0 || R == 0 || P == 0) return P3D_OK;
  if (!origins || (lengths && !directions) || !keys) return P3D_ERR_INVALID_ARG;
  const Rays ry{origins, directions, lengths, N, R, P};
  const Dims dm{(int)D, (int)H, (int)W, 1, 0, flags};
  const int64_t nsamples = N * R * P * 8;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("volume_sample_keys", s);
  volume_sample_keys_kernel<<<(unsigned)ceil_div(nsamples, kGroup), kGroup, 0, s>>>(ry, dm, shared ? 1 : 0, nsamples, keys);
  return launch_status();
}

P3D_API int p3di_volume_sample_ordered_backward(const float* grad_rays_densities, const float* grad_rays_features, int64_t Cd, int64_t Cf,
                                                int64_t D, int64_t H, int64_t W, int64_t shared, const float* origins,
                                                const float* directions, const float* lengths, int64_t N, int64_t R, int64_t P,
                                                unsigned flags, const int32_t* keys, const int64_t* sorted_samples, int64_t n_sorted,
                                                float* grad_densities, const int64_t gd_strides[5], float* grad_features, const int64_t gf_strides[5],
                                                void* workspace, size_t workspace_bytes, p3d_stream_t stream) {
  if (bad_sizes(Cd, Cf, D, H, W, N, R, P, flags) || (!lengths && P > 1) || n_sorted < 0) return P3D_ERR_INVALID_ARG;
  if (beyond_keys(D, H, W, shared, N, R, P)) return P3D_ERR_UNSUPPORTED;
  if (n_sorted > N * R * P * 8) return P3D_ERR_INVALID_ARG;
  if (N == 0 || R == 0 || P == 0 || n_sorted == 0 || (!grad_densities && !grad_features)) return P3D_OK;
  if (!origins || (lengths && !directions) || !keys || !sorted_samples) return P3D_ERR_INVALID_ARG;
  if ((grad_densities && bad_strides(gd_strides)) || (grad_features && (Cf == 0 || bad_strides(gf_strides)))) return P3D_ERR_INVALID_ARG;
  if (!grad_rays_densities && !(Cf > 0 && grad_rays_features)) return P3D_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < p3di_volume_sample_workspace_bytes(N, R, P, Cd, Cf)) return P3D_ERR_WORKSPACE;
  const Rays ry{origins, directions, lengths, N, R, P};
  const Dims dm{(int)D, (int)H, (int)W, (int)Cd, (int)Cf, flags};
  const GradGrid gnone{nullptr, 0, 0, 0, 0, 0};
  const VoxelOp op{ry, dm, grad_rays_densities, Cf > 0 ? grad_rays_features : nullptr,
                   grad_densities ? grad_grid_of(grad_densities, gd_strides) : gnone,
                   grad_features ? grad_grid_of(grad_features, gf_strides) : gnone, keys, N * R * P * 8,
                   (shared ? 1 : N) * D * H * W};
  return ordered::run(op, sorted_samples, n_sorted, (int)ceil_div(Cd + Cf, VoxelOp::R), workspace, (hipStream_t)stream,
                      "volume_sample_ordered_backward");
}
