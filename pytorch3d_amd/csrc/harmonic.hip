// harmonic.hip -- the per-point work of an implicit renderer that was left as torch chains: HarmonicEmbedding.forward (the
// reference's renderer/implicit/harmonic_embedding.py), forward and backward, and the stratified depths of its ray samplers
// (_jiggle_within_stratas of renderer/implicit/raysampling.py).  Contract: implicit_abi.h (p3di_harmonic_embedding_*,
// p3di_stratified_depths).  No atomic anywhere: every run and stream writes the same bits.
//
//   forward   harmonic_fwd_kernel<COV>   a workgroup takes tiles of P3D_HARMONIC_FWD_ROWS rows, a lane per OUTPUT element of the tile,
//                                        so the stores of the odd-width rows (W = 63, 27, ...) are whole cache lines; the dim floats of
//                                        a row are read by its W neighbouring lanes from cache.  Row and column of a lane's first
//                                        element come from one 32-bit division per tile and move by 256 / W and 256 % W from there;
//                                        the column splits into (s, i, k) with one 32-bit division by n.
//   backward  harmonic_bwd_kernel<COV, GX, GC>  a workgroup stages a tile of grad_out rows in LDS (coalesced loads, row stride W | 1),
//                                        then a lane per (row, i) sums its 2n (+1) terms from there in the order s = 0, 1; k ascending;
//                                        the appended slot last.
//   depths    stratified_kernel          a lane per output element; the centres are read through their two strides (a stride-0 expand
//                                        of one linspace is never materialised).
// Both embedding kernels are grid-stride loops over row tiles of at most P3D_HARMONIC_MAX_GROUPS workgroups.
// The arithmetic is sinf / cosf / expf of the device library at full range and the build's -ffp-contract=off: t = x f and t + c_s are
// two rounded operations, as the reference's multiply and add are.
#include "implicit_abi.h"
#include "p3d_common.h"

namespace p3d {
namespace {

constexpr int kGroup = 256;
constexpr int kFwdRows = P3D_HARMONIC_FWD_ROWS;
constexpr int kBwdRows = P3D_HARMONIC_BWD_ROWS;
constexpr int kBwdFloats = P3D_HARMONIC_BWD_LDS_FLOATS;
constexpr float kHalfPi = 1.57079637050628662109375f;  // float32(0.5 * pi): the reference's _zero_half_pi[1]
static_assert(kGroup % kWave == 0 && kFwdRows >= 1 && kBwdRows >= 1 && kBwdRows <= kBwdFloats, "launch constants");

struct Shape {
  int rows, dim, n, W, block;  // W = dim (2 n + append), block = dim n
  bool append;
};

// e of the contract: exp(fl(-0.5f * fl(cov * fl(f * f))))
__device__ __forceinline__ float damping(float cov, float f) { return expf(-0.5f * (cov * (f * f))); }

template <bool COV>
__global__ void __launch_bounds__(kGroup) harmonic_fwd_kernel(const float* __restrict__ x, const float* __restrict__ cov,
                                                               const float* __restrict__ freqs, Shape sh, int tiles,
                                                               float* __restrict__ out) {
  const unsigned W = (unsigned)sh.W, n = (unsigned)sh.n, dim = (unsigned)sh.dim, trig = 2u * (unsigned)sh.block;
  const unsigned step_row = kGroup / W, step_col = kGroup % W;
  for (int tile = (int)blockIdx.x; tile < tiles; tile += (int)gridDim.x) {
    const int row0 = tile * kFwdRows;
    const unsigned tile_rows = (unsigned)min(kFwdRows, sh.rows - row0);
    const unsigned count = tile_rows * W;  // <= rows W <= INT32_MAX
    const unsigned base = (unsigned)row0 * W;
    unsigned row = threadIdx.x / W, col = threadIdx.x % W;
    for (unsigned e = threadIdx.x; e < count; e += kGroup) {
      const unsigned xi = ((unsigned)row0 + row) * dim;
      float v;
      if (col < trig) {
        const unsigned q = col / n, k = col - q * n;  // q = s dim + i
        const bool second = q >= dim;
        const unsigned i = second ? q - dim : q;
        const float f = freqs[k];
        const float t = x[xi + i] * f;
        const float a = t + (second ? kHalfPi : 0.0f);
        v = sinf(a);
        if (COV) v = v * damping(cov[xi + i], f);
      } else {
        v = x[xi + (col - trig)];  // the appended input, bit for bit
      }
      out[base + e] = v;
      row += step_row;
      col += step_col;
      if (col >= W) {
        col -= W;
        ++row;
      }
    }
  }
}

// rows of one backward tile: what fits the LDS budget at the row stride W | 1, at most P3D_HARMONIC_BWD_ROWS
inline int bwd_tile_rows(int W) { return (int)min((int64_t)kBwdRows, (int64_t)kBwdFloats / (W | 1)); }

template <bool COV, bool GX, bool GC>
__global__ void __launch_bounds__(kGroup) harmonic_bwd_kernel(const float* __restrict__ x, const float* __restrict__ cov,
                                                               const float* __restrict__ freqs, const float* __restrict__ grad_out,
                                                               Shape sh, int tile_rows_max, int tiles, float* __restrict__ grad_x,
                                                               float* __restrict__ grad_cov) {
  __shared__ float g[kBwdFloats];
  const unsigned W = (unsigned)sh.W, stride = W | 1u, dim = (unsigned)sh.dim;
  const unsigned step_row = kGroup / W, step_col = kGroup % W;
  for (int tile = (int)blockIdx.x; tile < tiles; tile += (int)gridDim.x) {
    const int row0 = tile * tile_rows_max;
    const unsigned tile_rows = (unsigned)min(tile_rows_max, sh.rows - row0);
    const unsigned count = tile_rows * W;
    const unsigned base = (unsigned)row0 * W;
    unsigned row = threadIdx.x / W, col = threadIdx.x % W;
    for (unsigned e = threadIdx.x; e < count; e += kGroup) {
      g[row * stride + col] = grad_out[base + e];
      row += step_row;
      col += step_col;
      if (col >= W) {
        col -= W;
        ++row;
      }
    }
    __syncthreads();
    const unsigned items = tile_rows * dim;
    for (unsigned item = threadIdx.x; item < items; item += kGroup) {
      const unsigned r = item / dim, i = item - r * dim;
      const unsigned xi = (unsigned)row0 * dim + item;
      const float xv = x[xi];
      const float cv = COV ? cov[xi] : 0.0f;
      const float* grow = g + r * stride;
      float acc_x = 0.0f, acc_c = 0.0f;
      for (int s = 0; s < 2; ++s) {
        const float c = s ? kHalfPi : 0.0f;
        const float* gs = grow + ((unsigned)s * dim + i) * (unsigned)sh.n;
        for (int k = 0; k < sh.n; ++k) {
          const float f = freqs[k];
          const float a = xv * f + c;  // two rounded operations (-ffp-contract=off)
          const float gv = gs[k];
          if (COV) {
            const float ev = damping(cv, f);
            if (GX) acc_x = acc_x + ((gv * ev) * f) * cosf(a);
            if (GC) acc_c = acc_c + (gv * sinf(a)) * (ev * (-0.5f * (f * f)));
          } else if (GX) {
            acc_x = acc_x + (gv * f) * cosf(a);
          }
        }
      }
      if (GX) {
        if (sh.append) acc_x = acc_x + grow[2u * (unsigned)sh.block + i];
        grad_x[xi] = acc_x;
      }
      if (GC) grad_cov[xi] = acc_c;
    }
    __syncthreads();  // the next tile overwrites g
  }
}

__global__ void __launch_bounds__(kGroup) stratified_kernel(const float* __restrict__ centers, int64_t row_stride, int64_t col_stride,
                                                             int n, unsigned total, const float* __restrict__ uniforms,
                                                             float* __restrict__ out) {
  const unsigned lanes = gridDim.x * kGroup;
  // (total <= INT32_MAX and lanes <= 2^20: e + lanes stays below 2^32)
  for (unsigned e = blockIdx.x * kGroup + threadIdx.x; e < total; e += lanes) {
    const unsigned row = e / (unsigned)n;
    const int k = (int)(e - row * (unsigned)n);
    const float* c = centers + (int64_t)row * row_stride;
    const float here = c[(int64_t)k * col_stride];
    const float lower = k == 0 ? here : 0.5f * (here + c[(int64_t)(k - 1) * col_stride]);
    const float upper = k == n - 1 ? here : 0.5f * (c[(int64_t)(k + 1) * col_stride] + here);
    out[e] = lower + (upper - lower) * uniforms[e];
  }
}

// false: sizes the entries refuse (the Python layer takes its torch formulation there)
bool shape_of(int64_t rows, int64_t dim, int64_t n, int64_t append_input, Shape* sh) {
  if (rows < 0 || dim < 1 || n < 1 || (append_input != 0 && append_input != 1)) return false;
  if (dim > INT32_MAX || n > INT32_MAX / 2 - 1) return false;
  const int64_t per = 2 * n + append_input;
  if (dim > INT32_MAX / per) return false;
  const int64_t W = dim * per;
  if (W > P3D_HARMONIC_MAX_WIDTH) return false;
  if (rows > 0 && W > INT32_MAX / rows) return false;
  *sh = Shape{(int)rows, (int)dim, (int)n, (int)W, (int)(dim * n), append_input != 0};
  return true;
}

unsigned capped(int64_t groups) { return (unsigned)(groups > P3D_HARMONIC_MAX_GROUPS ? P3D_HARMONIC_MAX_GROUPS : groups); }

}  // namespace
}  // namespace p3d

using namespace p3d;
static_assert((P3D_HARMONIC_MAX_WIDTH | 1) <= P3D_HARMONIC_BWD_LDS_FLOATS && ((P3D_HARMONIC_MAX_WIDTH + 1) | 1) > P3D_HARMONIC_BWD_LDS_FLOATS,
              "P3D_HARMONIC_MAX_WIDTH is the widest row whose odd stride fits the backward's LDS tile");

P3D_API int p3di_harmonic_embedding_forward(const float* x, const float* diag_cov, const float* freqs, int64_t rows, int64_t dim, int64_t n,
                                            int64_t append_input, float* out, p3d_stream_t stream) {
  Shape sh;
  if (!shape_of(rows, dim, n, append_input, &sh)) return P3D_ERR_INVALID_ARG;
  if (rows == 0) return P3D_OK;
  if (!x || !freqs || !out) return P3D_ERR_INVALID_ARG;
  const int tiles = (int)ceil_div(rows, kFwdRows);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("harmonic_embedding_forward", s);
  if (diag_cov) harmonic_fwd_kernel<true><<<capped(tiles), kGroup, 0, s>>>(x, diag_cov, freqs, sh, tiles, out);
  else harmonic_fwd_kernel<false><<<capped(tiles), kGroup, 0, s>>>(x, nullptr, freqs, sh, tiles, out);
  return launch_status();
}

P3D_API int p3di_harmonic_embedding_backward(const float* x, const float* diag_cov, const float* freqs, const float* grad_out, int64_t rows,
                                             int64_t dim, int64_t n, int64_t append_input, float* grad_x, float* grad_cov,
                                             p3d_stream_t stream) {
  Shape sh;
  if (!shape_of(rows, dim, n, append_input, &sh) || (grad_cov && !diag_cov)) return P3D_ERR_INVALID_ARG;
  if (rows == 0 || (!grad_x && !grad_cov)) return P3D_OK;
  if (!x || !freqs || !grad_out) return P3D_ERR_INVALID_ARG;
  const int tile_rows = bwd_tile_rows(sh.W);
  const int tiles = (int)ceil_div(rows, tile_rows);
  const unsigned blocks = capped(tiles);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("harmonic_embedding_backward", s);
#define P3D_HE_LAUNCH(COV, GX, GC) \
  harmonic_bwd_kernel<COV, GX, GC><<<blocks, kGroup, 0, s>>>(x, diag_cov, freqs, grad_out, sh, tile_rows, tiles, grad_x, grad_cov)
  if (!diag_cov) P3D_HE_LAUNCH(false, true, false);
  else if (grad_x && grad_cov) P3D_HE_LAUNCH(true, true, true);
  else if (grad_x) P3D_HE_LAUNCH(true, true, false);
  else P3D_HE_LAUNCH(true, false, true);
#undef P3D_HE_LAUNCH
  return launch_status();
}

P3D_API int p3di_stratified_depths(const float* centers, const int64_t strides[2], int64_t rows, int64_t n, const float* uniforms, float* out,
                                   p3d_stream_t stream) {
  if (rows < 0 || n < 0 || (rows > 0 && n > INT32_MAX / rows)) return P3D_ERR_INVALID_ARG;
  if (rows == 0 || n == 0) return P3D_OK;
  if (!centers || !strides || strides[0] < 0 || strides[1] < 0 || !uniforms || !out) return P3D_ERR_INVALID_ARG;
  const int64_t total = rows * n;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope ls("stratified_depths", s);
  stratified_kernel<<<stream_blocks(total), kGroup, 0, s>>>(centers, strides[0], strides[1], (int)n, (unsigned)total, uniforms, out);
  return launch_status();
}
