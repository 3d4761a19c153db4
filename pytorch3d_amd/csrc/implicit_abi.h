/* implicit_abi.h -- the C ABI of csrc/implicit.hip (sample_pdf and emission-absorption raymarching), csrc/cubify.hip,
 * csrc/volume_sample.hip, csrc/harmonic.hip (harmonic embedding, stratified ray depths), csrc/marching_cubes.hip,
 * csrc/points_alignment.hip (iterative closest point, alignment of corresponding points) and csrc/mesh_laplacian.hip (the cotangent
 * Laplacian's smoothing loss, cot_laplacian and taubin_smoothing).
 *
 * An extension of include/p3d_amd.h with a header and a prefix of its own: the entries of that header (p3d_*) are a closed set that
 * the ABI tests count and compare with the library's exports, so these entries are named p3di_* and declared here.  Same
 * conventions: extern "C", P3D_OK / P3D_ERR_* status codes, p3d_stream_t, no host sync.  pytorch3d_amd/_lib.py reads this file the
 * way it reads p3d_amd.h (EXTENSION_DECLARATIONS; _lib.call serves both tables). */
#ifndef P3D_AMD_IMPLICIT_ABI_H_
#define P3D_AMD_IMPLICIT_ABI_H_

#include "../../include/p3d_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SamplePdf by the contract of the reference's compiled CPU operator (sample_pdf/sample_pdf_cpu.cpp with its binary search), in place:
 * per row, partial[i] = the float32 running sum of weights[0..i] in index order, total = partial[n_bins-1] + eps; per sample u =
 * outputs[row, j]: v = total * u; i = the first index in [0, n_bins - 1) with !(partial[i] < v), n_bins - 1 if there is none
 * (std::lower_bound's halving steps, also on unordered sums); if i > 0, v -= partial[i-1]; then outputs[row, j] =
 *   bins[i+1] if v > weights[i];  else bins[i] + (v / weights[i]) * (bins[i+1] - bins[i]) if weights[i] > eps;  else bins[i],
 * in float32 without FMA and with the correctly rounded quotient.  bins (B, n_bins+1), weights (B, n_bins), outputs (B, S)
 * contiguous f32.  Every index stays in [0, n_bins): NaN or negative data gives wrong numbers, never an access outside the arrays.
 *
 * p3di_sample_pdf (device): a workgroup of 256 lanes takes P3D_SAMPLE_PDF_ROWS rows (fewer when they do not fit) with their running
 * sums in LDS at the odd row stride n_bins | 1.  A row whose stride passes P3D_SAMPLE_PDF_LDS_FLOATS (n_bins >= that number) has
 * its sums made by one lane per row in the workspace and is searched there by the same function: no n_bins is refused.  workspace:
 * p3di_sample_pdf_workspace_bytes(B, n_bins) bytes (0 for the LDS form, which takes NULL; smaller: P3D_ERR_WORKSPACE).
 * p3di_sample_pdf_host: the same loop on host pointers.  The two write the same bits.
 * B or S of 0: P3D_OK without a launch.  n_bins < 1, negative sizes, missing pointers: P3D_ERR_INVALID_ARG.  No host sync. */
#define P3D_SAMPLE_PDF_ROWS 16
#define P3D_SAMPLE_PDF_LDS_FLOATS 8192
size_t p3di_sample_pdf_workspace_bytes(int64_t B, int64_t n_bins);
int p3di_sample_pdf(const float* bins, const float* weights, float* outputs, int64_t B, int64_t n_bins, int64_t S, float eps,
                   void* workspace, size_t workspace_bytes, p3d_stream_t stream);
int p3di_sample_pdf_host(const float* bins, const float* weights, float* outputs, int64_t B, int64_t n_bins, int64_t S, float eps);

/* Emission-absorption raymarching (renderer/implicit/raymarching.py) over N rays of P points with C feature channels, in float32:
 *   x_k = one_plus_eps - d_k;   a_k = 1 for k < shift, else prod_{j <= k - shift} x_j;   w_k = d_k a_k;
 *   out[n, c] = sum_k w_k f_kc (c < C);   out[n, C] = 1 - prod_k (1 - d_k);   weights[n, k] = w_k when weights is not NULL.
 * densities (N, P), features (N, P, C), out (N, C+1), weights (N, P) contiguous f32.  C == 0 is the absorption-only raymarcher:
 * out (N, 1), features and weights unused.  shift >= P: a = 1 everywhere.
 * backward: grad_out (N, C+1), grad_weights (N, P) or NULL -> grad_densities (N, P), grad_features (N, P, C), every entry written:
 *   g_f_kc = w_k gF_c;   g_w_k = sum_c gF_c f_kc (+ grad_weights_k);
 *   g_d_k = a_k g_w_k - L_k T_k + gO prod_{j != k} (1 - d_j),   L_k = prod_{j < k} x_j,   T_k = g_w_{k+shift} d_{k+shift} + x_{k+1} T_{k+1}
 * -- no division, so a density of exactly 1 has its exact gradient.  Lanes run along the ray (segments of next_pow2(P) lanes up to
 * 64, then chunks of 64 with a carry); products and sums are shuffle scans and butterflies whose order P, C and shift fix: no atomic,
 * the same bits on every run and stream.  workspace (backward, P > 64 only): p3di_ea_raymarch_backward_workspace_bytes(N, P) bytes,
 * the prefix carries of every chunk (smaller: P3D_ERR_WORKSPACE).
 * N == 0: P3D_OK without a launch.  P < 1, shift < 1, negative sizes, missing pointers: P3D_ERR_INVALID_ARG.  No host sync. */
int p3di_ea_raymarch_forward(const float* densities, const float* features, int64_t N, int64_t P, int64_t C, int64_t shift,
                            float one_plus_eps, float* out, float* weights, p3d_stream_t stream);
size_t p3di_ea_raymarch_backward_workspace_bytes(int64_t N, int64_t P);
int p3di_ea_raymarch_backward(const float* densities, const float* features, const float* grad_out, const float* grad_weights,
                             int64_t N, int64_t P, int64_t C, int64_t shift, float one_plus_eps, float* grad_densities,
                             float* grad_features, void* workspace, size_t workspace_bytes, p3d_stream_t stream);

/* cubify (csrc/cubify.hip): occupancy grids voxels (N, D, H, W), float32 read through voxel_strides (in elements: a slice, a squeeze or
 * a permuted view is read in place), to the merged cube meshes of the reference's pytorch3d/ops/cubify.py:
 *   occupied iff voxels[n, d, h, w] >= thresh (NaN and everything outside the grid: not);  x runs along W, y along H, z along D;
 *   voxels in (n, h, w, d) order, d fastest, each with the directions -x +y -z -y +x +z, a direction's two triangles iff the neighbour
 *   there is not occupied:  (0,1,2) (1,3,2) | (2,3,6) (3,7,6) | (0,2,6) (0,6,4) | (0,5,1) (0,4,5) | (6,7,5) (6,5,4) | (1,7,3) (1,5,7),
 *   corner c = 4x + 2y + z of voxel (h, w, d) being lattice point g = ((h + y)(W + 1) + (w + x))(D + 1) + (d + z);
 *   a lattice point is kept iff a triangle of its mesh names it; the kept ones of a mesh keep ascending g, a face stores their ranks.
 * Two entries around the caller's one host read:
 * p3di_cubify_count: fills the workspace (a byte of exposure bits per voxel, the block-local rank of every lattice point, and the
 *   exclusive scans of the totals of every scan block of P3D_CUBIFY_ITEMS items; a scan block never spans two meshes) and writes
 *   counts (N, 2) int64 = (V_n, F_n).  Three launches: a lane per voxel, a lane per lattice point, and two workgroups of
 *   P3D_CUBIFY_CARRY_BLOCK lanes over the block totals in rounds.  No workgroup waits for another.
 * p3di_cubify_emit: from that workspace, unchanged, on the same stream: verts (total_verts, 3) float32 with row first_vert[n] + rank =
 *   (coords[x], coords[W + 1 + y], coords[W + 1 + H + 1 + z]) -- coords: the (W + 1) + (H + 1) + (D + 1) coordinate values of the
 *   three axes, made by the caller --, faces (total_faces, 3) int64 with per-mesh ranks, and, where feats is not NULL and K > 0,
 *   face_feats (total_faces, K) = feats[n, :, d, h, w] of the face's voxel, feats (N, K, D, H, W) float32 read through feat_strides.
 *   total_verts and total_faces must be the sums of the counts: the outputs are written by those, not by these two numbers.
 * workspace: p3di_cubify_workspace_bytes(N, D, H, W) bytes for both (smaller: P3D_ERR_WORKSPACE), about 1 byte per voxel and 4 per
 * lattice point.  0 for sizes the entries refuse.
 * No atomic; the same bits on every run and stream.  N == 0 (count) and total_faces == 0 (emit): P3D_OK without a launch.  A dimension
 * below 1, negative sizes, missing pointers, and N (D+1)(H+1)(W+1) or 12 N D H W beyond INT32_MAX: P3D_ERR_INVALID_ARG.  No host sync. */
#define P3D_CUBIFY_BLOCK 256
#define P3D_CUBIFY_ITEMS 1024
#define P3D_CUBIFY_CARRY_BLOCK 1024
size_t p3di_cubify_workspace_bytes(int64_t N, int64_t D, int64_t H, int64_t W);
int p3di_cubify_count(const float* voxels, const int64_t voxel_strides[4], int64_t N, int64_t D, int64_t H, int64_t W, float thresh,
                      void* workspace, size_t workspace_bytes, int64_t* counts, p3d_stream_t stream);
int p3di_cubify_emit(const float* coords, const float* feats, const int64_t feat_strides[5], int64_t K, int64_t N, int64_t D, int64_t H,
                     int64_t W, int64_t total_verts, int64_t total_faces, const void* workspace, size_t workspace_bytes, float* verts,
                     int64_t* faces, float* face_feats, p3d_stream_t stream);

/* VolumeSampler (csrc/volume_sample.hip): steps 2 and 3 of the reference's VolumeSampler.forward (renderer/implicit/renderer.py) in
 * float32.  densities (N, Cd, D, H, W) and features (N, Cf, D, H, W) -- NULL: Cf = 0 -- are read through five element strides each
 * (a channel slice or an expand is read in place; a batch stride of 0 is ONE grid shared by the N ray batches).  origins (N, R, 3),
 * directions (N, R, 3), lengths (N, R, P) contiguous; lengths == NULL: P = 1 and the point is the origin itself, no arithmetic.
 *   point_k = o + l_k * d, one multiply then one add, no FMA; nothing of shape (N, R, P, 3) is stored.
 *   F.grid_sample on a 5-D input as ATen defines it: x indexes W, y indexes H, z indexes D; source index of c on an axis of S voxels
 *   ((c + 1) / 2) * (S - 1) with P3D_VOLUME_SAMPLE_CORNERS, ((c + 1) * S - 1) / 2 without; P3D_VOLUME_SAMPLE_BORDER clamps it to
 *   [0, S - 1] (NaN -> 0) with a zero coordinate gradient where clamped; bilinear: the corners tnw tne tsw tse bnw bne bsw bse with
 *   the weights (wx wy) wz, the in-range ones summed in that order from +0; P3D_VOLUME_SAMPLE_NEAREST: round half to even, no
 *   coordinate gradient.  Under zeros padding a source coordinate that is not finite or does not fit an int32 gives an empty sample.
 * forward -> rays_densities (N, R, P, Cd), rays_features (N, R, P, Cf) contiguous, every entry written; corners and weights once per
 *   point for all Cd + Cf channels.
 * backward: the two output gradients (either may be NULL: zero) -> grad_densities / grad_features through their own strides, ADDED by
 *   float atomics without return value (the caller zero-fills; a batch stride of 0: every ray batch adds into the one grid), two
 *   lanes per point so that the voxels of an x pair leave from adjacent lanes; and, each where its pointer is not NULL,
 *   grad_origins (N, R, 3) = sum_k g_k, grad_directions (N, R, 3) = sum_k l_k g_k, grad_lengths (N, R, P) = g_k . d with g_k the
 *   coordinate gradient of point k: shuffle trees along the ray with a carry over chunks of 32 points, no atomic, the same bits on
 *   every run.  With the three NULL the launch reads no volume (a compile-time switch); with both volume gradients NULL it is the
 *   ray gradients alone.
 * ordered form: p3di_volume_sample_keys writes keys (N R P 8) int32, sample 8 pt + k -> ((n D + z) H + y) W + x of corner k (n = 0
 *   for shared != 0) or -1; the caller sorts stably (sorted_samples: n_sorted int64 sample indices in key order; the samples
 *   with key -1 are best left out, or they form one long segment that a single lane walks) and
 *   p3di_volume_sample_ordered_backward adds the rows by ordered_sum.h, channels (densities, then features) in chunks of 4, and
 *   stores every voxel's sum once: the same bits on every run and stream.  workspace: p3di_volume_sample_workspace_bytes (smaller:
 *   P3D_ERR_WORKSPACE).  (shared ? 1 : N) D H W beyond an int32 or N R P beyond INT32_MAX / 8: P3D_ERR_UNSUPPORTED.
 * N, R or P of 0: P3D_OK without a launch.  D, H or W below 1, Cd < 1, negative sizes or strides, unknown flags, missing pointers:
 * P3D_ERR_INVALID_ARG.  No host sync.  The forward and the backward are grid-stride loops of at most P3D_VOLUME_SAMPLE_MAX_GROUPS
 * workgroups of 256 lanes (the forward over points, the backward over rounds of one wave: 32 / next_pow2(P) rays of P <=
 * P3D_VOLUME_SAMPLE_CHUNK points, or one longer ray in chunks of that many points). */
#define P3D_VOLUME_SAMPLE_NEAREST 1
#define P3D_VOLUME_SAMPLE_BORDER 2
#define P3D_VOLUME_SAMPLE_CORNERS 4
#define P3D_VOLUME_SAMPLE_MAX_GROUPS 8192
#define P3D_VOLUME_SAMPLE_CHUNK 32
int p3di_volume_sample_forward(const float* densities, const int64_t d_strides[5], const float* features, const int64_t f_strides[5],
                               int64_t Cd, int64_t Cf, int64_t D, int64_t H, int64_t W, const float* origins, const float* directions,
                               const float* lengths, int64_t N, int64_t R, int64_t P, unsigned flags, float* rays_densities,
                               float* rays_features, p3d_stream_t stream);
int p3di_volume_sample_backward(const float* grad_rays_densities, const float* grad_rays_features, const float* densities,
                                const int64_t d_strides[5], const float* features, const int64_t f_strides[5], int64_t Cd, int64_t Cf,
                                int64_t D, int64_t H, int64_t W, const float* origins, const float* directions, const float* lengths,
                                int64_t N, int64_t R, int64_t P, unsigned flags, float* grad_densities, const int64_t gd_strides[5],
                                float* grad_features, const int64_t gf_strides[5], float* grad_origins, float* grad_directions,
                                float* grad_lengths, p3d_stream_t stream);
size_t p3di_volume_sample_workspace_bytes(int64_t N, int64_t R, int64_t P, int64_t Cd, int64_t Cf);
int p3di_volume_sample_keys(int64_t D, int64_t H, int64_t W, int64_t shared, const float* origins, const float* directions,
                            const float* lengths, int64_t N, int64_t R, int64_t P, unsigned flags, int32_t* keys, p3d_stream_t stream);
int p3di_volume_sample_ordered_backward(const float* grad_rays_densities, const float* grad_rays_features, int64_t Cd, int64_t Cf,
                                        int64_t D, int64_t H, int64_t W, int64_t shared, const float* origins, const float* directions,
                                        const float* lengths, int64_t N, int64_t R, int64_t P, unsigned flags, const int32_t* keys,
                                        const int64_t* sorted_samples, int64_t n_sorted, float* grad_densities, const int64_t gd_strides[5],
                                        float* grad_features, const int64_t gf_strides[5], void* workspace, size_t workspace_bytes,
                                        p3d_stream_t stream);

/* HarmonicEmbedding (csrc/harmonic.hip): the reference's renderer/implicit/harmonic_embedding.py in float32, formula for formula.
 * x (rows, dim), diag_cov (rows, dim) or NULL, out (rows, W) with W = dim (2 n + append_input), all contiguous; freqs (n): the module's
 * _frequencies buffer (omega_0 already in it), any values.  -ffp-contract=off keeps every operation below a rounding of its own:
 *   t = x[r,i] * f[k];   a_s = t + c_s,  c_0 = 0.0f,  c_1 = float32(0.5 pi) (the reference's _zero_half_pi);
 *   out[r, (s dim + i) n + k] = sinf(a_s) * e     -- s = 0 the "sin" block, s = 1 the "cos" block = sin(t + pi/2), never cosf(t);
 *   e = 1 without diag_cov, else expf(-0.5f * (diag_cov[r,i] * (f[k] * f[k])));
 *   out[r, 2 dim n + i] = x[r,i], append_input only: a copy, bit for bit.
 * sinf, cosf and expf are the device library's full-range functions.
 * backward: grad_out (rows, W) -> each where its pointer is not NULL, every entry written,
 *   grad_x[r,i]   = sum g e f[k] cosf(a_s)   (terms ((g e) f) cos, without diag_cov (g f) cos), then + g of the appended slot;
 *   grad_cov[r,i] = sum (g sinf(a_s)) (e (-0.5f (f[k] f[k])));
 * float32 sums from +0 in the fixed order s = 0 then 1, k ascending, the appended slot last; no atomic: the same bits on every run and
 * stream.  grad_cov without diag_cov: P3D_ERR_INVALID_ARG.
 * Launches: workgroups of 256 lanes, grid-stride over row tiles, at most P3D_HARMONIC_MAX_GROUPS workgroups.  A forward tile is
 * P3D_HARMONIC_FWD_ROWS rows, a lane per output element.  A backward tile is min(P3D_HARMONIC_BWD_ROWS, P3D_HARMONIC_BWD_LDS_FLOATS /
 * (W | 1)) rows of grad_out staged in LDS at the odd row stride W | 1, then a lane per (row, i).
 * rows == 0: P3D_OK without a launch.  dim < 1, n < 1, append_input outside {0, 1}, W > P3D_HARMONIC_MAX_WIDTH (the widest row of that
 * LDS tile), rows W > INT32_MAX (the kernels index in 32 bits), missing pointers: P3D_ERR_INVALID_ARG.  No host sync. */
#define P3D_HARMONIC_FWD_ROWS 64
#define P3D_HARMONIC_BWD_ROWS 64
#define P3D_HARMONIC_BWD_LDS_FLOATS 8192
#define P3D_HARMONIC_MAX_WIDTH 8191
#define P3D_HARMONIC_MAX_GROUPS 8192
int p3di_harmonic_embedding_forward(const float* x, const float* diag_cov, const float* freqs, int64_t rows, int64_t dim, int64_t n,
                                    int64_t append_input, float* out, p3d_stream_t stream);
int p3di_harmonic_embedding_backward(const float* x, const float* diag_cov, const float* freqs, const float* grad_out, int64_t rows,
                                     int64_t dim, int64_t n, int64_t append_input, float* grad_x, float* grad_cov, p3d_stream_t stream);

/* Stratified depths (csrc/harmonic.hip): _jiggle_within_stratas of the reference's renderer/implicit/raysampling.py.  centers (rows, n)
 * float32 read through its two element strides (a stride-0 expand of one linspace is read in place), uniforms and out (rows, n)
 * contiguous:
 *   lower = k == 0 ? c[0] : 0.5f * (c[k] + c[k-1]);   upper = k == n - 1 ? c[n-1] : 0.5f * (c[k+1] + c[k]);
 *   out[r,k] = lower + (upper - lower) * uniforms[r,k]
 * in IEEE float32 without FMA: given the same uniforms, the bits of the reference's chain on the CPU and on the GPU.  n == 1: c[0] + 0 u.
 * rows or n of 0: P3D_OK without a launch.  Negative sizes or strides, rows n > INT32_MAX, missing pointers: P3D_ERR_INVALID_ARG. */
int p3di_stratified_depths(const float* centers, const int64_t strides[2], int64_t rows, int64_t n, const float* uniforms, float* out,
                           p3d_stream_t stream);

/* Marching cubes (csrc/marching_cubes.hip): scalar fields vol (N, D, H, W), float32 read through vol_strides (in elements: a channel
 * slice or a permuted view is read in place), to the isosurface meshes of the reference's pytorch3d/ops/marching_cubes.py.  x runs
 * along W, y along H, z along D; lattice point g = (z H + y) W + x; isolevels: N floats, one per volume.
 *   inside      a lattice point is inside iff its value < the isolevel, strictly; NaN: outside.
 *   cubes       the (D-1)(H-1)(W-1) cubes in the order of their low corner g.  Corner i of a cube is its low corner moved by
 *               (i & 1, i >> 1 & 1, i >> 2 & 1); the configuration byte has bit i set iff corner i is inside.  The triangles of a
 *               configuration are the rows of csrc/marching_cubes_tables.h: up to 15 entries 8 axis + corner, the edge that runs from
 *               `corner` one step along axis (0 = x, 1 = y, 2 = z).  The edges a configuration names are the edges whose ends differ.
 *   vertex      on the edge from p1 (value v1) to p2 (value v2), eps = 1e-5f: p1 if |iso - v1| < eps, else p2 if |iso - v2| < eps, else
 *               p1 if |v1 - v2| < eps, else with r = (iso - v1) / (v2 - v1) every coordinate p1 (1 - r) + p2 r -- products and sum
 *               rounded one by one, the two coordinates that do not vary included (csrc/marching_cubes_geom.h).
 * The DEVICE contract (what the reference returns for GPU tensors after its dedup) -- p3di_marching_cubes_count / _emit:
 *   a lattice edge carries a vertex iff its ends differ; it belongs to its LOW lattice point.  The vertices of a volume are in the order
 *   of (g, axis); every table triangle is kept, degenerate ones too; faces hold the per-volume vertex ranks (int64), cubes in g order,
 *   table order inside a cube; ids[v] = g (W + W H + W H D) + g', g' the edge's high lattice point: strictly ascending per volume.
 *   count: fills the workspace (a word per lattice point: the rank of its first vertex inside its scan block, its three edge flags and
 *     its cube's configuration byte; and the exclusive scans of the vertex and triangle totals of every scan block of
 *     P3D_MARCHING_CUBES_ITEMS lattice points -- a scan block never spans two volumes) and writes counts (N, 2) int64 = (V_n, F_n).
 *     Two launches: a lane per lattice point in rounds of P3D_MARCHING_CUBES_BLOCK, then two workgroups of
 *     P3D_MARCHING_CUBES_CARRY_BLOCK lanes over the block totals in rounds.  No workgroup waits for another.
 *   emit: from that workspace, unchanged, and the same vol and isolevels, on the same stream: verts (total_verts, 3) float32 -- world
 *     coordinates, or with local != 0 each coordinate c / ((size - 1) / 2) - 1 --, ids (total_verts) int64 and faces (total_faces, 3)
 *     int64.  total_verts and total_faces must be the sums of the counts.  Two launches, a lane per lattice point each; the table is
 *     staged in LDS.
 *   workspace: p3di_marching_cubes_workspace_bytes(N, D, H, W) bytes, about 4 per lattice point; 0 for sizes the entries refuse.
 *   No atomic; the same bits on every run and stream.  N == 0, or no cube (a dimension of 1): count writes zeros, without a scan.
 *   A dimension below 1, negative sizes, missing pointers, 15 N D H W beyond INT32_MAX: P3D_ERR_INVALID_ARG.  No host sync.
 * The CPU contract (what the reference's compiled CPU operator returns) -- p3di_marching_cubes_host, ONE volume (D, H, W) on host
 * pointers: cubes in the same order; a triangle of which two vertices are closer than 1e-5 in every coordinate is dropped, AND every
 *   later triangle of the same cube with it; the vertices of the kept triangles in order of first use, one per lattice edge.
 *   edge_rank: 3 D H W int64 the caller filled with -1 (scratch).  verts (cap_verts, 3) and faces (cap_faces, 3) are written as far as
 *   the capacities reach (both may be NULL with capacity 0: a counting call); counts[2] = (V, F) always. */
#define P3D_MARCHING_CUBES_BLOCK 256
#define P3D_MARCHING_CUBES_ITEMS 2048
#define P3D_MARCHING_CUBES_CARRY_BLOCK 1024
size_t p3di_marching_cubes_workspace_bytes(int64_t N, int64_t D, int64_t H, int64_t W);
int p3di_marching_cubes_count(const float* vol, const int64_t vol_strides[4], int64_t N, int64_t D, int64_t H, int64_t W,
                              const float* isolevels, void* workspace, size_t workspace_bytes, int64_t* counts, p3d_stream_t stream);
int p3di_marching_cubes_emit(const float* vol, const int64_t vol_strides[4], int64_t N, int64_t D, int64_t H, int64_t W,
                             const float* isolevels, int64_t local, int64_t total_verts, int64_t total_faces, const void* workspace,
                             size_t workspace_bytes, float* verts, int64_t* ids, int64_t* faces, p3d_stream_t stream);
int p3di_marching_cubes_host(const float* vol, const int64_t vol_strides[3], int64_t D, int64_t H, int64_t W, float isolevel,
                             int64_t* edge_rank, float* verts, int64_t cap_verts, int64_t* faces, int64_t cap_faces, int64_t* counts);

/* Points alignment (csrc/points_alignment.hip): the reference's pytorch3d/ops/points_alignment.py on padded float32 clouds of dimension
 * 3.  X (N, P1, 3), Y (N, P2, 3) contiguous; lengths1 / lengths2 (N) int64 or NULL (full; clamped into [0, P]); R (N, 3, 3), T (N, 3),
 * s (N): the similarity transform  Xt = s * (x R) + T  of a ROW vector, formed as s * ((x0 R[0][k] + x1 R[1][k]) + x2 R[2][k]) + T[k], every
 * operation a float32 rounding of its own.
 *   weights   the weight of row i of cloud n is (mask_len == NULL or i < mask_len[n] ? 1 : 0) * (weights == NULL ? 1 : weights[n, i]).
 *             With neither (`uniform`) the means are plain means over the P1 rows and the total weight is clamp(P1, 1); else the means
 *             are sum(w x) / clamp(sum w, eps) and the total weight clamp(sum w, eps) -- the reference's two forms.
 *   moments   Xc = (x - Xmu) w, Yc = (y - Ymu) w (uniform: no w): the weight enters every product squared, as in the reference.
 *             XYcov = sum Xc^T Yc / total, Xcov = sum Xc . Xc / total, float32.
 *   solve     float64 on the float32 XYcov: XYcov = U diag(sigma) V^T, sigma descending; R = U diag(1, 1, e) V^T with e = det(U V^T), or
 *             e = 1 with P3D_ALIGN_ALLOW_REFLECTION; s = (sigma1 + sigma2 + e sigma3) / clamp(Xcov, eps) with P3D_ALIGN_ESTIMATE_SCALE,
 *             else 1; T = Ymu - s Xmu R.  Each result is rounded to float32 once.  A zero covariance gives R = I.  status[1] is set to 1
 *             where some sigma <= 1e-15 and is never cleared: the caller zeroes status before its first call.
 *   sums      every per-cloud sum is csrc/fixed_sum.h's tree over the partials of waves of 64 consecutive rows: no atomic, the same
 *             bits on every run, stream and process.
 * p3di_points_alignment: corresponding_points_alignment -- y of row i is row i of Y (P2 = P1 = P).  Four launches.
 * p3di_icp_match: idx[n, i] (int64) = the nearest point of Y[n, :lengths2[n]] to Xt[n, i] (to x itself where R, T, s are NULL, all three)
 *   by squared distance ((dx dx + dy dy) + dz dz, unfused) in the order (dist, j): what p3d_knn_points_forward returns for K = 1 and
 *   norm 2 on the transformed points, bit for bit; 0 in the rows past lengths1[n], where the cloud of Y is empty, and for a row
 *   no point of Y has a distance below +inf to.  A workgroup is 64 rows and `split` waves, each scanning a slice of ceil(lengths2 /
 *   split) points of Y in LDS tiles of P3D_KNN_TILE; split in {1, 2, 4, 8}, or 0: doubled while N ceil(P1 / 64) split stays within
 *   the chip's SIMDs and split within ceil(P2 / P3D_KNN_TILE).  The result does not depend on it.
 * p3di_icp_iteration: one iteration of iterative_closest_point, six launches:  match with (R_in, T_in, s_in) (NULL: X as given);
 *   the alignment of X with its neighbours under the weights of mask_len -> (R_out, T_out, s_out);  Xt (N, P1, 3) = X under the new
 *   transform;  rmse[n] = sqrt(sum w |Xt - y|^2 / clamp(sum w, 1e-9)) with the neighbours of the match;  relative = (rmse_prev[n] -
 *   rmse[n]) / rmse_prev[n], an IEEE float32 quotient (0 / 0: NaN), or 1 where rmse_prev is NULL -- the FIRST iteration, which also
 *   computes Xmu into the workspace, where the later iterations of the call find it: the same workspace, untouched in between;
 *   status[0] = 1 if relative <= relative_rmse_thr in every cloud, else 0.  A row past lengths1[n] that mask_len does not mask keeps
 *   its weight and is paired with Y[n, 0]: the reference's mask rule.  eps is the reference's 1e-9.
 * workspace: p3di_icp_workspace_bytes(N, P1) bytes for all three (smaller, or NULL: P3D_ERR_WORKSPACE); 0 for sizes the entries refuse.
 * N P1 == 0: P3D_OK without a launch for match; P3D_ERR_INVALID_ARG for the other two (there is nothing to align: the caller answers).
 * Negative sizes, N, P1 or P2 beyond INT32_MAX, a split outside {0, 1, 2, 4, 8}, unknown flags, missing pointers, some but not all
 * of R, T, s: P3D_ERR_INVALID_ARG.  No host sync. */
#define P3D_ICP_MAX_SPLIT 8
#define P3D_ALIGN_ESTIMATE_SCALE 1
#define P3D_ALIGN_ALLOW_REFLECTION 2
size_t p3di_icp_workspace_bytes(int64_t N, int64_t P1);
int p3di_icp_match(const float* X, const float* Y, const int64_t* lengths1, const int64_t* lengths2, const float* R, const float* T,
                   const float* s, int64_t N, int64_t P1, int64_t P2, int split, int64_t* idx, void* workspace, size_t workspace_bytes,
                   p3d_stream_t stream);
int p3di_icp_iteration(const float* X, const float* Y, const int64_t* lengths1, const int64_t* lengths2, const int64_t* mask_len,
                       const float* R_in, const float* T_in, const float* s_in, const float* rmse_prev, int64_t N, int64_t P1, int64_t P2,
                       int split, unsigned flags, float relative_rmse_thr, float* R_out, float* T_out, float* s_out, int64_t* idx,
                       float* Xt, float* rmse, int32_t* status, void* workspace, size_t workspace_bytes, p3d_stream_t stream);
int p3di_points_alignment(const float* X, const float* Y, const int64_t* mask_len, const float* weights, int64_t N, int64_t P,
                          unsigned flags, float eps, float* R, float* T, float* s, int32_t* status, void* workspace,
                          size_t workspace_bytes, p3d_stream_t stream);

/* The cotangent Laplacian (csrc/mesh_laplacian.hip): mesh_laplacian_smoothing "cot" / "cotcurv", the entries of cot_laplacian
 * (pytorch3d/ops/laplacian_matrices.py:73-141) and taubin_smoothing (pytorch3d/ops/mesh_filtering.py) as gathers over int32 tables
 * that the faces alone give (pytorch3d_amd/mesh_losses.py: cot_tables) beside the tables of p3d_amd.h's mesh regularisers:
 *   adj_offsets (V + 1), adj (2 E), vert_mesh (V), num_verts (N): as there;  adj_edge (2 E): the edge id of every slot of adj;
 *   edge_corner_offsets (E + 1), edge_corners (3 F): the corners 3 f + k sorted stably by the edge opposite them;
 *   inc_offsets (V + 1), inc_corners (3 F): the corners sorted stably by their vertex.
 * V, 2 E and 3 F must fit an int32.  faces (F, 3) int64 packed vertex ids, verts (V, 3) float32.
 * p3di_mesh_cot_weights, two launches: face_cot (F, 3) <- per corner k (b^2 + c^2 - a^2) / area / 4.0 with a the side opposite the
 *   corner, the sides by norm, s = 0.5 (A + B + C), face_area (F) <- sqrt(max(s (s - A) (s - B) (s - C), eps)): the reference's
 *   operations in its order, one float32 rounding each;  edge_w (E) <- +0 plus face_cot of the edge's corners in list order:
 *   L[i, j] of the reference for the edge (i, j).
 * p3di_mesh_cot_inv_areas: inv_areas (V) <- A_v = +0 plus face_area of the vertex's corners in list order; 1 / A_v where A_v > 0.
 * p3di_mesh_cot_laplacian_forward: per vertex Lx = sum_j w_e x_j and rowsum = sum_j w_e over its row of adj in list order;
 *   curvature == 0 ("cot"):  scale = rowsum > 0 ? 1 / rowsum : rowsum,  r = Lx scale - x;
 *   curvature != 0 ("cotcurv"):  scale = 0.25 inv_area,  r = (Lx - rowsum x) scale;
 *   term = |r| (1.0f / num_verts[mesh]);  loss: ONE float, (the sum of the terms by the fixed tree of csrc/fixed_sum.h, depth
 *   D(V) = 8 + ceil(ceil(V / 256) / 256) + 8) / N.  d (V, 3) <- r weight / |r| (0 where the norm is 0), scale (V), rowsum (V): kept for
 *   the backward.  workspace: one partial sum per 256 vertices.  face_area and the incidence lists are read for curvature != 0 only.
 * p3di_mesh_cot_laplacian_backward, one launch: with y = scale d, grad_verts_u = (grad_loss / N) (sum_j w_e y_j - d_u) for "cot" and
 *   (grad_loss / N) (sum_j w_e y_j - rowsum_u y_u) for "cotcurv": L is symmetric and a constant of the step.  Every row is written.
 * p3di_mesh_taubin_smoothing, 2 num_iter launches: a half-step is out_v = c1 x_v + (c sum_j w x_j) / sum_j w with
 *   w = 1 / (|x_v - x_j| + eps) over the row of adj; a vertex without a neighbour gives NaN (0 / 0), the reference's answer.  Each
 *   iteration takes a half-step with (lambd_c1, lambd_c) into scratch (V, 3) and one with (mu_c1, mu_c) into out (V, 3); verts is
 *   only read and may not overlap either; num_iter == 0 copies verts to out.
 * No float atomics: the same bits on every run and stream.  A table that breaks its contract gives NaN or wrong numbers, never an
 * access outside the arrays (ids are range-checked, CSR offsets clamped).  Negative sizes, sizes beyond int32, N <= 0, missing
 * pointers: P3D_ERR_INVALID_ARG; a short workspace: P3D_ERR_WORKSPACE.  No host sync. */
size_t p3di_mesh_cot_laplacian_forward_workspace_bytes(int64_t V);
int p3di_mesh_cot_weights(const float* verts, const int64_t* faces, const int32_t* edge_corner_offsets, const int32_t* edge_corners,
                          int64_t V, int64_t F, int64_t E, float eps, float* face_cot, float* face_area, float* edge_w,
                          p3d_stream_t stream);
int p3di_mesh_cot_inv_areas(const float* face_area, const int32_t* inc_offsets, const int32_t* inc_corners, int64_t V, int64_t F,
                            float* inv_areas, p3d_stream_t stream);
int p3di_mesh_cot_laplacian_forward(const float* verts, const float* edge_w, const float* face_area, const int32_t* adj_offsets,
                                    const int32_t* adj, const int32_t* adj_edge, const int32_t* inc_offsets, const int32_t* inc_corners,
                                    const int32_t* vert_mesh, const int32_t* num_verts, int64_t V, int64_t E, int64_t F, int N,
                                    int curvature, float* d, float* scale, float* rowsum, void* workspace, size_t workspace_bytes,
                                    float* loss, p3d_stream_t stream);
int p3di_mesh_cot_laplacian_backward(const float* grad_loss, const float* d, const float* scale, const float* rowsum, const float* edge_w,
                                     const int32_t* adj_offsets, const int32_t* adj, const int32_t* adj_edge, int64_t V, int64_t E, int N,
                                     int curvature, float* grad_verts, p3d_stream_t stream);
int p3di_mesh_taubin_smoothing(const float* verts, const int32_t* adj_offsets, const int32_t* adj, int64_t V, int64_t E, float lambd_c1,
                               float lambd_c, float mu_c1, float mu_c, float eps, int num_iter, float* scratch, float* out,
                               p3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* P3D_AMD_IMPLICIT_ABI_H_ */
