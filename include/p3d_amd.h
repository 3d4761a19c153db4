/*
 * p3d_amd.h -- C ABI of libp3d_amd.so: the MI355X (gfx950) implementation of PyTorch3D's
 * differentiable-rasterization hot path.
 *
 * One entry point per operator of the reference's pybind surface `pytorch3d._C`
 * (pytorch3d/csrc/ext.cpp:38-73).  Every function
 *   - takes plain device pointers and sizes (no torch types),
 *   - is asynchronous on the HIP stream it is handed (no allocation, no host sync),
 *   - writes every element of its outputs (padding value -1 included: callers pass
 *     uninitialised memory, there is no pre-fill pass),
 *   - returns P3D_OK or a negative error code (p3d_error_string()).
 * Scratch memory comes from the caller: ask p3d_*_workspace_bytes() first.
 * The current HIP device must be the one that owns the pointers and the stream.
 *
 * Layouts are the reference's: packed AoS face_verts (F,3,3) f32; per-mesh
 * first-index/count vectors (N) i64; outputs (N,H,W,K[,3]).  Output pixel (y, x) looks
 * along flipped axes (+Y up, +X left), rasterize_meshes.cu:271-277.
 */
#ifndef P3D_AMD_H_
#define P3D_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P3D_ABI_VERSION 3

#define P3D_OK 0
#define P3D_ERR_INVALID_ARG (-1)   /* null pointer / negative size / bad mode                    */
#define P3D_ERR_K_TOO_LARGE (-2)   /* K > 150 (rasterization_utils.cuh:49, rasterize_meshes.cu:361) */
#define P3D_ERR_TOO_MANY_BINS (-3) /* bins per side >= 22 (rasterize_coarse.cu:244-249)           */
#define P3D_ERR_WORKSPACE (-4)     /* workspace smaller than p3d_*_workspace_bytes()              */
#define P3D_ERR_LAUNCH (-5)        /* HIP reported a launch failure                              */
#define P3D_ERR_UNSUPPORTED (-6)

#define P3D_MAX_K 150
#define P3D_MAX_BINS_PER_SIDE 21

typedef void* p3d_stream_t; /* hipStream_t */

int p3d_abi_version(void);
const char* p3d_error_string(int code);

/* ---- meshes -------------------------------------------------------------------------- */

/* Scratch bytes for p3d_rasterize_meshes / p3d_rasterize_meshes_coarse (0 when bin_size == 0).
 * Sized for the WORST case, because sizing it exactly would need a host sync: the bin lists are reserved as
 * min(F * bins, N * bins * max_faces_per_bin) int32 entries (every face in every bin, or every bin at its cap), plus
 * per-(mesh, bin) counters, offsets and the tile plan (~20 B per bin) and per-(1024-face chunk, bin) partial counts.
 * Only the used prefix is ever touched.  Examples at 512 x 512 (1024 internal bins per image), max_faces_per_bin =
 * max(10000, F / 5) as the reference's wrapper picks it: one 5.8k-face mesh 24 MB; the bench batch (N = 64, F = 321k)
 * 1.3 GB; an un-sharded batch of 512 such meshes 42 GB -- hand over a short workspace (below), shard the batch
 * (pytorch3d_amd/sharding.py) or lower max_faces_per_bin when that matters.  Reuse the workspace across calls; it carries no
 * state between them. */
size_t p3d_rasterize_meshes_workspace_bytes(int64_t F, int N, int H, int W, int bin_size, int max_faces_per_bin);

/* Short workspaces (p3d_rasterize_meshes and p3d_rasterize_meshes_ex only; the reference has no counterpart: its
 * coarse stage allocates the padded (N, BH, BW, max_faces_per_bin) tensor, rasterize_coarse.cu:353-354).
 * Those two calls accept ANY workspace of at least p3d_rasterize_meshes_short_workspace_bytes(..., list_entries = 0) bytes:
 * the bin lists get whatever room is left after the fixed arrays.  Whether the lists fit is decided on the device, after
 * the scan, with no host sync: when they do, the binned kernel runs as usual and a second, naive launch returns at once;
 * when they do not, the binned kernel returns at once and the naive kernel (every tile tests every face of its mesh)
 * writes the same outputs -- slower, bit-identical.  The int64 at byte p3d_rasterize_meshes_workspace_need_offset(...) of
 * the workspace holds, once the call has run, the number of list entries it needed: read it back whenever convenient and
 * size the next workspace with p3d_rasterize_meshes_short_workspace_bytes(..., that number plus headroom).  Bench batch:
 * 2.1 M entries = 8.4 MB of lists against the 1.3 GB worst case.  The cost of a short workspace is the second launch
 * (its workgroups exit on a scalar load): 0.026 ms for the 65 536 tiles of the bench batch, whose lists that do not fit cost
 * 6.7 ms instead of 1.5 (profiles/r04/r04c8/). */
size_t p3d_rasterize_meshes_short_workspace_bytes(int64_t F, int N, int H, int W, int bin_size, int max_faces_per_bin,
                                                  int64_t list_entries);
size_t p3d_rasterize_meshes_workspace_need_offset(int64_t F, int N, int H, int W, int bin_size, int max_faces_per_bin);

/* replaces RasterizeMeshes, pytorch3d/csrc/rasterize_meshes/rasterize_meshes.h:513-562
 * (_C.rasterize_meshes).  bin_size == 0 or max_faces_per_bin == 0 -> naive path, else
 * coarse binning + fine rasterization.  Outputs: pix_to_face (N,H,W,K) i64, zbuf (N,H,W,K) f32,
 * bary (N,H,W,K,3) f32, dists (N,H,W,K) f32. */
int p3d_rasterize_meshes(const float* face_verts, const int64_t* mesh_to_face_first_idx,
                         const int64_t* num_faces_per_mesh, const int64_t* clipped_faces_neighbor_idx, int64_t F, int N,
                         int H, int W, float blur_radius, int faces_per_pixel, int bin_size, int max_faces_per_bin,
                         int perspective_correct, int clip_barycentric_coords, int cull_backfaces, int64_t* pix_to_face,
                         float* zbuf, float* bary, float* dists, void* workspace, size_t workspace_bytes,
                         p3d_stream_t stream);

/* replaces RasterizeMeshesNaive, rasterize_meshes.h:108-156 (_C._rasterize_meshes_naive). */
int p3d_rasterize_meshes_naive(const float* face_verts, const int64_t* mesh_to_face_first_idx,
                               const int64_t* num_faces_per_mesh, const int64_t* clipped_faces_neighbor_idx, int64_t F,
                               int N, int H, int W, float blur_radius, int faces_per_pixel, int perspective_correct,
                               int clip_barycentric_coords, int cull_backfaces, int64_t* pix_to_face, float* zbuf,
                               float* bary, float* dists, p3d_stream_t stream);

/* replaces RasterizeMeshesCoarse, rasterize_meshes.h:292-329 (_C._rasterize_meshes_coarse).
 * bin_faces (N,BH,BW,M) i32, -1 padded, each bin's list ascending; a bin with more than M faces keeps
 * its first M (the reference drops an unspecified subset, rasterize_coarse.cu:186-201). */
int p3d_rasterize_meshes_coarse(const float* face_verts, const int64_t* mesh_to_face_first_idx,
                                const int64_t* num_faces_per_mesh, int64_t F, int N, int H, int W, float blur_radius,
                                int bin_size, int max_faces_per_bin, int32_t* bin_faces, void* workspace,
                                size_t workspace_bytes, p3d_stream_t stream);

/* Scratch bytes for p3d_rasterize_meshes_fine / p3d_rasterize_points_fine. */
size_t p3d_rasterize_fine_workspace_bytes(int N, int BH, int BW, int M);

/* replaces RasterizeMeshesFine, rasterize_meshes.h:406-441 (_C._rasterize_meshes_fine).
 * bin_faces (N,BH,BW,M) i32 with -1 sentinels anywhere. */
int p3d_rasterize_meshes_fine(const float* face_verts, const int32_t* bin_faces,
                              const int64_t* clipped_faces_neighbor_idx, int64_t F, int N, int BH, int BW, int M, int H,
                              int W, float blur_radius, int bin_size, int faces_per_pixel, int perspective_correct,
                              int clip_barycentric_coords, int cull_backfaces, int64_t* pix_to_face, float* zbuf,
                              float* bary, float* dists, void* workspace, size_t workspace_bytes, p3d_stream_t stream);

/* replaces RasterizeMeshesBackward, rasterize_meshes.h:211-252 (_C.rasterize_meshes_backward).
 * grad_face_verts (F,3,3) f32 is zeroed and accumulated here.  = p3d_rasterize_meshes_backward_ex(no faces, no records, no
 * cover, flags 0). */
int p3d_rasterize_meshes_backward(const float* face_verts, const int64_t* pix_to_face, const float* grad_zbuf,
                                  const float* grad_bary, const float* grad_dists, int64_t F, int N, int H, int W, int K,
                                  int perspective_correct, int clip_barycentric_coords, float* grad_face_verts,
                                  p3d_stream_t stream);

/* ---- the forward with what it can tell the backward, and the backward that uses it ------------------------------------
 *
 * Row cover (round 3).  The reference's autograd node saves pix_to_face for the backward (renderer/mesh/rasterize_meshes.py:
 * 291-296) and the backward kernel reads all N*H*W*K entries of it to find the samples that hold a face (rasterize_meshes.cu:
 * 593-603).  At the bench workload 68 % of those reads find nothing.  The forward can say so for free: `cover` is (N, ceil(H/16),
 * ceil(W/16)) int32; bit r of word (n, cy, cx) is set iff some pixel of output row 16*cy + r, columns 16*cx .. 16*cx+15 of
 * image n holds a face (pix_to_face[n, y, x, 0] >= 0).  The autograd nodes of pytorch3d_amd/rasterize_meshes.py save it
 * next to pix_to_face; a backward without cover (the `_C.rasterize_meshes_backward` drop-in) reads everything, as before.
 * The backward TRUSTS the cover: a clear bit skips the row without looking. */
size_t p3d_rasterize_meshes_cover_bytes(int N, int H, int W);

/* Is `cover` still the cover of `pix_to_face`?  *stale (one int32 on the device, written here) becomes non-zero iff some 16-pixel
 * row segment holds a face the cover does not know of -- the one way a cover can make the backward wrong (a set bit over an
 * empty segment only costs time).  For callers that cannot rule out writes into pix_to_face between the forward and the
 * backward (pytorch3d_amd._C with P3D_CHECK=1: tensors edited through `.data`); reads slot 0 of every pixel, ~0.2 ms at the
 * bench size -- about half of what the cover saves.  The reference has no counterpart (its backward reads every entry). */
int p3d_rasterize_meshes_cover_check(const int64_t* pix_to_face, const int32_t* cover, int N, int H, int W, int K, int32_t* stale,
                                     p3d_stream_t stream);

/* Cover list (round 6): a buffer of p3d_rasterize_meshes_cover_list_bytes holds the (N, ceil(H/16), ceil(W/16)) words of the
 * cover as above, an int32 counter (+ 15 spare), then room for one int32 per word.  The wave that sets the first bit of a word
 * appends the word's index to the list (one atomic per 16 x 16 pixel block that holds a face), so the backward finds its work
 * without a pass over the cover and without a workspace: two kernels fewer than with a plain cover (the list builder
 * mesh_backward_areas and the memset of its counter; 0.02 ms of the 2.3 ms bench step).  The words in front are a plain cover:
 * the buffer may be handed to every function that takes `cover`.  The list's order is the order in which the forward's tiles
 * finished.
 * When the forward's tiles are the words of the cover (binned, image sides multiples of 16, at most 512 pixels a side, a full
 * workspace) the list is filled from the tile plan of the coarse stage instead, without atomics: it then holds the word of EVERY
 * tile whose bin list holds a face, in the order the forward walks them (longest list first, or image order for small launches),
 * and the counter is the number of those tiles.  The list is then the list of the active tiles in walk order, including tiles whose
 * word is 0: a superset of the non-empty words -- a tile whose faces reach no pixel centre is listed with a word that ends up 0
 * (the backward finds no row there and returns).  No word is listed twice.
 * The words and the counter need no clearing by the caller: binned launches clear them in the first pass of the coarse stage, the
 * others with a memset. */
size_t p3d_rasterize_meshes_cover_list_bytes(int N, int H, int W);

/* flags of p3d_rasterize_meshes_ex (both) and p3d_rasterize_points_ex (P3D_RASTER_CUDA_TIE_ORDER only) */
#define P3D_RASTER_COVER_LIST 1u     /* `cover` is a cover-list buffer: the forward also writes the list behind the words       */
#define P3D_RASTER_CUDA_TIE_ORDER 2u /* the replay of the reference's CUDA tie procedure (below)                                 */

/* CUDA tie order (round 4).  The kernels of this library keep the K nearest faces under the total order (depth, face index), as
 * the reference's CPU and Python implementations do (rasterize_meshes_cpu.cpp:263-288, rasterize_meshes.py); its CUDA kernels keep
 * an unsorted array and replace "the" farthest entry only by a strictly nearer candidate (RasterizeMeshesFineCudaKernel /
 * CheckPixelInsideFace, rasterize_meshes.cu:112-237): the same depths, but among faces of exactly the K-th depth possibly other
 * survivors, depending on array positions, i.e. on the pixel's whole history (2 in 10^4 entries of the bench launch; zbuf is
 * bit-equal either way).  With P3D_RASTER_CUDA_TIE_ORDER the fine kernel marks the pixels in which the two procedures can differ
 * (an entry dropped at the depth of the last survivor while a nearer survivor has a larger face index; or the clipped-face
 * neighbour rule in play: 2 in 10^3 pixels of the bench launch) and a replay re-runs the reference's procedure, faces in
 * ascending index, for those: pix_to_face (and the rows that go with it) become what the reference's CUDA kernels return.  1.2 x
 * the time of p3d_rasterize_meshes on the bench batch (round 4: ~10 x).  The marks take the LAST N * ceil(H/8) * ceil(W/8) * 8
 * bytes (rounded up to 256) of the workspace when it is at least that much larger than the binning needs
 * (p3d_rasterize_meshes_workspace_bytes counts them in; a caller of the short-workspace size adds them); without that room the
 * replay finds the marks in the output itself (one pix_to_face entry of every pixel is read).  Diagnostic: with
 * P3D_TIE_SKIP_REPLAY set in the environment the replay is skipped and the marks (-2) stay in pix_to_face
 * (profiles/tie_order_timing.py --count-marks). */

/* clipped_faces_neighbor_idx of p3d_rasterize_meshes_ex, p3d_rasterize_meshes and p3d_rasterize_meshes_naive may be NULL: "no
 * face has a clipped neighbour", the same as F entries of -1 without the array, its fill and the 8 bytes the fine kernel gathers
 * of it per (tile, face).  p3d_rasterize_meshes_fine keeps requiring it.
 *
 * p3d_rasterize_meshes + the row cover of its output.  cover: p3d_rasterize_meshes_cover_bytes, or with P3D_RASTER_COVER_LIST a
 * p3d_rasterize_meshes_cover_list_bytes buffer; null: no cover (flags may then not hold P3D_RASTER_COVER_LIST).  Unknown bits,
 * or P3D_RASTER_CUDA_TIE_ORDER together with P3D_RASTER_COVER_LIST (a combination no caller reaches): P3D_ERR_INVALID_ARG.
 * Short workspaces are accepted (above). */
int p3d_rasterize_meshes_ex(const float* face_verts, const int64_t* mesh_to_face_first_idx, const int64_t* num_faces_per_mesh,
                            const int64_t* clipped_faces_neighbor_idx, int64_t F, int N, int H, int W, float blur_radius,
                            int faces_per_pixel, int bin_size, int max_faces_per_bin, int perspective_correct,
                            int clip_barycentric_coords, int cull_backfaces, int64_t* pix_to_face, float* zbuf, float* bary,
                            float* dists, int32_t* cover, unsigned flags, void* workspace, size_t workspace_bytes,
                            p3d_stream_t stream);

/* p3d_rasterize_meshes_ex on PACKED vertices: `face_verts = verts_packed[faces_packed]` (p3d_gather_face_verts[_pre] below, the same
 * index rules and the same bytes) is part of the call.  verts (V,3) f32, faces (F,3) i64 are read; face_verts (F,3,3) f32 and, when
 * not null, face_pre (F,4) f32 (16-byte aligned; the records of p3d_gather_face_verts_pre) are WRITTEN, for the caller's backward.
 * zero_verts: null, or (V,3) f32 that the call sets to zero -- the grad_out of the p3d_rasterize_meshes_backward_ex that follows,
 * handed over with P3D_BWD_GRAD_OUT_ZEROED.  Everything else as p3d_rasterize_meshes_ex, with the same results bit for bit.
 * A binned launch does all three inside the first pass of the coarse stage (the thread that forms a face's bin rectangle gathers
 * the face; the workgroups clear zero_verts and the cover as they start): no launch and no memset of their own.  It writes
 * face_verts / face_pre for every face inside a mesh's range [first, first + count) -- the faces a rasterization can return; faces
 * of the packed array that belong to no mesh are left as they were.  Naive launches (bin_size or max_faces_per_bin 0) and empty
 * outputs run the stand-alone gather and a memset first.
 * Refused before anything is launched (P3D_ERR_INVALID_ARG): unknown flag bits, V < 0, F < 0, F > 0 with a null verts, faces or
 * face_verts, a face_pre without face_verts or not 16-byte aligned. */
int p3d_rasterize_meshes_verts_ex(const float* verts, const int64_t* faces, int64_t V, float* face_verts, float* face_pre,
                                  float* zero_verts, const int64_t* mesh_to_face_first_idx, const int64_t* num_faces_per_mesh,
                                  const int64_t* clipped_faces_neighbor_idx, int64_t F, int N, int H, int W, float blur_radius,
                                  int faces_per_pixel, int bin_size, int max_faces_per_bin, int perspective_correct,
                                  int clip_barycentric_coords, int cull_backfaces, int64_t* pix_to_face, float* zbuf, float* bary,
                                  float* dists, int32_t* cover, unsigned flags, void* workspace, size_t workspace_bytes,
                                  p3d_stream_t stream);

/* Per-face records (round 6; the reference has no counterpart: its backward re-derives them per sample, geometry_utils.cuh:
 * 101-161, 365-385): face_pre (F, 4) f32, 16-byte aligned: 1 / (barycentric area), 1 / |v1 - v0|^2, 1 / |v2 - v0|^2,
 * 1 / |v2 - v1|^2 (-1 where the squared length is <= 1e-8: the degenerate-edge rule).  p3d_gather_face_verts_pre is
 * p3d_gather_face_verts with a thread per face that also writes them.  They belong to THOSE face_verts. */
int p3d_gather_face_verts_pre(const float* verts, const int64_t* faces, int64_t V, int64_t F, float* face_verts, float* face_pre,
                              p3d_stream_t stream);

/* Scratch of a backward with a plain cover: room for the list of covered 16 x 16 areas (built by mesh_backward_areas), so
 * that the launch holds only workgroups with work -- workgroups reach the CUs round robin, and a mix of empty and full ones
 * leaves CUs idle.  Without it (workspace null or smaller) the launch spans every area. */
size_t p3d_rasterize_meshes_backward_workspace_bytes(int N, int H, int W);

/* flags of p3d_rasterize_meshes_backward_ex */
#define P3D_BWD_COVER_HAS_LIST 1u /* `cover` is the front of a cover-list buffer: take the list, ignore the workspace            */
#define P3D_BWD_MAKE_FACE_PRE 2u  /* face_pre is scratch (F x 4 f32) that this call fills first with one small launch            */
#define P3D_BWD_GRAD_OUT_ZEROED 8u /* grad_out holds zeros already (p3d_rasterize_meshes_verts_ex: zero_verts): no memset here    */

/* The backward of p3d_rasterize_meshes[_ex].  faces null: grad_out is grad_face_verts (F,3,3).  faces (F,3) i64: grad_out is the
 * gradient of `face_verts = verts_packed[faces_packed]` (rasterize_meshes.py:146, torch indexing + its index_put backward)
 * fused in, grad_verts (V,3): the per-face partials are flushed straight to the vertices -- no (F,3,3) intermediate, no
 * separate scatter.  grad_out is zeroed (unless P3D_BWD_GRAD_OUT_ZEROED says it is) and accumulated here.
 * cover: the cover of THAT pix_to_face, or null (every row is read).
 * face_pre: per-face records (above), or null (formed per sample).  Without P3D_BWD_MAKE_FACE_PRE they are read as
 * p3d_gather_face_verts_pre wrote them.  Records are used by the launches with perspective_correct && clip_barycentric_coords
 * && K in {4, 8} only (P3D_BWD_MAKE_FACE_PRE launches nothing otherwise).
 * Unknown flag bits or a face_pre that is not 16-byte aligned: P3D_ERR_INVALID_ARG. */
int p3d_rasterize_meshes_backward_ex(const float* face_verts, const int64_t* faces, float* face_pre,
                                     const int64_t* pix_to_face, const float* grad_zbuf, const float* grad_bary,
                                     const float* grad_dists, const int32_t* cover, int64_t F, int64_t V, int N, int H, int W,
                                     int K, int perspective_correct, int clip_barycentric_coords, unsigned flags,
                                     float* grad_out, void* workspace, size_t workspace_bytes, p3d_stream_t stream);

/* ---- packed vertices <-> per-face vertices (optional fast path of the L2 function) ------ */

/* replaces the Python-side gather `face_verts = verts_packed[faces_packed]`
 * (pytorch3d/renderer/mesh/rasterize_meshes.py:144-148): verts (V,3) f32, faces (F,3) i64 -> face_verts (F,3,3). */
int p3d_gather_face_verts(const float* verts, const int64_t* faces, int64_t V, int64_t F, float* face_verts,
                          p3d_stream_t stream);
/* its autograd backward (torch: index_put_ accumulate, a sort on ROCm): grad_verts (V,3) is zeroed and
 * accumulated here with f32 atomics (order not deterministic). */
int p3d_scatter_face_grads(const float* grad_face_verts, const int64_t* faces, int64_t V, int64_t F, float* grad_verts,
                           p3d_stream_t stream);

/* ---- face areas / normals and vertex normals (csrc/normals.hip) -------------------------------- */

/* `_C.face_areas_normals_forward` (face_areas_normals.cu:14-70): verts (V,3) f32, faces (F,3) i64 -> areas (F), normals (F,3);
 * c = (v1 - v0) x (v2 - v0), area = |c| / 2, normal = c / max(|c|, 1e-6), IEEE sqrt and division.  Vertex ids as
 * p3d_gather_face_verts reads them: a negative id wraps once, an id still out of range makes the face NaN and nothing outside
 * `verts` is read (V == 0: every face NaN, by a fill). */
int p3d_face_areas_normals_forward(const float* verts, const int64_t* faces, int64_t V, int64_t F, float* areas, float* normals,
                                   p3d_stream_t stream);
/* Its backward up to the scatter: grad_face_verts (F,3,3), the gradient per corner, every element written; finish with
 * p3d_scatter_face_grads or p3d_scatter_face_grads_ordered.  The reference's derivative, its c_x-for-c_y term in d/d(v1.z)
 * (face_areas_normals.cu:183-184) included. */
int p3d_face_areas_normals_backward(const float* grad_areas, const float* grad_normals, const float* verts, const int64_t* faces,
                                    int64_t V, int64_t F, float* grad_face_verts, p3d_stream_t stream);

/* Area-weighted vertex normals (structures/meshes.py:884-926) in gather form: no float atomics, the same bits on every run.
 * The caller builds the incidence list once per topology: corners (offsets[V] <= 3 F entries) i32, the corners c = 3 f + j whose
 * vertex lies in [0, V) (negative ids wrap once), sorted STABLY by vertex; offsets (V + 1) i32, vertex v owns
 * corners[offsets[v] .. offsets[v + 1]).  3 F must fit an int32.  A list that breaks this gives wrong sums, never an access
 * outside the rows (offsets are clamped to [0, 3 F], corner ids outside [0, 3 F) skipped; `corners` must hold offsets[V] entries).
 *   forward: face_raw (F,3) workspace (p3d_verts_normals_forward_workspace_bytes) <- (v2 - v1) x (v0 - v1) per face;
 *     sums (V,3) <- +0 plus face_raw[corner / 3] over the vertex's corners in list order; normals (V,3) <- sums / max(|sums|, 1e-6).
 *     A vertex without a face gets zeros.  Keep `sums` for the backward.
 *   backward: face_rows (F,3,3) workspace (p3d_verts_normals_backward_workspace_bytes) <- per face the gradient of its three
 *     vertices through the normalisation ((g - n (n.g)) / |s| where |s| > 1e-6, g / 1e-6 where it is not) summed in corner order
 *     and taken through the cross product; grad_verts (V,3) <- the rows of the vertex's corners summed in list order.
 * Every output row is written; nothing is read before it is written. */
size_t p3d_verts_normals_forward_workspace_bytes(int64_t F);
size_t p3d_verts_normals_backward_workspace_bytes(int64_t F);
int p3d_verts_normals_forward(const float* verts, const int64_t* faces, const int32_t* offsets, const int32_t* corners, int64_t V,
                              int64_t F, float* face_raw, float* sums, float* normals, p3d_stream_t stream);
int p3d_verts_normals_backward(const float* grad_normals, const float* verts, const int64_t* faces, const float* sums,
                               const int32_t* offsets, const int32_t* corners, int64_t V, int64_t F, float* face_rows,
                               float* grad_verts, p3d_stream_t stream);

/* ---- mesh regularisers: edge loss, uniform Laplacian, normal consistency (pytorch3d/loss/mesh_*.py) --------------
 *
 * Gather kernels over int32 tables the caller builds once per topology (pytorch3d_amd/mesh_losses.py: mesh_loss_topology):
 *   edges (E,2): the unique undirected edges (lo, hi) in packed vertex ids; edge_mesh (E), vert_mesh (V), pair_mesh (P): the mesh of
 *   each; num_edges / num_verts / num_pairs (N): the counts per mesh (a term's weight is 1.0f / count of its mesh);
 *   adj_offsets (V + 1), adj (2 E): the vertex adjacency as a CSR, the neighbours of a vertex ascending;
 *   pairs (P,4): the wing pairs (v0, v1, a, b) of normal consistency -- (v0, v1) an edge, a and b the vertices opposite it on two
 *   of its faces; offsets (V + 1), slots (4 P): per vertex the slots 4 pair + role that name it, sorted stably by vertex.
 * 4 P, 2 E and V must fit an int32; N > 0.  loss: ONE float, (sum of the terms) / N.  grad_loss: ONE float on the device.
 * No float atomics: every sum of n terms is the fixed tree of csrc/fixed_sum.h over blocks of 256 terms, of depth
 *   D(n) = 8 + ceil(ceil(n / 256) / 256) + 8,
 * so a loss and its gradient have the same bits on every run and stream.  Forward workspaces hold one
 * partial sum per 256 terms; every byte that is read was written by the same call.  A table that breaks its contract gives NaN
 * or wrong numbers, never an access outside the arrays (ids are range-checked, CSR offsets clamped). */
size_t p3d_mesh_edge_loss_forward_workspace_bytes(int64_t E);
size_t p3d_mesh_laplacian_forward_workspace_bytes(int64_t V);
size_t p3d_mesh_normal_consistency_forward_workspace_bytes(int64_t P);
size_t p3d_mesh_normal_consistency_backward_workspace_bytes(int64_t P);
/* term_e = (|x_lo - x_hi| - target_length)^2 * weight (mesh_edge_loss.py:47-52) */
int p3d_mesh_edge_loss_forward(const float* verts, const int32_t* edges, const int32_t* edge_mesh, const int32_t* num_edges, int64_t V,
                               int64_t E, int N, float target_length, void* workspace, size_t workspace_bytes, float* loss,
                               p3d_stream_t stream);
/* grad_verts (V,3), every row written: one lane per vertex walks its row of adj; 0 from an edge of length 0 (torch's norm backward) */
int p3d_mesh_edge_loss_backward(const float* grad_loss, const float* verts, const int32_t* adj_offsets, const int32_t* adj,
                                const int32_t* vert_mesh, const int32_t* num_edges, int64_t V, int64_t E, int N, float target_length,
                                float* grad_verts, p3d_stream_t stream);
/* mesh_laplacian_smoothing, method "uniform": r_v = (sum of the neighbours) / deg(v) - x_v (the sum term 0 for deg 0),
 * term_v = |r_v| * weight; q (V,3) <- r_v weight / |r_v| (0 where the norm is 0), kept for the backward */
int p3d_mesh_laplacian_forward(const float* verts, const int32_t* adj_offsets, const int32_t* adj, const int32_t* vert_mesh,
                               const int32_t* num_verts, int64_t V, int64_t E, int N, float* q, void* workspace, size_t workspace_bytes,
                               float* loss, p3d_stream_t stream);
/* grad_verts_v = (grad_loss / N) (sum over adj(v) of q_u / deg(u) - q_v) */
int p3d_mesh_laplacian_backward(const float* grad_loss, const float* q, const int32_t* adj_offsets, const int32_t* adj, int64_t V, int64_t E,
                                int N, float* grad_verts, p3d_stream_t stream);
/* term_p = (1 - cos(n0, n1)) * weight with n0 = (x_v1 - x_v0) x (x_a - x_v0), n1 = -(x_v1 - x_v0) x (x_b - x_v0) and the cosine of
 * torch.cosine_similarity(eps=1e-8): (n0 / max(|n0|, eps)) . (n1 / max(|n1|, eps)) */
int p3d_mesh_normal_consistency_forward(const float* verts, const int32_t* pairs, const int32_t* pair_mesh, const int32_t* num_pairs,
                                        int64_t V, int64_t P, int N, void* workspace, size_t workspace_bytes, float* loss,
                                        p3d_stream_t stream);
/* workspace: (P,4,3) f32, the gradient of each pair to its four vertices; grad_verts (V,3) <- the rows of the vertex's slots summed
 * in list order, every row written */
int p3d_mesh_normal_consistency_backward(const float* grad_loss, const float* verts, const int32_t* pairs, const int32_t* pair_mesh,
                                         const int32_t* num_pairs, const int32_t* offsets, const int32_t* slots, int64_t V, int64_t P,
                                         int N, void* workspace, size_t workspace_bytes, float* grad_verts, p3d_stream_t stream);

/* ---- world -> NDC vertex transform fused into the gather ---------------- */

/* replaces MeshRasterizer.transform (pytorch3d/renderer/mesh/rasterizer.py:171-216: two batched 4x4 transform_points
 * with homogeneous divides on padded vertices, z taken from view space) + the gather `verts_packed[faces_packed]`
 * (renderer/mesh/rasterize_meshes.py:144-148) by ONE launch: verts_world (V,3) f32, faces (F,3) i64 packed,
 * mesh_to_face_first_idx (N) i64, matrices (num_matrices,2,4,4) f32 row-major in the reference's row-vector convention
 * ([.][0] world->view, [.][1] view->NDC), num_matrices = N or 1 -> face_verts (F,3,3) in NDC (x, y) + view depth. */
int p3d_transform_gather_face_verts(const float* verts_world, const int64_t* faces, const int64_t* mesh_to_face_first_idx,
                                    const float* matrices, int64_t V, int64_t F, int N, int num_matrices, float* face_verts,
                                    p3d_stream_t stream);
/* the same transform per packed vertex (for callers that need the NDC vertices themselves) ... */
int p3d_transform_verts_forward(const float* verts_world, const int64_t* mesh_to_vert_first_idx, const float* matrices,
                                int64_t V, int N, int num_matrices, float* verts_ndc, p3d_stream_t stream);
/* ... and its backward: grad_verts_world (V,3) = J^T grad_verts_ndc (V,3), i.e. what torch autograd computes through the
 * two transform_points calls; applied to the grad_verts of p3d_rasterize_meshes_backward_ex it gives the gradient of the
 * rasterization wrt world-space vertices. */
int p3d_transform_verts_backward(const float* verts_world, const int64_t* mesh_to_vert_first_idx, const float* matrices,
                                 const float* grad_verts_ndc, int64_t V, int N, int num_matrices, float* grad_verts_world,
                                 p3d_stream_t stream);
/* The same backward with the gradient of the CAMERAS: grad_matrices (num_matrices,2,4,4), the layout of `matrices`, fully written:
 *   grad_matrices[n][0][i][j] = sum_v (x, y, z, 1)_i * dL/d((p, 1) @ A)_j,   grad_matrices[n][1][i][j] = sum_v (view, 1)_i * dL/d((view, 1) @ B)_j
 * over the vertices that share matrix n (mesh n, or all of them when num_matrices == 1); a mesh without vertices gets zeros, and
 * column j = 2 of the second matrix is exactly 0 (the depth is taken from view space).  A two-stage segmented sum without float
 * atomics: the same input gives the same bits on every run and stream.  grad_verts_world (V,3) comes from the same pass, bit-equal
 * to p3d_transform_verts_backward's, or is skipped when NULL.  workspace: at least p3d_transform_backward_workspace_bytes(...)
 * bytes, 16-byte aligned (a shorter one: P3D_ERR_INVALID_ARG, nothing is launched); V == 0: zeros, no launch, no workspace. */
size_t p3d_transform_backward_workspace_bytes(int64_t V, int N, int num_matrices);
int p3d_transform_backward_cameras(const float* verts_world, const int64_t* mesh_to_vert_first_idx, const float* matrices,
                                   const float* grad_verts_ndc, int64_t V, int N, int num_matrices, float* grad_verts_world,
                                   float* grad_matrices, void* workspace, size_t workspace_bytes, p3d_stream_t stream);

/* ---- point clouds -------------------------------------------------------------------- */

size_t p3d_rasterize_points_workspace_bytes(int64_t P, int N, int H, int W, int bin_size, int max_points_per_bin);
size_t p3d_rasterize_points_short_workspace_bytes(int64_t P, int N, int H, int W, int bin_size, int max_points_per_bin,
                                                  int64_t list_entries);
size_t p3d_rasterize_points_workspace_need_offset(int64_t P, int N, int H, int W, int bin_size, int max_points_per_bin);

/* The point forward.  Outputs idxs (N,H,W,K) i32, zbuf, dists (squared) f32; bin_size == 0 or max_points_per_bin == 0 -> naive
 * path, else coarse binning + fine rasterization.
 *   Short workspaces, exactly as for the meshes (above): any workspace of at least p3d_rasterize_points_short_workspace_bytes(...,
 *     0) bytes is accepted, the lists take what is left, the device decides whether they fit and the naive kernel writes the same
 *     outputs when they do not.  (1M points, 512 x 512, max_points_per_bin = P / 5: worst case 0.8 GB for one cloud, 1.3 M entries
 *     = 5 MB needed.)
 *   flags: 0 or P3D_RASTER_CUDA_TIE_ORDER.  The reference's point kernels keep the same unsorted array as its mesh kernels
 *     (rasterize_points.cu:38-84) and sort it by depth ALONE (rasterize_points.cu:26-28, stable): where points tie exactly in depth,
 *     the survivors at the K-th place and the order of the tied entries follow the array positions.  With the flag a replay re-runs
 *     that procedure, points in ascending index, for every pixel whose K slots are full.
 *   images non-null: PointsRenderer's chain in the same call (round 6; renderer/points/renderer.py:56-76: fragments =
 *     rasterize_points(...), weights = 1 - dists / r^2, images = alpha_composite(idx, weights, features); the reference has no
 *     single operator for it, the patched PointsRenderer (pytorch3d_amd.shim) and pytorch3d_amd.render_points use it).  images
 *     (N, H, W, C) f32 = the compositing of features (P, C) f32 rows, C in 1..4, with alpha = 1 - dists * inv_r2, inv_r2 =
 *     float(1) / float(r * r) (how torch evaluates `dists / (r * r)`); composite_mode P3D_COMPOSITE_ALPHA (AlphaCompositor,
 *     alpha_composite.cu:24-68) or P3D_COMPOSITE_NORM_SUM (NormWeightedCompositor, norm_weighted_sum.cu:24-154; the constants are
 *     defined with the compositing operators below).  The pixel is formed in the fine kernel's epilogue while its K entries are in
 *     LDS (K <= 28, binned; with a short workspace whose lists did not fit: by a pass behind the stand-by kernel, decided on the
 *     device), else by a pass behind the rasterizer.  Bit-equal to the three operators run one after the other.  images null:
 *     composite_mode, features, C and inv_r2 are ignored.
 * Unknown flag bits, P3D_RASTER_COVER_LIST, or P3D_RASTER_CUDA_TIE_ORDER together with images: P3D_ERR_INVALID_ARG. */
int p3d_rasterize_points_ex(const float* points, const int64_t* cloud_to_packed_first_idx, const int64_t* num_points_per_cloud,
                            const float* radius, int64_t P, int N, int H, int W, int points_per_pixel, int bin_size,
                            int max_points_per_bin, int32_t* idxs, float* zbuf, float* dists, int composite_mode,
                            const float* features, int C, float inv_r2, float* images, unsigned flags, void* workspace,
                            size_t workspace_bytes, p3d_stream_t stream);

/* replaces RasterizePoints, pytorch3d/csrc/rasterize_points/rasterize_points.h:343-374 (_C.rasterize_points).
 * = p3d_rasterize_points_ex(no images, flags 0). */
int p3d_rasterize_points(const float* points, const int64_t* cloud_to_packed_first_idx,
                         const int64_t* num_points_per_cloud, const float* radius, int64_t P, int N, int H, int W,
                         int points_per_pixel, int bin_size, int max_points_per_bin, int32_t* idxs, float* zbuf,
                         float* dists, void* workspace, size_t workspace_bytes, p3d_stream_t stream);

/* replaces RasterizePointsNaive, rasterize_points.h:70-99 (_C._rasterize_points_naive). */
int p3d_rasterize_points_naive(const float* points, const int64_t* cloud_to_packed_first_idx,
                               const int64_t* num_points_per_cloud, const float* radius, int64_t P, int N, int H, int W,
                               int points_per_pixel, int32_t* idxs, float* zbuf, float* dists, p3d_stream_t stream);

/* replaces RasterizePointsCoarse, rasterize_points.h:146-191 (_C._rasterize_points_coarse). */
int p3d_rasterize_points_coarse(const float* points, const int64_t* cloud_to_packed_first_idx,
                                const int64_t* num_points_per_cloud, const float* radius, int64_t P, int N, int H, int W,
                                int bin_size, int max_points_per_bin, int32_t* bin_points, void* workspace,
                                size_t workspace_bytes, p3d_stream_t stream);

/* replaces RasterizePointsFine, rasterize_points.h:222-247. */
int p3d_rasterize_points_fine(const float* points, const int32_t* bin_points, const float* radius, int64_t P, int N,
                              int BH, int BW, int M, int H, int W, int bin_size, int points_per_pixel, int32_t* idxs,
                              float* zbuf, float* dists, void* workspace, size_t workspace_bytes, p3d_stream_t stream);

/* The backward of p3d_rasterize_points_ex with images: grad_points (P, 3) [z column zero: the chain does not expose zbuf] and
 * grad_features (P, C), both fully written, from grad_images (N, H, W, C): alphaCompositeCudaBackwardKernel (alpha_composite.cu:72-141),
 * grad_dists = -grad_alphas * inv_r2 and RasterizePointsBackwardCudaKernel (rasterize_points.cu:366-411) as ONE kernel whose two
 * scatters share a wave-private table.  K <= 16, C in 1..4 (P3D_ERR_INVALID_ARG otherwise: run the three operators instead). */
int p3d_rasterize_points_composite_backward(int mode, const float* points, const float* features, const int32_t* idxs,
                                            const float* dists, const float* grad_images, int64_t P, int C, int N, int H, int W,
                                            int points_per_pixel, float inv_r2, float* grad_points, float* grad_features,
                                            p3d_stream_t stream);

/* replaces RasterizePointsBackward, rasterize_points.h:281-305 (_C.rasterize_points_backward). */
int p3d_rasterize_points_backward(const float* points, const int32_t* idxs, const float* grad_zbuf,
                                  const float* grad_dists, int64_t P, int N, int H, int W, int K, float* grad_points,
                                  p3d_stream_t stream);

/* ---- compositors --------------------------------------------------------------------- */

#define P3D_COMPOSITE_ALPHA 0    /* alphaComposite*,  compositing/alpha_composite.h:59-115    */
#define P3D_COMPOSITE_NORM_SUM 1 /* weightedSumNorm*, compositing/norm_weighted_sum.h:57-115  */
#define P3D_COMPOSITE_SUM 2      /* weightedSum*,     compositing/weighted_sum.h:55-111       */

/* alphas / points_idx are logically (N,K,H,W) and addressed through element strides (so the permuted (N,H,W,K) views the renderers
 * pass need no copy); result (N,C,H,W) f32 contiguous.  features are logically (C,P) f32, addressed through the element strides
 * (channel, point) of feature_strides: (P, 1) is the contiguous (C,P) tensor of the reference's operators, (1, C) the transposed
 * view of a (P, C) tensor -- what PointsRenderer passes (renderer/points/renderer.py:67: `features_packed().permute(1, 0)`; the
 * reference's launchers copy it to (C,P) first, compositing/alpha_composite.h:63-65).  With (1, C) a point's channels share a cache
 * line: the gathers of a pixel cost one memory request per entry instead of C.  Null strides: (P, 1).  Any other layout:
 * P3D_ERR_INVALID_ARG. */
int p3d_composite_forward(int mode, const float* features, const int64_t feature_strides[2], const float* alphas,
                          const int64_t* points_idx, int N, int C, int64_t P, int K, int H, int W, const int64_t alphas_strides[4],
                          const int64_t idx_strides[4], float* result, p3d_stream_t stream);

/* grad_alphas (N,K,H,W) contiguous and grad_features (C * P floats of one allocation in the layout grad_feature_strides names, null:
 * (P, 1)), both fully written. */
int p3d_composite_backward(int mode, const float* grad_outputs, const float* features, const int64_t feature_strides[2],
                           const float* alphas, const int64_t* points_idx, int N, int C, int64_t P, int K, int H, int W,
                           const int64_t alphas_strides[4], const int64_t idx_strides[4], float* grad_features,
                           const int64_t grad_feature_strides[2], float* grad_alphas, p3d_stream_t stream);

/* ---- interpolate_face_attributes ----------------------------------------------------- */

/* replaces InterpFaceAttrsForward/Backward, pytorch3d/csrc/interp_face_attrs/interp_face_attrs.h:46-116.
 * dtype: 0 = f32, 1 = f64 (the reference dispatches both).  pix_attrs (P,D) fully written. */
int p3d_interp_face_attrs_forward(int dtype, const int64_t* pix_to_face, const void* barycentric_coords,
                                  const void* face_attrs, int64_t P, int64_t F, int64_t D, void* pix_attrs,
                                  p3d_stream_t stream);
int p3d_interp_face_attrs_backward(int dtype, const int64_t* pix_to_face, const void* barycentric_coords,
                                   const void* face_attrs, const void* grad_pix_attrs, int64_t P, int64_t F, int64_t D,
                                   void* grad_barycentric_coords, void* grad_face_attrs, p3d_stream_t stream);

/* ---- frustum culling / z-plane clipping before rasterization, un-clipping after -------- */

/* Together these replace clip_faces and convert_clipped_rasterization_to_original_faces,
 * pytorch3d/renderer/mesh/clip.py:324-615, 618-734 (pure torch in the reference).
 *
 * plan:  classify every face (1 kept, 2 removed, 3 clipped to one triangle, 4 clipped to two) and scan the
 *        destination indices.  `plan` is caller-allocated scratch of p3d_clip_faces_plan_bytes(F) that must stay
 *        alive until emit / backward; its first four int64 receive {F_clipped, T3, T4, F} -- read them (one sync,
 *        as in the reference) to size the outputs.  planes = {left, right, top, bottom, znear, zfar}, bit i of
 *        plane_mask set when plane i is used; cull as ClipFrustum.cull.
 * emit:  face_verts_clipped (F_clipped,3,3), mesh_to_face_first_idx / num_faces_per_mesh (N),
 *        faces_clipped_to_unclipped_idx (F_clipped); when T3 + T4 > 0 also barycentric_conversion (T3 + 2*T4,3,3),
 *        faces_clipped_to_conversion_idx and clipped_faces_neighbor_idx (F_clipped).
 * backward: gradient of (face_verts_clipped, barycentric_conversion) w.r.t. face_verts, with the reference's
 *        autograd semantics (w3 detached, clip.py:291). */
size_t p3d_clip_faces_plan_bytes(int64_t F);
int p3d_clip_faces_plan(const float* face_verts, int64_t F, const float planes[6], int plane_mask, int cull,
                        int has_z_clip, float z_clip_value, void* plan, size_t plan_bytes, p3d_stream_t stream);
int p3d_clip_faces_emit(const float* face_verts, int64_t F, const int64_t* mesh_to_face_first_idx, int N,
                        const void* plan, size_t plan_bytes, int64_t F_clipped, int64_t T3, int64_t T4,
                        float z_clip_value, int perspective_correct, float* face_verts_clipped,
                        int64_t* mesh_to_face_first_idx_clipped, int64_t* num_faces_per_mesh_clipped,
                        int64_t* faces_clipped_to_unclipped_idx, float* barycentric_conversion,
                        int64_t* faces_clipped_to_conversion_idx, int64_t* clipped_faces_neighbor_idx,
                        p3d_stream_t stream);
int p3d_clip_faces_backward(const float* face_verts, int64_t F, const void* plan, size_t plan_bytes, int64_t T3,
                            int64_t T4, float z_clip_value, int perspective_correct,
                            const float* grad_face_verts_clipped, const float* grad_barycentric_conversion,
                            float* grad_face_verts, p3d_stream_t stream);
/* pix_to_face (S) / bary (S,3) of the clipped faces -> of the original faces; S = N*H*W*K samples.
 * barycentric_conversion may be null (only culling happened).  Backward: grad_bary_clipped (S,3) fully written,
 * grad_barycentric_conversion (T,3,3) zeroed and accumulated (may be null). */
int p3d_convert_clipped_forward(const int64_t* pix_to_face_clipped, const float* bary_coords_clipped,
                                const int64_t* faces_clipped_to_unclipped_idx, const float* barycentric_conversion,
                                const int64_t* faces_clipped_to_conversion_idx, int64_t num_samples,
                                int64_t* pix_to_face_unclipped, float* bary_coords_unclipped, p3d_stream_t stream);
int p3d_convert_clipped_backward(const int64_t* pix_to_face_clipped, const float* bary_coords_clipped,
                                 const float* barycentric_conversion, const int64_t* faces_clipped_to_conversion_idx,
                                 const float* grad_bary_unclipped, int64_t num_samples, int64_t T,
                                 float* grad_bary_clipped, float* grad_barycentric_conversion, p3d_stream_t stream);

/* ---- fragment blending (the step right after rasterization) --------------------------- */

/* Alignment, for every entry of this section and the depth entries below: the kernels move a pixel's K-row with 16-byte
 * accesses when the row is a multiple of 16 bytes, so the base of such a row must be 16-byte aligned -- pix_to_face (i64) when
 * K % 2 == 0; dists, zbuf, grad_dists, grad_zbuf (f32) and colors, grad_colors (3 f32 per slot) when K % 4 == 0.  The RGBA
 * images out / grad_out of the softmax entries and out of the hard entry are moved as one float4 per pixel: 16-byte aligned
 * for every K.  A base that is not: P3D_ERR_INVALID_ARG, nothing is launched.  (A contiguous torch view at a storage
 * offset is such a base; the Python wrappers copy it first.)  Negative npix / N / pix_per_image / K and a missing pointer
 * are P3D_ERR_INVALID_ARG as well; npix == 0 is P3D_OK without a launch. */

/* replaces SigmoidAlphaBlend / SigmoidAlphaBlendBackward, pytorch3d/csrc/blending/sigmoid_alpha_blend.h:73-103
 * (_C.sigmoid_alpha_blend[_backward]).  dists, pix_to_face (npix,K); alphas, grad_alphas (npix); grad_dists
 * (npix,K) fully written.  npix = N*H*W.  K == 0: the forward writes alphas = 0, the backward is P3D_OK without a launch. */
int p3d_sigmoid_alpha_blend_forward(const float* dists, const int64_t* pix_to_face, float sigma, int64_t npix, int K,
                                    float* alphas, p3d_stream_t stream);
int p3d_sigmoid_alpha_blend_backward(const float* grad_alphas, const float* alphas, const float* dists,
                                     const int64_t* pix_to_face, float sigma, int64_t npix, int K, float* grad_dists,
                                     p3d_stream_t stream);

/* replaces the Python function softmax_rgb_blend (pytorch3d/renderer/blending.py:147-244: ~20 elementwise torch
 * ops over (N,H,W,K)) and its autograd graph.  colors (N*P,K,3), pix_to_face / dists / zbuf (N*P,K) with
 * P = pix_per_image; znear / zfar either the scalars or, when the pointers are non-null, per-image device arrays
 * (N); out (N*P,4) RGBA.  Backward: grad_out (N*P,4) -> grad_colors (N*P,K,3), grad_dists, grad_zbuf (N*P,K). */
int p3d_softmax_rgb_blend_forward(const float* colors, const int64_t* pix_to_face, const float* dists,
                                  const float* zbuf, float sigma, float gamma, const float background[3], float znear,
                                  float zfar, const float* znear_per_image, const float* zfar_per_image, int64_t N,
                                  int64_t pix_per_image, int K, float* out, p3d_stream_t stream);
int p3d_softmax_rgb_blend_backward(const float* grad_out, const float* colors, const int64_t* pix_to_face,
                                   const float* dists, const float* zbuf, float sigma, float gamma,
                                   const float background[3], float znear, float zfar, const float* znear_per_image,
                                   const float* zfar_per_image, int64_t N, int64_t pix_per_image, int K,
                                   float* grad_colors, float* grad_dists, float* grad_zbuf, p3d_stream_t stream);

/* The same backward when the caller knows that the P samples are image-shaped fragments (N,H,W,K) -- what
 * interpolate_face_attributes has before it flattens them (pytorch3d/ops/interp_face_attrs.py:57-63): lanes map to
 * 8x8 pixel tiles instead of 64 consecutive samples.  f32, D <= 4. */
int p3d_interp_face_attrs_backward_nhwk(const int64_t* pix_to_face, const float* barycentric_coords,
                                        const float* face_attrs, const float* grad_pix_attrs, int N, int H, int W, int K,
                                        int64_t F, int D, float* grad_barycentric_coords, float* grad_face_attrs,
                                        p3d_stream_t stream);

/* ---- per-pixel Phong shading of the fragments ------------------------ */

/* replaces the Python function phong_shading (pytorch3d/renderer/mesh/shading.py:59-112: two
 * interpolate_face_attributes calls + lights.diffuse / lights.specular, renderer/lighting.py:17-159, + the colour
 * mix; ~45 torch kernels over (N,H,W,K,3) tensors and their autograd graph) with one kernel each way.
 *   face_attrs (F,3,D): D = 6 -> [vertex xyz | vertex normal] per face corner and `texels` (N,H,W,K,3) given per
 *                       sample (the reference's signature);  D = 9 -> [.. | vertex colour], texels interpolated
 *                       in the kernel (TexturesVertex), `texels` / `grad_texels` unused (may be null).
 *   params (N, P3D_SHADE_PARAM_FLOATS): light ambient, diffuse, specular colour (3 each), light location
 *                       (P3D_LIGHT_POINT) or direction (P3D_LIGHT_DIRECTIONAL), material ambient, diffuse,
 *                       specular colour, shininess, camera centre -- already broadcast to the batch.
 *                       AmbientLights = directional with zero diffuse and specular colour.
 *   colors (N,H,W,K,3) fully written.  Backward: grad_bary (N,H,W,K,3) and grad_texels fully written,
 *   grad_face_attrs (F,3,D) zeroed and accumulated; grad_params (N, P3D_SHADE_PARAM_FLOATS), the gradient of the
 *   lights / materials / camera centre, zeroed and accumulated when non-null (null: not computed). */
#define P3D_SHADE_PARAM_FLOATS 25
#define P3D_LIGHT_DIRECTIONAL 0
#define P3D_LIGHT_POINT 1
int p3d_phong_shade_forward(const int64_t* pix_to_face, const float* bary_coords, const float* face_attrs, int D,
                            const float* texels, const float* params, int light_kind, int N, int H, int W, int K,
                            int64_t F, float* colors, p3d_stream_t stream);
int p3d_phong_shade_backward(const float* grad_colors, const int64_t* pix_to_face, const float* bary_coords,
                             const float* face_attrs, int D, const float* texels, const float* params, int light_kind,
                             int N, int H, int W, int K, int64_t F, float* grad_bary_coords, float* grad_face_attrs,
                             float* grad_texels, float* grad_params, p3d_stream_t stream);

/* ---- SoftPhongShader in one kernel each way: Phong shading fused with softmax_rgb_blend --------------------------------
 *
 * replaces SoftPhongShader.forward (pytorch3d/renderer/mesh/shader.py:113-147): phong_shading (renderer/mesh/shading.py:
 * 100-125) followed by softmax_rgb_blend (renderer/blending.py:147-244).  Same inputs as p3d_phong_shade_* plus the
 * fragments' dists / zbuf and the blend parameters of p3d_softmax_rgb_blend_*; the per-sample colours (N,H,W,K,3) and
 * their gradient never reach memory.  K must be 1, 2, 4, 8 or 16 (p3d_soft_phong_supported_k; other K: run the two
 * operators one after the other), otherwise P3D_ERR_INVALID_ARG.
 *   forward: out (N,H,W,4) RGBA fully written.
 *   backward: grad_out (N,H,W,4) -> grad_bary (N,H,W,K,3), grad_dists, grad_zbuf (N,H,W,K) [and grad_texels (N,H,W,K,3)
 *   with D = 6] fully written; grad_face_attrs (F,3,D) zeroed and accumulated; grad_params (N, 25) zeroed and
 *   accumulated when non-null. */
int p3d_soft_phong_supported_k(int K);
int p3d_soft_phong_forward(const int64_t* pix_to_face, const float* bary_coords, const float* dists, const float* zbuf,
                           const float* face_attrs, int D, const float* texels, const float* params, int light_kind,
                           float sigma, float gamma, const float background[3], float znear, float zfar,
                           const float* znear_per_image, const float* zfar_per_image, int N, int H, int W, int K, int64_t F,
                           float* out, p3d_stream_t stream);
int p3d_soft_phong_backward(const float* grad_out, const int64_t* pix_to_face, const float* bary_coords, const float* dists,
                            const float* zbuf, const float* face_attrs, int D, const float* texels, const float* params,
                            int light_kind, float sigma, float gamma, const float background[3], float znear, float zfar,
                            const float* znear_per_image, const float* zfar_per_image, int N, int H, int W, int K, int64_t F,
                            float* grad_bary, float* grad_dists, float* grad_zbuf, float* grad_face_attrs, float* grad_texels,
                            float* grad_params, p3d_stream_t stream);

/* replaces TexturesUV.sample_textures (pytorch3d/renderer/mesh/textures.py:1190-1268, one map per mesh):
 * interpolate_face_attributes of the per-face uvs + torch.lerp to grid coordinates + F.grid_sample on K expanded
 * NCHW copies of the maps + permutes, and their autograd graph, with one kernel each way reading the maps in their
 * own (N, Hm, Wm, C) layout.  face_uvs (F,3,2) = verts_uvs[faces_uvs]; texels (N,H,W,K,C) fully written.
 * Backward: grad_bary (N,H,W,K,3) fully written; grad_face_uvs (F,3,2) and grad_maps (N,Hm,Wm,C) zeroed and
 * accumulated.  A sample with pix_to_face >= F reads as zero and has no gradient.  padding "reflection" is not provided. */
#define P3D_PAD_ZEROS 0
#define P3D_PAD_BORDER 1
#define P3D_SAMPLE_BILINEAR 0
#define P3D_SAMPLE_NEAREST 1
int p3d_sample_uv_forward(const int64_t* pix_to_face, const float* bary_coords, const float* face_uvs, const float* maps,
                          int N, int H, int W, int K, int64_t F, int Hm, int Wm, int C, int align_corners,
                          int padding_mode, int sampling_mode, float* texels, p3d_stream_t stream);
int p3d_sample_uv_backward(const float* grad_texels, const int64_t* pix_to_face, const float* bary_coords,
                           const float* face_uvs, const float* maps, int N, int H, int W, int K, int64_t F, int Hm, int Wm,
                           int C, int align_corners, int padding_mode, int sampling_mode, float* grad_bary_coords,
                           float* grad_face_uvs, float* grad_maps, p3d_stream_t stream);

/* replaces the maps_ids branch of TexturesUV.sample_textures (pytorch3d/renderer/mesh/textures.py:1270-1313, several
 * texture maps per mesh): maps (N,M,Hm,Wm,C) with M >= 2; maps_ids = the flattened maps_ids_padded (L entries), indexed
 * by the packed face index as the reference's gather does; background samples use face 0's map at uv = (0,0).  The map
 * index is the z coordinate of the reference's 3-D grid_sample: "bilinear" blends neighbouring maps wherever the
 * un-normalised z is not an integer (always with align_corners = 0) -- restated in csrc/uvm_sample.h.  Outputs as
 * p3d_sample_uv_forward / _backward (grad_maps (N,M,Hm,Wm,C)); faces >= L or >= F read as zero. */
int p3d_sample_uv_multi_forward(const int64_t* pix_to_face, const float* bary_coords, const float* face_uvs,
                                const float* maps, const int64_t* maps_ids, int64_t L, int N, int H, int W, int K, int64_t F,
                                int M, int Hm, int Wm, int C, int align_corners, int padding_mode, int sampling_mode,
                                float* texels, p3d_stream_t stream);
int p3d_sample_uv_multi_backward(const float* grad_texels, const int64_t* pix_to_face, const float* bary_coords,
                                 const float* face_uvs, const float* maps, const int64_t* maps_ids, int64_t L, int N, int H,
                                 int W, int K, int64_t F, int M, int Hm, int Wm, int C, int align_corners, int padding_mode,
                                 int sampling_mode, float* grad_bary_coords, float* grad_face_uvs, float* grad_maps,
                                 p3d_stream_t stream);

/* replaces TexturesAtlas.sample_textures (pytorch3d/renderer/mesh/textures.py:565-612): the nearest-cell lookup of a
 * per-face R x R atlas (F,R,R,C) by the first two barycentrics of each of the P = N*H*W*K samples -> texels (P,C), fully
 * written (zero for pix_to_face < 0).  Cell arithmetic: csrc/atlas_cell.h.  Indices the reference fails on (torch raises
 * IndexError: face >= F, cell outside [-R, R-1]) read as zero.  Backward: grad_atlas (F,R,R,C) zeroed and accumulated;
 * the barycentrics have no gradient (nearest sampling), as in the reference. */
int p3d_sample_atlas_forward(const int64_t* pix_to_face, const float* bary_coords, const float* atlas, int64_t P, int64_t F,
                             int R, int C, float* texels, p3d_stream_t stream);
int p3d_sample_atlas_backward(const float* grad_texels, const int64_t* pix_to_face, const float* bary_coords, int64_t P,
                              int64_t F, int R, int C, float* grad_atlas, p3d_stream_t stream);

/* replaces hard_rgb_blend (pytorch3d/renderer/blending.py:54-88: mask, masked_scatter of the background colour, cat with
 * the alpha channel): colors (npix,K,3), pix_to_face (npix,K) -> out (npix,4), 16-byte aligned: RGB of slot 0 and
 * alpha 1 where pix_to_face[...,0] >= 0, else the background colour and alpha 0.  Backward: grad_colors (npix,K,3)
 * fully written (slot 0 of covered pixels = grad_out[..., :3], zero elsewhere). */
int p3d_hard_rgb_blend_forward(const float* colors, const int64_t* pix_to_face, const float background[3], int64_t npix,
                               int K, float* out, p3d_stream_t stream);
int p3d_hard_rgb_blend_backward(const float* grad_out, const int64_t* pix_to_face, int64_t npix, int K, float* grad_colors,
                                p3d_stream_t stream);

/* replace HardDepthShader.forward / SoftDepthShader.forward (pytorch3d/renderer/mesh/shader.py:377-445).  Fragment rows
 * (npix,K) as above: dists, zbuf f32, pix_to_face i64; 1 <= K <= 150 (P3D_ERR_K_TOO_LARGE above, P3D_ERR_INVALID_ARG below);
 * rows that are a multiple of 16 bytes must start 16-byte aligned; depth / grad_depth (npix) f32; zfar one number; npix == 0
 * is a no-op.  One launch each, no atomics: bit-identical from run to run.
 *   hard: depth = pix_to_face[.,0] >= 0 ? zbuf[.,0] : zfar.  Backward: grad_zbuf (npix,K) fully written -- grad_depth in
 *   slot 0 of covered pixels, zero elsewhere.
 *   soft (sigma > 0): p_k = pix_to_face_k >= 0 ? sigmoid(-dists_k / sigma) : 0, c_k = p_0 + .. + p_k as a running float sum in
 *   slot order, C_k = min(c_k, 1), w_k = C_k - C_{k-1}, depth = sum_k w_k zbuf_k + (1 - C_{K-1}) zfar; the slots are taken
 *   in their stored order, sorted or not.  Backward: grad_zbuf_k = g w_k; grad_dists_j = -g p_j (1 - p_j) / sigma * sum over
 *   k >= j with c_k <= 1 of (zbuf_k - zbuf_{k+1}), zbuf_K := zfar, zero where pix_to_face_j < 0.  A null grad_dists or
 *   grad_zbuf is not wanted and not written; the other one is fully written. */
int p3d_soft_depth_blend_forward(const float* dists, const float* zbuf, const int64_t* pix_to_face, float sigma, float zfar,
                                 int64_t npix, int K, float* depth, p3d_stream_t stream);
int p3d_soft_depth_blend_backward(const float* grad_depth, const float* dists, const float* zbuf, const int64_t* pix_to_face,
                                  float sigma, float zfar, int64_t npix, int K, float* grad_dists, float* grad_zbuf,
                                  p3d_stream_t stream);
int p3d_hard_depth_blend_forward(const float* zbuf, const int64_t* pix_to_face, float zfar, int64_t npix, int K, float* depth,
                                 p3d_stream_t stream);
int p3d_hard_depth_blend_backward(const float* grad_depth, const int64_t* pix_to_face, int64_t npix, int K, float* grad_zbuf,
                                  p3d_stream_t stream);

/* ---- SplatterPhongShader's blend ------------------------------------------------------------------------------------
 *
 * replaces SplatterBlender.forward (pytorch3d/renderer/splatter_blend.py) after its camera call: masking, the 9-direction
 * occlusion layers, the splat weights, the three-buffer accumulation, normalisation and back-to-front compositing in one
 * launch, nothing of size 9 x K per pixel in memory.  colors (N,H,W,K,3), screen_coords (N,H,W,K,3) =
 * cameras.transform_points_screen(..., with_xyflip=False), both contiguous f32; background_mask (N,H,W,K) one byte per
 * entry, nonzero where pix_to_face < 0 (a torch.bool tensor); sigma > 0; any K >= 1, any H, W.
 *   forward: out (N,H,W,4) RGBA, 16-byte aligned, fully written.
 *   backward: grad_out (N,H,W,4) -> grad_colors, grad_screen_coords (N,H,W,K,3) fully written (zero at background
 *   entries, zero z).  Gather form without atomics: bit-identical from run to run.  The workspace (16-byte aligned)
 *   holds one 96-byte record per pixel: p3d_splatter_blend_backward_workspace_bytes(). */
size_t p3d_splatter_blend_backward_workspace_bytes(int N, int H, int W);
int p3d_splatter_blend_forward(const float* colors, const float* screen_coords, const uint8_t* background_mask, float sigma,
                               const float background[3], int N, int H, int W, int K, float* out, p3d_stream_t stream);
int p3d_splatter_blend_backward(const float* grad_out, const float* colors, const float* screen_coords,
                                const uint8_t* background_mask, float sigma, const float background[3], int N, int H, int W,
                                int K, float* grad_colors, float* grad_screen_coords, void* workspace, size_t workspace_bytes,
                                p3d_stream_t stream);

/* ---- deterministic backwards (torch.use_deterministic_algorithms(True)) -----------------------------------------------
 *
 * The backwards above end in float atomics: the order of the additions, and with it the last bits of a gradient, changes
 * from run to run.  The *_ordered entries compute the same sums in an order that only their inputs decide (csrc/ordered_sum.h;
 * DESIGN.md section 8.8): no float atomic in LDS or in memory, every output row written (zeros for primitives nobody hit),
 * nothing read from an output or the workspace before it is written.  They are not bit-equal to the atomic entries.
 *   sorted_samples (num_sorted) i64: the linear indices of the samples that hold a primitive (index >= 0), sorted STABLY by
 *     that primitive: ascending primitive, ascending sample index inside one primitive.  The linear index counts the logical
 *     shape of the index tensor: (N, H, W, K) for pix_to_face / idxs, (N, K, H, W) for the compositors' points_idx, (P) for
 *     interp.  The caller builds it (torch: nonzero + stable sort; one host sync for num_sorted).  An index outside the tensor
 *     or a primitive outside the output is skipped.  A list that is not sorted as described gives wrong sums, never a write
 *     outside the outputs.
 *   sorted_corners (num_corners) i64: the same for the corners c = 3 f + j of faces (F, 3) with a vertex inside [0, V),
 *     sorted stably by vertex (negative ids wrap once, as torch indexing does).
 *   workspace: p3d_*_ordered_workspace_bytes(...) bytes, 16-byte aligned; smaller: P3D_ERR_WORKSPACE.  Arguments are checked
 *     before anything is launched. */
size_t p3d_rasterize_meshes_backward_ordered_workspace_bytes(int64_t F, int through_faces, int64_t num_sorted);
/* p3d_rasterize_meshes_backward_ex's two forms: faces null -> grad_out (F,3,3); faces (F,3) -> grad_out (V,3) (the per-face sums go
 * to the workspace, then the corners of a vertex are summed in the order of sorted_corners). */
int p3d_rasterize_meshes_backward_ordered(const float* face_verts, const int64_t* faces, const int64_t* pix_to_face,
                                          const float* grad_zbuf, const float* grad_bary, const float* grad_dists,
                                          const int64_t* sorted_samples, int64_t num_sorted, const int64_t* sorted_corners,
                                          int64_t num_corners, int64_t F, int64_t V, int N, int H, int W, int K,
                                          int perspective_correct, int clip_barycentric_coords, float* grad_out, void* workspace,
                                          size_t workspace_bytes, p3d_stream_t stream);
size_t p3d_scatter_face_grads_ordered_workspace_bytes(int64_t F);
int p3d_scatter_face_grads_ordered(const float* grad_face_verts, const int64_t* faces, const int64_t* sorted_corners,
                                   int64_t num_corners, int64_t V, int64_t F, float* grad_verts, void* workspace,
                                   size_t workspace_bytes, p3d_stream_t stream);
size_t p3d_rasterize_points_backward_ordered_workspace_bytes(int64_t num_sorted);
int p3d_rasterize_points_backward_ordered(const float* points, const int32_t* idxs, const float* grad_zbuf, const float* grad_dists,
                                          const int64_t* sorted_samples, int64_t num_sorted, int64_t P, int N, int H, int W, int K,
                                          float* grad_points, void* workspace, size_t workspace_bytes, p3d_stream_t stream);
/* p3d_rasterize_points_composite_backward; any K <= 150 (the pixel part runs per pixel, grad_alphas and the entries' weights pass
 * through the workspace). */
size_t p3d_rasterize_points_composite_backward_ordered_workspace_bytes(int N, int H, int W, int K, int C, int64_t num_sorted);
int p3d_rasterize_points_composite_backward_ordered(int mode, const float* points, const float* features, const int32_t* idxs,
                                                    const float* dists, const float* grad_images, const int64_t* sorted_samples,
                                                    int64_t num_sorted, int64_t P, int C, int N, int H, int W, int points_per_pixel,
                                                    float inv_r2, float* grad_points, float* grad_features, void* workspace,
                                                    size_t workspace_bytes, p3d_stream_t stream);
/* p3d_composite_backward: grad_alphas per pixel as before (no scatter), grad_features ordered; any C, both feature layouts. */
size_t p3d_composite_backward_ordered_workspace_bytes(int N, int K, int H, int W, int C, int64_t num_sorted);
int p3d_composite_backward_ordered(int mode, const float* grad_outputs, const float* features, const int64_t feature_strides[2],
                                   const float* alphas, const int64_t* points_idx, const int64_t* sorted_samples, int64_t num_sorted,
                                   int N, int C, int64_t P, int K, int H, int W, const int64_t alphas_strides[4],
                                   const int64_t idx_strides[4], float* grad_features, const int64_t grad_feature_strides[2],
                                   float* grad_alphas, void* workspace, size_t workspace_bytes, p3d_stream_t stream);
/* p3d_interp_face_attrs_backward for float32 (float64 has no ordered form), any D; image-shaped samples take the same entry. */
size_t p3d_interp_face_attrs_backward_ordered_workspace_bytes(int64_t D, int64_t num_sorted);
int p3d_interp_face_attrs_backward_ordered(const int64_t* pix_to_face, const float* barycentric_coords, const float* face_attrs,
                                           const float* grad_pix_attrs, const int64_t* sorted_samples, int64_t num_sorted, int64_t P,
                                           int64_t F, int64_t D, float* grad_barycentric_coords, float* grad_face_attrs,
                                           void* workspace, size_t workspace_bytes, p3d_stream_t stream);

/* ---- nearest neighbours and chamfer distance (pytorch3d/ops/knn.py, pytorch3d/loss/chamfer.py) ------------------------
 *
 * p1 (N,P1,D), p2 (N,P2,D) contiguous f32; lengths1 / lengths2 (N) i64 or NULL (every cloud full; a length is clamped to
 * [0, P]); norm 1 (L1) or 2 (squared L2); D in {2, 3} and 1 <= K <= P3D_KNN_MAX_K, otherwise P3D_ERR_UNSUPPORTED (the caller
 * owns a formulation for the rest: pytorch3d_amd/knn.py).
 * Forward: for n and i < lengths1[n] the min(K, lengths2[n]) smallest dist(p1[n,i], p2[n,j]), j < lengths2[n], ascending by
 * (dist, j) -- a tie goes to the smaller index.  dist: per coordinate the difference, then |.| or its square, accumulated in
 * coordinate order, one float32 operation each, NOT fused (the library is built with -ffp-contract=off; every instantiation the
 * same).  idx (N,P1,K) i64, dists (N,P1,K) f32: every entry is written, 0 in both for rows i >= lengths1[n] and slots
 * k >= lengths2[n]; no memset in front.  A NaN distance is never selected (a slot that finds nothing holds idx 0, dist +inf).
 * One lane per query, p2 staged in LDS tiles of P3D_KNN_TILE points (csrc/knn.hip). */
#define P3D_KNN_MAX_K 32
#define P3D_KNN_TILE 512
int p3d_knn_points_forward(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2, int64_t N, int64_t P1,
                           int64_t P2, int D, int K, int norm, int64_t* idx, float* dists, p3d_stream_t stream);
/* One direction of chamfer_distance: the K = 1 forward (idx, dists (N,P1), masked as above) and, in the same launch, the terms
 * dists[n,i] * weights[n] (weights (N) f32 or NULL) summed per wave; a second small launch sums a cloud's partials:
 * sums (N) f32 <- the cloud's sum, divided by max(lengths1[n], 1) when point_mean != 0.  No float atomic: the sum of a cloud's P1
 * terms is the fixed tree of csrc/fixed_sum.h over waves of 64 queries, depth D(P1) = 6 + ceil(ceil(P1 / 64) / 256) + 8.
 * workspace: p3d_chamfer_forward_workspace_bytes(N, P1) bytes, every byte read was written by the same call. */
size_t p3d_chamfer_forward_workspace_bytes(int64_t N, int64_t P1);
int p3d_chamfer_forward(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2, const float* weights,
                        int64_t N, int64_t P1, int64_t P2, int D, int norm, int point_mean, int64_t* idx, float* dists, float* sums,
                        void* workspace, size_t workspace_bytes, p3d_stream_t stream);
/* Backward (knn_cpu.cpp:101-126).  For i < lengths1[n], k < min(K, lengths2[n]), j = idx[n,i,k] (an entry outside [0, P2) is
 * skipped) and g = grad_dists[n,i,k] (NULL: 1) * cloud_scale[n] (NULL: 1):
 *   norm 2: grad_p1[n,i] += 2 g (p1[n,i] - p2[n,j]);  norm 1: grad_p1[n,i] += g s, s = +1 where p1 > p2 and -1 otherwise;
 *   grad_p2[n,j] gets the negative.
 * grad_p1 (N,P1,D), NULL to skip: a gather, one lane per (n, i), k ascending, every entry written.  grad_p2 (N,P2,D), NULL to
 * skip: float atomics, the D values of one hit from adjacent lanes; zero-filled first unless flags has P3D_KNN_ACCUMULATE_P2
 * (then the hits are added to what grad_p2 holds). */
#define P3D_KNN_ACCUMULATE_P2 1u
int p3d_knn_points_backward(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2, const int64_t* idx,
                            const float* grad_dists, const float* cloud_scale, int64_t N, int64_t P1, int64_t P2, int D, int K,
                            int norm, unsigned flags, float* grad_p1, float* grad_p2, p3d_stream_t stream);
/* The grad_p2 part of p3d_knn_points_backward in a fixed order (see "deterministic backwards" above): sorted_samples holds the
 * linear indices into (N,P1,K) of the valid hits, sorted stably by n * P2 + idx. */
size_t p3d_knn_points_ordered_backward_workspace_bytes(int64_t num_sorted);
int p3d_knn_points_ordered_backward(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2,
                                    const int64_t* idx, const float* grad_dists, const float* cloud_scale,
                                    const int64_t* sorted_samples, int64_t num_sorted, int64_t N, int64_t P1, int64_t P2, int D, int K,
                                    int norm, unsigned flags, float* grad_p2, void* workspace, size_t workspace_bytes,
                                    p3d_stream_t stream);

/* ---- point-mesh distances (pytorch3d/loss/point_mesh_distance.py; csrc/point_mesh.hip, csrc/point_mesh_geom.h) ------------
 *
 * Brute force between the points of a cloud and the faces or edges of its mesh, per batch element.  A direction is a (query kind,
 * target kind) pair: (POINT, TRIANGLE) point_face, (TRIANGLE, POINT) face_point, (POINT, SEGMENT) point_edge, (SEGMENT, POINT)
 * edge_point; anything else is P3D_ERR_INVALID_ARG.  Packed layouts, as the reference's operators take them: points (P,3), tris
 * (T,3,3), segms (S,2,3) contiguous f32; query_first_idx / target_first_idx (N) i64, element n owning [first[n], first[n+1]) (the
 * last one up to the total; values are clamped into the arrays).  Q / T: the number of query / target objects.
 * Forward: dists (Q) f32 <- the smallest squared distance from query q to a target of its element, idxs (Q) i64 <- that target's
 * PACKED index.  Among equal distances the LARGEST target index wins (the reference's CPU loop: ascending with <=); a NaN distance
 * is never selected.  An element without targets: dists FLT_MAX, idxs 0.  max_queries: a host-side upper bound of the elements'
 * query counts (the grid is sized from it, rows past an element's count exit; a bound that is too small leaves rows unwritten).
 * Every entry of dists / idxs is written, no memset.  The pair functions are those of point_mesh_geom.h: float32, one operation
 * each, NOT fused; min_triangle_area is compared with the face's area in double (segment directions ignore it).
 * One lane per query, a wave = 64 consecutive queries of one element, targets staged in LDS tiles of P3D_POINT_MESH_TILE records.
 * split: waves per workgroup that share the 64 queries and take every split-th tile, 1 / 2 / 4 / 8, or 0 = chosen from the workgroup
 * count and the device's CU count.  The result is bit-equal for every split.
 * sums != NULL fuses one direction of the loss: dists[q] * weights[n] (weights (N) f32 or NULL = 1) summed per wave of 64 queries,
 * then per element by a second launch -- the fixed tree of csrc/fixed_sum.h: sums (N) f32.  No float atomic.  workspace: p3d_point_mesh_forward_workspace_bytes(N, max_queries) bytes (sums only). */
#define P3D_POINT_MESH_POINT 0
#define P3D_POINT_MESH_SEGMENT 1
#define P3D_POINT_MESH_TRIANGLE 2
#define P3D_POINT_MESH_TILE 64
size_t p3d_point_mesh_forward_workspace_bytes(int64_t N, int64_t max_queries);
int p3d_point_mesh_forward(int query_kind, int target_kind, const float* queries, const float* targets,
                           const int64_t* query_first_idx, const int64_t* target_first_idx, int64_t N, int64_t Q, int64_t T,
                           int64_t max_queries, double min_triangle_area, int split, const float* weights, float* dists,
                           int64_t* idxs, float* sums, void* workspace, size_t workspace_bytes, p3d_stream_t stream);
/* Backward: the hit of query q is (q, idxs[q]); an idxs entry outside [0, T) is no hit.  Its upstream gradient is grad_dists[q]
 * (NULL: 1) * elem_scale[n] (NULL: 1).  With the first-index arrays (both or neither; elem_scale needs them) a query of an element
 * WITHOUT targets is no hit either and nothing of `targets` is read for it.
 * grad_queries (Q, 3 / 6 / 9), NULL to skip: one lane per query, a plain store to every row (zeros for no hit), or an add to what
 * the row holds under P3D_POINT_MESH_ACCUMULATE_QUERIES.
 * grad_targets (T, 3 / 6 / 9), NULL to skip: zero-filled first unless P3D_POINT_MESH_ACCUMULATE_TARGETS; then the hits are added
 * with float atomics, the 3 / 6 / 9 values of one hit from adjacent lanes -- or, with sorted_hits != NULL (the Q query indices sorted
 * stably by idxs), by the ordered segmented sum of the deterministic backwards: the same bits on every run.
 * workspace: p3d_point_mesh_backward_workspace_bytes(target_kind, Q) bytes, needed with sorted_hits only. */
#define P3D_POINT_MESH_ACCUMULATE_QUERIES 1u
#define P3D_POINT_MESH_ACCUMULATE_TARGETS 2u
size_t p3d_point_mesh_backward_workspace_bytes(int target_kind, int64_t Q);
int p3d_point_mesh_backward(int query_kind, int target_kind, const float* queries, const float* targets, const int64_t* idxs,
                            const float* grad_dists, const float* elem_scale, const int64_t* query_first_idx,
                            const int64_t* target_first_idx, int64_t N, int64_t Q, int64_t T, double min_triangle_area,
                            unsigned flags, const int64_t* sorted_hits, float* grad_queries, float* grad_targets, void* workspace,
                            size_t workspace_bytes, p3d_stream_t stream);

/* ---- sample_points_from_meshes (pytorch3d/ops/sample_points_from_meshes.py; csrc/sample_points.hip) ------------------------
 *
 * Points on the surface of every mesh of a packed batch, a face drawn with probability proportional to its area and the point
 * uniform on the face.  The randomness is an input: uniforms (N,S,3) f32 in [0, 1); the outputs are a pure function of it.
 * verts (V,3) f32, faces (F,3) i64 packed vertex ids (a negative id wraps once, an id still out of range gives NaN coordinates),
 * mesh_to_faces_first_idx / num_faces_per_mesh (N) i64: mesh n owns the faces [first[n], first[n] + num[n]), clamped into [0, F);
 * first is ascending, as a packed batch has it.
 * Forward.  (1) cdf (F) f32 in the workspace: per mesh the inclusive prefix sum of the areas |(v1 - v0) x (v2 - v0)| / 2 (the
 * arithmetic of p3d_face_areas_normals_forward), restarting at every entry of mesh_to_faces_first_idx: a two-level segmented
 * tree sum whose shape the face counts alone decide, followed by the running maximum over the faces of non-zero area -- exact in any
 * order -- so that the table is non-decreasing inside a mesh and a face of zero area repeats its predecessor's value (0 at a mesh's
 * start).  No float atomic, no host round trip; an entry is within D(F) 2^-24 total of the exact prefix sum of the float32 areas,
 * D(F) = 19 + 4 ceil(ceil(F / 256) / 256).  (2) one lane per sample (n, s): t = u0 * total_n with total_n the mesh's last entry, the
 * face is the first f of the mesh with cdf[f] > t, t clamped into [0, total_n) -- a product that rounds up to the total takes the
 * last face of non-zero area; a face of zero area is never taken.  r = sqrt(u1), w0 = 1 - r, w1 = r (1 - u2), w2 = r u2,
 * sample = (w0 v0 + w1 v1) + w2 v2, normal = c / max(|c|, DBL_EPSILON) with c = (v1 - v0) x (v2 - v1): float32, one operation
 * each, NOT fused, IEEE sqrt and division.
 * samples (N,S,3) f32, normals (N,S,3) f32 or NULL, face_idxs (N,S) i64 packed face indices, bary (N,S,3) f32 (w0, w1, w2): every
 * entry is written, no memset in front.  An empty mesh, or one whose total area is zero or not finite: zero rows, face_idxs -1.
 * workspace: p3d_sample_points_forward_workspace_bytes(F) bytes; its first F floats are the table. */
size_t p3d_sample_points_forward_workspace_bytes(int64_t F);
int p3d_sample_points_forward(const float* verts, const int64_t* faces, const int64_t* mesh_to_faces_first_idx,
                              const int64_t* num_faces_per_mesh, const float* uniforms, int64_t V, int64_t F, int64_t N, int64_t S,
                              float* samples, float* normals, int64_t* face_idxs, float* bary, void* workspace,
                              size_t workspace_bytes, p3d_stream_t stream);
/* Backward, with the face choice and the weights held fixed: grad_face_verts (F,3,3) f32, every entry written, to be summed per
 * vertex by p3d_scatter_face_grads or p3d_scatter_face_grads_ordered.  Sample i with f = face_idxs[i] in [0, F) (anything else
 * contributes nothing) adds bary[i,k] * grad_samples[i] to corner k of face f and, grad_normals != NULL, grad_normals[i] to the
 * face's normal sum G; one lane per face then adds G through the Jacobian of c / max(|c|, DBL_EPSILON) -- (G - n (n . G)) / |c|, or
 * G / DBL_EPSILON where the clamp holds -- and of c = (v1 - v0) x (v2 - v1), once per face.  grad_samples (num_samples,3),
 * grad_normals (num_samples,3) or NULL.  The per-face sums: float atomics after a merge in LDS; or, with sorted_samples != NULL (the
 * num_sorted samples that hold a face, sorted stably by face), the ordered segmented sum of the deterministic backwards: the same
 * bits on every run.  workspace: p3d_sample_points_backward_workspace_bytes(F, grad_normals != NULL, num_sorted or 0) bytes. */
size_t p3d_sample_points_backward_workspace_bytes(int64_t F, int with_normals, int64_t num_sorted);
int p3d_sample_points_backward(const float* grad_samples, const float* grad_normals, const float* verts, const int64_t* faces,
                               const int64_t* face_idxs, const float* bary, const int64_t* sorted_samples, int64_t num_sorted,
                               int64_t V, int64_t F, int64_t num_samples, float* grad_face_verts, void* workspace,
                               size_t workspace_bytes, p3d_stream_t stream);

/* ---- farthest point sampling and ball query (pytorch3d/ops/sample_farthest_points.py, ball_query.py; csrc/fps_ball.hip) ------
 *
 * Clouds as for the nearest neighbours: (N,P,D) contiguous f32, lengths (N) i64 or NULL (full), clamped into [0, P]; D in {2, 3},
 * otherwise P3D_ERR_UNSUPPORTED (the caller owns a formulation for the rest).  A squared distance is, per coordinate in order, the
 * difference and its square, accumulated: one float32 operation each, NOT fused.
 *
 * Farthest point sampling (sample_farthest_points_cpu.cpp).  K (N) i64 or NULL (max_K for every cloud), clamped into [0, max_K];
 * start_idxs (N) i64 or NULL (0), clamped into [0, length).  Row n of idx (N,max_K) i64 holds count = min(K[n], lengths[n])
 * indices and -1 behind them; every entry is written, no memset in front.  idx[n,0] = start_idxs[n]; every further entry is the
 * point with the LARGEST minimum squared distance to the entries before it, the minimum kept as d < m ? d : m from +inf; equal
 * minima go to the LOWEST index, so a cloud of coinciding points repeats index 0 (std::max_element).  A row with count 0 is all
 * -1 (the reference writes index 0 there).  Coordinates that are not finite are outside the contract; the entries stay inside
 * [0, length) all the same.
 * One workgroup per cloud, nothing between workgroups (a small N uses few CUs).  P <= P3D_FPS_REGISTER_POINTS: the cloud lives in
 * the workgroup's registers and needs no workspace; above: p3d_sample_farthest_points_workspace_bytes(N, P) bytes for the minimum
 * distances (N,P), every byte read was written by the same call.  N, P or max_K of 0: P3D_OK without a launch. */
#define P3D_FPS_REGISTER_POINTS 16384
size_t p3d_sample_farthest_points_workspace_bytes(int64_t N, int64_t P);
int p3d_sample_farthest_points(const float* points, const int64_t* lengths, const int64_t* K, const int64_t* start_idxs, int64_t N,
                               int64_t P, int D, int64_t max_K, int64_t* idx, void* workspace, size_t workspace_bytes,
                               p3d_stream_t stream);
/* Ball query (ball_query_cpu.cpp).  For n and i < lengths1[n]: the pairs j < lengths2[n] in ASCENDING j with
 * dist2(p1[n,i], p2[n,j]) < radius2 -- strictly; radius2 = radius * radius in float32 --, the first K of them: idx (N,P1,K) i64
 * <- j, dists (N,P1,K) f32 <- dist2, in the order found (not sorted by distance).  The slots behind a row's hits and the rows
 * i >= lengths1[n] hold -1 / 0; every entry is written, no memset in front.  A NaN distance is no hit.  Any K >= 1.  The backward is
 * p3d_knn_points_backward with norm 2: it skips negative indices.  One lane per query, p2 staged in LDS tiles of P3D_KNN_TILE
 * points; a wave leaves the scan once all its rows are full.  N or P1 of 0: P3D_OK without a launch. */
int p3d_ball_query(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2, int64_t N, int64_t P1,
                   int64_t P2, int D, int K, float radius, int64_t* idx, float* dists, p3d_stream_t stream);

/* ---- point clouds into voxel grids (pytorch3d/ops/points_to_volumes.py; csrc/points_to_volumes.hip) ----------------------------
 *
 * The contract of the reference's compiled operator (csrc/points_to_volumes/points_to_volumes_cpu.cpp, .cu), NOT of its Python
 * twin.  points (N,P,3) and feats (N,P,C) contiguous f32, in the volume's local coordinates; grid_sizes (N,3) i64 contiguous:
 * depth, height, width of cloud n's grid, at most the tensors' (D,H,W) (a larger one is cut at the tensor's extent); mask f32 or NULL
 * (every point counts), element (n,p) at mask[n * mask_stride_n + p * mask_stride_p] (a stride of 0 is fine), a point with
 * mask == 0 is skipped.  densities (N,1,D,H,W) and features (N,C,D,H,W) f32 are read through their five ELEMENT strides (host
 * arrays of 5 i64), so a strided view is updated in place; contributions are ADDED to what they hold.
 *   location on an axis   (p + 1) * 0.5 * (grid - (align_corners ? 1 : 0)) - (align_corners ? 0 : 0.5): p + 1 in f32, the rest in f64
 *   splat == 0 (nearest)  voxel = the f64 location rounded half AWAY from zero (lround); weight 1
 *   splat != 0            the location rounded once to f32, x = trunc (toward ZERO), rx = location - x; corner (x+ux, y+uy, z+uz) has
 *                         weight (ux ? rx : 1 - rx)(uy ? ry : 1 - ry)(uz ? rz : 1 - rz), an f32 product from the left.  A location in
 *                         (-1, 0) therefore EXTRAPOLATES: voxel 0 gets 1 - rx > 1, voxel 1 gets rx < 0 (the reference does the same)
 *   a corner adds weight * point_weight to its density and feats[c] * weight * point_weight to feature c (f32, from the left)
 * A corner outside [0, grid) on any axis is skipped, in the forward and in both gradients; so is a point whose location is not
 * finite or does not fit an i64.  N, P, D, H or W of 0: P3D_OK without a launch.
 *
 * Forward, atomic form (keys == sorted_samples == NULL): float atomics, the two voxels of an x pair from adjacent lanes.
 * Forward, ordered form: p3d_points_to_volumes_keys writes the voxel n * D*H*W + (z * H + y) * W + x, or -1, of each of the
 * N * P * (splat ? 8 : 1) samples (sample = point * 8 + corner, corners in the reference's order ux, uy, uz = bit 2, 1, 0) into keys
 * (i32); the caller sorts the sample indices STABLY by key into sorted_samples (i64) and passes both with a workspace of
 * p3d_points_to_volumes_workspace_bytes(N, P, C, splat) bytes.  The rows of a voxel (1 + C floats) are summed by the fixed tree of
 * ordered_sum.h and the total is added to the volume once: no float atomic, the same bits on every run.  N * D * H * W beyond
 * INT32_MAX: P3D_ERR_UNSUPPORTED from both entries.
 *
 * Backward: a gather per point, no atomics.  grad_feats (N,P,C)[c] += grad_features[c][voxel] * weight * point_weight over the
 * corners in the reference's order (f32); with splat, grad_points (N,P,3) per axis += source * (+-1) * (the other two axis
 * weights) * 0.5 * (grid - scale offset) * point_weight in f64, rounded to f32 once per corner, where source = grad_densities[voxel]
 * + sum_c feats[c] * grad_features[c][voxel] (each product in f32, the sum in f64, as the reference's GPU operator has it).
 * Both outputs are contiguous and ADDED to (the caller zero-fills).  Without splat grad_points, feats and grad_densities are not
 * touched and may be NULL.  The gradient volumes are read through their element strides (an expanded gradient has strides of 0). */
size_t p3d_points_to_volumes_workspace_bytes(int64_t N, int64_t P, int64_t C, int splat);
int p3d_points_to_volumes_keys(const float* points, const int64_t* grid_sizes, const float* mask, int64_t mask_stride_n,
                               int64_t mask_stride_p, int64_t N, int64_t P, int64_t D, int64_t H, int64_t W, int align_corners,
                               int splat, int32_t* keys, p3d_stream_t stream);
int p3d_points_to_volumes_forward(const float* points, const float* feats, const int64_t* grid_sizes, const float* mask,
                                  int64_t mask_stride_n, int64_t mask_stride_p, int64_t N, int64_t P, int64_t C, int64_t D, int64_t H,
                                  int64_t W, float* densities, const int64_t* densities_strides, float* features,
                                  const int64_t* features_strides, float point_weight, int align_corners, int splat,
                                  const int32_t* keys, const int64_t* sorted_samples, void* workspace, size_t workspace_bytes,
                                  p3d_stream_t stream);
int p3d_points_to_volumes_backward(const float* points, const float* feats, const int64_t* grid_sizes, const float* mask,
                                   int64_t mask_stride_n, int64_t mask_stride_p, int64_t N, int64_t P, int64_t C, int64_t D, int64_t H,
                                   int64_t W, const float* grad_densities, const int64_t* grad_densities_strides,
                                   const float* grad_features, const int64_t* grad_features_strides, float point_weight,
                                   int align_corners, int splat, float* grad_points, float* grad_feats, p3d_stream_t stream);

/* ---- point-cloud covariances, curvatures and local coordinate frames (pytorch3d/ops/points_normals.py; csrc/point_frames.hip) ----
 *
 * points (N,P,3) contiguous f32, lengths (N) i64 or NULL (full), clamped into [0, P]; D must be 3 and 1 <= K <= P3D_FRAMES_MAX_K,
 * otherwise P3D_ERR_UNSUPPORTED (the caller owns a formulation for the rest).  The points are taken as they come: the reference's
 * `points - cloud mean` is the caller's (pytorch3d_amd/points_normals.py does it with the reference's expression, since it changes
 * the float32 bits of every distance).  For n and i < lengths[n], in one pass:
 *   neighbours   the kn = min(K, lengths[n]) points j of the same cloud with the smallest (dist, j), i itself included; dist as for
 *                the nearest neighbours above (per coordinate the difference and its square, accumulated, NOT fused), ties to the
 *                lower index: the rows of p3d_knn_points_forward(points, points) for any K it takes
 *   covariance   mean = (sum of the neighbours, k ascending) / kn; cov = (sum of the outer products of neighbour - mean, k ascending)
 *                / kn; float32 (ops/utils.py get_point_covariances)
 *   curvatures   (3) ascending, frames (3,3) with the vectors in the COLUMNS, column 0 the normal: the reference's symeig3x3
 *                (common/workaround/symeig3x3.py) with eps = float32 eps, operation for operation -- p1.clamp(eps), acos / cos with r
 *                clamped to +-(1 - eps), the exp(-(p1 / (6 eps))^2) blend of the eigenvalues towards the sorted diagonal, the
 *                cross-product eigenvectors with their +-eps regularisers.  It is NOT a true eigen-decomposition where the
 *                off-diagonal energy p1 is about 1e-6 or below, and is not meant to be
 *   P3D_FRAMES_DISAMBIGUATE (flags)  column 0 and column 2 are negated where fewer than 0.5 * kn neighbours have
 *                (x_k - x_i) . v > 0, then column 1 = column 0 x column 2 (_disambiguate_vector_directions)
 * Rows i >= lengths[n] are zeros in every output.  curvatures (N,P,3) and frames (N,P,3,3) come together or are both NULL (then the
 * eigen step is skipped); cov_out (N,P,3,3) and idx_out (N,P,K) i64 (slots k >= kn hold 0) are optional; at least one output.  Every
 * entry of a given output is written, no memset in front.  No workspace, no atomics: the same bits on every run and stream.  There
 * is no backward entry.  One lane per query, the cloud staged in LDS tiles of P3D_KNN_TILE points, a register queue of up to 64
 * entries; the grid is p3d_point_frames_workgroups(N, P) workgroups, each owning its rows: no loop over the grid.  N or P of 0: P3D_OK, no launch. */
#define P3D_FRAMES_MAX_K 64
#define P3D_FRAMES_DISAMBIGUATE 1u
/* The number of workgroups (of P3D_FRAMES_ROWS_PER_GROUP rows each) that p3d_point_frames launches for (N, P): N * ceil(P /
 * P3D_FRAMES_ROWS_PER_GROUP), or -1 where that does not fit a launch (the entry then returns P3D_ERR_INVALID_ARG). */
#define P3D_FRAMES_ROWS_PER_GROUP 64
int64_t p3d_point_frames_workgroups(int64_t N, int64_t P);
int p3d_point_frames(const float* points, const int64_t* lengths, int64_t N, int64_t P, int D, int K, unsigned flags,
                     float* curvatures, float* frames, float* cov_out, int64_t* idx_out, p3d_stream_t stream);

/* ---- box3d_overlap: intersection volume and IoU of oriented 3D boxes (csrc/box3d.hip) ---- */

/* IoUBox3D by the contract of the reference's CPU operator (iou_box3d/iou_box3d_cpu.cpp over iou_utils.h): for every pair the 12
 * triangles of each box are clipped through the 6 inward planes of the other, box-2 fragments coplanar with a box-1 fragment of area
 * > 1e-4 are dropped, and vol = sum |v0 . (v1 x v2)| / 6 about the mean of the face centres, iou = vol / (vol1 + vol2 - vol); a pair
 * without fragments is exactly (0, 0).  No list is capped and no pair truncated.  There is no backward.
 * boxes1 (N,8,3), boxes2 (M,8,3) contiguous f32, corners in the reference's order; vol, iou (N,M) f32, every entry written.
 *
 * p3d_iou_box3d (device): one wave per pair with its lists in LDS, lds_capacity triangles per list (P3D_BOX3D_LDS_CAPACITY is the
 * default; tests pass less; outside [12, P3D_BOX3D_LDS_CAPACITY]: P3D_ERR_INVALID_ARG).  A pair whose list would pass it is appended
 * to a list in the workspace and redone by a second launch, always issued, with lists of P3D_BOX3D_SLAB_CAPACITY = 12 * 2^6
 * triangles -- more than a pair can produce -- in the workspace.  After the call the first 4 bytes of the workspace hold the number
 * of such pairs (u32).  Results do not depend on lds_capacity, the run or the stream.  The first launch is at most
 * P3D_BOX3D_MAX_GROUPS workgroups of P3D_BOX3D_WAVES_PER_GROUP waves and loops beyond that; the second is min(N * M,
 * P3D_BOX3D_SLAB_WAVES) waves.  workspace: p3d_iou_box3d_workspace_bytes(N, M) bytes, 256-byte aligned (smaller: P3D_ERR_WORKSPACE).
 * N * M > INT32_MAX: P3D_ERR_UNSUPPORTED.  N or M of 0: P3D_OK without a launch.  No host sync.
 *
 * p3d_iou_box3d_host: the same contract on host pointers, a serial loop over the pairs on the same geometry functions. */
#define P3D_BOX3D_LDS_CAPACITY 64
#define P3D_BOX3D_SLAB_CAPACITY 768
#define P3D_BOX3D_WAVES_PER_GROUP 4
#define P3D_BOX3D_MAX_GROUPS 4096
#define P3D_BOX3D_SLAB_WAVES 256
size_t p3d_iou_box3d_workspace_bytes(int64_t N, int64_t M);
int p3d_iou_box3d(const float* boxes1, const float* boxes2, int64_t N, int64_t M, int lds_capacity, float* vol, float* iou,
                  void* workspace, size_t workspace_bytes, p3d_stream_t stream);
int p3d_iou_box3d_host(const float* boxes1, const float* boxes2, int64_t N, int64_t M, float* vol, float* iou);

/* ---- graph convolution: per-vertex sums of neighbour rows (csrc/graph_conv.hip) ---- */

/* The neighbour sum of pytorch3d.ops.GraphConv / gather_scatter (gather_scatter/gather_scatter.h) through an inverted index, forward
 * and backward (the backward is the same call on the transposed table):
 *   out[v, :] = (base ? base[v, :] : +0.0f) + (((+0.0f + rows[e_0, :]) + rows[e_1, :]) + ...),   e_i = entries[offsets[v] + i],
 * in list order, in float32.  rows: n_rows rows of D floats, rows_stride floats apart; base (or NULL) and out: V rows of D floats at
 * base_stride / out_stride; offsets (V + 1) and entries (n_entries) int32.  Offsets outside [0, n_entries] are clamped and entries
 * outside [0, n_rows) skipped: a broken table gives wrong sums, never a read outside the arrays.  No atomic, no zero fill, no
 * workspace; every (v, d) is summed by one lane, so the bits are the same for every launch shape, run and stream.  A row of any
 * length is summed sequentially.  float4 requests when D, the strides and the pointers allow it (multiples of 4 / 16 bytes), else
 * dwords; the results are the same.  The grid is at most P3D_NEIGHBOR_SUM_MAX_GROUPS workgroups of 256 lanes, each serving
 * 256 / lanes_per_row vertices per round (lanes_per_row = min(64, next_pow2(D / 4 or D))), and loops beyond that.
 * V, D or n_entries of 0: P3D_OK without a gather (n_entries of 0 still writes base or zeros; offsets and entries are not read).
 * Negative sizes, n_entries > INT32_MAX, out_stride < D, a negative stride or a missing pointer: P3D_ERR_INVALID_ARG.  No host sync. */
#define P3D_NEIGHBOR_SUM_MAX_GROUPS 2048
int p3d_neighbor_sum(const float* rows, int64_t rows_stride, int64_t n_rows, const float* base, int64_t base_stride,
                     const int32_t* offsets, const int32_t* entries, int64_t V, int64_t n_entries, int64_t D, float* out,
                     int64_t out_stride, p3d_stream_t stream);

/* ---- vert_align: image features pooled at vertex positions (csrc/vert_align.hip) ---- */

/* pytorch3d.ops.vert_align for one feature map: ATen's grid_sampler_2d restated in float32 (bilinear or nearest; zeros or border
 * padding; align_corners or not -- the flags below).  The source coordinate of c on an axis of S pixels is ((c + 1) / 2) * (S - 1)
 * with P3D_VERT_ALIGN_CORNERS, ((c + 1) * S - 1) / 2 without.  Border: clamped to [0, S - 1], NaN -> 0, gradient 0 where it was at
 * or beyond an end.  Bilinear: x0 = floor(ix), y0 = floor(iy), corners nw, ne, sw, se with weights (x0+1-ix)(y0+1-iy), (ix-x0)(y0+1-iy),
 * (x0+1-ix)(iy-y0), (ix-x0)(iy-y0), the in-range corners summed in that order from +0.  Nearest: round half to even; no coordinate
 * gradient.  OUTSIDE WHAT THE REFERENCE PINS: under zeros padding a source coordinate that is not finite or does not fit an int32
 * (tested as a float, before the conversion) makes the sample empty -- a zero row, zero gradients.
 * feat (N,C,H,W) f32 read through its four element strides (NCHW, channels-last and sliced views alike); verts (N,V,>=2) f32 read
 * through v_sn, v_sv, v_sd (x, then y one v_sd on).  Row r of the output is the padded vertex packed_idx[r] (int64, an index into
 * (N*V); outside it: an empty sample), or r itself when packed_idx is NULL (then n_rows <= N*V).  forward writes out[r*out_stride + c],
 * c < C: `out` points at this map's column block of a wider (rows, sum C) tensor.  float4 requests when f_sc == 1 and C, the strides
 * and the pointers are multiples of 4 floats / 16 bytes, else dwords; the same results.
 * backward: grad_out as `out`; grad_verts (N,V,3) contiguous or NULL, ADDED to (zero-fill once, then one call per map): the x and y
 * gradients, z untouched, a gather without atomics; grad_feat (strides g_*) zero-filled by the caller or NULL: float atomics.
 * Ordered form of grad_feat (no atomics, the same bits on every run): p3d_vert_align_keys writes for sample 4 r + k the pixel
 * n*H*W + y*W + x of corner k of row r or -1; the caller sorts the samples stably by key (sorted_samples, int64) and
 * p3d_vert_align_ordered_backward sums them (ordered_sum.h; channels in chunks of 4; workspace of p3d_vert_align_workspace_bytes,
 * smaller: P3D_ERR_WORKSPACE).  N*H*W >= 2^31 or 4 n_rows > INT32_MAX: P3D_ERR_UNSUPPORTED from both.
 * n_rows or C of 0: P3D_OK without a launch.  Unknown flags, negative sizes, missing pointers: P3D_ERR_INVALID_ARG.  No host sync. */
#define P3D_VERT_ALIGN_NEAREST 1u
#define P3D_VERT_ALIGN_BORDER 2u
#define P3D_VERT_ALIGN_CORNERS 4u
#define P3D_VERT_ALIGN_MAX_GROUPS 4096
int p3d_vert_align_forward(const float* feat, int64_t N, int64_t C, int64_t H, int64_t W, int64_t f_sn, int64_t f_sc, int64_t f_sh,
                           int64_t f_sw, const float* verts, int64_t V, int64_t v_sn, int64_t v_sv, int64_t v_sd,
                           const int64_t* packed_idx, int64_t n_rows, unsigned flags, float* out, int64_t out_stride,
                           p3d_stream_t stream);
int p3d_vert_align_backward(const float* grad_out, int64_t go_stride, const float* feat, int64_t N, int64_t C, int64_t H, int64_t W,
                            int64_t f_sn, int64_t f_sc, int64_t f_sh, int64_t f_sw, const float* verts, int64_t V, int64_t v_sn,
                            int64_t v_sv, int64_t v_sd, const int64_t* packed_idx, int64_t n_rows, unsigned flags, float* grad_feat,
                            int64_t g_sn, int64_t g_sc, int64_t g_sh, int64_t g_sw, float* grad_verts, p3d_stream_t stream);
size_t p3d_vert_align_workspace_bytes(int64_t n_rows, int64_t C);
int p3d_vert_align_keys(int64_t N, int64_t H, int64_t W, const float* verts, int64_t V, int64_t v_sn, int64_t v_sv, int64_t v_sd,
                        const int64_t* packed_idx, int64_t n_rows, unsigned flags, int32_t* keys, p3d_stream_t stream);
int p3d_vert_align_ordered_backward(const float* grad_out, int64_t go_stride, int64_t N, int64_t C, int64_t H, int64_t W,
                                    const float* verts, int64_t V, int64_t v_sn, int64_t v_sv, int64_t v_sd,
                                    const int64_t* packed_idx, int64_t n_rows, unsigned flags, const int32_t* keys,
                                    const int64_t* sorted_samples, float* grad_feat, int64_t g_sn, int64_t g_sc, int64_t g_sh,
                                    int64_t g_sw, void* workspace, size_t workspace_bytes, p3d_stream_t stream);

/* ---- built-in per-kernel timing (HIP events on the launch stream) --------------------- */

/* enable != 0: every kernel launch is bracketed by hipEventRecord on its stream. */
void p3d_profile_enable(int enable);
/* Synchronise the recorded events and fold them into per-kernel totals. */
void p3d_profile_collect(void);
/* Number of distinct kernel names seen; name/launch count/total milliseconds of entry i. */
int p3d_profile_num_entries(void);
const char* p3d_profile_entry(int i, int64_t* launches, double* total_ms);
void p3d_profile_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* P3D_AMD_H_ */
