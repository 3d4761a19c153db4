"""The `pytorch3d._C` operator surface for the rasterization hot path, on MI355X.

Same names, positional signatures, return conventions and error behaviour as the reference's
pybind module (pytorch3d/csrc/ext.cpp:38-73); each function validates like the reference's
dispatcher, allocates outputs with torch (caching allocator, uninitialised -- the kernels write
every element), and calls the C ABI of libp3d_amd.so on torch's current HIP stream.

GPU tensors only: there is no CPU implementation and no fallback in this package.
"""
import ctypes
import os

import torch

from . import _lib

# constants pytorch3d/renderer/points/pulsar/renderer.py reads at import (ext.cpp:180-185)
EPS = 1e-6
MAX_FLOAT = 3.4e38
MAX_INT = 2147483647
MAX_UINT = 4294967295
MAX_USHORT = 65535
PULSAR_MAX_GRAD_SPHERES = 128

kMaxPointsPerPixel = _lib.MAX_K
kMaxItemsPerBin = _lib.MAX_BINS_PER_SIDE + 1


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() > 0 else None)


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _need_gpu(t, name):
    if not t.is_cuda:
        # mirrors CHECK_CUDA (pytorch3d_cutils.h:12-21) -- but there is no CPU path to fall to.
        raise RuntimeError(f"{name} must be a CUDA/HIP tensor: pytorch3d_amd implements the GPU path only.")


def _same_device(*named):
    dev = named[0][1].device
    for name, t in named:
        _need_gpu(t, name)
        if t.device != dev:
            raise RuntimeError(f"Expected all tensors to be on the same GPU, but {name} is on {t.device} "
                               f"and {named[0][0]} is on {dev}")
    return dev


def _check_fragments(who, pix_to_face, **floats):
    """The fragment tensors a fused kernel is about to reinterpret: pix_to_face must be int64 (rasterize_points returns
    int32 idx -- a mix-up would be misread, not rejected, by a kernel that takes a raw pointer), the float tensors
    float32, and everything on pix_to_face's GPU."""
    _need_gpu(pix_to_face, "pix_to_face")
    if pix_to_face.dtype != torch.int64:
        raise RuntimeError(f"{who}: pix_to_face must be int64, got {pix_to_face.dtype}")
    for name, t in floats.items():
        _need_gpu(t, name)
        if t.dtype != torch.float32:
            raise RuntimeError(f"{who}: {name} must be float32, got {t.dtype}")
        if t.device != pix_to_face.device:
            raise RuntimeError(f"Expected all tensors to be on the same GPU, but {name} is on {t.device} and pix_to_face is on "
                               f"{pix_to_face.device}")


def _c(t, dtype):
    if t.dtype != dtype:
        raise RuntimeError(f"expected dtype {dtype}, got {t.dtype}")
    return t.contiguous()


def _aligned(t):
    """`t` contiguous with its first element on a 16-byte boundary, as the blend entries want their rows (include/p3d_amd.h,
    "Alignment"): `t` itself when it already is, else a copy.  A contiguous view at a storage offset -- buf[1:1 + n].view(N, H, W, K)
    -- is the case .contiguous() leaves where it is; fresh allocations are aligned."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _hw(image_size):
    h, w = image_size
    return int(h), int(w)


def _check_k(K):
    if K > kMaxPointsPerPixel:
        raise RuntimeError(f"Must have points_per_pixel <= {kMaxPointsPerPixel}")


def _refuse_when_deterministic(op_name):
    """The backwards scatter with float atomics, like the reference's (rasterize_meshes.cu:587 alertNotDeterministic)."""
    if torch.are_deterministic_algorithms_enabled() and not torch.is_deterministic_algorithms_warn_only_enabled():
        raise RuntimeError(f"{op_name} does not have a deterministic implementation")


def _ordered():
    """torch.use_deterministic_algorithms(True), not warn-only: the backwards take the *_ordered entries (include/p3d_amd.h) --
    sums in an order that only the inputs decide -- instead of float atomics.  Off or warn-only: the atomic entries, as ever."""
    return torch.are_deterministic_algorithms_enabled() and not torch.is_deterministic_algorithms_warn_only_enabled()


def _sorted_hits(index):
    """The linear indices (logical shape, row-major) of the entries of `index` that hold a primitive (>= 0), sorted stably by
    that primitive: what the *_ordered entries take as sorted_samples.  torch.nonzero waits for the device once (the count);
    the deterministic mode pays that, the atomic path never comes here."""
    flat = index.reshape(-1)
    hits = torch.nonzero(flat >= 0).squeeze(1)  # ascending linear index
    order = torch.sort(flat[hits], stable=True).indices
    return hits[order].contiguous()


def _sorted_corners(faces, V):
    """The corners 3 f + j of faces (F, 3) whose vertex lies in [0, V) (negative ids wrap once, as torch indexing does), sorted stably
    by vertex: a vertex's faces in a fixed order."""
    flat = faces.reshape(-1)
    flat = torch.where(flat < 0, flat + V, flat)
    ok = torch.nonzero((flat >= 0) & (flat < V)).squeeze(1)
    order = torch.sort(flat[ok], stable=True).indices
    return ok[order].contiguous()


def _num_bins(H, W, bin_size, who):
    by, bx = 1 + (H - 1) // bin_size, 1 + (W - 1) // bin_size
    if by >= kMaxItemsPerBin or bx >= kMaxItemsPerBin:
        raise RuntimeError(f"In {who} got num_bins_y: {by}, num_bins_x: {bx}, ; that's too many!")
    return by, bx


def _workspace(nbytes, device):
    """Scratch for the coarse stage, sized by the C ABI (include/p3d_amd.h).  A request the allocator cannot serve is reported
    with what to do about it instead of as a bare out-of-memory error."""
    n = max(int(nbytes), 256)
    try:
        return torch.empty((n,), dtype=torch.uint8, device=device)
    except RuntimeError as e:  # torch.OutOfMemoryError is a RuntimeError
        if "out of memory" not in str(e).lower():
            raise
        raise RuntimeError(f"the coarse stage's workspace of {n / 2**30:.1f} GiB does not fit on {device}: rasterize the "
                           "batch in smaller pieces (pytorch3d_amd.sharding.partition, or bench.py --jobs style sub-batches of 64 "
                           "meshes), pass a smaller max_faces_per_bin (the worst case is capped by N * bins * max_faces_per_bin * 4 "
                           "bytes) or set pytorch3d_amd._C.SHORT_WORKSPACE = 'always'") from e


# Short workspaces for rasterize_meshes and rasterize_points (include/p3d_amd.h "Short workspaces"; csrc/binning.h).  The worst case of the bin
# lists is 100-1000 x what a batch needs (bench batch: 1.3 GB against 8.4 MB; 512 such meshes in one call: 42 GB), and
# what it needs is only known on the device.  With a short workspace the call sizes the lists from what the SAME call shape
# needed before (read back asynchronously: no host sync anywhere) plus a quarter of headroom, and the library decides on
# the device whether they fit (if not, its naive kernel writes the same bits, once; the next call has the new size).
#   'auto'    short when the worst case is above SHORT_WORKSPACE_ABOVE bytes (the stand-by launch costs 0.026 ms on the 65 536
#             tiles of the bench batch, 1 % of its step: profiles/r04/r04c8/measure.json)
#   'always'  every binned call        'never'  always the worst case
SHORT_WORKSPACE = os.environ.get("P3D_SHORT_WORKSPACE", "auto")
SHORT_WORKSPACE_ABOVE = 2 << 30
SHORT_WORKSPACE_FIRST_GUESS = None  # tests: list entries of a shape's first call (default 32 per face + 256k)
WORKSPACE_STATS = {"short_calls": 0, "last_bytes": 0, "last_entries": None}
_NEEDS = {}  # call shape -> _Need


class _Need:
    """What one call shape needed, refreshed from the device without ever waiting for it.

    `entries` is a running maximum with slow decay (a report below it pulls it down by an eighth of the difference), not the
    last report: a scene whose lists grow -- mesh fitting, a camera zooming in -- would otherwise size every call by a stale
    smaller number.  A report is requested on every call while the last one was within 20 % of the capacity the call was given
    (or above it: the naive kernel ran), and every 8th call otherwise (up to seven consecutive calls could
    run the every-tile-tests-every-face stand-by).  Caveat (documented in INTEGRATION.md): the stand-by is bit-identical to the
    binned path only while no bin reaches max_faces_per_bin -- the binned path drops a bin's faces beyond that limit as the
    reference does (rasterize_coarse.cu:186-201), the naive kernel has no bins."""

    def __init__(self):
        self.entries = None   # running maximum (slow decay) of what the calls that reported back needed
        self.last = None      # the last report itself
        self.capacity = None  # list entries of the call that produced the pending / last report
        self.calls = 0
        self.pinned = None
        self.event = None

    def collect(self):
        if self.event is not None and self.event.query():
            self.last = int(self.pinned[0])
            self.entries = self.last if self.entries is None or self.last >= self.entries else self.entries - (self.entries - self.last) // 8
            self.event = None

    def tight(self):
        """The last report used more than 80 % of what its call was given (or overflowed it)."""
        return self.last is not None and self.capacity is not None and self.last * 5 > self.capacity * 4

    def report_later(self, ws, offset, capacity=None):
        # the first calls of a shape and calls with tight lists report every time, the others every 8th: an 8-byte copy is
        # still a copy on the stream
        self.calls += 1
        if self.event is not None or (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()):
            return
        if not (self.calls <= 4 or self.calls % 8 == 0 or self.tight()):
            return
        if self.pinned is None:
            self.pinned = torch.empty((1,), dtype=torch.int64, pin_memory=True)
        self.pinned.copy_(ws[offset:offset + 8].view(torch.int64), non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()
        if capacity is not None:
            self.capacity = int(capacity)


def _mesh_workspace(lib, F, N, H, W, bin_size, M, dev, what="meshes", extra=0):
    """(workspace, _Need or None, byte offset of the call's needed-entries word, list entries the workspace was sized for or None);
    what: "meshes" (F faces) or "points"; extra: bytes the entry point takes off the END of the workspace (the marks of the CUDA
    tie order) -- p3d_rasterize_meshes_workspace_bytes counts them in already (include/p3d_amd.h), the short size does not."""
    worst_fn = getattr(lib, f"p3d_rasterize_{what}_workspace_bytes")
    short_fn = getattr(lib, f"p3d_rasterize_{what}_short_workspace_bytes")
    at_fn = getattr(lib, f"p3d_rasterize_{what}_workspace_need_offset")
    worst = worst_fn(F, N, H, W, bin_size, M)
    if SHORT_WORKSPACE == "never" or (SHORT_WORKSPACE != "always" and worst <= SHORT_WORKSPACE_ABOVE):
        WORKSPACE_STATS["last_bytes"], WORKSPACE_STATS["last_entries"] = worst, None
        return _workspace(worst, dev), None, 0, None
    key = (what, dev.index, F, N, H, W, bin_size, M)
    need = _NEEDS.get(key)
    if need is None:
        if len(_NEEDS) >= 64:
            _NEEDS.pop(next(iter(_NEEDS)))
        need = _NEEDS[key] = _Need()
    if not torch.cuda.is_current_stream_capturing():
        need.collect()
    if need.entries is not None:
        entries = need.entries + need.entries // 4 + 4096
    else:
        entries = SHORT_WORKSPACE_FIRST_GUESS if SHORT_WORKSPACE_FIRST_GUESS is not None else 32 * F + (1 << 18)
    nbytes = min(short_fn(F, N, H, W, bin_size, M, int(entries)) + extra, worst)
    WORKSPACE_STATS["short_calls"] += 1
    WORKSPACE_STATS["last_bytes"], WORKSPACE_STATS["last_entries"] = nbytes, int(entries)
    # (the entries go back to the caller, who hands them to report_later: the module-wide stats are another thread's too)
    return _workspace(nbytes, dev), need, at_fn(F, N, H, W, bin_size, M), int(entries)


# ----------------------------------------------------------------------------------------------
# meshes
# ----------------------------------------------------------------------------------------------
# CUDA tie order (include/p3d_amd.h: P3D_RASTER_CUDA_TIE_ORDER).  False: the K nearest faces of a pixel under the total
# order (depth, face index), as the reference's CPU and Python implementations return them.  True: where faces tie EXACTLY in
# depth at the K-th place, the survivors the reference's CUDA kernels keep (bit-identical pix_to_face to a CUDA render; the fine
# kernel marks the pixels concerned and a replay kernel rewrites those: profiles/tie_order_timing.py).  rasterize_points obeys it too (there the reference's CUDA kernels also ORDER tied
# entries by array position: rasterize_points.cu:26-28).  Also: P3D_CUDA_TIE_ORDER=1 in the environment.
CUDA_TIE_ORDER = os.environ.get("P3D_CUDA_TIE_ORDER", "0") not in ("", "0")


def _check_face_verts(face_verts):
    if not (face_verts.dim() == 3 and face_verts.size(1) == 3 and face_verts.size(2) == 3):
        raise RuntimeError("face_verts must have dimensions (num_faces, 3, 3)")


def _mesh_outputs(N, H, W, K, device):
    p2f = torch.empty((N, H, W, K), dtype=torch.int64, device=device)
    zbuf = torch.empty((N, H, W, K), dtype=torch.float32, device=device)
    bary = torch.empty((N, H, W, K, 3), dtype=torch.float32, device=device)
    dists = torch.empty((N, H, W, K), dtype=torch.float32, device=device)
    return p2f, zbuf, bary, dists


def rasterize_meshes(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx, image_size,
                     blur_radius, faces_per_pixel, bin_size, max_faces_per_bin, perspective_correct,
                     clip_barycentric_coords, cull_backfaces):
    """RasterizeMeshes, rasterize_meshes.h:513-562.  Returns (pix_to_face, zbuf, bary, dists).

    The row cover of the output (include/p3d_amd.h: p3d_rasterize_meshes_ex) is written as well and remembered for the
    pix_to_face tensor returned here (_remember_cover): the reference's autograd node hands that very tensor to
    `rasterize_meshes_backward` (renderer/mesh/rasterize_meshes.py:312-357), which then walks only the rows that hold a face --
    the operator signatures stay the reference's."""
    out, cover = _rasterize_meshes_covered(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx,
                                           image_size, blur_radius, faces_per_pixel, bin_size, max_faces_per_bin, perspective_correct,
                                           clip_barycentric_coords, cull_backfaces, want_cover=True)
    if cover is not None:
        _remember_cover(out[0], cover)
    return out


# The row cover of a pix_to_face tensor returned by rasterize_meshes rides ON that tensor object (a Python attribute: it lives
# exactly as long as the object does, and nothing else can ever be mistaken for it -- until round 5 a module-wide map keyed by
# the tensor's address played this part).  The reference's autograd node saves the very object and hands it back to
# `rasterize_meshes_backward` (renderer/mesh/rasterize_meshes.py:291-357: pix_to_face is a non-differentiable output, autograd
# keeps the original).  The cover is used only if the tensor has not been written in place since (version counter) and still has
# the shape the cover was made for; a copy, a view, another tensor: no cover, the backward reads every row.
#
# Writes that bypass the version counter (`pix_to_face.data[...] = x`, an external kernel writing through data_ptr()) are not seen
# by that test: a row the stale cover calls empty would be skipped and the faces written into it would get no gradient.  Three
# ways to be safe: CHECK_COVERS (P3D_CHECK=1) verifies every recalled cover on the device before it is trusted
# (p3d_rasterize_meshes_cover_check: one read of slot 0 of every pixel and a host sync -- about half of what the cover saves) and
# falls back to reading every row, with a warning, when the tensor holds a face the cover does not know of;
# `forget_cover(pix_to_face)` after such a write; RECALL_COVERS = False (P3D_RECALL_COVERS=0) switches the recall off (+0.5 ms on
# the bench batch).  Pinned by tests/test_gpu_cover.py.
RECALL_COVERS = os.environ.get("P3D_RECALL_COVERS", "1") not in ("", "0")
# the forward appends the non-empty words of its cover to a list behind it (include/p3d_amd.h: P3D_RASTER_COVER_LIST); 0: the plain
# cover, the backward builds the list itself (mesh_backward_areas)
COVER_LIST = os.environ.get("P3D_COVER_LIST", "1") not in ("", "0")
# the backward of perspective + clip launches with K = 4 / 8 reads per-face records (include/p3d_amd.h: p3d_gather_face_verts_pre):
# written by the fused vertex node's gather (pytorch3d_amd/rasterize_meshes.py), made in the call for rasterize_meshes_backward.
# 0: formed per sample.  Read at call time, by both.
FACE_PRE = os.environ.get("P3D_FACE_PRE", "1") not in ("", "0")
# The step chain of the fused vertex node (pytorch3d_amd/rasterize_meshes.py: _RasterizeMeshVerts), one switch per item, read at call
# time (profiles/step_chain_mi355x.txt measures each):
#   NULL_NEIGHBOR    no clipping: no clipped_faces_neighbor_idx tensor at all (a null pointer: include/p3d_amd.h) instead of F x -1
#   FUSED_GATHER     the face gather inside the count pass of the binning (p3d_rasterize_meshes_verts_ex) instead of its own launch
#   PRECLEARED_GRAD  the backward's grad_verts allocated by the forward and cleared by that count pass (needs FUSED_GATHER)
NULL_NEIGHBOR = os.environ.get("P3D_NULL_NEIGHBOR", "1") not in ("", "0")
FUSED_GATHER = os.environ.get("P3D_FUSED_GATHER", "1") not in ("", "0")
PRECLEARED_GRAD = os.environ.get("P3D_PRECLEARED_GRAD", "1") not in ("", "0")
CHECK_COVERS = os.environ.get("P3D_CHECK", "0") not in ("", "0")
COVER_RECALLS = [0, 0]  # backward calls without an explicit cover: [found the forward's, found none] (read by tests / profiles)
COVER_CHECKS = [0, 0]   # CHECK_COVERS: [covers verified, of which stale]
_COVER_ATTR = "_p3d_row_cover"


def _remember_cover(p2f, cover):
    setattr(p2f, _COVER_ATTR, (cover, p2f._version))


def forget_cover(pix_to_face):
    """Drop the row cover that rides on a pix_to_face tensor (after writing into it behind autograd's back: see above)."""
    if hasattr(pix_to_face, _COVER_ATTR):
        delattr(pix_to_face, _COVER_ATTR)


def cover_is_current(p2f, cover):
    """CHECK_COVERS: True unless `p2f` holds a face in a 16-pixel row segment that `cover` calls empty (device check + host sync)."""
    N, H, W, K = p2f.shape
    stale = torch.empty((1,), dtype=torch.int32, device=p2f.device)
    _lib.call("p3d_rasterize_meshes_cover_check", "rasterize_meshes_cover_check", p2f.device, p2f, cover, N, H, W, K, stale)
    bad = bool(int(stale.item()))
    COVER_CHECKS[0] += 1
    COVER_CHECKS[1] += int(bad)
    return not bad


def checked_cover(p2f, cover):
    """For the autograd nodes that carry their cover themselves (pytorch3d_amd/rasterize_meshes.py): `cover`, or None when CHECK_COVERS
    finds it stale."""
    if cover is None or not CHECK_COVERS or torch.cuda.is_current_stream_capturing() or cover_is_current(p2f, cover):
        return cover
    import warnings

    warnings.warn("pytorch3d_amd: pix_to_face holds faces its forward's row cover does not know of (written through .data or by "
                  "another kernel since the forward?); the backward reads every row instead", RuntimeWarning)
    return None


def _recall_cover(p2f):
    e = getattr(p2f, _COVER_ATTR, None) if RECALL_COVERS and p2f.dtype == torch.int64 and p2f.is_contiguous() and p2f.dim() == 4 else None
    ok = e is not None and p2f._version == e[1] and e[0].device == p2f.device and \
        tuple(e[0].shape) == (p2f.shape[0], (p2f.shape[1] + 15) // 16, (p2f.shape[2] + 15) // 16)
    if ok and CHECK_COVERS and not torch.cuda.is_current_stream_capturing() and not cover_is_current(p2f, e[0]):
        import warnings

        warnings.warn("pytorch3d_amd: pix_to_face holds faces its forward's row cover does not know of (written through .data or by "
                      "another kernel since the forward?); the backward reads every row instead", RuntimeWarning)
        forget_cover(p2f)
        ok = False
    if not ok:
        COVER_RECALLS[1] += 1
        return None
    COVER_RECALLS[0] += 1
    return e[0]


def _rasterize_meshes_covered(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx, image_size,
                              blur_radius, faces_per_pixel, bin_size, max_faces_per_bin, perspective_correct,
                              clip_barycentric_coords, cull_backfaces, want_cover=True, packed=None):
    """rasterize_meshes + the row cover of its output (include/p3d_amd.h: p3d_rasterize_meshes_ex) for the autograd
    nodes of this package: ((pix_to_face, zbuf, bary, dists), cover or None).
    clipped_faces_neighbor_idx None (the nodes of this package only): no face has a clipped neighbour, a null pointer.
    packed = (verts (V,3) f32, faces (F,3) i64, face_pre (F,4) or None, zero_verts (V,3) or None), all contiguous: face_verts is an
    uninitialised (F,3,3) OUTPUT, gathered inside the call, face_pre and zero_verts with it (p3d_rasterize_meshes_verts_ex)."""
    dev = _same_device(("face_verts", face_verts), ("mesh_to_face_first_idx", mesh_to_face_first_idx),
                       ("num_faces_per_mesh", num_faces_per_mesh),
                       *([("clipped_faces_neighbor_idx", clipped_faces_neighbor_idx)] if clipped_faces_neighbor_idx is not None else []))
    _check_face_verts(face_verts)
    if num_faces_per_mesh.size(0) != mesh_to_face_first_idx.size(0):
        raise RuntimeError("num_faces_per_mesh must have save size first dimension as mesh_to_faces_packed_first_idx")
    if clipped_faces_neighbor_idx is not None and clipped_faces_neighbor_idx.size(0) != face_verts.size(0):
        raise RuntimeError("clipped_faces_neighbor_idx must have save size first dimension as face_verts")
    K = int(faces_per_pixel)
    _check_k(K)
    H, W = _hw(image_size)
    bin_size, M = int(bin_size), int(max_faces_per_bin)
    binned = bin_size > 0 and M > 0
    if binned:
        _num_bins(H, W, bin_size, "RasterizeCoarseCuda")
    fv = _c(face_verts, torch.float32)
    first, count = _c(mesh_to_face_first_idx, torch.int64), _c(num_faces_per_mesh, torch.int64)
    nb = _c(clipped_faces_neighbor_idx, torch.int64) if clipped_faces_neighbor_idx is not None else None
    N, F = count.size(0), fv.size(0)
    lib = _lib.load()
    with torch.cuda.device(dev):
        out = _mesh_outputs(N, H, W, K, dev)
        if out[0].numel() == 0:
            if packed is not None:
                raise RuntimeError("packed vertices with an empty output: gather the faces with p3d_gather_face_verts instead")
            return out, None
        # (the naive launch needs no workspace; with the CUDA tie order it takes one for the lane masks of the marked pixels --
        # without it the replay finds its pixels by reading a pix_to_face entry of every pixel)
        marks = N * ((H + 7) // 8) * ((W + 7) // 8) * 8 + 1024 if CUDA_TIE_ORDER else 0
        ws, need, need_at, entries = _mesh_workspace(lib, F, N, H, W, bin_size, M, dev, extra=marks) if binned else (_workspace(marks, dev), None, 0, None)
        cover, flags = None, _lib.RASTER_CUDA_TIE_ORDER if CUDA_TIE_ORDER else 0
        if want_cover and not CUDA_TIE_ORDER and COVER_LIST:
            # the cover with the list of its non-empty words behind it (include/p3d_amd.h: P3D_RASTER_COVER_LIST): what is handed on
            # is the (N, CY, CX) view of the buffer's first words -- a plain cover to everybody; the backward of this package sees
            # the room behind it (cover_has_list) and takes the list
            words = N * ((H + 15) // 16) * ((W + 15) // 16)
            buf = torch.empty((lib.p3d_rasterize_meshes_cover_list_bytes(N, H, W) // 4,), dtype=torch.int32, device=dev)
            cover = buf[:words].view(N, (H + 15) // 16, (W + 15) // 16)
            flags |= _lib.RASTER_COVER_LIST
        elif want_cover:
            cover = torch.empty((N, (H + 15) // 16, (W + 15) // 16), dtype=torch.int32, device=dev)
        tail = (first, count, nb, F, N, H, W, float(blur_radius), K, bin_size if binned else 0,
                M if binned else 0, int(bool(perspective_correct)), int(bool(clip_barycentric_coords)), int(bool(cull_backfaces)),
                out[0], out[1], out[2], out[3], cover, flags, ws, ws.numel())
        if packed is not None:
            verts, faces, face_pre, zero_verts = packed
            if fv is not face_verts:
                raise RuntimeError("packed vertices: face_verts must be the contiguous float32 buffer the call fills")
            _lib.call("p3d_rasterize_meshes_verts_ex", "rasterize_meshes", dev, verts, faces, verts.size(0), fv, face_pre, zero_verts, *tail)
        else:
            _lib.call("p3d_rasterize_meshes_ex", "rasterize_meshes", dev, fv, *tail)
        if need is not None:
            need.report_later(ws, need_at, entries)
    return out, cover


def _rasterize_meshes_naive(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx,
                            image_size, blur_radius, faces_per_pixel, perspective_correct, clip_barycentric_coords,
                            cull_backfaces):
    """RasterizeMeshesNaive, rasterize_meshes.h:108-156."""
    return rasterize_meshes(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx,
                            image_size, blur_radius, faces_per_pixel, 0, 0, perspective_correct,
                            clip_barycentric_coords, cull_backfaces)


def _rasterize_meshes_coarse(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, image_size, blur_radius, bin_size,
                             max_faces_per_bin):
    """RasterizeMeshesCoarse, rasterize_meshes.h:292-329.  Returns bin_faces (N,BH,BW,M) int32."""
    dev = _same_device(("face_verts", face_verts), ("mesh_to_face_first_idx", mesh_to_face_first_idx),
                       ("num_faces_per_mesh", num_faces_per_mesh))
    _check_face_verts(face_verts)
    H, W = _hw(image_size)
    bin_size, M = int(bin_size), int(max_faces_per_bin)
    BH, BW = _num_bins(H, W, bin_size, "RasterizeCoarseCuda")
    fv = _c(face_verts, torch.float32)
    first, count = _c(mesh_to_face_first_idx, torch.int64), _c(num_faces_per_mesh, torch.int64)
    N, F = count.size(0), fv.size(0)
    lib = _lib.load()
    out = torch.empty((N, BH, BW, M), dtype=torch.int32, device=dev)
    if out.numel() == 0:
        return out
    ws = _workspace(lib.p3d_rasterize_meshes_workspace_bytes(F, N, H, W, bin_size, M), dev)
    _lib.call("p3d_rasterize_meshes_coarse", "_rasterize_meshes_coarse", dev, fv, first, count, F, N, H, W, float(blur_radius), bin_size, M, out,
              ws, ws.numel())
    return out


def _rasterize_meshes_fine(face_verts, bin_faces, clipped_faces_neighbor_idx, image_size, blur_radius, bin_size,
                           faces_per_pixel, perspective_correct, clip_barycentric_coords, cull_backfaces):
    """RasterizeMeshesFine, rasterize_meshes.h:406-441."""
    dev = _same_device(("face_verts", face_verts), ("bin_faces", bin_faces),
                       ("clipped_faces_neighbor_idx", clipped_faces_neighbor_idx))
    _check_face_verts(face_verts)
    if bin_faces.dim() != 4:
        raise RuntimeError("bin_faces must have 4 dimensions")
    if clipped_faces_neighbor_idx.size(0) != face_verts.size(0):
        raise RuntimeError("clipped_faces_neighbor_idx must have the same first dimension as face_verts")
    K = int(faces_per_pixel)
    if K > kMaxPointsPerPixel:
        raise RuntimeError("Must have num_closest <= 150")
    H, W = _hw(image_size)
    fv = _c(face_verts, torch.float32)
    bf = _c(bin_faces, torch.int32)
    nb = _c(clipped_faces_neighbor_idx, torch.int64)
    N, BH, BW, M = bf.shape
    lib = _lib.load()
    out = _mesh_outputs(N, H, W, K, dev)
    if out[0].numel() == 0:
        return out
    ws = _workspace(lib.p3d_rasterize_fine_workspace_bytes(N, BH, BW, M), dev)
    _lib.call("p3d_rasterize_meshes_fine", "_rasterize_meshes_fine", dev, fv, bf, nb, fv.size(0), N, BH, BW, M, H, W, float(blur_radius),
              int(bin_size), K, int(bool(perspective_correct)), int(bool(clip_barycentric_coords)), int(bool(cull_backfaces)), out[0], out[1],
              out[2], out[3], ws, ws.numel())
    return out


def checked_cover_of(cover, N, H, W):
    """A row cover after checking that it is the cover of an (N, H, W, .) rasterization; None stays None (a null pointer)."""
    if cover is None:
        return None
    if cover.dtype != torch.int32 or tuple(cover.shape) != (N, (H + 15) // 16, (W + 15) // 16) or not cover.is_contiguous():
        raise RuntimeError("row cover does not belong to this pix_to_face")
    return cover


def cover_ptr(cover, N, H, W):
    """Its pointer, for raw calls on _lib.load() (the tests), like _ptr and _stream above."""
    return None if cover is None else _ptr(checked_cover_of(cover, N, H, W))


def cover_has_list(cover, N, H, W):
    """Is `cover` the front of a buffer of p3d_rasterize_meshes_cover_list_bytes, as _rasterize_meshes_covered makes them (the list of
    its non-empty words behind it)?  A clone, a cover from elsewhere, a slice: no."""
    if cover is None or cover.storage_offset() != 0 or not cover.is_contiguous():
        return False
    need = _lib.load().p3d_rasterize_meshes_cover_list_bytes(N, H, W)
    return need > 0 and cover.untyped_storage().nbytes() == need


def backward_workspace(cover, N, H, W, dev):
    """Scratch of the covered backward (the list of areas with work); empty without a cover, or when the cover brings its list."""
    n = _lib.load().p3d_rasterize_meshes_backward_workspace_bytes(N, H, W) if (cover is not None and not cover_has_list(cover, N, H, W)) else 0
    return _workspace(n, dev)


# The one call into p3d_rasterize_meshes_backward_ex, for rasterize_meshes_backward below and the autograd nodes of
# pytorch3d_amd/rasterize_meshes.py.  Which kernels a backward launches depends on the caller and the switches as follows:
#
#   caller                               face_pre                                          cover
#   rasterize_meshes_backward,           made in the call (BWD_MAKE_FACE_PRE) iff          the list if cover_has_list; else the
#   _RasterizeFaceVerts (faces None)     FACE_PRE and persp and clip and K in (4, 8)       workspace + mesh_backward_areas if a
#                                                                                          cover; else every row
#   _RasterizeMeshVerts                  the gather's records iff they exist and (the      the same
#                                        cover has a list or there is no cover)
#   _RasterizeMeshWorld                  never                                             the same
#
# QUIRK, kept on purpose: _RasterizeMeshVerts with a cover WITHOUT a list (COVER_LIST off, or CUDA_TIE_ORDER) forms the
# reciprocals per sample although it has the records -- the entry point that took the records had no workspace argument.
# Dropping the clause changes results on degenerate edges: a fix of its own.
def _mesh_backward(face_verts, faces, V, pix_to_face, grad_zbuf, grad_bary, grad_dists, perspective_correct, clip_barycentric_coords,
                   cover, face_pre=None, zeroed_out=None):
    """grad_face_verts (F,3,3) when faces is None, else grad_verts (V,3) through faces (F,3).  Missing grads count as zeros;
    cover: the row cover of THIS pix_to_face or None; face_pre: the records of p3d_gather_face_verts_pre (faces given) or None.
    zeroed_out (faces given): a (V,3) float32 buffer of zeros that nobody else holds -- the forward's count pass cleared it
    (p3d_rasterize_meshes_verts_ex: zero_verts): it becomes the result, and the call clears nothing (BWD_GRAD_OUT_ZEROED).  The
    deterministic form needs no zeros and ignores it."""
    dev = pix_to_face.device
    zeros = lambda *tail: torch.zeros(tuple(pix_to_face.shape) + tail, dtype=torch.float32, device=dev)
    gz = _c(grad_zbuf, torch.float32) if grad_zbuf is not None else zeros()
    gb = _c(grad_bary, torch.float32) if grad_bary is not None else zeros(3)
    gd = _c(grad_dists, torch.float32) if grad_dists is not None else zeros()
    fv, p2f = _c(face_verts, torch.float32), _c(pix_to_face, torch.int64)
    N, H, W, K = p2f.shape
    F = fv.size(0)
    persp, clip = int(bool(perspective_correct)), int(bool(clip_barycentric_coords))
    has_list = cover_has_list(cover, N, H, W)
    flags = _lib.BWD_COVER_HAS_LIST if has_list else 0
    if faces is None:
        out = torch.empty((F, 3, 3), dtype=torch.float32, device=dev)
        if FACE_PRE and persp and clip and K in (4, 8):
            face_pre = torch.empty((F, 4), dtype=torch.float32, device=dev)  # scratch the call fills first (one small launch)
            flags |= _lib.BWD_MAKE_FACE_PRE
    else:
        faces = _c(faces, torch.int64)
        # (zeros: with F == 0 nothing is called -- a null faces pointer would ask for the per-face form)
        if zeroed_out is not None and F and not _ordered() and tuple(zeroed_out.shape) == (V, 3) and zeroed_out.dtype == torch.float32 \
                and zeroed_out.device == dev and zeroed_out.is_contiguous():
            out = zeroed_out
            flags |= _lib.BWD_GRAD_OUT_ZEROED
        else:
            out = (torch.empty if F else torch.zeros)((V, 3), dtype=torch.float32, device=dev)
        if not (has_list or cover is None):
            face_pre = None  # the QUIRK above
    if F == 0:
        return out
    if _ordered():
        # the same bits whatever the cover, the records or the caller (the cover only says where NOT to look; the list below
        # is made from pix_to_face itself)
        lib = _lib.load()
        hits = _sorted_hits(p2f)
        corners = _sorted_corners(faces, V) if faces is not None else None
        ws = _workspace(lib.p3d_rasterize_meshes_backward_ordered_workspace_bytes(F, int(faces is not None), hits.numel()), dev)
        _lib.call("p3d_rasterize_meshes_backward_ordered", "rasterize_meshes_backward", dev, fv, faces, p2f, gz, gb, gd, hits, hits.numel(),
                  corners, corners.numel() if corners is not None else 0, F, V, N, H, W, K, persp, clip, out, ws, ws.numel())
        return out
    ws = backward_workspace(cover, N, H, W, dev)
    _lib.call("p3d_rasterize_meshes_backward_ex", "rasterize_meshes_backward", dev, fv, faces, face_pre, p2f, gz, gb, gd,
              checked_cover_of(cover, N, H, W), F, V, N, H, W, K, persp, clip, flags, out, ws, ws.numel())
    return out


def scatter_face_grads(grad_face_verts, faces, V):
    """The backward of `verts[faces]` (include/p3d_amd.h: p3d_scatter_face_grads[_ordered]): grad_face_verts (F, 3, 3), faces (F, 3)
    int64 -> grad_verts (V, 3)."""
    dev = grad_face_verts.device
    g, faces = _c(grad_face_verts, torch.float32), _c(faces, torch.int64)
    F = faces.shape[0]
    lib = _lib.load()
    out = torch.empty((V, 3), dtype=torch.float32, device=dev)
    if not V:
        return out
    if _ordered():
        corners = _sorted_corners(faces, V)
        ws = _workspace(lib.p3d_scatter_face_grads_ordered_workspace_bytes(F), dev)
        _lib.call("p3d_scatter_face_grads_ordered", "scatter_face_grads", dev, g, faces, corners, corners.numel(), V, F, out, ws, ws.numel())
    else:
        _lib.call("p3d_scatter_face_grads", "scatter_face_grads", dev, g, faces, V, F, out)
    return out


def rasterize_meshes_backward(face_verts, pix_to_face, grad_zbuf, grad_bary, grad_dists, perspective_correct,
                              clip_barycentric_coords, _cover=None):
    """RasterizeMeshesBackward, rasterize_meshes.h:211-252.  Returns grad_face_verts (F,3,3).
    _cover (not part of the reference's signature): the row cover of THIS pix_to_face from _rasterize_meshes_covered."""
    _same_device(("face_verts", face_verts), ("pix_to_face", pix_to_face), ("grad_zbuf", grad_zbuf), ("grad_bary", grad_bary),
                 ("grad_dists", grad_dists))
    if _cover is None:
        _cover = _recall_cover(pix_to_face)  # the forward of this very tensor left its row cover (see rasterize_meshes)
    return _mesh_backward(face_verts, None, 0, pix_to_face, grad_zbuf, grad_bary, grad_dists, perspective_correct,
                          clip_barycentric_coords, _cover)


# ----------------------------------------------------------------------------------------------
# point clouds
# ----------------------------------------------------------------------------------------------
def _check_points(points):
    if not (points.dim() == 2 and points.size(1) == 3):
        raise RuntimeError("points must have dimensions (num_points, 3)")


def _point_outputs(N, H, W, K, device):
    idx = torch.empty((N, H, W, K), dtype=torch.int32, device=device)
    zbuf = torch.empty((N, H, W, K), dtype=torch.float32, device=device)
    dists = torch.empty((N, H, W, K), dtype=torch.float32, device=device)
    return idx, zbuf, dists


_SPLAT_MODES = {"alpha": _lib.COMPOSITE_ALPHA, "norm": _lib.COMPOSITE_NORM_SUM}  # AlphaCompositor / NormWeightedCompositor


def _rasterize_points(who, points, cloud_to_packed_first_idx, num_points_per_cloud, image_size, radius, points_per_pixel, bin_size,
                      max_points_per_bin, features=None, inv_r2=0.0, mode="alpha"):
    """The one call into p3d_rasterize_points_ex, for rasterize_points and rasterize_points_composite: ((idxs int32, zbuf, dists2),
    images (N, H, W, C) or None).  features None: no compositing, in the tie order CUDA_TIE_ORDER asks for; else the default order."""
    splat = features is not None
    dev = _same_device(("points", points), ("cloud_to_packed_first_idx", cloud_to_packed_first_idx),
                       ("num_points_per_cloud", num_points_per_cloud), ("radius", radius), *((("features", features),) if splat else ()))
    _check_points(points)
    if radius.dim() != 1 or radius.size(0) != points.size(0):
        raise RuntimeError("radius must be of shape (P,)")
    if splat and (features.dim() != 2 or features.size(0) != points.size(0) or not 1 <= features.size(1) <= 4):
        raise RuntimeError("features must be of shape (P, C) with C in 1..4")
    K = int(points_per_pixel)
    _check_k(K)
    H, W = _hw(image_size)
    bin_size, M = int(bin_size), int(max_points_per_bin)
    binned = bin_size > 0 and M > 0
    if binned:
        _num_bins(H, W, bin_size, "RasterizeCoarseCuda")
    pts, rad = _c(points, torch.float32), _c(radius, torch.float32)
    feats = _c(features, torch.float32) if splat else None
    first, count = _c(cloud_to_packed_first_idx, torch.int64), _c(num_points_per_cloud, torch.int64)
    N, P, C = count.size(0), pts.size(0), feats.size(1) if splat else 0
    lib = _lib.load()
    with torch.cuda.device(dev):
        out = _point_outputs(N, H, W, K, dev)
        images = torch.empty((N, H, W, C), dtype=torch.float32, device=dev) if splat else None
        if (images if splat else out[0]).numel() == 0:
            return out, images
        ws, need, need_at, entries = _mesh_workspace(lib, P, N, H, W, bin_size, M, dev, "points") if binned else (_workspace(0, dev), None, 0, None)
        flags = _lib.RASTER_CUDA_TIE_ORDER if CUDA_TIE_ORDER and not splat else 0
        _lib.call("p3d_rasterize_points_ex", who, dev, pts, first, count, rad, P, N, H, W, K, bin_size if binned else 0, M if binned else 0, out[0],
                  out[1], out[2], _SPLAT_MODES[mode] if splat else 0, feats, C, float(inv_r2), images, flags, ws, ws.numel())
        if need is not None:
            need.report_later(ws, need_at, entries)
    return out, images


def rasterize_points(points, cloud_to_packed_first_idx, num_points_per_cloud, image_size, radius, points_per_pixel,
                     bin_size, max_points_per_bin):
    """RasterizePoints, rasterize_points.h:343-374.  Returns (idxs int32, zbuf, dists2)."""
    return _rasterize_points("rasterize_points", points, cloud_to_packed_first_idx, num_points_per_cloud, image_size, radius,
                             points_per_pixel, bin_size, max_points_per_bin)[0]


def _rasterize_points_naive(points, cloud_to_packed_first_idx, num_points_per_cloud, image_size, radius,
                            points_per_pixel):
    """RasterizePointsNaive, rasterize_points.h:70-99."""
    return rasterize_points(points, cloud_to_packed_first_idx, num_points_per_cloud, image_size, radius,
                            points_per_pixel, 0, 0)


def _rasterize_points_coarse(points, cloud_to_packed_first_idx, num_points_per_cloud, image_size, radius, bin_size,
                             max_points_per_bin):
    """RasterizePointsCoarse, rasterize_points.h:146-191.  Returns bin_points (N,BH,BW,M) int32."""
    dev = _same_device(("points", points), ("cloud_to_packed_first_idx", cloud_to_packed_first_idx),
                       ("num_points_per_cloud", num_points_per_cloud), ("radius", radius))
    _check_points(points)
    H, W = _hw(image_size)
    bin_size, M = int(bin_size), int(max_points_per_bin)
    BH, BW = _num_bins(H, W, bin_size, "RasterizeCoarseCuda")
    pts, rad = _c(points, torch.float32), _c(radius, torch.float32)
    first, count = _c(cloud_to_packed_first_idx, torch.int64), _c(num_points_per_cloud, torch.int64)
    N, P = count.size(0), pts.size(0)
    lib = _lib.load()
    out = torch.empty((N, BH, BW, M), dtype=torch.int32, device=dev)
    if out.numel() == 0:
        return out
    ws = _workspace(lib.p3d_rasterize_points_workspace_bytes(P, N, H, W, bin_size, M), dev)
    _lib.call("p3d_rasterize_points_coarse", "_rasterize_points_coarse", dev, pts, first, count, rad, P, N, H, W, bin_size, M, out, ws,
              ws.numel())
    return out


def _rasterize_points_fine(points, bin_points, image_size, radius, bin_size, points_per_pixel):
    """RasterizePointsFine, rasterize_points.h:222-247."""
    dev = _same_device(("points", points), ("bin_points", bin_points), ("radius", radius))
    _check_points(points)
    K = int(points_per_pixel)
    if K > kMaxPointsPerPixel:
        raise RuntimeError("Must have num_closest <= 150")
    H, W = _hw(image_size)
    pts, rad = _c(points, torch.float32), _c(radius, torch.float32)
    bp = _c(bin_points, torch.int32)
    N, BH, BW, M = bp.shape
    lib = _lib.load()
    out = _point_outputs(N, H, W, K, dev)
    if out[0].numel() == 0:
        return out
    ws = _workspace(lib.p3d_rasterize_fine_workspace_bytes(N, BH, BW, M), dev)
    _lib.call("p3d_rasterize_points_fine", "_rasterize_points_fine", dev, pts, bp, rad, pts.size(0), N, BH, BW, M, H, W, int(bin_size), K,
              out[0], out[1], out[2], ws, ws.numel())
    return out


def rasterize_points_backward(points, idxs, grad_zbuf, grad_dists):
    """RasterizePointsBackward, rasterize_points.h:281-305.  Returns grad_points (P,3)."""
    dev = _same_device(("points", points), ("idxs", idxs), ("grad_zbuf", grad_zbuf), ("grad_dists", grad_dists))
    pts = _c(points, torch.float32)
    ix = _c(idxs, torch.int32)
    gz, gd = _c(grad_zbuf, torch.float32), _c(grad_dists, torch.float32)
    N, H, W, K = ix.shape
    P = pts.size(0)
    lib = _lib.load()
    out = torch.empty((P, 3), dtype=torch.float32, device=dev)
    if P == 0:
        return out
    if _ordered():
        hits = _sorted_hits(ix)
        ws = _workspace(lib.p3d_rasterize_points_backward_ordered_workspace_bytes(hits.numel()), dev)
        _lib.call("p3d_rasterize_points_backward_ordered", "rasterize_points_backward", dev, pts, ix, gz, gd, hits, hits.numel(), P, N, H, W, K,
                  out, ws, ws.numel())
    else:
        _lib.call("p3d_rasterize_points_backward", "rasterize_points_backward", dev, pts, ix, gz, gd, P, N, H, W, K, out)
    return out


def inv_r2_of(radius):
    """float32(1) / float32(r * r): `dists / (r * r)` with a Python scalar is a multiplication by this on the device
    (renderer/points/renderer.py:62-64 under torch's div-by-scalar kernel)."""
    import numpy as np

    return float(np.float32(1.0) / np.float32(float(radius) * float(radius)))


def rasterize_points_composite(points, cloud_to_packed_first_idx, num_points_per_cloud, image_size, radius, features, inv_r2,
                               points_per_pixel, bin_size, max_points_per_bin, mode="alpha"):
    """include/p3d_amd.h: p3d_rasterize_points_ex with images.  rasterize_points's arguments + features (P, C), C in 1..4, inv_r2
    (inv_r2_of) and the compositor ("alpha" / "norm"); CUDA_TIE_ORDER does not apply.  Returns (idxs int32, zbuf, dists2, images
    (N, H, W, C))."""
    out, images = _rasterize_points("rasterize_points_composite", points, cloud_to_packed_first_idx, num_points_per_cloud, image_size,
                                    radius, points_per_pixel, bin_size, max_points_per_bin, features, inv_r2, mode)
    return out + (images,)


def rasterize_points_composite_backward(points, features, idxs, dists, grad_images, inv_r2, mode="alpha"):
    """include/p3d_amd.h: p3d_rasterize_points_composite_backward.  Returns (grad_points (P, 3), grad_features (P, C))."""
    dev = _same_device(("points", points), ("features", features), ("idxs", idxs), ("dists", dists), ("grad_images", grad_images))
    pts, feats = _c(points, torch.float32), _c(features, torch.float32)
    ix, ds, gi = _c(idxs, torch.int32), _c(dists, torch.float32), _c(grad_images, torch.float32)
    N, H, W, K = ix.shape
    P, C = pts.size(0), feats.size(1)
    if tuple(gi.shape) != (N, H, W, C):
        raise RuntimeError("grad_images must be of shape (N, H, W, C)")
    lib = _lib.load()
    gp = torch.empty((P, 3), dtype=torch.float32, device=dev)
    gf = torch.empty((P, C), dtype=torch.float32, device=dev)
    if P == 0:
        return gp, gf
    if _ordered():
        hits = _sorted_hits(ix)
        ws = _workspace(lib.p3d_rasterize_points_composite_backward_ordered_workspace_bytes(N, H, W, K, C, hits.numel()), dev)
        _lib.call("p3d_rasterize_points_composite_backward_ordered", "rasterize_points_composite_backward", dev, _SPLAT_MODES[mode], pts, feats,
                  ix, ds, gi, hits, hits.numel(), P, C, N, H, W, K, float(inv_r2), gp, gf, ws, ws.numel())
    else:
        _lib.call("p3d_rasterize_points_composite_backward", "rasterize_points_composite_backward", dev, _SPLAT_MODES[mode], pts, feats, ix, ds,
                  gi, P, C, N, H, W, K, float(inv_r2), gp, gf)
    return gp, gf


# ----------------------------------------------------------------------------------------------
# compositors
# ----------------------------------------------------------------------------------------------
_ALPHA, _NORM, _SUM = _lib.COMPOSITE_ALPHA, _lib.COMPOSITE_NORM_SUM, _lib.COMPOSITE_SUM


def _composite_check(features, alphas, points_idx):
    dev = _same_device(("features", features), ("alphas", alphas), ("points_idx", points_idx))
    if features.dim() != 2:
        raise RuntimeError("features must have 2 dimensions (C, P)")
    if alphas.dim() != 4 or points_idx.dim() != 4 or alphas.shape != points_idx.shape:
        raise RuntimeError("alphas and points_idx must both have shape (N, K, H, W)")
    if features.dtype != torch.float32 or alphas.dtype != torch.float32 or points_idx.dtype != torch.int64:
        raise RuntimeError("features/alphas must be float32 and points_idx int64")
    return dev


def _feature_layout(features):
    """(tensor to hand over, its (channel, point) element strides, interleaved?).  Two layouts go to the kernels as they are: the
    contiguous (C, P) tensor of the reference's operators, and the transposed view of a contiguous (P, C) tensor -- what
    PointsRenderer passes (renderer/points/renderer.py:67); there a point's channels are adjacent and the gathers of a pixel cost
    one memory request per entry instead of C (include/p3d_amd.h: p3d_composite_forward).  Anything else is copied."""
    C, P = features.shape
    st = features.stride()
    if C > 1 and P > 1 and st[0] == 1 and st[1] == C:
        return features, (1, C), True
    f = features.contiguous()
    return f, (P, 1), False


def _composite_forward(mode, name, features, alphas, points_idx):
    dev = _composite_check(features, alphas, points_idx)
    feats, fst, _ = _feature_layout(features)
    N, K, H, W = alphas.shape
    C, P = feats.shape
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=dev)
    if out.numel() == 0:
        return out
    _lib.call("p3d_composite_forward", name, dev, mode, feats, fst, alphas, points_idx, N, C, P, K, H, W, alphas.stride(), points_idx.stride(), out)
    return out


def _composite_backward(mode, name, grad_outputs, features, alphas, points_idx):
    dev = _composite_check(features, alphas, points_idx)
    _need_gpu(grad_outputs, "grad_outputs")
    feats, fst, interleaved = _feature_layout(features)
    go = _c(grad_outputs, torch.float32)
    N, K, H, W = alphas.shape
    C, P = feats.shape
    lib = _lib.load()
    # grad_features in the layout of the features: (C, P) planes, or -- for the renderers' transposed (P, C) view -- the
    # transposed view of a (P, C) tensor (the permute in front of the operator then hands autograd a contiguous gradient)
    if interleaved:
        gf = torch.empty((P, C), dtype=torch.float32, device=dev).t()
    else:
        gf = torch.empty((C, P), dtype=torch.float32, device=dev)
    ga = torch.empty((N, K, H, W), dtype=torch.float32, device=dev)
    if _ordered():
        hits = _sorted_hits(points_idx)  # in the logical (N, K, H, W) order, whatever the strides
        ws = _workspace(lib.p3d_composite_backward_ordered_workspace_bytes(N, K, H, W, C, hits.numel()), dev)
        _lib.call("p3d_composite_backward_ordered", name, dev, mode, go, feats, fst, alphas, points_idx, hits, hits.numel(), N, C, P, K, H, W,
                  alphas.stride(), points_idx.stride(), gf, fst, ga, ws, ws.numel())
    else:
        _lib.call("p3d_composite_backward", name, dev, mode, go, feats, fst, alphas, points_idx, N, C, P, K, H, W, alphas.stride(),
                  points_idx.stride(), gf, fst, ga)
    return gf, ga


def accum_alphacomposite(features, alphas, points_idx):
    """alphaCompositeForward, compositing/alpha_composite.h:59-82."""
    return _composite_forward(_ALPHA, "accum_alphacomposite", features, alphas, points_idx)


def accum_alphacomposite_backward(grad_outputs, features, alphas, points_idx):
    """alphaCompositeBackward, alpha_composite.h:84-115.  Returns (grad_features, grad_alphas)."""
    return _composite_backward(_ALPHA, "accum_alphacomposite_backward", grad_outputs, features, alphas, points_idx)


def accum_weightedsumnorm(features, alphas, points_idx):
    """weightedSumNormForward, compositing/norm_weighted_sum.h:57-80."""
    return _composite_forward(_NORM, "accum_weightedsumnorm", features, alphas, points_idx)


def accum_weightedsumnorm_backward(grad_outputs, features, alphas, points_idx):
    return _composite_backward(_NORM, "accum_weightedsumnorm_backward", grad_outputs, features, alphas, points_idx)


def accum_weightedsum(features, alphas, points_idx):
    """weightedSumForward, compositing/weighted_sum.h:55-78."""
    return _composite_forward(_SUM, "accum_weightedsum", features, alphas, points_idx)


def accum_weightedsum_backward(grad_outputs, features, alphas, points_idx):
    return _composite_backward(_SUM, "accum_weightedsum_backward", grad_outputs, features, alphas, points_idx)


# ----------------------------------------------------------------------------------------------
# interpolate_face_attributes
# ----------------------------------------------------------------------------------------------
_DTYPES = {torch.float32: 0, torch.float64: 1}


def interp_face_attrs_forward(pix_to_face, barycentric_coords, face_attrs):
    """InterpFaceAttrsForward, interp_face_attrs/interp_face_attrs.h:46-66.  Returns pix_attrs (P, D)."""
    dev = _same_device(("pix_to_face", pix_to_face), ("barycentric_coords", barycentric_coords),
                       ("face_attributes", face_attrs))
    if barycentric_coords.dtype != face_attrs.dtype or face_attrs.dtype not in _DTYPES:
        raise RuntimeError("barycentric_coords and face_attributes must have the same floating dtype")
    P = pix_to_face.size(0)
    if barycentric_coords.dim() != 2 or barycentric_coords.size(0) != P or barycentric_coords.size(1) != 3:
        raise RuntimeError("barycentric_coords must have size (P, 3)")
    if face_attrs.dim() != 3 or face_attrs.size(1) != 3:
        raise RuntimeError("face_attrs must have size (F, 3, D)")
    p2f = _c(pix_to_face, torch.int64)
    bary, attrs = barycentric_coords.contiguous(), face_attrs.contiguous()
    F, _, D = attrs.shape
    out = torch.empty((P, D), dtype=attrs.dtype, device=dev)
    if out.numel() == 0:
        return out
    _lib.call("p3d_interp_face_attrs_forward", "interp_face_attrs_forward", dev, _DTYPES[attrs.dtype], p2f, bary, attrs, P, F, D, out)
    return out


def interp_face_attrs_backward(pix_to_face, barycentric_coords, face_attrs, grad_pix_attrs, image_shape=None):
    """InterpFaceAttrsBackward, interp_face_attrs.h:95-116.  Returns (grad_bary (P,3), grad_face_attrs (F,3,D)).
    image_shape=(N,H,W,K) (ours, optional): the P samples are image-shaped fragments -> tile-mapped kernel."""
    dev = _same_device(("pix_to_face", pix_to_face), ("barycentric_coords", barycentric_coords),
                       ("face_attributes", face_attrs), ("pix_attrs", grad_pix_attrs))
    if not (barycentric_coords.dtype == face_attrs.dtype == grad_pix_attrs.dtype) or face_attrs.dtype not in _DTYPES:
        raise RuntimeError("barycentric_coords, face_attributes and pix_attrs must have the same floating dtype")
    if _ordered() and face_attrs.dtype != torch.float32:
        raise RuntimeError("InterpFaceAttrsBackwardCuda does not have a deterministic implementation for float64 (float32 has one)")
    P = pix_to_face.size(0)
    if barycentric_coords.dim() != 2 or barycentric_coords.size(0) != P or barycentric_coords.size(1) != 3:
        raise RuntimeError("barycentric_coords must have size (P, 3)")
    if face_attrs.dim() != 3 or face_attrs.size(1) != 3:
        raise RuntimeError("face_attrs must have size (F, 3, D)")
    F, _, D = face_attrs.shape
    if grad_pix_attrs.dim() != 2 or grad_pix_attrs.size(0) != P or grad_pix_attrs.size(1) != D:
        raise RuntimeError("grad_pix_attrs must have size (P, D)")
    p2f = _c(pix_to_face, torch.int64)
    bary, attrs, g = barycentric_coords.contiguous(), face_attrs.contiguous(), grad_pix_attrs.contiguous()
    lib = _lib.load()
    gb = torch.empty((P, 3), dtype=attrs.dtype, device=dev)
    gf = torch.empty((F, 3, D), dtype=attrs.dtype, device=dev)
    if _ordered():  # (image-shaped or not: one entry, the same bits)
        hits = _sorted_hits(p2f)
        ws = _workspace(lib.p3d_interp_face_attrs_backward_ordered_workspace_bytes(D, hits.numel()), dev)
        _lib.call("p3d_interp_face_attrs_backward_ordered", "interp_face_attrs_backward", dev, p2f, bary, attrs, g, hits, hits.numel(), P, F, D,
                  gb, gf, ws, ws.numel())
        return gb, gf
    if (image_shape is not None and attrs.dtype == torch.float32 and 1 <= D <= 4 and F > 0
            and image_shape[0] * image_shape[1] * image_shape[2] * image_shape[3] == P):
        n_, h_, w_, k_ = (int(x) for x in image_shape)
        _lib.call("p3d_interp_face_attrs_backward_nhwk", "interp_face_attrs_backward", dev, p2f, bary, attrs, g, n_, h_, w_, k_, F, D, gb, gf)
        return gb, gf
    _lib.call("p3d_interp_face_attrs_backward", "interp_face_attrs_backward", dev, _DTYPES[attrs.dtype], p2f, bary, attrs, g, P, F, D, gb, gf)
    return gb, gf


# ----------------------------------------------------------------------------------------------
# blending
# ----------------------------------------------------------------------------------------------
def sigmoid_alpha_blend(distances, pix_to_face, sigma):
    """SigmoidAlphaBlend, blending/sigmoid_alpha_blend.h:73-84.  distances, pix_to_face (N,H,W,K) -> alphas (N,H,W)."""
    dev = _same_device(("distances", distances), ("pix_to_face", pix_to_face))
    if distances.dim() != 4 or pix_to_face.shape != distances.shape:
        raise RuntimeError("distances and pix_to_face must both have shape (N, H, W, K)")
    d, p2f = _aligned(_c(distances, torch.float32)), _aligned(_c(pix_to_face, torch.int64))
    N, H, W, K = d.shape
    out = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    if out.numel() == 0:
        return out
    _lib.call("p3d_sigmoid_alpha_blend_forward", "sigmoid_alpha_blend", dev, d, p2f, float(sigma), N * H * W, K, out)
    return out


def sigmoid_alpha_blend_backward(grad_alphas, alphas, distances, pix_to_face, sigma):
    """SigmoidAlphaBlendBackward, sigmoid_alpha_blend.h:86-103.  Returns grad_distances (N,H,W,K)."""
    dev = _same_device(("distances", distances), ("pix_to_face", pix_to_face), ("alphas", alphas),
                       ("grad_alphas", grad_alphas))
    d, p2f = _aligned(_c(distances, torch.float32)), _aligned(_c(pix_to_face, torch.int64))
    ga, al = _c(grad_alphas, torch.float32), _c(alphas, torch.float32)
    N, H, W, K = d.shape
    out = torch.empty((N, H, W, K), dtype=torch.float32, device=dev)
    if out.numel() == 0:
        return out
    _lib.call("p3d_sigmoid_alpha_blend_backward", "sigmoid_alpha_blend_backward", dev, ga, al, d, p2f, float(sigma), N * H * W, K, out)
    return out


# ----------------------------------------------------------------------------------------------
# nearest neighbours (csrc/knn.hip).  NOT in HOT_PATH_EXPORTS: the shim module keeps `pytorch3d._C.knn_points_idx` a stub that
# raises; pytorch3d_amd.knn.knn_points (and, under patch_python, the reference's knn_points) come here.
def _knn_check(p1, p2, lengths1, lengths2, K, who):
    dev = _same_device(("p1", p1), ("p2", p2))
    if p1.dim() != 3 or p2.dim() != 3 or p1.shape[0] != p2.shape[0] or p1.shape[2] != p2.shape[2]:
        raise RuntimeError(f"{who}: p1 (N, P1, D) and p2 (N, P2, D) must share N and D")
    if p1.shape[2] not in (2, 3) or not 1 <= K <= _lib.KNN_MAX_K:
        raise RuntimeError(f"{who}: the kernels take D in (2, 3) and 1 <= K <= {_lib.KNN_MAX_K}; pytorch3d_amd.knn.knn_points has a "
                           "torch formulation for the rest")
    out = []
    for name, t in (("lengths1", lengths1), ("lengths2", lengths2)):
        if t is not None:
            _same_device(("p1", p1), (name, t))
            if t.shape != (p1.shape[0],):
                raise RuntimeError(f"{who}: {name} must have shape (N,)")
            t = _c(t, torch.int64)
        out.append(t)
    return dev, out[0], out[1]


def knn_points_idx(p1, p2, lengths1, lengths2, norm, K, version=-1, _out=None):
    """KNearestNeighborIdx (knn.h): (idx (N, P1, K) int64, dists (N, P1, K)), sorted ascending by (dist, j); `version` is ignored.
    lengths1 / lengths2 may be None (every cloud full).  _out (not part of the reference's signature): (idx, dists) buffers to write
    into -- the kernel writes every entry."""
    if norm not in (1, 2):
        raise ValueError("Support for 1 or 2 norm.")
    K = int(K)
    dev, lengths1, lengths2 = _knn_check(p1, p2, lengths1, lengths2, K, "knn_points_idx")
    p1, p2 = _c(p1, torch.float32), _c(p2, torch.float32)
    N, P1, D = p1.shape
    if _out is None:
        idx = torch.empty((N, P1, K), dtype=torch.int64, device=dev)
        dists = torch.empty((N, P1, K), dtype=torch.float32, device=dev)
    else:
        idx, dists = _out
        if (idx.shape != (N, P1, K) or dists.shape != (N, P1, K) or idx.dtype != torch.int64 or dists.dtype != torch.float32
                or not idx.is_contiguous() or not dists.is_contiguous() or idx.device != dev or dists.device != dev):
            raise RuntimeError("knn_points_idx: _out must be contiguous (N, P1, K) int64 and float32 tensors on the inputs' GPU")
    _lib.call("p3d_knn_points_forward", "knn_points_idx", dev, p1, p2, lengths1, lengths2, N, P1, p2.shape[1], D, K, int(norm), idx, dists)
    return idx, dists


def knn_points_backward(p1, p2, lengths1, lengths2, idxs, norm, grad_dists, _needs=(True, True)):
    """KNearestNeighborBackward (knn.h): (grad_p1 (N, P1, D), grad_p2 (N, P2, D)).  grad_p1 is a gather; grad_p2 a scatter with
    float atomics or, under torch.use_deterministic_algorithms(True), the ordered sum.  _needs (not part of the reference's
    signature): which of the two to compute (the other is None)."""
    from . import knn as _knn

    if norm not in (1, 2):
        raise ValueError("Support for 1 or 2 norm.")
    _same_device(("p1", p1), ("idxs", idxs), ("grad_dists", grad_dists))
    if idxs.dim() != 3 or idxs.shape[:2] != p1.shape[:2] or grad_dists.shape != idxs.shape:
        raise RuntimeError("knn_points_backward: idxs and grad_dists must have shape (N, P1, K)")
    K = int(idxs.shape[2])
    dev, lengths1, lengths2 = _knn_check(p1, p2, lengths1, lengths2, max(1, min(K, _lib.KNN_MAX_K)), "knn_points_backward")
    p1, p2, idxs = _c(p1, torch.float32), _c(p2, torch.float32), _c(idxs, torch.int64)
    g = grad_dists.to(torch.float32).contiguous()
    grad_p1 = torch.empty_like(p1) if _needs[0] else None
    grad_p2 = torch.empty_like(p2) if _needs[1] else None
    if K == 0:
        return (None if grad_p1 is None else grad_p1.zero_()), (None if grad_p2 is None else grad_p2.zero_())
    _knn.backward_kernels(p1, p2, lengths1, lengths2, idxs, K, int(norm), g, None, grad_p1, grad_p2)
    return grad_p1, grad_p2


# ----------------------------------------------------------------------------------------------
# farthest point sampling and ball query (csrc/fps_ball.hip), behind the wrappers of pytorch3d_amd.sample_farthest_points /
# pytorch3d_amd.ball_query (shim.EXPORTS), which come here for float32 GPU tensors with D in (2, 3).
def _int64_arg(t, N, dev, name, who):
    if t is None:
        return None
    _need_gpu(t, name)
    if t.device != dev:
        raise RuntimeError(f"Expected all tensors to be on the same GPU, but {name} is on {t.device} and points is on {dev}")
    if t.shape != (N,):
        raise RuntimeError(f"{who}: {name} must have shape (N,)")
    return _c(t, torch.int64)


def sample_farthest_points(points, lengths, K, start_idxs, max_K_known=-1):
    """FarthestPointSampling (sample_farthest_points.h): idx (N, max_K) int64, row n holding min(K[n], lengths[n]) indices from
    start_idxs[n] on and -1 behind them (include/p3d_amd.h).  max_K_known < 0: max(K) is read from the device, once.  lengths, K
    and start_idxs may be None (full clouds, max_K_known samples each, start at 0) -- not part of the reference's signature."""
    who = "sample_farthest_points"
    _need_gpu(points, "points")
    if points.dim() != 3 or points.shape[2] not in (2, 3):
        raise RuntimeError(f"{who}: the kernels take points (N, P, D) with D in (2, 3); pytorch3d_amd.sample_farthest_points has a "
                           "torch formulation for the rest")
    dev = points.device
    N, P, D = points.shape
    lengths, K, start_idxs = (_int64_arg(t, N, dev, name, who) for t, name in ((lengths, "lengths"), (K, "K"), (start_idxs, "start_idxs")))
    max_K = int(max_K_known)
    if max_K < 0:
        if K is None:
            raise RuntimeError(f"{who}: K is None and max_K_known is not given")
        max_K = int(K.max()) if N > 0 else 0
    max_K = max(max_K, 0)
    points = _c(points, torch.float32)
    lib = _lib.load()
    if N == 0 or P == 0 or max_K == 0:
        return torch.full((N, max_K), -1, dtype=torch.int64, device=dev)
    idx = torch.empty((N, max_K), dtype=torch.int64, device=dev)
    nbytes = lib.p3d_sample_farthest_points_workspace_bytes(N, P)
    ws = _workspace(nbytes, dev) if nbytes else None
    _lib.call("p3d_sample_farthest_points", who, dev, points, lengths, K, start_idxs, N, P, D, max_K, idx, ws, nbytes)
    return idx


def ball_query(p1, p2, lengths1, lengths2, K, radius, skip_points_outside_cube=False):
    """BallQuery (ball_query.h): (idx (N, P1, K) int64, dists (N, P1, K)): per query the first K points of its cloud, ascending in
    index, with a squared distance < radius^2 (float32); -1 / 0 behind them and in the rows past lengths1.  lengths1 / lengths2 may
    be None (every cloud full).  skip_points_outside_cube is accepted and ignored: it cannot change a result."""
    who = "ball_query"
    dev = _same_device(("p1", p1), ("p2", p2))
    if p1.dim() != 3 or p2.dim() != 3 or p1.shape[0] != p2.shape[0] or p1.shape[2] != p2.shape[2]:
        raise RuntimeError(f"{who}: p1 (N, P1, D) and p2 (N, P2, D) must share N and D")
    K = int(K)
    if p1.shape[2] not in (2, 3) or K < 1:
        raise RuntimeError(f"{who}: the kernel takes D in (2, 3) and K >= 1; pytorch3d_amd.ball_query has a torch formulation for the rest")
    N, P1, D = p1.shape
    lengths1, lengths2 = _int64_arg(lengths1, N, dev, "lengths1", who), _int64_arg(lengths2, N, dev, "lengths2", who)
    p1, p2 = _c(p1, torch.float32), _c(p2, torch.float32)
    idx = torch.empty((N, P1, K), dtype=torch.int64, device=dev)
    dists = torch.empty((N, P1, K), dtype=torch.float32, device=dev)
    _lib.call("p3d_ball_query", who, dev, p1, p2, lengths1, lengths2, N, P1, p2.shape[1], D, K, float(radius), idx, dists)
    return idx, dists


# ----------------------------------------------------------------------------------------------
# point-cloud covariances, curvatures and local coordinate frames (csrc/point_frames.hip).  NOT in HOT_PATH_EXPORTS: the reference
# has no compiled operator of this kind; pytorch3d_amd.points_normals (and, under patch_python, the reference's two functions) come here.
def point_frames(points, lengths, K, disambiguate_directions=True, frames=True, cov=False, idx=False):
    """(curvatures (N, P, 3), frames (N, P, 3, 3), cov (N, P, 3, 3), idx (N, P, K) int64) of p3d_point_frames (include/p3d_amd.h) on
    the points AS GIVEN (the caller recentres), None for what was not asked for.  lengths (N,) int64 on the GPU or None (full clouds)."""
    who = "point_frames"
    _need_gpu(points, "points")
    K = int(K)
    if points.dim() != 3 or points.shape[2] != 3 or not 1 <= K <= _lib.FRAMES_MAX_K:
        raise RuntimeError(f"{who}: the kernel takes points (N, P, 3) and 1 <= K <= {_lib.FRAMES_MAX_K}; pytorch3d_amd.points_normals "
                           "has a torch formulation for the rest")
    if not (frames or cov or idx):
        raise RuntimeError(f"{who}: nothing asked for")
    dev = points.device
    N, P, D = points.shape
    lengths = _int64_arg(lengths, N, dev, "lengths", who)
    points = _c(points, torch.float32)
    curv_t = torch.empty((N, P, 3), dtype=torch.float32, device=dev) if frames else None
    frames_t = torch.empty((N, P, 3, 3), dtype=torch.float32, device=dev) if frames else None
    cov_t = torch.empty((N, P, 3, 3), dtype=torch.float32, device=dev) if cov else None
    idx_t = torch.empty((N, P, K), dtype=torch.int64, device=dev) if idx else None
    flags = _lib.FRAMES_DISAMBIGUATE if disambiguate_directions else 0
    _lib.call("p3d_point_frames", who, dev, points, lengths, N, P, D, K, flags, curv_t, frames_t, cov_t, idx_t)
    return curv_t, frames_t, cov_t, idx_t


# ----------------------------------------------------------------------------------------------
# box3d_overlap (csrc/box3d.hip), behind pytorch3d_amd.iou_box3d.iou_box3d_op (shim.EXPORTS): iou_box3d for GPU tensors,
# iou_box3d_host for CPU tensors.
def _check_boxes(boxes1, boxes2, who):
    for name, b in (("boxes1", boxes1), ("boxes2", boxes2)):
        if b.dim() != 3 or tuple(b.shape[1:]) != (8, 3):
            raise RuntimeError(f"{who}: {name} must have shape (B, 8, 3), got {tuple(b.shape)}")
        if b.dtype != torch.float32:
            raise RuntimeError(f"{who}: {name} must be float32, got {b.dtype}")
    if boxes1.device != boxes2.device:
        raise RuntimeError(f"Expected all tensors to be on the same device, but boxes2 is on {boxes2.device} and boxes1 is on {boxes1.device}")


def iou_box3d(boxes1, boxes2, lds_capacity=None, return_overflow=False):
    """IoUBox3D (iou_box3d.h) on GPU tensors: (vol (N, M), iou (N, M)) float32 of p3d_iou_box3d (include/p3d_amd.h).  The boxes are
    made contiguous here.  lds_capacity: triangles per fragment list of the first launch (default P3D_BOX3D_LDS_CAPACITY; results do
    not depend on it); return_overflow: also a 0-dim int32 tensor on the device, the number of pairs the second launch redid."""
    who = "iou_box3d"
    _check_boxes(boxes1, boxes2, who)
    dev = _same_device(("boxes1", boxes1), ("boxes2", boxes2))
    N, M = boxes1.shape[0], boxes2.shape[0]
    cap = _lib.BOX3D_LDS_CAPACITY if lds_capacity is None else int(lds_capacity)
    boxes1, boxes2 = boxes1.contiguous(), boxes2.contiguous()
    lib = _lib.load()
    vol = torch.empty((N, M), dtype=torch.float32, device=dev)
    iou = torch.empty((N, M), dtype=torch.float32, device=dev)
    if N * M == 0:
        return (vol, iou, torch.zeros((), dtype=torch.int32, device=dev)) if return_overflow else (vol, iou)
    nbytes = lib.p3d_iou_box3d_workspace_bytes(N, M)
    ws = _workspace(nbytes, dev)
    _lib.call("p3d_iou_box3d", who, dev, boxes1, boxes2, N, M, cap, vol, iou, ws, nbytes)
    if return_overflow:
        return vol, iou, ws[:4].view(torch.int32)[0].clone()
    return vol, iou


def iou_box3d_host(boxes1, boxes2):
    """The same contract on CPU tensors: p3d_iou_box3d_host, a serial loop over the pairs."""
    who = "iou_box3d_host"
    _check_boxes(boxes1, boxes2, who)
    if boxes1.is_cuda:
        raise RuntimeError(f"{who}: the host loop takes CPU tensors")
    N, M = boxes1.shape[0], boxes2.shape[0]
    boxes1, boxes2 = boxes1.contiguous(), boxes2.contiguous()
    vol = torch.empty((N, M), dtype=torch.float32)
    iou = torch.empty((N, M), dtype=torch.float32)
    if N * M:
        _lib.call("p3d_iou_box3d_host", who, None, boxes1, boxes2, N, M, vol, iou)
    return vol, iou


# ----------------------------------------------------------------------------------------------
# implicit rendering (csrc/implicit.hip), behind pytorch3d_amd.implicit (shim.EXPORTS: sample_pdf -> implicit.sample_pdf_op).
def _check_pdf(bins, weights, outputs, who):
    for name, t in (("bins", bins), ("weights", weights), ("outputs", outputs)):
        if t.dim() != 2:
            raise RuntimeError(f"{who}: {name} must have 2 dimensions, got {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{who}: {name} must be float32, got {t.dtype}")
        if t.device != bins.device:
            raise RuntimeError(f"Expected all tensors to be on the same device, but {name} is on {t.device} and bins is on {bins.device}")
    B, n_bins = weights.shape
    if tuple(bins.shape) != (B, n_bins + 1) or outputs.shape[0] != B:
        raise RuntimeError(f"{who}: bins (B, n_bins + 1), weights (B, n_bins), outputs (B, S) expected, got {tuple(bins.shape)}, "
                           f"{tuple(weights.shape)}, {tuple(outputs.shape)}")
    if n_bins < 1:
        raise RuntimeError(f"{who}: n_bins must be at least 1")
    if not outputs.is_contiguous():
        raise RuntimeError(f"{who}: outputs must be contiguous")
    return B, n_bins, outputs.shape[1]


def sample_pdf(bins, weights, outputs, eps):
    """SamplePdf (sample_pdf/sample_pdf.h) on GPU tensors: p3di_sample_pdf (csrc/implicit_abi.h) in place over outputs (B, S), whose
    version counter is bumped.  bins and weights are made contiguous here.  Returns None, as the reference's operator does."""
    who = "sample_pdf"
    B, n_bins, S = _check_pdf(bins, weights, outputs, who)
    dev = _same_device(("bins", bins), ("weights", weights), ("outputs", outputs))
    if B * S:
        nbytes = _lib.load().p3di_sample_pdf_workspace_bytes(B, n_bins)
        with torch.cuda.device(dev):
            ws = _workspace(nbytes, dev) if nbytes else None
        _lib.call("p3di_sample_pdf", who, dev, bins.contiguous(), weights.contiguous(), outputs, B, n_bins, S, float(eps), ws, nbytes)
    torch.autograd.graph.increment_version(outputs)


def sample_pdf_host(bins, weights, outputs, eps):
    """The same contract on CPU tensors: p3di_sample_pdf_host, a serial loop over the rows."""
    who = "sample_pdf_host"
    B, n_bins, S = _check_pdf(bins, weights, outputs, who)
    if bins.is_cuda:
        raise RuntimeError(f"{who}: the host loop takes CPU tensors")
    if B * S:
        _lib.call("p3di_sample_pdf_host", who, None, bins.contiguous(), weights.contiguous(), outputs, B, n_bins, S, float(eps))
    torch.autograd.graph.increment_version(outputs)


def _check_rays(who, densities, features):
    _need_gpu(densities, "densities")
    if densities.dim() != 2 or densities.dtype != torch.float32 or densities.shape[1] < 1:
        raise RuntimeError(f"{who}: densities must be float32 (N, P) with P >= 1, got {densities.dtype} {tuple(densities.shape)}")
    N, P = densities.shape
    if features is None:
        return N, P, 0
    if features.dtype != torch.float32 or features.dim() != 3 or tuple(features.shape[:2]) != (N, P) or features.device != densities.device:
        raise RuntimeError(f"{who}: features must be float32 (N, P, C) on the densities' device, got {features.dtype} "
                           f"{tuple(features.shape)} on {features.device}")
    return N, P, features.shape[2]


def ea_raymarch_forward(densities, features, shift, one_plus_eps, return_weights=False):
    """p3di_ea_raymarch_forward (csrc/implicit_abi.h): densities (N, P), features (N, P, C) or None (absorption only) -> out (N, C + 1)
    and the weights (N, P) or None."""
    who = "ea_raymarch_forward"
    N, P, C = _check_rays(who, densities, features)
    dev = densities.device
    with torch.cuda.device(dev):
        out = torch.empty((N, C + 1), dtype=torch.float32, device=dev)
        weights = torch.empty((N, P), dtype=torch.float32, device=dev) if return_weights else None
    if N:
        _lib.call("p3di_ea_raymarch_forward", who, dev, densities.contiguous(), None if features is None else features.contiguous(), N, P, C,
                  int(shift), float(one_plus_eps), out, weights)
    return out, weights


def ea_raymarch_backward(densities, features, grad_out, grad_weights, shift, one_plus_eps):
    """p3di_ea_raymarch_backward: (grad_densities (N, P), grad_features (N, P, C) or None)."""
    who = "ea_raymarch_backward"
    N, P, C = _check_rays(who, densities, features)
    dev = densities.device
    if grad_out.dtype != torch.float32 or tuple(grad_out.shape) != (N, C + 1):
        raise RuntimeError(f"{who}: grad_out must be float32 (N, C + 1), got {grad_out.dtype} {tuple(grad_out.shape)}")
    if grad_weights is not None and (grad_weights.dtype != torch.float32 or tuple(grad_weights.shape) != (N, P)):
        raise RuntimeError(f"{who}: grad_weights must be float32 (N, P), got {grad_weights.dtype} {tuple(grad_weights.shape)}")
    with torch.cuda.device(dev):
        gd = torch.empty((N, P), dtype=torch.float32, device=dev)
        gf = torch.empty((N, P, C), dtype=torch.float32, device=dev) if features is not None else None
        nbytes = _lib.load().p3di_ea_raymarch_backward_workspace_bytes(N, P)
        ws = _workspace(nbytes, dev) if nbytes else None
    if N:
        _lib.call("p3di_ea_raymarch_backward", who, dev, densities.contiguous(), None if features is None else features.contiguous(),
                  grad_out.contiguous(), None if grad_weights is None else grad_weights.contiguous(), N, P, C, int(shift),
                  float(one_plus_eps), gd, gf, ws, nbytes)
    return gd, gf


# ----------------------------------------------------------------------------------------------
# GraphConv / gather_scatter neighbour sums (csrc/graph_conv.hip), behind pytorch3d_amd.graph_conv.gather_scatter_op (shim.EXPORTS),
# which builds (or recalls) the table and comes here.
def neighbor_sum(rows, offsets, entries, base=None):
    """p3d_neighbor_sum (include/p3d_amd.h): out (V, D) float32 with out[v] = (base[v] or +0) + the rows of v's entries in list order.
    rows (n_rows, D) and base (V, D) float32 GPU tensors whose last dimension is contiguous (any row stride: views are read in
    place); offsets (V + 1,) and entries (n_entries,) contiguous int32.  No atomics, no zero fill; the same bits on every run."""
    who = "neighbor_sum"
    named = [("rows", rows), ("offsets", offsets), ("entries", entries)] + ([("base", base)] if base is not None else [])
    dev = _same_device(*named)
    if rows.dim() != 2 or rows.dtype != torch.float32:
        raise RuntimeError(f"{who}: rows must be (n_rows, D) float32, got {tuple(rows.shape)} {rows.dtype}")
    if offsets.dim() != 1 or offsets.numel() < 1 or offsets.dtype != torch.int32 or entries.dim() != 1 or entries.dtype != torch.int32:
        raise RuntimeError(f"{who}: offsets (V + 1,) and entries (n_entries,) must be int32")
    n_rows, D = rows.shape
    V = offsets.numel() - 1
    if base is not None and (base.dtype != torch.float32 or tuple(base.shape) != (V, D)):
        raise RuntimeError(f"{who}: base must be ({V}, {D}) float32, got {tuple(base.shape)} {base.dtype}")

    def row_view(t):  # rows of D contiguous floats at a non-negative stride; anything else is copied
        return t if t.numel() == 0 or D == 1 and t.stride(0) >= 0 or t.stride(1) == 1 and t.stride(0) >= 0 else t.contiguous()

    rows = row_view(rows)
    base = row_view(base) if base is not None else None
    offsets, entries = offsets.contiguous(), entries.contiguous()
    out = torch.empty((V, D), dtype=torch.float32, device=dev)
    if V * D == 0:
        return out
    _lib.call("p3d_neighbor_sum", who, dev, rows, rows.stride(0) if rows.numel() else 0, n_rows, base, base.stride(0) if base is not None else 0,
              offsets, entries, V, entries.numel(), D, out, D)
    return out


# ----------------------------------------------------------------------------------------------
# vert_align (csrc/vert_align.hip).  No `_C` operator of the reference stands behind it (its vert_align is torch): used by
# pytorch3d_amd.vert_align alone.
VERT_ALIGN_CALLS = {"atomic": 0, "ordered": 0}  # backwards of grad_feats by path (tests read it)
# A map whose channels are NOT adjacent in memory (NCHW) sends the 64 lanes of an atomic wave-instruction to 64 different lines; on one
# MI355X that ran 4.5 ms against the torch chain's 3.1 ms and the ordered form's 1.4 ms at (32, 256, 56, 56)
# (profiles/mesh_refine_mi355x.txt; 512 channels alike).  From this many channels on such a map takes the ordered form even without
# the deterministic flag; below it (not measured) the sort is assumed to cost more than the atomics.
VERT_ALIGN_STRIDED_ORDERED_MIN_C = 32


def _vert_align_args(who, feats, grid, packed_idx):
    named = [("verts", grid)] + [("feats[%d]" % i, f) for i, f in enumerate(feats)] + ([("packed_idx", packed_idx)] if packed_idx is not None else [])
    dev = _same_device(*named)
    if grid.dim() != 3 or grid.shape[2] < 2 or grid.dtype != torch.float32:
        raise RuntimeError(f"{who}: verts must be (N, V, >= 2) float32, got {tuple(grid.shape)} {grid.dtype}")
    for f in feats:
        if f.dim() != 4 or f.dtype != torch.float32 or f.shape[0] != grid.shape[0]:
            raise RuntimeError(f"{who}: every feature map must be (N, C, H, W) float32 with the verts' N, got {tuple(f.shape)} {f.dtype}")
        if f.numel() and min(f.stride()) < 0:
            raise RuntimeError(f"{who}: negative strides are not supported")
    if packed_idx is not None and (packed_idx.dim() != 1 or packed_idx.dtype != torch.int64):
        raise RuntimeError(f"{who}: packed_idx must be (rows,) int64")
    N, V = grid.shape[:2]
    rows = N * V if packed_idx is None else packed_idx.numel()
    return dev, N, V, rows, (None if packed_idx is None else packed_idx.contiguous())


def vert_align_forward(feats, grid, packed_idx, flags):
    """(rows, sum C) float32: one launch per map of `feats` into its column block (p3d_vert_align_forward, include/p3d_amd.h).
    grid (N, V, >= 2) and the maps are read through their strides; packed_idx: the padded vertex of every output row, or None."""
    who = "vert_align_forward"
    dev, N, V, rows, packed_idx = _vert_align_args(who, feats, grid, packed_idx)
    total = sum(f.shape[1] for f in feats)
    out = torch.empty((rows, total), dtype=torch.float32, device=dev)
    col = 0
    for f in feats:
        C, H, W = f.shape[1:]
        if H * W == 0 and rows * C:
            raise RuntimeError(f"{who}: a feature map without pixels")
        if rows * C:
            _lib.call("p3d_vert_align_forward", who, dev, f, N, C, H, W, *f.stride(), grid, V, *grid.stride(), packed_idx, rows, flags,
                      out[:, col:], total)
        col += C
    return out


def vert_align_backward(grad_out, feats, grid, packed_idx, flags, need_feats, need_verts):
    """(list of grad_feats or None per map, grad_verts (N, V, 3) or None) for grad_out (rows, sum C).  grad_verts is a gather;
    grad_feats float atomics, or the keys / stable sort / segmented sum form (the same bits on every run): under _ordered() always,
    else for a map without adjacent channels from VERT_ALIGN_STRIDED_ORDERED_MIN_C channels on.  Under _ordered() a map whose
    N * H * W does not fit an int32 cannot be keyed: NotImplementedError, and the caller falls back."""
    who = "vert_align_backward"
    dev, N, V, rows, packed_idx = _vert_align_args(who, feats, grid, packed_idx)
    total = sum(f.shape[1] for f in feats)
    if grad_out.dtype != torch.float32 or tuple(grad_out.shape) != (rows, total) or grad_out.device != dev:
        raise RuntimeError(f"{who}: grad_out must be ({rows}, {total}) float32 on {dev}")
    grad_out = grad_out.contiguous()
    strict = _ordered()
    if strict and any(nf and N * f.shape[2] * f.shape[3] > MAX_INT for f, nf in zip(feats, need_feats)):
        raise NotImplementedError(f"{who}: the deterministic form keys a pixel by an int32 and N * H * W does not fit")
    lib = _lib.load()
    grad_verts = torch.zeros((N, V, 3), dtype=torch.float32, device=dev) if need_verts else None
    grads = []
    col = 0
    for f, nf in zip(feats, need_feats):
        C, H, W = f.shape[1:]
        gf = torch.zeros_like(f) if nf else None
        go = grad_out[:, col:]  # this map's column block; the row stride stays `total`
        ordered = strict or (f.stride(1) != 1 and C >= VERT_ALIGN_STRIDED_ORDERED_MIN_C and N * H * W <= MAX_INT)
        if rows * C and H * W and (nf or need_verts):
            atomic = nf and not ordered
            if atomic or need_verts:
                _lib.call("p3d_vert_align_backward", who, dev, go, total, f, N, C, H, W, *f.stride(), grid, V, *grid.stride(), packed_idx, rows,
                          flags, gf if atomic else None, *(gf.stride() if atomic else (0, 0, 0, 0)), grad_verts)
            if nf and ordered:
                keys = torch.empty((rows * 4,), dtype=torch.int32, device=dev)
                _lib.call("p3d_vert_align_keys", who, dev, N, H, W, grid, V, *grid.stride(), packed_idx, rows, flags, keys)
                order = torch.sort(keys, stable=True).indices
                nbytes = lib.p3d_vert_align_workspace_bytes(rows, C)
                ws = _workspace(nbytes, dev)
                _lib.call("p3d_vert_align_ordered_backward", who, dev, go, total, N, C, H, W, grid, V, *grid.stride(), packed_idx, rows, flags,
                          keys, order, gf, *gf.stride(), ws, nbytes)
            if nf:
                VERT_ALIGN_CALLS["ordered" if ordered else "atomic"] += 1
        grads.append(gf)
        col += C
    return grads, grad_verts


# ----------------------------------------------------------------------------------------------
# point clouds into voxel grids (csrc/points_to_volumes.hip), behind the wrappers of pytorch3d_amd.points_to_volumes (shim.EXPORTS),
# which come here for float32 GPU tensors.
POINTS_TO_VOLUMES_CALLS = {"atomic": 0, "ordered": 0}  # forward launches by form: what actually ran (tests read it)


def _p2v_cloud(who, points_3d, grid_sizes, mask, **others):
    """(device, N, P, contiguous points, contiguous grid sizes, mask with its two element strides) after the shape checks."""
    dev = _same_device(("points_3d", points_3d), ("grid_sizes", grid_sizes), ("mask", mask), *others.items())
    if points_3d.dim() != 3 or points_3d.shape[2] != 3:
        raise RuntimeError(f"{who}: points_3d must have shape (N, P, 3)")
    N, P, _ = points_3d.shape
    if grid_sizes.shape != (N, 3) or mask.shape != (N, P):
        raise RuntimeError(f"{who}: grid_sizes must have shape (N, 3) and mask (N, P)")
    if mask.dtype != torch.float32:
        raise RuntimeError(f"expected dtype torch.float32, got {mask.dtype}")
    return dev, N, P, _c(points_3d, torch.float32), _c(grid_sizes, torch.int64), mask


def _p2v_volume(who, name, t, N, C, DHW, dev):
    """The five element strides of a float32 (N, C, D, H, W) volume, as the C ABI takes them: a host array behind a `const int64_t*`, so
    its address goes to _lib.call as a plain int (no tensor view can stand for host memory there)."""
    if t.dtype != torch.float32 or t.device != dev or t.dim() != 5 or t.shape[0] != N or t.shape[1] != C or tuple(t.shape[2:]) != DHW:
        raise RuntimeError(f"{who}: {name} must be a float32 tensor of shape ({N}, {C}, {DHW[0]}, {DHW[1]}, {DHW[2]}) on {dev}")
    return (ctypes.c_int64 * 5)(*t.stride())


def points_to_volumes_forward(points_3d, points_features, volume_densities, volume_features, grid_sizes, mask, point_weight,
                              align_corners, splat):
    """PointsToVolumesForward (points_to_volumes.h): adds the clouds to volume_densities (N, 1, D, H, W) and volume_features
    (N, C, D, H, W) IN PLACE, through their strides, and returns nothing (include/p3d_amd.h has the arithmetic).  Float atomics or,
    under torch.use_deterministic_algorithms(True), the ordered sum over the (point, corner) samples sorted by voxel on the device:
    the same bits on every run.  There N * D * H * W must fit an int32."""
    who = "points_to_volumes_forward"
    dev, N, P, points, grid, mask = _p2v_cloud(who, points_3d, grid_sizes, mask, points_features=points_features,
                                               volume_densities=volume_densities, volume_features=volume_features)
    if points_features.dim() != 3 or points_features.shape[:2] != (N, P):
        raise RuntimeError(f"{who}: points_features must have shape (N, P, C)")
    C = int(points_features.shape[2])
    if volume_densities.dim() != 5:
        raise RuntimeError(f"{who}: volume_densities must have shape (N, 1, D, H, W)")
    DHW = tuple(int(v) for v in volume_densities.shape[2:])
    dstr = _p2v_volume(who, "volume_densities", volume_densities, N, 1, DHW, dev)
    fstr = _p2v_volume(who, "volume_features", volume_features, N, C, DHW, dev)
    feats = _c(points_features, torch.float32)
    splat, align = int(bool(splat)), int(bool(align_corners))
    lib = _lib.load()
    keys = order = ws = None
    nbytes = 0
    if _ordered() and N * P > 0 and DHW[0] * DHW[1] * DHW[2] > 0:
        if N * DHW[0] * DHW[1] * DHW[2] > MAX_INT:
            raise RuntimeError(f"{who}: the deterministic form keys a voxel by an int32 and N * D * H * W = "
                               f"{N * DHW[0] * DHW[1] * DHW[2]} does not fit; add the batch in pieces")
        keys = torch.empty((N * P * (8 if splat else 1),), dtype=torch.int32, device=dev)
        _lib.call("p3d_points_to_volumes_keys", who, dev, points, grid, mask, mask.stride(0), mask.stride(1), N, P, *DHW, align, splat, keys)
        order = torch.sort(keys, stable=True).indices
        nbytes = lib.p3d_points_to_volumes_workspace_bytes(N, P, C, splat)
        ws = _workspace(nbytes, dev)
    _lib.call("p3d_points_to_volumes_forward", who, dev, points, feats, grid, mask, mask.stride(0), mask.stride(1), N, P, C, *DHW,
              volume_densities, ctypes.addressof(dstr), volume_features, ctypes.addressof(fstr), float(point_weight), align, splat, keys, order,
              ws, nbytes)
    POINTS_TO_VOLUMES_CALLS["ordered" if order is not None else "atomic"] += 1


def points_to_volumes_backward(points_3d, points_features, grid_sizes, mask, point_weight, align_corners, splat, grad_volume_densities,
                               grad_volume_features, grad_points_3d, grad_points_features):
    """PointsToVolumesBackward: ADDS to grad_points_features (N, P, C) and, with splat, to grad_points_3d (N, P, 3), in place; returns
    nothing.  A gather per point without atomics: the same bits on every run.  The gradient volumes are read through their strides
    (an expanded gradient is fine).  Without splat points_features and grad_points_3d are not touched (the reference passes
    expanded placeholders)."""
    who = "points_to_volumes_backward"
    dev, N, P, points, grid, mask = _p2v_cloud(who, points_3d, grid_sizes, mask, grad_volume_densities=grad_volume_densities,
                                               grad_volume_features=grad_volume_features, grad_points_features=grad_points_features)
    if grad_points_features.dim() != 3 or grad_points_features.shape[:2] != (N, P) or grad_points_features.dtype != torch.float32:
        raise RuntimeError(f"{who}: grad_points_features must be a float32 tensor of shape (N, P, C)")
    C = int(grad_points_features.shape[2])
    if grad_volume_densities.dim() != 5:
        raise RuntimeError(f"{who}: grad_volume_densities must have shape (N, 1, D, H, W)")
    DHW = tuple(int(v) for v in grad_volume_densities.shape[2:])
    dstr = _p2v_volume(who, "grad_volume_densities", grad_volume_densities, N, 1, DHW, dev)
    fstr = _p2v_volume(who, "grad_volume_features", grad_volume_features, N, C, DHW, dev)
    splat = int(bool(splat))
    feats = gp = None
    if splat:
        _same_device(("points_3d", points_3d), ("points_features", points_features), ("grad_points_3d", grad_points_3d))
        if points_features.shape != (N, P, C) or grad_points_3d.shape != (N, P, 3) or grad_points_3d.dtype != torch.float32:
            raise RuntimeError(f"{who}: points_features must have shape (N, P, C) and grad_points_3d be float32 of shape (N, P, 3)")
        feats = _c(points_features, torch.float32)
        gp = grad_points_3d.contiguous()  # (a copy only for a strided buffer; written back below)
    gf = grad_points_features.contiguous()
    _lib.call("p3d_points_to_volumes_backward", who, dev, points, feats, grid, mask, mask.stride(0), mask.stride(1), N, P, C, *DHW,
              grad_volume_densities, ctypes.addressof(dstr), grad_volume_features, ctypes.addressof(fstr), float(point_weight),
              int(bool(align_corners)), splat, gp, gf)
    if gf is not grad_points_features:
        grad_points_features.copy_(gf)
    if splat and gp is not grad_points_3d:
        grad_points_3d.copy_(gp)


# ----------------------------------------------------------------------------------------------
# point-mesh distances (csrc/point_mesh.hip), behind pytorch3d_amd.point_mesh (shim.EXPORTS), which comes here for float32 GPU tensors.
_PM_KINDS = {"point_face": (_lib.POINT_MESH_POINT, _lib.POINT_MESH_TRIANGLE), "face_point": (_lib.POINT_MESH_TRIANGLE, _lib.POINT_MESH_POINT),
             "point_edge": (_lib.POINT_MESH_POINT, _lib.POINT_MESH_SEGMENT), "edge_point": (_lib.POINT_MESH_SEGMENT, _lib.POINT_MESH_POINT)}


def _pm_check(direction, points, prims, who, **others):
    corners = 3 if "face" in direction else 2
    dev = _same_device(("points", points), ("tris" if corners == 3 else "segms", prims), *others.items())
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f"{who}: points must have shape (P, 3)")
    if prims.dim() != 3 or tuple(prims.shape[1:]) != (corners, 3):
        raise RuntimeError(f"{who}: {'tris' if corners == 3 else 'segms'} must have shape (T, {corners}, 3)")
    return dev, _c(points, torch.float32), _c(prims, torch.float32)


def _pm_first(points_first_idx, prims_first_idx, who):
    a, b = _c(points_first_idx, torch.int64), _c(prims_first_idx, torch.int64)
    if a.dim() != 1 or a.shape != b.shape:
        raise RuntimeError(f"{who}: the two first-index tensors must have the same shape (N,)")
    return a, b


def point_mesh_forward(direction, points, points_first_idx, prims, prims_first_idx, max_queries, min_triangle_area=5e-3, split=0,
                       weights=None, with_sums=False):
    """One direction ("point_face", "face_point", "point_edge", "edge_point") of include/p3d_amd.h: p3d_point_mesh_forward ->
    (dists, idxs) over the QUERY objects -- points for point_*, tris / segms for face_point / edge_point --, idxs packed target
    indices; with_sums: also sums (N,), the element sums of dists * weights[n]."""
    who = direction + "_dist_forward"
    dev, points, prims = _pm_check(direction, points, prims, who, points_first_idx=points_first_idx, prims_first_idx=prims_first_idx)
    pfirst, sfirst = _pm_first(points_first_idx, prims_first_idx, who)
    qk, tk = _PM_KINDS[direction]
    point_query = qk == _lib.POINT_MESH_POINT
    q, t, qf, tf = (points, prims, pfirst, sfirst) if point_query else (prims, points, sfirst, pfirst)
    N, Q, T = int(qf.shape[0]), int(q.shape[0]), int(t.shape[0])
    max_queries = min(int(max_queries), Q)
    if weights is not None:
        _same_device(("points", points), ("weights", weights))
        weights = _c(weights, torch.float32)
        if weights.shape != (N,):
            raise RuntimeError(f"{who}: weights must have shape (N,)")
    lib = _lib.load()
    dists = torch.empty((Q,), dtype=torch.float32, device=dev)
    idxs = torch.empty((Q,), dtype=torch.int64, device=dev)
    sums, ws, nbytes = None, None, 0
    if with_sums:
        sums = torch.empty((N,), dtype=torch.float32, device=dev)
        nbytes = lib.p3d_point_mesh_forward_workspace_bytes(N, max_queries)
        ws = _workspace(nbytes, dev)
    _lib.call("p3d_point_mesh_forward", who, dev, qk, tk, q, t, qf, tf, N, Q, T, max_queries, float(min_triangle_area), int(split), weights,
              dists, idxs, sums, ws, nbytes)
    return (dists, idxs, sums) if with_sums else (dists, idxs)


def point_mesh_backward(direction, points, prims, idxs, grad_dists, min_triangle_area=5e-3, points_first_idx=None, prims_first_idx=None,
                        elem_scale=None, grad_points=None, grad_prims=None, accumulate=False):
    """p3d_point_mesh_backward -> (grad_points (P, 3), grad_prims like prims).  The query side is a store, the target side float
    atomics or, under torch.use_deterministic_algorithms(True), the ordered sum over the hits sorted by target on the device (a sort
    of Q entries: no nonzero, no host sync).  grad_dists may be None (1).  With the first-index tensors a query of an element without
    targets contributes nothing, and elem_scale (N,) multiplies the upstream gradient per element.  grad_points / grad_prims:
    buffers to use; accumulate: ADD to what both hold (the second direction of a loss)."""
    who = direction + "_dist_backward"
    others = {"idxs": idxs}
    if grad_dists is not None:
        others["grad_dists"] = grad_dists
    dev, points, prims = _pm_check(direction, points, prims, who, **others)
    qk, tk = _PM_KINDS[direction]
    point_query = qk == _lib.POINT_MESH_POINT
    idxs = _c(idxs, torch.int64)
    pfirst = sfirst = None
    if points_first_idx is not None:
        pfirst, sfirst = _pm_first(points_first_idx, prims_first_idx, who)
    q, t, qf, tf = (points, prims, pfirst, sfirst) if point_query else (prims, points, sfirst, pfirst)
    N, Q, T = (0 if qf is None else int(qf.shape[0])), int(q.shape[0]), int(t.shape[0])
    if idxs.shape != (Q,) or (grad_dists is not None and grad_dists.shape != (Q,)):
        raise RuntimeError(f"{who}: idxs and grad_dists must have one entry per query object")
    g = None if grad_dists is None else grad_dists.to(torch.float32).contiguous()
    scale = None if elem_scale is None else _c(elem_scale, torch.float32)
    lib = _lib.load()
    for name, buf, like in (("grad_points", grad_points, points), ("grad_prims", grad_prims, prims)):
        if buf is not None and (buf.shape != like.shape or buf.dtype != torch.float32 or buf.device != dev or not buf.is_contiguous()):
            raise RuntimeError(f"{who}: {name} must be a contiguous float32 tensor shaped like its input, on the inputs' GPU")
    if accumulate and (grad_points is None or grad_prims is None):
        raise RuntimeError(f"{who}: accumulate needs both gradient buffers")
    grad_points = torch.empty_like(points) if grad_points is None else grad_points
    grad_prims = torch.empty_like(prims) if grad_prims is None else grad_prims
    gq, gt = (grad_points, grad_prims) if point_query else (grad_prims, grad_points)
    flags = (_lib.POINT_MESH_ACCUMULATE_QUERIES | _lib.POINT_MESH_ACCUMULATE_TARGETS) if accumulate else 0
    hits, ws, nbytes = None, None, 0
    if _ordered() and Q > 0 and T > 0:
        hits = torch.sort(idxs, stable=True).indices.contiguous()
        nbytes = lib.p3d_point_mesh_backward_workspace_bytes(tk, Q)
        ws = _workspace(nbytes, dev)
    _lib.call("p3d_point_mesh_backward", who, dev, qk, tk, q, t, idxs, g, scale, qf, tf, N, Q, T, float(min_triangle_area), flags, hits, gq, gt,
              ws, nbytes)
    return grad_points, grad_prims


def point_face_dist_forward(points, points_first_idx, tris, tris_first_idx, max_points, min_triangle_area=5e-3):
    """PointFaceDistanceForward (point_mesh_cuda.h): (dists (P,), idxs (P,) packed face indices)."""
    return point_mesh_forward("point_face", points, points_first_idx, tris, tris_first_idx, max_points, min_triangle_area)


def point_face_dist_backward(points, tris, idxs, grad_dists, min_triangle_area=5e-3):
    return point_mesh_backward("point_face", points, tris, idxs, grad_dists, min_triangle_area)


def face_point_dist_forward(points, points_first_idx, tris, tris_first_idx, max_tris, min_triangle_area=5e-3):
    """FacePointDistanceForward: (dists (T,), idxs (T,) packed point indices)."""
    return point_mesh_forward("face_point", points, points_first_idx, tris, tris_first_idx, max_tris, min_triangle_area)


def face_point_dist_backward(points, tris, idxs, grad_dists, min_triangle_area=5e-3):
    return point_mesh_backward("face_point", points, tris, idxs, grad_dists, min_triangle_area)


def point_edge_dist_forward(points, points_first_idx, segms, segms_first_idx, max_points):
    """PointEdgeDistanceForward: (dists (P,), idxs (P,) packed edge indices)."""
    return point_mesh_forward("point_edge", points, points_first_idx, segms, segms_first_idx, max_points)


def point_edge_dist_backward(points, segms, idxs, grad_dists):
    return point_mesh_backward("point_edge", points, segms, idxs, grad_dists)


def edge_point_dist_forward(points, points_first_idx, segms, segms_first_idx, max_segms):
    """EdgePointDistanceForward: (dists (S,), idxs (S,) packed point indices)."""
    return point_mesh_forward("edge_point", points, points_first_idx, segms, segms_first_idx, max_segms)


def edge_point_dist_backward(points, segms, idxs, grad_dists):
    return point_mesh_backward("edge_point", points, segms, idxs, grad_dists)


# ----------------------------------------------------------------------------------------------
# cubify (csrc/cubify.hip, csrc/implicit_abi.h), behind pytorch3d_amd.cubify.  No `_C` operator of the reference: nothing in shim.EXPORTS.
def cubify_fits(N, D, H, W):
    """Whether the kernels' int32 indices cover the sizes (else p3di_cubify_count refuses them)."""
    return min(D, H, W) >= 1 and N * (D + 1) * (H + 1) * (W + 1) <= 2**31 - 1 and 12 * N * D * H * W <= 2**31 - 1


def cubify_count(voxels, thresh):
    """p3di_cubify_count: voxels (N, D, H, W) float32 on a GPU, any strides -> (workspace, counts (N, 2) int64 = (V_n, F_n)), both on
    the device and not synchronised.  The workspace goes to cubify_emit unchanged."""
    who = "cubify_count"
    _need_gpu(voxels, "voxels")
    if voxels.dim() != 4 or voxels.dtype != torch.float32:
        raise RuntimeError(f"{who}: voxels must be float32 (N, D, H, W), got {voxels.dtype} {tuple(voxels.shape)}")
    N, D, H, W = voxels.shape
    if not cubify_fits(N, D, H, W):
        raise RuntimeError(f"{who}: {tuple(voxels.shape)} is beyond the kernels' int32 indices")
    dev = voxels.device
    nbytes = _lib.load().p3di_cubify_workspace_bytes(N, D, H, W)
    with torch.cuda.device(dev):
        ws = _workspace(nbytes, dev)
        counts = torch.empty((N, 2), dtype=torch.int64, device=dev)
    _lib.call("p3di_cubify_count", who, dev, voxels, voxels.stride(), N, D, H, W, float(thresh), ws, nbytes, counts)
    return ws, counts


def cubify_emit(workspace, shape, coords, feats, total_verts, total_faces):
    """p3di_cubify_emit from cubify_count's workspace: shape = (N, D, H, W), coords the (W + 1) + (H + 1) + (D + 1) float32 axis values,
    feats (N, K, D, H, W) float32 with any strides or None, the totals summed from the counts -> (verts (total_verts, 3) float32,
    faces (total_faces, 3) int64 with per-mesh indices, face_feats (total_faces, K) or None)."""
    who = "cubify_emit"
    N, D, H, W = shape
    dev = _same_device(("workspace", workspace), ("coords", coords), *([("feats", feats)] if feats is not None else []))
    if coords.dtype != torch.float32 or coords.numel() != D + H + W + 3 or not coords.is_contiguous():
        raise RuntimeError(f"{who}: coords must be {D + H + W + 3} contiguous float32 values, got {coords.dtype} {tuple(coords.shape)}")
    K = 0
    if feats is not None:
        if feats.dtype != torch.float32 or feats.dim() != 5 or (feats.shape[0],) + tuple(feats.shape[2:]) != (N, D, H, W):
            raise RuntimeError(f"{who}: feats must be float32 (N, K, D, H, W) over the voxels' grid, got {feats.dtype} {tuple(feats.shape)}")
        K = feats.shape[1]
    with torch.cuda.device(dev):
        verts = torch.empty((total_verts, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((total_faces, 3), dtype=torch.int64, device=dev)
        face_feats = torch.empty((total_faces, K), dtype=torch.float32, device=dev) if feats is not None else None
    if total_faces:
        _lib.call("p3di_cubify_emit", who, dev, coords, feats if K else None, feats.stride() if K else (0,) * 5, K, N, D, H, W,
                  int(total_verts), int(total_faces), workspace, workspace.numel(), verts, faces, face_feats)
    return verts, faces, face_feats


# ----------------------------------------------------------------------------------------------
# marching cubes (csrc/marching_cubes.hip, csrc/implicit_abi.h), behind pytorch3d_amd.marching_cubes; the reference's `_C.marching_cubes`
# is pytorch3d_amd.marching_cubes.marching_cubes_op over these (shim.EXPORTS).
def marching_cubes_fits(N, D, H, W):
    """Whether the kernels' int32 indices cover the sizes (else p3di_marching_cubes_count refuses them)."""
    return min(D, H, W) >= 1 and 15 * max(N, 1) * D * H * W <= 2**31 - 1


def marching_cubes_count(vol, isolevels):
    """p3di_marching_cubes_count: vol (N, D, H, W) float32 on a GPU, any strides, isolevels (N,) float32 -> (workspace, counts (N, 2)
    int64 = (V_n, F_n)), both on the device and not synchronised.  The workspace goes to marching_cubes_emit unchanged."""
    who = "marching_cubes_count"
    dev = _same_device(("vol", vol), ("isolevels", isolevels))
    if vol.dim() != 4 or vol.dtype != torch.float32:
        raise RuntimeError(f"{who}: vol must be float32 (N, D, H, W), got {vol.dtype} {tuple(vol.shape)}")
    N, D, H, W = vol.shape
    if isolevels.dtype != torch.float32 or isolevels.shape != (N,) or not isolevels.is_contiguous():
        raise RuntimeError(f"{who}: isolevels must be {N} contiguous float32 values, got {isolevels.dtype} {tuple(isolevels.shape)}")
    if not marching_cubes_fits(N, D, H, W):
        raise RuntimeError(f"{who}: {tuple(vol.shape)} is beyond the kernels' int32 indices")
    nbytes = _lib.load().p3di_marching_cubes_workspace_bytes(N, D, H, W)
    with torch.cuda.device(dev):
        ws = _workspace(nbytes, dev)
        counts = torch.empty((N, 2), dtype=torch.int64, device=dev)
    _lib.call("p3di_marching_cubes_count", who, dev, vol, vol.stride(), N, D, H, W, isolevels, ws, nbytes, counts)
    return ws, counts


def marching_cubes_emit(workspace, vol, isolevels, local, total_verts, total_faces):
    """p3di_marching_cubes_emit from marching_cubes_count's workspace and the same vol and isolevels, the totals summed from the counts
    -> (verts (total_verts, 3) float32, ids (total_verts,) int64, faces (total_faces, 3) int64 with per-volume indices)."""
    who = "marching_cubes_emit"
    dev = _same_device(("workspace", workspace), ("vol", vol), ("isolevels", isolevels))
    N, D, H, W = vol.shape
    with torch.cuda.device(dev):
        verts = torch.empty((total_verts, 3), dtype=torch.float32, device=dev)
        ids = torch.empty((total_verts,), dtype=torch.int64, device=dev)
        faces = torch.empty((total_faces, 3), dtype=torch.int64, device=dev)
    if total_faces:
        _lib.call("p3di_marching_cubes_emit", who, dev, vol, vol.stride(), N, D, H, W, isolevels, int(bool(local)), int(total_verts),
                  int(total_faces), workspace, workspace.numel(), verts, ids, faces)
    return verts, ids, faces


def marching_cubes_host(vol, isolevel):
    """p3di_marching_cubes_host: ONE volume (D, H, W) float32 on the CPU, any strides -> (verts (V, 3) float32 in world coordinates,
    faces (F, 3) int64) by the reference's CPU contract: a counting call, then a writing one."""
    who = "marching_cubes_host"
    if vol.is_cuda or vol.dim() != 3 or vol.dtype != torch.float32:
        raise RuntimeError(f"{who}: vol must be a float32 (D, H, W) CPU tensor, got {vol.dtype} {tuple(vol.shape)} on {vol.device}")
    D, H, W = vol.shape
    counts = torch.zeros((2,), dtype=torch.int64)
    none = torch.empty((0,), dtype=torch.int64)
    _lib.call("p3di_marching_cubes_host", who, None, vol, vol.stride(), D, H, W, float(isolevel),
              torch.full((3 * vol.numel(),), -1, dtype=torch.int64), None, 0, none, 0, counts)
    V, F = (int(c) for c in counts)
    verts, faces = torch.empty((V, 3), dtype=torch.float32), torch.empty((F, 3), dtype=torch.int64)
    if F:
        _lib.call("p3di_marching_cubes_host", who, None, vol, vol.stride(), D, H, W, float(isolevel),
                  torch.full((3 * vol.numel(),), -1, dtype=torch.int64), verts, V, faces, F, counts)
    return verts, faces


# ----------------------------------------------------------------------------------------------
# VolumeSampler (csrc/volume_sample.hip, csrc/implicit_abi.h), behind pytorch3d_amd.volume_sampler.  No `_C` operator of the reference.
VOLUME_SAMPLE_CALLS = {"atomic": 0, "ordered": 0}  # backwards of the volume gradients by path (tests read it)


def _volume_sample_args(who, densities, features, origins, directions, lengths):
    """(device, Cd, Cf, (D, H, W), N, R, P, shared, contiguous rays) of volumes (Nv, C, D, H, W) with Nv in (1, N) read through
    their strides (Nv == 1 against N > 1, or a batch stride of 0: one shared grid) and rays (N, R, 3), (N, R, 3), (N, R, P) or None."""
    named = [("densities", densities), ("origins", origins)] + [(k, v) for k, v in (("features", features), ("directions", directions),
                                                                                     ("lengths", lengths)) if v is not None]
    dev = _same_device(*named)
    for name, t in named:
        if t.dtype != torch.float32:
            raise RuntimeError(f"{who}: {name} must be float32, got {t.dtype}")
    if origins.dim() != 3 or origins.shape[2] != 3:
        raise RuntimeError(f"{who}: origins must be (N, R, 3), got {tuple(origins.shape)}")
    N, R = origins.shape[:2]
    P = 1
    if lengths is not None:
        if directions is None or tuple(directions.shape) != (N, R, 3) or lengths.dim() != 3 or tuple(lengths.shape[:2]) != (N, R):
            raise RuntimeError(f"{who}: directions (N, R, 3) and lengths (N, R, P) expected with the origins' N and R")
        P = lengths.shape[2]
    if densities.dim() != 5 or densities.shape[0] not in (1, N) or densities.shape[1] < 1 or min(densities.shape[2:]) < 1:
        raise RuntimeError(f"{who}: densities must be (N or 1, Cd >= 1, D, H, W), got {tuple(densities.shape)}")
    if features is not None and (features.dim() != 5 or features.shape[0] != densities.shape[0] or features.shape[2:] != densities.shape[2:]):
        raise RuntimeError(f"{who}: features must be (Nv, Cf, D, H, W) over the densities' batch and grid, got {tuple(features.shape)}")
    shared = N > 1 and densities.shape[0] == 1
    Cf = 0 if features is None else features.shape[1]
    rays = (origins.contiguous(), None if lengths is None else directions.contiguous(), None if lengths is None else lengths.contiguous())
    return dev, densities.shape[1], Cf, tuple(densities.shape[2:]), N, R, P, shared, rays


def _volume_strides(t, shared):
    if t is None or t.numel() == 0:
        return (0,) * 5
    return ((0,) if shared or t.shape[0] == 1 else (t.stride(0),)) + tuple(t.stride()[1:])


def volume_sample_fits(Nv, D, H, W, N, R, P):
    """Whether the ordered form's int32 keys cover the sizes (else volume_sample_backward raises NotImplementedError under _ordered())."""
    return Nv * D * H * W <= MAX_INT and N * R * P <= MAX_INT // 8


def volume_sample_forward(densities, features, origins, directions, lengths, flags):
    """p3di_volume_sample_forward: (rays_densities (N, R, P, Cd), rays_features (N, R, P, Cf)).  lengths None: P = 1, the points are
    the origins.  The volumes are read in place through their strides."""
    who = "volume_sample_forward"
    dev, Cd, Cf, (D, H, W), N, R, P, shared, (o, d, l) = _volume_sample_args(who, densities, features, origins, directions, lengths)
    with torch.cuda.device(dev):
        out_d = torch.empty((N, R, P, Cd), dtype=torch.float32, device=dev)
        out_f = torch.empty((N, R, P, Cf), dtype=torch.float32, device=dev)
    if N * R * P:
        _lib.call("p3di_volume_sample_forward", who, dev, densities, _volume_strides(densities, shared), features if Cf else None,
                  _volume_strides(features, shared), Cd, Cf, D, H, W, o, d, l, N, R, P, flags, out_d, out_f)
    return out_d, out_f


def volume_sample_backward(grad_d, grad_f, densities, features, origins, directions, lengths, flags, need_volumes, need_rays):
    """(grad_densities, grad_features, grad_origins, grad_directions, grad_lengths), None where not needed: need_volumes = (densities,
    features), need_rays = (origins, directions, lengths).  grad_d (N, R, P, Cd) / grad_f (N, R, P, Cf) or None (zero).  The volume
    gradients have the volumes' own shapes ((1, C, D, H, W) for a shared grid) and are float atomics, or under _ordered() the keys /
    stable sort / segmented sum form, the same bits on every run; there sizes beyond an int32 key raise NotImplementedError and the
    caller falls back.  The ray gradients are shuffle trees without atomics in both modes."""
    who = "volume_sample_backward"
    dev, Cd, Cf, (D, H, W), N, R, P, shared, (o, d, l) = _volume_sample_args(who, densities, features, origins, directions, lengths)
    for name, g, C in (("grad_rays_densities", grad_d, Cd), ("grad_rays_features", grad_f, Cf)):
        if g is not None and (g.dtype != torch.float32 or tuple(g.shape) != (N, R, P, C) or g.device != dev):
            raise RuntimeError(f"{who}: {name} must be float32 ({N}, {R}, {P}, {C}) on {dev}")
    grad_d = None if grad_d is None else grad_d.contiguous()
    grad_f = None if grad_f is None or Cf == 0 else grad_f.contiguous()
    need_d, need_f = bool(need_volumes[0]), bool(need_volumes[1]) and Cf > 0
    need_o, need_dir, need_l = (bool(x) for x in need_rays)
    if lengths is None:
        need_dir = need_l = False
    strict = _ordered() and (need_d or need_f)
    if strict and not volume_sample_fits(densities.shape[0], D, H, W, N, R, P):
        raise NotImplementedError(f"{who}: the deterministic form keys a voxel and a sample by an int32 and the sizes do not fit")
    with torch.cuda.device(dev):
        gd = torch.zeros(densities.shape, dtype=torch.float32, device=dev) if need_d else None
        gf = torch.zeros(features.shape, dtype=torch.float32, device=dev) if need_f else None
        go = torch.zeros((N, R, 3), dtype=torch.float32, device=dev) if need_o else None
        gdir = torch.zeros((N, R, 3), dtype=torch.float32, device=dev) if need_dir else None
        gl = torch.zeros((N, R, P), dtype=torch.float32, device=dev) if need_l else None
    nothing = grad_d is None and grad_f is None
    if N * R * P and not nothing and (need_d or need_f or need_o or need_dir or need_l):
        atomic = not strict
        vols = (densities, _volume_strides(densities, shared), features if Cf else None, _volume_strides(features, shared))
        if (atomic and (need_d or need_f)) or need_o or need_dir or need_l:
            _lib.call("p3di_volume_sample_backward", who, dev, grad_d, grad_f, *vols, Cd, Cf, D, H, W, o, d, l, N, R, P, flags,
                      gd if atomic else None, _volume_strides(gd, shared), gf if atomic else None, _volume_strides(gf, shared), go, gdir, gl)
        if strict:
            with torch.cuda.device(dev):
                keys = torch.empty((N * R * P * 8,), dtype=torch.int32, device=dev)
                _lib.call("p3di_volume_sample_keys", who, dev, D, H, W, int(shared), o, d, l, N, R, P, flags, keys)
                order = _sorted_hits(keys)  # the samples that have a voxel, sorted stably by it (one host sync: the count)
                nbytes = _lib.load().p3di_volume_sample_workspace_bytes(N, R, P, Cd, Cf)
                ws = _workspace(nbytes, dev)
            _lib.call("p3di_volume_sample_ordered_backward", who, dev, grad_d, grad_f, Cd, Cf, D, H, W, int(shared), o, d, l, N, R, P, flags,
                      keys, order, order.numel(), gd, _volume_strides(gd, shared), gf, _volume_strides(gf, shared), ws, nbytes)
        if need_d or need_f:
            VOLUME_SAMPLE_CALLS["ordered" if strict else "atomic"] += 1
    return gd, gf, go, gdir, gl


# ----------------------------------------------------------------------------------------------
# HarmonicEmbedding and the stratified ray depths (csrc/harmonic.hip, csrc/implicit_abi.h), behind pytorch3d_amd.harmonic_embedding and
# pytorch3d_amd.raysampling.  No `_C` operator of the reference.
def harmonic_embedding_width(dim, n, append_input):
    return dim * (2 * n + int(bool(append_input)))


def harmonic_embedding_fits(rows, dim, n, append_input):
    """Whether the entries take the sizes: a row that fits the backward's LDS tile, 32-bit element indices."""
    W = harmonic_embedding_width(dim, n, append_input)
    return dim >= 1 and n >= 1 and W <= _lib.HARMONIC_MAX_WIDTH and rows * W <= MAX_INT


def harmonic_embedding_backward_tile_rows(W):
    """Rows of one backward tile at the output width W (implicit_abi.h)."""
    return min(_lib.HARMONIC_BWD_ROWS, _lib.HARMONIC_BWD_LDS_FLOATS // (W | 1))


def _harmonic_args(who, x, diag_cov, frequencies):
    _need_gpu(x, "x")
    dev = _same_device(("x", x), ("frequencies", frequencies), *([("diag_cov", diag_cov)] if diag_cov is not None else []))
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous() or x.shape[1] < 1:
        raise RuntimeError(f"{who}: x must be contiguous float32 (rows, dim) with dim >= 1, got {x.dtype} {tuple(x.shape)}")
    if frequencies.dim() != 1 or frequencies.dtype != torch.float32 or frequencies.shape[0] < 1 or not frequencies.is_contiguous():
        raise RuntimeError(f"{who}: frequencies must be contiguous float32 (n,) with n >= 1, got {frequencies.dtype} {tuple(frequencies.shape)}")
    if diag_cov is not None and (diag_cov.dtype != torch.float32 or diag_cov.shape != x.shape or not diag_cov.is_contiguous()):
        raise RuntimeError(f"{who}: diag_cov must be contiguous float32 of x's shape, got {diag_cov.dtype} {tuple(diag_cov.shape)}")
    return dev, x.shape[0], x.shape[1], frequencies.shape[0]


def harmonic_embedding_forward(x, diag_cov, frequencies, append_input):
    """p3di_harmonic_embedding_forward: x (rows, dim), diag_cov of the same shape or None, frequencies (n,) -> (rows, dim (2 n + append))."""
    who = "harmonic_embedding_forward"
    dev, rows, dim, n = _harmonic_args(who, x, diag_cov, frequencies)
    if not harmonic_embedding_fits(rows, dim, n, append_input):
        raise RuntimeError(f"{who}: {rows} rows of width {harmonic_embedding_width(dim, n, append_input)} are beyond the kernels' sizes")
    with torch.cuda.device(dev):
        out = torch.empty((rows, harmonic_embedding_width(dim, n, append_input)), dtype=torch.float32, device=dev)
    if rows:
        _lib.call("p3di_harmonic_embedding_forward", who, dev, x, diag_cov, frequencies, rows, dim, n, int(bool(append_input)), out)
    return out


def harmonic_embedding_backward(x, diag_cov, frequencies, grad_out, append_input, need_x=True, need_cov=False):
    """p3di_harmonic_embedding_backward: (grad_x or None, grad_cov or None), each of x's shape; what is not needed is not computed."""
    who = "harmonic_embedding_backward"
    dev, rows, dim, n = _harmonic_args(who, x, diag_cov, frequencies)
    W = harmonic_embedding_width(dim, n, append_input)
    if grad_out.dtype != torch.float32 or tuple(grad_out.shape) != (rows, W) or grad_out.device != dev:
        raise RuntimeError(f"{who}: grad_out must be float32 ({rows}, {W}) on {dev}, got {grad_out.dtype} {tuple(grad_out.shape)} on {grad_out.device}")
    if not harmonic_embedding_fits(rows, dim, n, append_input):
        raise RuntimeError(f"{who}: {rows} rows of width {W} are beyond the kernels' sizes")
    need_cov = bool(need_cov) and diag_cov is not None
    with torch.cuda.device(dev):
        gx = torch.empty_like(x) if need_x else None
        gc = torch.empty_like(x) if need_cov else None
    if rows and (need_x or need_cov):
        _lib.call("p3di_harmonic_embedding_backward", who, dev, x, diag_cov, frequencies, grad_out.contiguous(), rows, dim, n,
                  int(bool(append_input)), gx, gc)
    return gx, gc


def stratified_depths(centers, uniforms):
    """p3di_stratified_depths: centers (rows, n) float32 with any two strides (an expand is read in place), uniforms (rows, n) -> the
    jiggled depths (rows, n), contiguous.  uniforms is only read."""
    who = "stratified_depths"
    _need_gpu(centers, "centers")
    dev = _same_device(("centers", centers), ("uniforms", uniforms))
    if centers.dim() != 2 or centers.dtype != torch.float32 or uniforms.dtype != torch.float32 or uniforms.shape != centers.shape:
        raise RuntimeError(f"{who}: centers and uniforms must be float32 (rows, n), got {centers.dtype} {tuple(centers.shape)} and "
                           f"{uniforms.dtype} {tuple(uniforms.shape)}")
    rows, n = centers.shape
    if rows * n > MAX_INT:
        raise RuntimeError(f"{who}: {rows} x {n} is beyond the kernel's int32 indices")
    with torch.cuda.device(dev):
        out = torch.empty((rows, n), dtype=torch.float32, device=dev)
    if rows * n:
        _lib.call("p3di_stratified_depths", who, dev, centers, centers.stride(), rows, n, uniforms.contiguous(), out)
    return out


# ----------------------------------------------------------------------------------------------
# iterative_closest_point / corresponding_points_alignment (csrc/points_alignment.hip, the contract: csrc/implicit_abi.h), behind
# pytorch3d_amd.points_alignment.  The reference has no compiled operator of this kind: nothing here is an export of the shim module.
def points_alignment_fits(N, P1, P2):
    """Whether the entries take clouds of these sizes (their indices are int32 per cloud, their grid N ceil(P1 / 64) workgroups)."""
    return 0 < N <= MAX_INT and 0 < P1 <= MAX_INT and 0 <= P2 <= MAX_INT and N * ((P1 + 63) // 64) <= MAX_INT


def _align_clouds(who, X, Y, *lengths):
    dev = _same_device(("X", X), ("Y", Y))
    if X.dim() != 3 or Y.dim() != 3 or X.shape[2] != 3 or Y.shape[2] != 3 or X.shape[0] != Y.shape[0]:
        raise RuntimeError(f"{who}: the kernels take X (N, P1, 3) and Y (N, P2, 3), got {tuple(X.shape)} and {tuple(Y.shape)}; "
                           "pytorch3d_amd.points_alignment has a torch formulation for the rest")
    if not points_alignment_fits(X.shape[0], X.shape[1], Y.shape[1]):
        raise RuntimeError(f"{who}: clouds of {tuple(X.shape)} and {tuple(Y.shape)} are empty or beyond the kernels' int32 indices")
    names = ("lengths1", "lengths2", "mask_len")
    return (dev, _c(X, torch.float32), _c(Y, torch.float32)) + tuple(_int64_arg(t, X.shape[0], dev, names[k], who) for k, t in enumerate(lengths))


def _align_transform(who, R, T, s, N, dev):
    if R is None and T is None and s is None:
        return None, None, None
    if R is None or T is None or s is None or R.shape != (N, 3, 3) or T.shape != (N, 3) or s.shape != (N,):
        raise RuntimeError(f"{who}: R (N, 3, 3), T (N, 3) and s (N,) come together")
    _same_device(("R", R), ("T", T), ("s", s))
    if R.device != dev:
        raise RuntimeError(f"Expected all tensors to be on the same GPU, but R is on {R.device} and X is on {dev}")
    return _c(R, torch.float32), _c(T, torch.float32), _c(s, torch.float32)


def _align_flags(estimate_scale, allow_reflection):
    return (_lib.ALIGN_ESTIMATE_SCALE if estimate_scale else 0) | (_lib.ALIGN_ALLOW_REFLECTION if allow_reflection else 0)


def icp_workspace(N, P1, device):
    """(workspace, its bytes) of the three entries for clouds of (N, P1) rows: one allocation serves every iteration of a call."""
    nbytes = _lib.load().p3di_icp_workspace_bytes(N, P1)
    return _workspace(nbytes, device), nbytes


def icp_match(X, Y, lengths1=None, lengths2=None, R=None, T=None, s=None, split=0):
    """p3di_icp_match: idx (N, P1) int64, the nearest point of Y[n, :lengths2[n]] to s * (X[n, i] R) + T (to X[n, i] itself without a
    transform): knn_points_idx(K=1)'s indices on the transformed points.  split: waves per workgroup, 0 (the launch decides), 1, 2, 4, 8."""
    who = "icp_match"
    dev, X, Y, lengths1, lengths2 = _align_clouds(who, X, Y, lengths1, lengths2)
    N, P1, _ = X.shape
    R, T, s = _align_transform(who, R, T, s, N, dev)
    idx = torch.empty((N, P1), dtype=torch.int64, device=dev)
    ws, nbytes = icp_workspace(N, P1, dev)
    _lib.call("p3di_icp_match", who, dev, X, Y, lengths1, lengths2, R, T, s, N, P1, Y.shape[1], int(split), idx, ws, nbytes)
    return idx


def icp_iteration(workspace, X, Y, lengths1, lengths2, mask_len, transform, rmse_prev, split, estimate_scale, allow_reflection,
                  relative_rmse_thr, R_out, T_out, s_out, idx, Xt, rmse, status):
    """p3di_icp_iteration on buffers of the caller (pytorch3d_amd.points_alignment holds them for the whole call): six launches, no
    host read.  workspace: icp_workspace's pair; transform: (R, T, s) or None (X as given); rmse_prev None: the first iteration."""
    who = "iterative_closest_point"
    N, P1, _ = X.shape
    R, T, s = transform if transform is not None else (None, None, None)
    _lib.call("p3di_icp_iteration", who, X.device, X, Y, lengths1, lengths2, mask_len, R, T, s, rmse_prev, N, P1, Y.shape[1], int(split),
              _align_flags(estimate_scale, allow_reflection), float(relative_rmse_thr), R_out, T_out, s_out, idx, Xt, rmse, status,
              workspace[0], workspace[1])


def points_alignment(X, Y, mask_len, weights, estimate_scale, allow_reflection, eps):
    """p3di_points_alignment: (R (N, 3, 3), T (N, 3), s (N,), status (2,) int32 on the device -- status[1]: some singular value
    <= 1e-15) of corresponding rows of X and Y (N, P, 3).  mask_len (N,) int64 or None, weights (N, P) float32 or None."""
    who = "corresponding_points_alignment"
    dev, X, Y, mask_len = _align_clouds(who, X, Y, mask_len)
    if X.shape != Y.shape:
        raise RuntimeError(f"{who}: X and Y must have one shape, got {tuple(X.shape)} and {tuple(Y.shape)}")
    N, P, _ = X.shape
    if weights is not None:
        _same_device(("X", X), ("weights", weights))
        if weights.shape != (N, P):
            raise RuntimeError(f"{who}: weights must have shape (N, P)")
        weights = _c(weights, torch.float32)
    R = torch.empty((N, 3, 3), dtype=torch.float32, device=dev)
    T = torch.empty((N, 3), dtype=torch.float32, device=dev)
    s = torch.empty((N,), dtype=torch.float32, device=dev)
    status = torch.zeros((2,), dtype=torch.int32, device=dev)
    ws, nbytes = icp_workspace(N, P, dev)
    _lib.call("p3di_points_alignment", who, dev, X, Y, mask_len, weights, N, P, _align_flags(estimate_scale, allow_reflection), float(eps),
              R, T, s, status, ws, nbytes)
    return R, T, s, status


POINT_MESH_EXPORTS = ("point_face_dist_forward", "point_face_dist_backward", "face_point_dist_forward", "face_point_dist_backward",
                      "point_edge_dist_forward", "point_edge_dist_backward", "edge_point_dist_forward", "edge_point_dist_backward")
# operators both flavours serve through Python wrappers of their own modules (shim.EXPORTS holds the whole table)
POINT_CLOUD_EXPORTS = ("sample_farthest_points", "ball_query")
BOX3D_EXPORTS = ("iou_box3d",)
GRAPH_EXPORTS = ("gather_scatter",)
IMPLICIT_EXPORTS = ("sample_pdf",)

# the reference's hot path: what each flavour implements itself (the pybind flavour reads this list)
HOT_PATH_EXPORTS = (
    "rasterize_meshes", "rasterize_meshes_backward", "_rasterize_meshes_naive", "_rasterize_meshes_coarse",
    "_rasterize_meshes_fine", "rasterize_points", "rasterize_points_backward", "_rasterize_points_naive",
    "_rasterize_points_coarse", "_rasterize_points_fine", "accum_alphacomposite", "accum_alphacomposite_backward",
    "accum_weightedsumnorm", "accum_weightedsumnorm_backward", "accum_weightedsum", "accum_weightedsum_backward",
    "interp_face_attrs_forward", "interp_face_attrs_backward", "sigmoid_alpha_blend", "sigmoid_alpha_blend_backward",
)
