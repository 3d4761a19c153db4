"""cubify: voxel occupancy grids to merged cube meshes (Mesh R-CNN's voxel branch) on csrc/cubify.hip.

    cubify(voxels, thresh, *, feats=None, device=None, align="topleft")            the reference's signature and result
    cubify_packed(voxels, thresh, feats=None, align="topleft")                     the packed tensors behind it

The contract (pytorch3d/ops/cubify.py restated; checked against the reference's CPU function through tests/golden/cubify_ref.npz).
voxels (N, D, H, W); x runs along W, y along H, z along D.
  occupancy   voxels[n, d, h, w] >= thresh with thresh rounded to the tensor's dtype (`Tensor.ge`); NaN and everything outside the
              grid are unoccupied.
  faces       voxels in (n, h, w, d) order, d fastest; per occupied voxel the directions -x +y -z -y +x +z, each emitting its two
              triangles iff the neighbour there is unoccupied.  Corners c = 4x + 2y + z; triangles _TRIANGLES.  Corner c of voxel
              (h, w, d) is lattice point g = ((h + y)(W + 1) + (w + x))(D + 1) + (d + z).
  vertices    a lattice point is kept iff a triangle of its mesh names it, that is iff one of the 8 voxels around it is occupied and
              exposes one of the three sides meeting there.  The kept points of a mesh keep ascending g; faces hold their ranks (int64).
  values      float32, index i on an axis of size S: t = float(i); t -= 0.5 for "center"; t * 2.0 / (S - margin) - 1.0 with margin 0
              for "corner", else 1.  Made on the CPU (IEEE multiply, divide, subtract), three small tables the kernel gathers from;
              kept per (shape, align, device).
  result      per mesh (V_n, 3) float32 and (F_n, 3) int64, (0, 3) for a mesh without an occupied voxel; if the whole batch has none,
              every entry is an empty 1-D tensor; N == 0 gives empty lists.
  feats       (N, K, D, H, W), only with align == "center": every face of voxel (n, d, h, w) gets feats[n, :, d, h, w], returned as
              TexturesAtlas of (F_n, 1, 1, K); ignored under the other modes.
  errors      an unknown align: ValueError("Align mode must be one of (topleft, corner, center)."); D, H or W of 1: ValueError naming
              the dimension (the reference dies in conv3d there, and "topleft" would divide by zero).

The kernels take float32 voxels (any strides) on a GPU with float32 feats on the same GPU, `device` None or that GPU, and sizes with
12 N D H W and N (D+1)(H+1)(W+1) within int32: `kernel_path`.  One host read per call -- the (N, 2) counts, between the count and the
emit entry (csrc/implicit_abi.h); the reference has N + 2.  Everything else takes `cubify_packed_torch`, the same contract in torch
(shifted occupancy compares, a cumsum, masked selects), which returns the same bits.  No gradient: the reference has none.
"""
import functools

import torch
import torch.nn.functional as F

from . import _C, structures

CALLS = {"fused": 0, "formulation": 0}  # what ran (the shim's PATCH_CALLS and the tests read it)

ALIGN_MODES = ("topleft", "corner", "center")
# (dh, dw, dd) of the six directions, in emission order
_DIRECTIONS = ((0, -1, 0), (1, 0, 0), (0, 0, -1), (-1, 0, 0), (0, 1, 0), (0, 0, 1))
# corners c = 4x + 2y + z of the twelve triangles, two per direction
_TRIANGLES = ((0, 1, 2), (1, 3, 2), (2, 3, 6), (3, 7, 6), (0, 2, 6), (0, 6, 4), (0, 5, 1), (0, 4, 5), (6, 7, 5), (6, 5, 4), (1, 7, 3), (1, 5, 7))


def _check(voxels, feats, align):
    if align not in ALIGN_MODES:
        raise ValueError("Align mode must be one of (topleft, corner, center).")
    if voxels.dim() != 4:
        raise ValueError(f"voxels must have shape (N, D, H, W), got {tuple(voxels.shape)}")
    if voxels.shape[0] == 0:
        return
    for name, size in zip("DHW", voxels.shape[1:]):
        if size < 2:
            raise ValueError(f"cubify needs at least 2 voxels along every axis, got {name} = {size} in voxels of shape {tuple(voxels.shape)}")
    if feats is not None and align == "center" and (feats.dim() != 5 or (feats.shape[0],) + tuple(feats.shape[2:]) != tuple(voxels.shape)):
        raise ValueError(f"feats must have shape (N, K, D, H, W) over the voxels' grid {tuple(voxels.shape)}, got {tuple(feats.shape)}")


def axis_values(size, align):
    """The size + 1 float32 coordinate values of an axis (CPU)."""
    t = torch.arange(size + 1, dtype=torch.float32)
    if align == "center":
        t = t - 0.5
    return t * 2.0 / (size - (0.0 if align == "corner" else 1.0)) - 1.0


@functools.lru_cache(maxsize=64)
def _coords(D, H, W, align, device):
    """x values (W + 1), y values (H + 1), z values (D + 1) in one tensor on `device`."""
    return torch.cat([axis_values(W, align), axis_values(H, align), axis_values(D, align)]).to(device)


def kernel_path(voxels, feats=None, device=None, align="center"):
    """Whether cubify(voxels, ..., feats=feats, device=device, align=align) runs csrc/cubify.hip (else: cubify_packed_torch)."""
    if not (torch.is_tensor(voxels) and voxels.is_cuda and voxels.dtype == torch.float32 and voxels.dim() == 4):
        return False
    if device is not None:
        device = torch.device(device)
        if device.type != "cuda" or (device.index if device.index is not None else torch.cuda.current_device()) != voxels.device.index:
            return False
    if feats is not None and align == "center" and not (torch.is_tensor(feats) and feats.dtype == torch.float32 and feats.device == voxels.device):
        return False
    return voxels.shape[0] == 0 or _C.cubify_fits(*voxels.shape)


def _empty_packed(N, device):
    """Nothing occupied in the whole batch: 1-D empties, which split into N empty 1-D tensors, and no features (the reference returns
    before it looks at feats)."""
    zeros = torch.zeros((N,), dtype=torch.int64, device=device)
    return torch.zeros((0,), dtype=torch.float32, device=device), torch.zeros((0,), dtype=torch.int64, device=device), zeros, zeros.clone(), None


def cubify_packed_torch(voxels, thresh, feats=None, align="topleft", _wrong=None):
    """The contract in torch, on the voxels' device, for any dtype `ge` takes.  Returns what cubify_packed returns.
    _wrong (the tests only): one of three deliberately wrong readings of the contract that the tests' comparison has to reject --
    "gt" (occupied iff above the threshold), "memory_order" (voxels visited in (n, d, h, w) order), "all_vertices" (no lattice point
    dropped)."""
    _check(voxels, feats, align)
    N, D, H, W = voxels.shape
    dev = voxels.device
    if feats is not None and align != "center":
        feats = None
    occ = (voxels.gt(thresh) if _wrong == "gt" else voxels.ge(thresh)).permute(0, 2, 3, 1)  # (N, H, W, D): the output order
    if N == 0 or not bool(occ.any()):
        return _empty_packed(N, dev)
    padded = F.pad(occ, (1, 1, 1, 1, 1, 1))
    exposed = torch.stack([occ & ~padded[:, 1 + dh:1 + dh + H, 1 + dw:1 + dw + W, 1 + dd:1 + dd + D] for dh, dw, dd in _DIRECTIONS], -1)
    # kept lattice points: corner (x, y, z) of a voxel is named iff the voxel exposes the x, the y or the z side that meets there
    kept = torch.zeros((N, H + 1, W + 1, D + 1), dtype=torch.bool, device=dev)
    for x in (0, 1):
        for y in (0, 1):
            for z in (0, 1):
                sides = exposed[..., 4 if x else 0] | exposed[..., 1 if y else 3] | exposed[..., 5 if z else 2]
                kept[:, y:y + H, x:x + W, z:z + D] |= sides
    if _wrong == "all_vertices":
        kept |= True
    L = (H + 1) * (W + 1) * (D + 1)
    rank = kept.view(N, L).cumsum(1) - 1
    n, h, w, d, k = exposed.nonzero().unbind(1)  # row-major: (n, h, w, d) order, then the directions in theirs
    if _wrong == "memory_order":
        n, d, h, w, k = exposed.permute(0, 3, 1, 2, 4).nonzero().unbind(1)
    corners = torch.tensor(_TRIANGLES, dtype=torch.int64, device=dev).view(6, 2, 3)[k]  # (E, 2, 3)
    g = (((h[:, None, None] + ((corners >> 1) & 1)) * (W + 1) + w[:, None, None] + ((corners >> 2) & 1)) * (D + 1)
         + d[:, None, None] + (corners & 1))
    faces = rank[n[:, None, None].expand_as(g), g].reshape(-1, 3)
    vn, vy, vx, vz = kept.nonzero().unbind(1)  # ascending (n, g)
    xs, ys, zs = (axis_values(s, align).to(dev) for s in (W, H, D))
    verts = torch.stack([xs[vx], ys[vy], zs[vz]], 1)
    num_verts = kept.view(N, L).sum(1)
    num_faces = 2 * exposed.reshape(N, -1).sum(1)
    face_feats = None
    if feats is not None:
        face_feats = feats.permute(0, 3, 4, 2, 1)[n, h, w, d].repeat_interleave(2, 0).reshape(-1, 1, 1, feats.shape[1])
    return verts, faces, num_verts, num_faces, face_feats


def _fused(voxels, thresh, feats, align):
    """cubify_packed on the kernels, and the (N, 2) counts on the host (from the call's one read)."""
    _check(voxels, feats, align)
    CALLS["fused"] += 1
    N, D, H, W = voxels.shape
    dev = voxels.device
    if feats is not None and align != "center":
        feats = None
    if N == 0:
        return _empty_packed(0, dev), torch.zeros((0, 2), dtype=torch.int64)
    ws, counts = _C.cubify_count(voxels, thresh)
    host = counts.cpu()  # the one host read of the call
    total_verts, total_faces = (int(t) for t in host.sum(0))
    if total_faces == 0:
        return _empty_packed(N, dev), host
    verts, faces, face_feats = _C.cubify_emit(ws, (N, D, H, W), _coords(D, H, W, align, dev), feats, total_verts, total_faces)
    return (verts, faces, counts[:, 0], counts[:, 1], None if face_feats is None else face_feats.view(-1, 1, 1, feats.shape[1])), host


def cubify_packed(voxels, thresh, feats=None, align="topleft"):
    """(verts_packed (V, 3) float32, faces_packed (F, 3) int64 with per-mesh-local indices, num_verts_per_mesh (N,), num_faces_per_mesh
    (N,) on the device, face_feats (F, 1, 1, K) or None).  An all-empty batch gives 1-D empty verts and faces.  Runs under no_grad."""
    with torch.no_grad():
        if kernel_path(voxels, feats, None, align):
            return _fused(voxels, thresh, feats, align)[0]
        CALLS["formulation"] += 1
        return cubify_packed_torch(voxels, thresh, feats, align)


def _reference_classes():
    try:
        import importlib

        return (importlib.import_module("pytorch3d.structures").Meshes,
                importlib.import_module("pytorch3d.renderer.mesh.textures").TexturesAtlas)
    except ImportError:
        return None


def cubify(voxels, thresh, *, feats=None, device=None, align="topleft"):
    """pytorch3d.ops.cubify.  Returns the reference's Meshes (with TexturesAtlas when feats is given and align == "center") where
    pytorch3d can be imported, else structures.PackedMeshes (whose `textures` is then the list of per-mesh (F_n, 1, 1, K) tensors, or
    None).  The lists are `split` views of the packed tensors."""
    with torch.no_grad():
        if kernel_path(voxels, feats, device, align):
            (verts, faces, _, _, face_feats), host = _fused(voxels, thresh, feats, align)
        else:
            CALLS["formulation"] += 1
            verts, faces, num_verts, num_faces, face_feats = cubify_packed_torch(voxels, thresh, feats, align)
            host = torch.stack([num_verts, num_faces], 1).cpu()
            if device is not None and torch.device(device) != verts.device:
                verts, faces, face_feats = (None if t is None else t.to(device) for t in (verts, faces, face_feats))
        num_verts, num_faces = host[:, 0].tolist(), host[:, 1].tolist()
        verts_list, faces_list = list(verts.split(num_verts, 0)), list(faces.split(num_faces, 0))
        feats_list = None if face_feats is None else list(face_feats.split(num_faces, 0))
    classes = _reference_classes()
    if classes is not None:
        Meshes, TexturesAtlas = classes
        return Meshes(verts=verts_list, faces=faces_list, textures=None if feats_list is None else TexturesAtlas(feats_list))
    meshes = structures.PackedMeshes(verts_list, faces_list)
    meshes.textures = feats_list
    return meshes
