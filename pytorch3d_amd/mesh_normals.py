"""Face areas / normals and area-weighted vertex normals of a packed mesh batch on the HIP kernels (csrc/normals.hip).

    face_areas_normals(verts, faces)            -> (areas (F,), normals (F, 3))      pytorch3d/ops/mesh_face_areas_normals.py
    verts_normals(verts, faces, incidence=None) -> normals (V, 3)                    Meshes._compute_vertex_normals, meshes.py:884-926
    vert_incidence(faces, V)                    -> (offsets (V + 1,), corners) int32  the topology part of verts_normals

Every lit shader reads one of the two, and in a fitting loop the vertices move every step.  The reference's vertex normals are a
torch chain -- gather, cross product, three index_add with float atomics, normalize, and twice that in autograd, ending in a sort --
whose forward already differs in its last bits from run to run.  Here they are a GATHER: the corners are sorted by vertex once per
topology (vert_incidence: the only host sync, never repeated while the faces stay), each step stores one row per face and sums, per
vertex, the rows of its list in list order.  No float atomic in either direction: the same bits on every run, stream and process,
with torch.use_deterministic_algorithms on or off.  The backward of face_areas_normals ends in the package's face-gradient scatter
(atomic; ordered under the strict deterministic flag, like every other backward: DESIGN.md 8.8).

float32 tensors on the GPU only, like the other operators of the package.
"""
import torch

from . import _C, _lib


def _check(verts, faces, who):
    _C._same_device(("verts", verts), ("faces", faces))
    if verts.dim() != 2 or verts.size(1) != 3:
        raise RuntimeError(f"{who}: verts must have shape (V, 3)")
    if faces.dim() != 2 or faces.size(1) != 3:
        raise RuntimeError(f"{who}: faces must have shape (F, 3)")
    return _C._c(verts, torch.float32), _C._c(faces, torch.int64)


# ---- face areas and normals ------------------------------------------------------------------------------------------------------
def face_areas_normals_forward(verts, faces):
    """`_C.face_areas_normals_forward` (face_areas_normals.cu:14-70): (areas (F,), normals (F, 3))."""
    v, f = _check(verts, faces, "face_areas_normals_forward")
    V, F = v.size(0), f.size(0)
    dev = v.device
    areas = torch.empty((F,), dtype=torch.float32, device=dev)
    normals = torch.empty((F, 3), dtype=torch.float32, device=dev)
    _lib.call("p3d_face_areas_normals_forward", "face_areas_normals_forward", dev, v, f, V, F, areas, normals)
    return areas, normals


def face_areas_normals_backward(grad_areas, grad_normals, verts, faces):
    """`_C.face_areas_normals_backward` (face_areas_normals.cu:64-216): grad_verts (V, 3).  One kernel writes the gradient per corner,
    the package's scatter sums the corners of a vertex (_C.scatter_face_grads: ordered under the strict deterministic flag)."""
    v, f = _check(verts, faces, "face_areas_normals_backward")
    _C._same_device(("verts", verts), ("grad_areas", grad_areas), ("grad_normals", grad_normals))
    V, F = v.size(0), f.size(0)
    ga, gn = _C._c(grad_areas, torch.float32), _C._c(grad_normals, torch.float32)
    if tuple(ga.shape) != (F,) or tuple(gn.shape) != (F, 3):
        raise RuntimeError("face_areas_normals_backward: grad_areas must have shape (F,) and grad_normals (F, 3)")
    dev = v.device
    per_corner = torch.empty((F, 3, 3), dtype=torch.float32, device=dev)
    _lib.call("p3d_face_areas_normals_backward", "face_areas_normals_backward", dev, ga, gn, v, f, V, F, per_corner)
    return _C.scatter_face_grads(per_corner, f, V)


class _FaceAreasNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, faces):
        ctx.save_for_backward(verts, faces)
        return face_areas_normals_forward(verts, faces)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_areas, grad_normals):
        verts, faces = ctx.saved_tensors
        return face_areas_normals_backward(grad_areas.contiguous(), grad_normals.contiguous(), verts, faces), None


def face_areas_normals(verts, faces):
    """verts (V, 3) float32, faces (F, 3) int64, both on the GPU -> (areas (F,), normals (F, 3)), differentiable in verts."""
    return _FaceAreasNormals.apply(verts, faces)


# ---- vertex normals --------------------------------------------------------------------------------------------------------------
def vert_incidence(faces, V):
    """The incidence list of a topology (include/p3d_amd.h: p3d_verts_normals_forward): (offsets (V + 1,) int32, corners int32).
    corners holds the corners 3 f + j of faces (F, 3) whose vertex lies in [0, V) (negative ids wrap once, ids still out of range
    are dropped), sorted stably by vertex -- `_C._sorted_corners`; vertex v owns corners[offsets[v]:offsets[v + 1]].  Plain torch,
    on the device of `faces` (CPU tensors too); one host sync for the number of valid corners."""
    V = int(V)
    if faces.dim() != 2 or faces.size(1) != 3:
        raise RuntimeError("vert_incidence: faces must have shape (F, 3)")
    if faces.numel() >= 2 ** 31:
        raise RuntimeError("vert_incidence: 3 F must fit an int32")
    corners = _C._sorted_corners(faces, V)
    flat = faces.reshape(-1)[corners]
    vert = torch.where(flat < 0, flat + V, flat)  # ascending: the corners are sorted by it
    offsets = torch.searchsorted(vert, torch.arange(V + 1, dtype=vert.dtype, device=vert.device))
    return offsets.to(torch.int32).contiguous(), corners.to(torch.int32).contiguous()


def _check_incidence(incidence, V, F, dev):
    offsets, corners = incidence
    for name, t in (("offsets", offsets), ("corners", corners)):
        if t.dtype != torch.int32 or t.device != dev or not t.is_contiguous() or t.dim() != 1:
            raise RuntimeError(f"verts_normals: incidence {name} must be a contiguous int32 vector on {dev} (vert_incidence makes them)")
    if offsets.numel() != V + 1 or corners.numel() > 3 * F:
        raise RuntimeError("verts_normals: the incidence list belongs to another topology (offsets must have V + 1 entries, corners at "
                           "most 3 F)")
    return offsets, corners


def _float_rows(ws):
    """The float32 view of a contiguous workspace: the byte buffers of _C._workspace go where the header declares `float*`."""
    if ws.dtype == torch.float32:
        return ws
    raw = ws.reshape(-1).view(torch.uint8)
    return raw[:raw.numel() // 4 * 4].view(torch.float32)


def verts_normals_forward(verts, faces, offsets, corners, face_raw=None):
    """(normals (V, 3), sums (V, 3)): sums are the un-normalised area-weighted sums the backward needs.  face_raw: the (F, 3) float32
    workspace, made here when None (every row is written before it is read)."""
    v, f = _check(verts, faces, "verts_normals")
    V, F = v.size(0), f.size(0)
    dev = v.device
    offsets, corners = _check_incidence((offsets, corners), V, F, dev)
    lib = _lib.load()
    if face_raw is None:
        face_raw = _C._workspace(lib.p3d_verts_normals_forward_workspace_bytes(F), dev)
    elif face_raw.device != dev or not face_raw.is_contiguous() or face_raw.numel() * face_raw.element_size() < F * 12:
        raise RuntimeError("verts_normals: face_raw must be a contiguous workspace of F * 3 floats on the device of verts")
    sums = torch.empty((V, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((V, 3), dtype=torch.float32, device=dev)
    _lib.call("p3d_verts_normals_forward", "verts_normals_forward", dev, v, f, offsets, corners, V, F, _float_rows(face_raw), sums, normals)
    return normals, sums


def verts_normals_backward(grad_normals, verts, faces, sums, offsets, corners, face_rows=None):
    """grad_verts (V, 3).  face_rows: the (F, 3, 3) float32 workspace, made here when None."""
    v, f = _check(verts, faces, "verts_normals_backward")
    _C._same_device(("verts", verts), ("grad_normals", grad_normals), ("sums", sums))
    V, F = v.size(0), f.size(0)
    dev = v.device
    offsets, corners = _check_incidence((offsets, corners), V, F, dev)
    g, s = _C._c(grad_normals, torch.float32), _C._c(sums, torch.float32)
    if tuple(g.shape) != (V, 3) or tuple(s.shape) != (V, 3):
        raise RuntimeError("verts_normals_backward: grad_normals and sums must have shape (V, 3)")
    lib = _lib.load()
    if face_rows is None:
        face_rows = _C._workspace(lib.p3d_verts_normals_backward_workspace_bytes(F), dev)
    elif face_rows.device != dev or not face_rows.is_contiguous() or face_rows.numel() * face_rows.element_size() < F * 36:
        raise RuntimeError("verts_normals_backward: face_rows must be a contiguous workspace of F * 9 floats on the device of verts")
    out = torch.empty((V, 3), dtype=torch.float32, device=dev)
    _lib.call("p3d_verts_normals_backward", "verts_normals_backward", dev, g, v, f, s, offsets, corners, V, F, _float_rows(face_rows), out)
    return out


class _VertsNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, faces, offsets, corners):
        normals, sums = verts_normals_forward(verts, faces, offsets, corners)
        ctx.save_for_backward(verts, faces, sums, offsets, corners)
        return normals

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_normals):
        verts, faces, sums, offsets, corners = ctx.saved_tensors
        return verts_normals_backward(grad_normals.contiguous(), verts, faces, sums, offsets, corners), None, None, None


def verts_normals(verts, faces, incidence=None):
    """verts (V, 3) float32, faces (F, 3) int64, both on the GPU -> unit vertex normals (V, 3), differentiable in verts: the sum of
    (v2 - v1) x (v0 - v1) over the faces of a vertex (area weighting: the cross product's length is twice the area), divided by
    max(|sum|, 1e-6) -- zeros for a vertex without a face.  incidence: vert_incidence(faces, V); built here when None (a host sync:
    build it once per topology and pass it in a loop)."""
    _check(verts, faces, "verts_normals")
    if incidence is None:
        incidence = vert_incidence(faces, verts.size(0))
    return _VertsNormals.apply(verts, faces, incidence[0], incidence[1])
