"""sample_points_from_meshes on the HIP kernels of csrc/sample_points.hip (pytorch3d/ops/sample_points_from_meshes.py).

    sample_points_from_meshes(meshes, num_samples=10000, return_normals=False, return_textures=False, *, generator=None,
                              uniforms=None, check_finite=True, return_face_idxs=False)
    sample_points_packed(verts_packed, faces_packed, mesh_to_faces_packed_first_idx, num_faces_per_mesh, num_samples, uniforms,
                         return_normals=False)  -> (samples, normals or None, sample_face_idxs, bary)      the same on plain tensors

The reference's signature, return shapes, tuple order and ValueErrors for the first four arguments; `meshes` is the reference's Meshes
or this package's PackedMeshes (anything with verts_packed / faces_packed / mesh_to_faces_packed_first_idx / num_faces_per_mesh).

RANDOMNESS IS AN INPUT.  Everything is a deterministic function of `uniforms`, a float32 (N, S, 3) tensor in [0, 1): u0 picks the face,
u1 and u2 the point on it.  When it is not given it is torch.rand((N, S, 3), generator=generator, device=...): one launch, reproducible
under torch.manual_seed.  torch's own multinomial stream is NOT reproduced; the contract is the distribution -- a face with probability
proportional to its area, the point uniform on the face -- and this arithmetic:
    cdf         per mesh the inclusive prefix sum of the float32 face areas, non-decreasing, a face of zero area repeating its
                predecessor's value (include/p3d_amd.h: the scan tree and its depth)
    face        the first face f of the mesh with cdf[f] > u0 * total (never a face of zero area; u0 * total clamped below the total)
    weights     r = sqrt(u1), w0 = 1 - r, w1 = r (1 - u2), w2 = r u2          the reference's _rand_barycentric_coords
    sample      (w0 v0 + w1 v1) + w2 v2                                        the reference's line 112, its operation order
    normal      c / max(|c|, sys.float_info.epsilon), c = (v1 - v0) x (v2 - v1)  the sampler's own normal, not face_areas_normals' 1e-6
A float32 table cannot resolve a face whose area is below 2^-24 of the running total inside its mesh: it is absorbed and never drawn
(the reference's float32 multinomial normalisation has a limit of the same order).

An empty mesh gives zero rows, and so does a mesh whose total area is zero or not finite (sample_face_idxs -1) -- the reference raises
from multinomial in the zero-total case; here the row is zeros and the call goes on.

float32 vertices on the GPU are ONE autograd node: four launches forward with no host wait, the backward sums a row per face (w_k
grad_sample per corner and the plain sum of grad_normals: the normal depends on the face alone, so its Jacobian is applied once per
face) and ends in the package's face-gradient scatter -- float atomics, or the ordered sums under the strict deterministic flag.
No gradient flows into uniforms or through the choice of face (the reference chooses under no_grad too).  Anything else -- CPU
tensors, float64 -- takes the torch formulation of the same contract below, differentiated by autograd.

check_finite=True keeps the reference's isfinite(verts).all() check and its message; it costs one host sync.  With False nothing in
the call waits for the device.
"""
import collections
import sys

import torch

from . import _C, _lib

_EPS = sys.float_info.epsilon
_Fragments = collections.namedtuple("Fragments", ["pix_to_face", "zbuf", "bary_coords", "dists"])
_ISEMPTY_KEY = "_p3d_amd_isempty"  # kept per topology by the patches of pytorch3d_amd.shim


def kernel_path(verts):
    """Whether sampling from these packed vertices runs on the kernels."""
    return torch.is_tensor(verts) and verts.is_cuda and verts.dtype == torch.float32


def _check(verts, faces, first, nf, num_samples, uniforms, who):
    if verts.dim() != 2 or verts.size(1) != 3:
        raise RuntimeError(f"{who}: verts_packed must have shape (V, 3)")
    if faces.dim() != 2 or faces.size(1) != 3:
        raise RuntimeError(f"{who}: faces_packed must have shape (F, 3)")
    if first.dim() != 1 or nf.dim() != 1 or first.numel() != nf.numel():
        raise RuntimeError(f"{who}: mesh_to_faces_packed_first_idx and num_faces_per_mesh must have one entry per mesh")
    N, S = int(first.numel()), int(num_samples)
    if S < 0:
        raise RuntimeError(f"{who}: num_samples must not be negative")
    if tuple(uniforms.shape) != (N, S, 3) or uniforms.dtype != torch.float32:
        raise RuntimeError(f"{who}: uniforms must be a float32 tensor of shape (N, num_samples, 3) = {(N, S, 3)}")
    for name, t in (("faces_packed", faces), ("mesh_to_faces_packed_first_idx", first), ("num_faces_per_mesh", nf), ("uniforms", uniforms)):
        if t.device != verts.device:
            raise RuntimeError(f"{who}: {name} is on {t.device}, verts_packed on {verts.device}")
    return N, S


# ---- the torch formulation (CPU, float64) ------------------------------------------------------------------------------------------
def face_table(verts, faces, first, nf):
    """(cdf (N, max_F) padded, total (N,)): per mesh the running sum of its faces' areas, in the dtype of verts.  torch.cumsum runs
    along a row in order, so the table is non-decreasing and a face of zero area repeats its predecessor.  Syncs (max_F)."""
    N, F = int(first.numel()), int(faces.shape[0])
    max_f = int(nf.max()) if N else 0
    if max_f == 0 or F == 0:
        return verts.new_zeros((N, 0)), verts.new_zeros((N,))
    fv = verts[faces]
    a, b = fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0]
    # one operation each, as the kernel has them (torch.cross may fuse a product into the subtraction, and then a x a is not 0)
    cx, cy, cz = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    areas = torch.sqrt(cx * cx + cy * cy + cz * cz) / 2.0
    col = torch.arange(max_f, device=verts.device)[None, :]
    valid = col < nf[:, None]
    padded = torch.where(valid, areas[(first[:, None] + col).clamp(0, F - 1)], areas.new_zeros(()))
    cdf = torch.cumsum(padded, dim=1)
    return cdf, cdf[:, -1]


def choose_faces(cdf, total, first, nf, u0):
    """sample_face_idxs (N, S) int64, packed; -1 for a mesh that is empty or whose total is zero or not finite."""
    N, S = u0.shape
    ok = (nf > 0) & (total > 0) & torch.isfinite(total)
    if cdf.shape[1] == 0:
        return torch.full((N, S), -1, dtype=torch.int64, device=u0.device)
    tot = torch.where(ok, total, torch.ones_like(total))[:, None]
    t = u0.to(cdf.dtype) * tot
    t = torch.where(t < tot, t, torch.nextafter(tot, torch.zeros_like(tot)).expand_as(t))
    t = torch.where(t >= 0, t, torch.zeros_like(t))
    local = torch.searchsorted(cdf.contiguous(), t.contiguous(), right=True).clamp(max=cdf.shape[1] - 1)  # the first cdf > t
    return torch.where(ok[:, None], first[:, None] + local, torch.full_like(local, -1))


def barycentric_weights(uniforms):
    # the root through float64: rounding a float64 root to float32 is the correctly rounded float32 root (53 >= 2 x 24 + 2 bits), which
    # is what the kernel computes -- torch's float32 sqrt on the CPU is off by one ulp on some hosts
    r = uniforms[..., 1].double().sqrt().to(uniforms.dtype)
    return torch.stack([1.0 - r, r * (1.0 - uniforms[..., 2]), r * uniforms[..., 2]], -1)


def _torch_sample(verts, faces, first, nf, uniforms, return_normals):
    with torch.no_grad():
        cdf, total = face_table(verts, faces, first, nf)
        idx = choose_faces(cdf, total, first, nf, uniforms[..., 0])
    hit = idx >= 0
    w = torch.where(hit[..., None], barycentric_weights(uniforms.to(verts.dtype)), verts.new_zeros(()))
    if faces.shape[0] == 0:
        z = verts.new_zeros(tuple(idx.shape) + (3,))
        return z, (z.clone() if return_normals else None), idx, w
    f = faces[idx.clamp_min(0)]  # (N, S, 3)
    a, b, c = verts[f[..., 0]], verts[f[..., 1]], verts[f[..., 2]]
    samples = torch.where(hit[..., None], (w[..., 0:1] * a + w[..., 1:2] * b) + w[..., 2:3] * c, verts.new_zeros(()))
    normals = None
    if return_normals:
        fv = verts[faces]
        n = torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 1], dim=1)
        n = n / n.norm(dim=1, p=2, keepdim=True).clamp(min=_EPS)
        normals = torch.where(hit[..., None], n[idx.clamp_min(0)], verts.new_zeros(()))
    return samples, normals, idx, w


# ---- the kernels -------------------------------------------------------------------------------------------------------------------
def _forward(verts, faces, first, nf, uniforms, S, return_normals, table_out=None, out=None):
    lib, dev = _lib.load(), verts.device
    V, F, N = verts.shape[0], faces.shape[0], first.numel()
    if F > 2 ** 31 - 1:
        raise RuntimeError("sample_points: F must fit an int32")
    if out is not None:  # tests: outputs that hold poison, to show that every entry is written
        samples, normals, idx, bary = out
        for t, shape, dt in ((samples, (N, S, 3), torch.float32), (normals, (N, S, 3), torch.float32), (idx, (N, S), torch.int64),
                             (bary, (N, S, 3), torch.float32)):
            if t is not None and (tuple(t.shape) != shape or t.dtype != dt or t.device != dev or not t.is_contiguous()):
                raise RuntimeError("sample_points: _out must hold contiguous (samples, normals, sample_face_idxs, bary) of the call's shapes")
        normals = normals if return_normals else None
    else:
        samples = torch.empty((N, S, 3), dtype=torch.float32, device=dev)
        normals = torch.empty((N, S, 3), dtype=torch.float32, device=dev) if return_normals else None
        idx = torch.empty((N, S), dtype=torch.int64, device=dev)
        bary = torch.empty((N, S, 3), dtype=torch.float32, device=dev)
    nbytes = lib.p3d_sample_points_forward_workspace_bytes(F)
    ws = _C._workspace(nbytes, dev)
    _lib.call("p3d_sample_points_forward", "sample_points_from_meshes forward", dev, verts, faces, first, nf, uniforms, V, F, N, S, samples,
              normals, idx, bary, ws, nbytes)
    if table_out is not None:  # tests: the table is the workspace's first F floats
        table_out.append(ws[:F * 4].view(torch.float32).clone())
    return samples, normals, idx, bary


def _backward(grad_samples, grad_normals, verts, faces, idx, bary):
    lib, dev = _lib.load(), verts.device
    V, F, NS = verts.shape[0], faces.shape[0], idx.numel()
    if F == 0 or V == 0:
        return torch.zeros_like(verts)
    gs = torch.zeros_like(bary) if grad_samples is None else _C._c(grad_samples, torch.float32)
    gn = None if grad_normals is None else _C._c(grad_normals, torch.float32)
    sorted_samples = _C._sorted_hits(idx) if _C._ordered() else None
    num_sorted = 0 if sorted_samples is None else sorted_samples.numel()
    if sorted_samples is not None and num_sorted == 0:  # (a NULL pointer would select the atomic path)
        return torch.zeros_like(verts)
    nbytes = lib.p3d_sample_points_backward_workspace_bytes(F, 0 if gn is None else 1, num_sorted)
    ws = _C._workspace(nbytes, dev)
    per_corner = torch.empty((F, 3, 3), dtype=torch.float32, device=dev)
    _lib.call("p3d_sample_points_backward", "sample_points_from_meshes backward", dev, gs, gn, verts, faces, idx, bary, sorted_samples,
              num_sorted, V, F, NS, per_corner, ws, nbytes)
    return _C.scatter_face_grads(per_corner, faces, V)


class _SamplePoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, faces, first, nf, uniforms, S, return_normals, table_out, out):
        v = _C._c(verts, torch.float32)
        samples, normals, idx, bary = _forward(v, faces, first, nf, uniforms, S, return_normals, table_out, out)
        ctx.save_for_backward(v, faces, idx, bary)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(idx, bary)
        return samples, normals, idx, bary

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_samples, grad_normals, _grad_idx, _grad_bary):
        v, faces, idx, bary = ctx.saved_tensors
        if grad_samples is None and grad_normals is None:
            return (None,) * 9
        return (_backward(grad_samples, grad_normals, v, faces, idx, bary),) + (None,) * 8


def sample_points_packed(verts_packed, faces_packed, mesh_to_faces_packed_first_idx, num_faces_per_mesh, num_samples, uniforms,
                         return_normals=False, _table_out=None, _out=None):
    """verts_packed (V, 3), faces_packed (F, 3) integer, mesh_to_faces_packed_first_idx / num_faces_per_mesh (N,) integer, uniforms
    (N, num_samples, 3) float32 in [0, 1), all on one device -> (samples (N, S, 3), normals (N, S, 3) or None, sample_face_idxs (N, S)
    int64 in packed indexing, bary (N, S, 3)): differentiable in verts_packed through samples and normals.  float32 on the GPU runs
    the kernels, anything else the torch formulation of the same contract (the module docstring).
    _table_out (tests): a list that receives the kernels' cumulative table (F,); _out (tests): the four outputs, allocated by the
    caller (kernels only)."""
    verts, faces = verts_packed, faces_packed.to(torch.int64).contiguous()
    first = mesh_to_faces_packed_first_idx.to(torch.int64).contiguous()
    nf = num_faces_per_mesh.to(torch.int64).contiguous()
    _, S = _check(verts, faces, first, nf, num_samples, uniforms, "sample_points_packed")
    if kernel_path(verts):
        return _SamplePoints.apply(verts, faces, first, nf, uniforms.contiguous(), S, bool(return_normals), _table_out, _out)
    return _torch_sample(verts, faces, first, nf, uniforms, bool(return_normals))


# ---- on meshes -----------------------------------------------------------------------------------------------------------------------
def _isempty(meshes):
    """The reference's Meshes.isempty() -- no mesh, or no mesh with a face -- from the flag kept with the topology where the object
    carries it, else from the packed faces' shape: no host sync either way."""
    flag = getattr(meshes, "__dict__", {}).get(_ISEMPTY_KEY)
    if flag is not None:
        return bool(flag)
    return len(meshes) == 0 or int(meshes.faces_packed().shape[0]) == 0


def sample_points_from_meshes(meshes, num_samples: int = 10000, return_normals: bool = False, return_textures: bool = False, *,
                              generator=None, uniforms=None, check_finite: bool = True, return_face_idxs: bool = False):
    """Points sampled uniformly from the surface of every mesh of the batch, a face drawn with probability proportional to its area.

    Returns samples (N, num_samples, 3), then normals (N, num_samples, 3) if return_normals, then textures (N, num_samples, C) if
    return_textures -- the reference's tuple order, a bare tensor when neither is asked for -- and last sample_face_idxs
    (N, num_samples) int64 in packed indexing if return_face_idxs.  Rows of an empty mesh are zeros (face index -1); so are the rows of
    a mesh whose total area is zero or not finite, where the reference raises from multinomial.
    generator / uniforms: the randomness (the module docstring); check_finite=False skips the isfinite check and its host sync.
    Raises ValueError for an empty batch, for textures that the meshes do not have, and (check_finite) for nan / inf vertices."""
    if _isempty(meshes):
        raise ValueError("Meshes are empty.")
    verts = meshes.verts_packed()
    if check_finite and not torch.isfinite(verts).all():
        raise ValueError("Meshes contain nan or inf.")
    if return_textures and getattr(meshes, "textures", None) is None:
        raise ValueError("Meshes do not contain textures.")
    N, S = len(meshes), int(num_samples)
    if uniforms is None:
        uniforms = torch.rand((N, S, 3), generator=generator, dtype=torch.float32, device=verts.device)
    samples, normals, idx, bary = sample_points_packed(verts, meshes.faces_packed(), meshes.mesh_to_faces_packed_first_idx(),
                                                       meshes.num_faces_per_mesh(), S, uniforms, return_normals)
    out = [samples]
    if return_normals:
        out.append(normals)
    if return_textures:
        # the reference's lines 126-138: fragments of shape (N, H = S, W = 1, K = 1); zbuf and dists are not read by sample_textures
        try:
            from pytorch3d.renderer.mesh.rasterizer import Fragments
        except ImportError:  # textures of another package on a duck-typed batch: the same four fields
            Fragments = _Fragments

        dummy = torch.zeros((N, S, 1, 1), dtype=torch.float32, device=verts.device)
        fragments = Fragments(pix_to_face=idx.view(N, S, 1, 1), zbuf=dummy, bary_coords=bary.to(torch.float32).view(N, S, 1, 1, 3),
                              dists=dummy)
        out.append(meshes.sample_textures(fragments)[:, :, 0, 0, :])
    if return_face_idxs:
        out.append(idx)
    return out[0] if len(out) == 1 else tuple(out)
