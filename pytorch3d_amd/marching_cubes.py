"""marching_cubes: scalar fields to isosurface meshes on csrc/marching_cubes.hip.

    marching_cubes(vol_batch, isolevel=None, return_local_coords=True)          the reference's signature and result: two lists
    marching_cubes_packed(vol_batch, isolevel=None, return_local_coords=True)   (verts_packed, faces_packed, num_verts_per_mesh,
                                                                                 num_faces_per_mesh), no lists built
    marching_cubes_torch(...)                                                   the device contract as a torch formulation, any device
    marching_cubes_op(vol, isolevel)                                            `pytorch3d._C.marching_cubes` of the shim: one volume

The contract (pytorch3d/ops/marching_cubes.py and csrc/marching_cubes restated; checked against the reference's compiled CPU operator
through tests/golden/marching_cubes_ref.npz; in full: csrc/implicit_abi.h).  vol_batch (N, D, H, W) float32; x runs along W, y along H,
z along D.
  isolevel    a number, rounded to float32; None: (max + min) / 2 per volume in float32 (made on the device: no host read).
  inside      value < isolevel, strictly; NaN: outside.
  vertex      on a lattice edge whose two ends differ, by the reference's snapping chain and p1 (1 - r) + p2 r on every coordinate.
  GPU tensors the DEVICE contract: every table triangle, degenerate ones too, cubes with x fastest; one vertex per crossed lattice edge in
              the order of the reference's sorted edge ids = (lattice point x fastest, axis x y z).
  CPU tensors the CPU contract (the library's host loop): vertices in order of first use; a triangle with two vertices closer than 1e-5 in
              every coordinate is dropped and every later triangle of its cube with it.
  local       return_local_coords: each coordinate c / ((size - 1) / 2) - 1 in float32, a division and a subtraction.  The reference
              goes through a 4 x 4 inverse and a matmul there: the tests gate this at 4 x the reference's own float32 rounding.
  result      per volume (V_n, 3) float32 and (F_n, 3) int64 with indices local to the volume; the Python list `[]` for a volume
              without a face.  Other dtypes than float32 raise RuntimeError, as the reference's operator does.
  autograd    no gradient; as in the reference the result hangs on an autograd node whose backward raises
              ValueError("marching_cubes backward is not supported") when the volume requires grad.

The kernels take float32 GPU volumes (any strides) with 15 N D H W within int32: `kernel_path`.  One host read per call, whatever N is
and with isolevel None too -- the (N, 2) counts, between the count and the emit entry; the reference has three per volume and a
torch.unique over 3 F keys.  Larger GPU inputs take `marching_cubes_torch`, the same contract in torch with int64 indices.
"""
import functools
import os
import re

import torch

from . import _C

CALLS = {"fused": 0, "formulation": 0, "host": 0}  # what ran (the shim's PATCH_CALLS and the tests read it)

EPS = 1e-5
_TABLE_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "marching_cubes_tables.h")


@functools.lru_cache(maxsize=1)
def triangle_table():
    """The 256 rows of csrc/marching_cubes_tables.h as tuples of entries 8 * axis + corner (the header is the one copy of the table)."""
    with open(_TABLE_HEADER) as f:
        body = re.search(r"entries\[256\]\[16\] = \{(.*?)\};", f.read(), re.S).group(1)
    rows = [tuple(int(e) for e in row.split(",") if int(e) != 255) for row in re.findall(r"\{([^{}]*)\}", body)]
    assert len(rows) == 256 and all(len(r) % 3 == 0 for r in rows)
    return tuple(rows)


@functools.lru_cache(maxsize=8)
def _table_tensors(device):
    rows = triangle_table()
    return (torch.tensor([list(r) + [255] * (16 - len(r)) for r in rows], dtype=torch.int64, device=device),
            torch.tensor([len(r) // 3 for r in rows], dtype=torch.int64, device=device))


def _check(vol_batch):
    if not torch.is_tensor(vol_batch) or vol_batch.dim() != 4:
        raise ValueError(f"vol_batch must be a tensor of shape (N, D, H, W), got {tuple(getattr(vol_batch, 'shape', ()))}")
    if vol_batch.dtype != torch.float32:
        raise RuntimeError(f"marching_cubes: expected scalar type Float but found {vol_batch.dtype}")


def isolevels(vol_batch, isolevel):
    """(N,) float32 thresholds on the volumes' device: the number rounded to float32, or (max + min) / 2 per volume."""
    N = vol_batch.shape[0]
    if isolevel is not None:
        return torch.full((N,), float(isolevel), dtype=torch.float32, device=vol_batch.device)
    if vol_batch[0].numel() == 0 or N == 0:
        return torch.zeros((N,), dtype=torch.float32, device=vol_batch.device)
    return (vol_batch.amax((1, 2, 3)) + vol_batch.amin((1, 2, 3))) / 2


def kernel_path(vol_batch, isolevel=None, return_local_coords=True):
    """Whether marching_cubes(vol_batch, ...) runs csrc/marching_cubes.hip (else: the host loop for CPU tensors, marching_cubes_torch
    for GPU sizes beyond int32)."""
    return bool(torch.is_tensor(vol_batch) and vol_batch.is_cuda and vol_batch.dtype == torch.float32 and vol_batch.dim() == 4
                and _C.marching_cubes_fits(*vol_batch.shape))


def to_local(verts, D, H, W):
    """World coordinates (x in [0, W - 1], ...) -> [-1, 1]^3: c / ((size - 1) / 2) - 1."""
    return verts / ((torch.tensor([W, H, D], dtype=torch.float32, device=verts.device) - 1) * 0.5) - 1


def _torch_packed(vol, iso, local):
    """The device contract over (N, D, H, W) with thresholds iso (N,) -> (verts, ids, faces, num_verts, num_faces) on vol's device."""
    N, D, H, W = vol.shape
    dev = vol.device
    L = D * H * W
    inside = vol < iso.view(N, 1, 1, 1)
    flags = torch.zeros((N, D, H, W, 3), dtype=torch.bool, device=dev)
    flags[:, :, :, :-1, 0] = inside[:, :, :, :-1] != inside[:, :, :, 1:]
    flags[:, :, :-1, :, 1] = inside[:, :, :-1] != inside[:, :, 1:]
    flags[:, :-1, :, :, 2] = inside[:, :-1] != inside[:, 1:]
    if min(D, H, W) < 2:
        flags.zero_()  # no cube: nothing is returned
    flat = flags.view(N, 3 * L)
    rank = flat.cumsum(1) - 1
    num_verts = flat.sum(1)
    n, z, y, x, a = flags.nonzero().unbind(1)  # row-major: (n, lattice point, axis) order
    step = torch.nn.functional.one_hot(a, 3)  # (x, y, z) of the edge's direction
    v1, v2 = vol[n, z, y, x], vol[n, z + step[:, 2], y + step[:, 1], x + step[:, 0]]
    p1 = torch.stack([x, y, z], 1).to(torch.float32)
    p2 = p1 + step.to(torch.float32)
    level = iso[n]
    r = (level - v1) / (v2 - v1)
    interp = p1 * (1 - r)[:, None] + p2 * r[:, None]
    at1, at2, flat12 = (level - v1).abs() < EPS, (level - v2).abs() < EPS, (v1 - v2).abs() < EPS
    verts = torch.where((at1 | (~at2 & flat12))[:, None], p1, torch.where(at2[:, None], p2, interp))
    if local:
        verts = to_local(verts, D, H, W)
    g = (z * H + y) * W + x
    ids = g * (W + W * H + L) + g + (step * torch.tensor([1, W, W * H], device=dev)).sum(1)
    if min(D, H, W) < 2:
        return verts, ids, torch.zeros((0, 3), dtype=torch.int64, device=dev), num_verts, torch.zeros_like(num_verts)
    config = torch.zeros((N, D - 1, H - 1, W - 1), dtype=torch.int64, device=dev)
    for i in range(8):
        dx, dy, dz = i & 1, i >> 1 & 1, i >> 2 & 1
        config |= inside[:, dz:D - 1 + dz, dy:H - 1 + dy, dx:W - 1 + dx].to(torch.int64) << i
    table, counts = _table_tensors(dev)
    num_faces = counts[config].view(N, -1).sum(1)
    cn, cz, cy, cx = (counts[config] > 0).nonzero().unbind(1)  # the cubes that emit, in cube order
    entries = table[config[cn, cz, cy, cx]]  # (A, 16)
    valid = entries != 255
    which = valid.nonzero()[:, 0]
    e = entries[valid]
    axis = e >> 3
    owner = ((cz[which] + (e >> 2 & 1)) * H + cy[which] + (e >> 1 & 1)) * W + cx[which] + (e & 1)
    faces = rank[cn[which], 3 * owner + axis].view(-1, 3)
    return verts, ids, faces, num_verts, num_faces


def marching_cubes_torch(vol_batch, isolevel=None, return_local_coords=True):
    """The device contract in torch, on the volumes' device (CPU tensors too: the device contract, not the host loop's).  Returns what
    marching_cubes_packed returns."""
    _check(vol_batch)
    with torch.no_grad():
        verts, _, faces, num_verts, num_faces = _torch_packed(vol_batch, isolevels(vol_batch, isolevel), return_local_coords)
    return verts, faces, num_verts, num_faces


def _fused(vol, iso, local):
    """The kernels: (verts, ids, faces, counts (N, 2) on the device, the same counts on the host -- the call's one read)."""
    CALLS["fused"] += 1
    N = vol.shape[0]
    if N == 0:
        counts = torch.zeros((0, 2), dtype=torch.int64, device=vol.device)
        return (*_C.marching_cubes_emit(counts, vol, iso, local, 0, 0), counts, counts.cpu())
    ws, counts = _C.marching_cubes_count(vol, iso)
    host = counts.cpu()  # the one host read of the call
    total_verts, total_faces = (int(t) for t in host.sum(0))
    verts, ids, faces = _C.marching_cubes_emit(ws, vol, iso, local, total_verts, total_faces)
    return verts, ids, faces, counts, host


def _host(vol, iso, local):
    """The library's host loop volume by volume -> packed tensors and the (N, 2) counts."""
    CALLS["host"] += 1
    D, H, W = vol.shape[1:]
    pairs = [_C.marching_cubes_host(v, float(t)) for v, t in zip(vol, iso)]
    counts = torch.tensor([[len(v), len(f)] for v, f in pairs], dtype=torch.int64).reshape(-1, 2)
    verts = torch.cat([v for v, _ in pairs]) if pairs else torch.zeros((0, 3))
    faces = torch.cat([f for _, f in pairs]) if pairs else torch.zeros((0, 3), dtype=torch.int64)
    return (to_local(verts, D, H, W) if local and len(verts) else verts), torch.zeros((len(verts),), dtype=torch.int64), faces, counts, counts.clone()


def _run(vol, isolevel, local):
    """(verts, ids, faces, counts on the volumes' device, counts on the host) by the path the input takes."""
    _check(vol)
    with torch.no_grad():
        vol = vol.detach()
        iso = isolevels(vol, isolevel)
        if kernel_path(vol):
            return _fused(vol, iso, local)
        if not vol.is_cuda:
            return _host(vol, iso, local)
        CALLS["formulation"] += 1
        verts, ids, faces, num_verts, num_faces = _torch_packed(vol, iso, local)
        counts = torch.stack([num_verts, num_faces], 1)
        return verts, ids, faces, counts, counts.cpu()


class _MarchingCubes(torch.autograd.Function):
    """No gradient exists; as in the reference, asking for one raises instead of returning silence."""

    @staticmethod
    def forward(ctx, vol, isolevel, local):
        verts, ids, faces, counts, host = _run(vol, isolevel, local)
        ctx.mark_non_differentiable(ids, faces, counts, host)
        return verts, ids, faces, counts, host

    @staticmethod
    def backward(ctx, *grads):
        raise ValueError("marching_cubes backward is not supported")


def marching_cubes_packed(vol_batch, isolevel=None, return_local_coords=True):
    """(verts_packed (V, 3) float32, faces_packed (F, 3) int64 with per-volume indices, num_verts_per_mesh (N,), num_faces_per_mesh
    (N,)) on the volumes' device; a volume without a face has no vertex either."""
    verts, _, faces, counts, _ = _MarchingCubes.apply(vol_batch, isolevel, bool(return_local_coords))
    return verts, faces, counts[:, 0], counts[:, 1]


def marching_cubes(vol_batch, isolevel=None, return_local_coords=True):
    """pytorch3d.ops.marching_cubes: (verts list, faces list), `[]` in both for a volume without a face.  The entries are `split`
    views of the packed tensors."""
    verts, _, faces, _, host = _MarchingCubes.apply(vol_batch, isolevel, bool(return_local_coords))
    num_verts, num_faces = host[:, 0].tolist(), host[:, 1].tolist()
    return ([v if k else [] for v, k in zip(verts.split(num_verts, 0), num_faces)],
            [f if k else [] for f, k in zip(faces.split(num_faces, 0), num_faces)])


def marching_cubes_op(vol, isolevel):
    """`pytorch3d._C.marching_cubes(vol, isolevel)` of the shim module: ONE volume (D, H, W) -> (verts (V, 3) in world coordinates,
    faces (F, 3) int64, ids (V,) int64).  GPU: each vertex once with its strictly ascending edge id, so that the reference wrapper's
    torch.unique is the identity and its result the device contract; CPU: the host loop with ids of zeros, as the reference's."""
    if not torch.is_tensor(vol) or vol.dim() != 3:
        raise ValueError(f"marching_cubes: vol must be a tensor of shape (D, H, W), got {tuple(getattr(vol, 'shape', ()))}")
    verts, ids, faces, _, _ = _run(vol[None], isolevel, False)
    return verts, faces, ids
