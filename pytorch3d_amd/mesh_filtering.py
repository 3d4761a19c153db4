"""Taubin smoothing on csrc/mesh_laplacian.hip.

    taubin_smoothing(meshes, lambd=0.53, mu=-0.53, num_iter=10)            pytorch3d/ops/mesh_filtering.py
    taubin_smooth_packed(verts, topology, lambd, mu, num_iter)             the same on packed vertices
    taubin_smooth_torch(verts, edges, lambd, mu, num_iter)                 the reference's chain restated

Each iteration takes two half-steps  x := (1 - c) x + c (L x) / (L 1)  with c = lambd, then c = mu, where L[i, j] =
1 / (|x_i - x_j| + 1e-12) over the edges (norm_laplacian).  The reference rebuilds a sparse V x V matrix for every half-step, sums
its rows through torch.sparse.sum and multiplies with torch.mm.  Here a half-step is ONE launch, one lane per vertex over its row of
the adjacency the loss tables already hold (mesh_losses.mesh_loss_topology): 2 num_iter launches between two ping-pong buffers, no
host read, no atomics, the same bits on every run.  1 - c and c are formed in double on the host and rounded to float32 once, as
torch does with a Python scalar; the grouping (c (L x)) / (L 1) is the reference's.  A vertex without a neighbour gives 0 / 0 = NaN,
the reference's answer.

The kernel path runs for float32 GPU vertices that need no gradient -- not (torch.is_grad_enabled() and verts.requires_grad).  The
reference's function is differentiable through the weights: inputs that require grad, CPU tensors and float64 take the chain restated,
differentiated by autograd.  CALLS counts which of the two ran.
"""
import numpy as np
import torch

from . import _C, _lib
from .mesh_losses import MeshLossTopology, topology_of

CALLS = {"fused": 0, "chain": 0}
EPS = 1e-12  # norm_laplacian's default


def taubin_smooth_torch(verts, edges, lambd=0.53, mu=-0.53, num_iter=10):
    """mesh_filtering.py:49-56 with norm_laplacian (laplacian_matrices.py:159-172) on verts (V, 3) and edges (E, 2) int64.  The sparse
    matrix has the dtype of verts (the reference hard-codes float32 there and raises on float64 vertices)."""
    V = verts.shape[0]
    e01 = edges.t()
    for _ in range(int(num_iter)):
        for c in (lambd, mu):
            v0, v1 = verts[edges[:, 0]], verts[edges[:, 1]]
            w01 = torch.reciprocal((v0 - v1).norm(dim=1) + EPS)
            L = torch.sparse_coo_tensor(e01, w01, (V, V), dtype=verts.dtype)
            L = L + L.t()
            total_weight = torch.sparse.sum(L, dim=1).to_dense().view(-1, 1)
            verts = (1 - c) * verts + c * torch.mm(L, verts) / total_weight
    return verts


def kernel_path(verts):
    """Whether taubin_smooth_packed of these vertices runs the kernel (else: the chain)."""
    return (torch.is_tensor(verts) and verts.is_cuda and verts.dtype == torch.float32 and verts.dim() == 2 and verts.size(1) == 3
            and not (torch.is_grad_enabled() and verts.requires_grad))


def _f32(x):
    return float(np.float32(x))


def taubin_smooth_packed(verts, topology, lambd=0.53, mu=-0.53, num_iter=10):
    """verts (V, 3), topology: mesh_loss_topology(...).  The smoothed vertices (V, 3), a new tensor."""
    t = topology
    if not isinstance(t, MeshLossTopology):
        raise RuntimeError("taubin_smooth_packed: topology must come from mesh_loss_topology")
    if verts.dim() != 2 or verts.size(1) != 3 or verts.size(0) != t.V:
        raise RuntimeError(f"taubin_smooth_packed: verts must have shape (V, 3) with the V = {t.V} of the topology")
    if verts.device != t.device:
        raise RuntimeError(f"taubin_smooth_packed: verts are on {verts.device}, the topology is on {t.device}")
    if t.repeated:
        raise ValueError("taubin_smooth_packed: a face names one vertex twice; the tables do not model its self edge (use the "
                         "reference's function)")
    num_iter = int(num_iter)
    if num_iter < 0:
        raise ValueError("taubin_smooth_packed: num_iter must not be negative")
    if not kernel_path(verts):
        CALLS["chain"] += 1
        return taubin_smooth_torch(verts, t.edges.long(), lambd, mu, num_iter)
    CALLS["fused"] += 1
    v = _C._c(verts.detach(), torch.float32)
    out, scratch = torch.empty_like(v), torch.empty_like(v)
    _lib.call("p3di_mesh_taubin_smoothing", "taubin_smoothing", v.device, v, t.adj_offsets, t.adj, t.V, t.E, _f32(1 - lambd), _f32(lambd),
              _f32(1 - mu), _f32(mu), _f32(EPS), num_iter, scratch, out)
    return out


def taubin_smoothing(meshes, lambd: float = 0.53, mu: float = -0.53, num_iter: int = 10):
    """Taubin smoothing of every mesh of the batch: a new mesh object with the smoothed vertices.  A PackedMeshes comes back through
    update_verts_packed (the tables are handed on); anything else with verts_packed / faces_packed / num_verts_per_mesh /
    num_faces_per_mesh / faces_list -- the reference's Meshes -- as the reference builds it: type(meshes)(verts=list,
    faces=meshes.faces_list()), without textures."""
    from .structures import PackedMeshes

    verts = meshes.verts_packed()
    smoothed = taubin_smooth_packed(verts, topology_of(meshes), lambd, mu, num_iter) if verts.shape[0] else verts.clone()
    if isinstance(meshes, PackedMeshes):
        return meshes.update_verts_packed(smoothed)
    counts = meshes.num_verts_per_mesh().tolist()
    return type(meshes)(verts=list(smoothed.split(counts, 0)), faces=meshes.faces_list())
