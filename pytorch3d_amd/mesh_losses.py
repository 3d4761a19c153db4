"""The three mesh regularisers of a fitting loop on the HIP kernels of csrc/mesh_losses.hip.

    mesh_edge_loss(meshes, target_length=0.0)            pytorch3d/loss/mesh_edge_loss.py
    mesh_laplacian_smoothing(meshes, method="uniform")   pytorch3d/loss/mesh_laplacian_smoothing.py
    mesh_normal_consistency(meshes)                      pytorch3d/loss/mesh_normal_consistency.py
    edge_loss / laplacian_smoothing / normal_consistency (verts, topology, ...)   the same on packed vertices
    mesh_loss_topology(faces_packed, num_verts_per_mesh, num_faces_per_mesh)      the tables, once per topology

Same names, defaults and return values as the reference; `meshes` is this package's PackedMeshes or the reference's Meshes (anything
with verts_packed / faces_packed / num_verts_per_mesh / num_faces_per_mesh).  The reference redoes the topology's work on every call
(unique edges, a sort and a host round trip for the wing pairs, a sparse V x V matrix) and differentiates through gathers whose
backward adds with float atomics.  Here everything that depends on the faces alone is a set of int32 tables built once
(mesh_loss_topology, kept on the mesh object and inherited by the copies offset_verts / update_verts_packed make), each loss is one
autograd node, and every sum is a gather or a fixed tree: no float atomic, the same bits on every run, stream and process, with
torch.use_deterministic_algorithms on or off (include/p3d_amd.h: the tree and its depth).

float32 vertices on the GPU take the kernels.  CPU tensors, float64 and the methods "cot" / "cotcurv" take the torch formulation of
the same arithmetic below (differentiated by autograd).
"""
import torch

from . import _C, _lib

_TOPOLOGY_KEY = "_p3d_amd_loss_topology"


# ---- the wing-pair index (also `pytorch3d._C.mesh_normal_consistency_find_verts`: pytorch3d_amd/_aux_ops.py) ---------------------
def find_pair_positions(edge_num):
    """edge_num (E,) integers: how many entries each edge owns in an array sorted by edge.  Returns (P, 2) int64, P = sum k (k - 1) / 2:
    with o_e the offset of edge e, every (o_e + i, o_e + j) with i < j < edge_num[e]; edges ascending, then j, then i.  Vectorised, on
    the device of edge_num."""
    k = edge_num.reshape(-1).to(torch.int64)
    dev = k.device
    first = torch.cumsum(k, 0) - k
    nj = (k - 1).clamp_min(0)  # the (edge, j) rows: j = 1 .. k - 1
    row_edge = torch.repeat_interleave(torch.arange(k.numel(), device=dev), nj)
    j = torch.arange(row_edge.numel(), device=dev) - (torch.cumsum(nj, 0) - nj)[row_edge] + 1
    pair_row = torch.repeat_interleave(torch.arange(j.numel(), device=dev), j)  # row (edge, j) owns j pairs: i = 0 .. j - 1
    i = torch.arange(pair_row.numel(), device=dev) - (torch.cumsum(j, 0) - j)[pair_row]
    base = first[row_edge[pair_row]]
    return torch.stack([base + i, base + j[pair_row]], 1)


# ---- the tables --------------------------------------------------------------------------------------------------------------------
class MeshLossTopology:
    """What the three losses need from the faces alone (include/p3d_amd.h: mesh regularisers).  int32, contiguous, on the faces' device:
        edges (E, 2), edge_mesh (E,), num_edges (N,)            the set and order of Meshes.edges_packed()
        adj_offsets (V + 1,), adj (2 E,), vert_mesh (V,), num_verts (N,)   neighbours of a vertex ascending; deg(v) from the offsets
        pairs (P, 4), pair_mesh (P,), num_pairs (N,)            rows (v0, v1, a, b)
        pair_offsets (V + 1,), pair_slots (4 P,)                 per vertex its slots 4 pair + role, sorted stably by vertex
    and on the host N, V, E, P, `empty` (no mesh, no vertex or no face: the reference's isempty()) and `repeated`: some face names one
    vertex twice.  Such a face has a self edge (lo == hi), which the tables would count as an edge of length 0 and a neighbour of
    itself where the reference does something else: the losses refuse such a topology and the shim hands it to the reference."""

    __slots__ = ("N", "V", "E", "P", "empty", "repeated", "device", "edges", "edge_mesh", "num_edges", "adj_offsets", "adj", "vert_mesh", "num_verts",
                 "pairs", "pair_mesh", "num_pairs", "pair_offsets", "pair_slots")


def _i32(t):
    return t.to(torch.int32).contiguous()


def mesh_loss_topology(faces_packed, num_verts_per_mesh, num_faces_per_mesh):
    """faces_packed (F, 3) integer packed vertex ids, num_verts_per_mesh / num_faces_per_mesh (N,).  Plain torch on the device of the
    faces (CPU tensors too); syncs with the host -- build it once per topology."""
    faces = faces_packed
    if faces.dim() != 2 or faces.size(1) != 3:
        raise RuntimeError("mesh_loss_topology: faces_packed must have shape (F, 3)")
    if faces.numel() >= 2 ** 31:
        raise RuntimeError("mesh_loss_topology: 3 F must fit an int32")
    dev = faces.device
    faces = faces.to(torch.int64)
    nv = torch.as_tensor(num_verts_per_mesh).reshape(-1).to(device=dev, dtype=torch.int64)
    nf = torch.as_tensor(num_faces_per_mesh).reshape(-1).to(device=dev, dtype=torch.int64)
    if nv.numel() != nf.numel():
        raise RuntimeError("mesh_loss_topology: num_verts_per_mesh and num_faces_per_mesh must have one entry per mesh")
    t = MeshLossTopology()
    t.device = dev
    t.N, F = int(nv.numel()), int(faces.size(0))
    t.V = int(nv.sum()) if t.N else 0
    if t.N and int(nf.sum()) != F:
        raise RuntimeError("mesh_loss_topology: num_faces_per_mesh does not add up to the rows of faces_packed")
    V = t.V
    t.empty = t.N == 0 or V == 0 or F == 0
    vert_mesh = torch.repeat_interleave(torch.arange(t.N, device=dev), nv)
    # the unique undirected edges, ascending by lo * V + hi; corner 3 f + k of a face names the edge OPPOSITE its vertex k
    opposite = torch.stack([faces[:, [1, 2]], faces[:, [2, 0]], faces[:, [0, 1]]], 1)  # (F, 3, 2)
    lo, hi = opposite.amin(2), opposite.amax(2)
    key, corner_edge = torch.unique((lo * max(V, 1) + hi).reshape(-1), return_inverse=True)
    edges = torch.stack([key // max(V, 1), key % max(V, 1)], 1)
    t.E = int(edges.size(0))
    t.repeated = bool((lo == hi).any())
    edge_mesh = vert_mesh[edges[:, 0]] if t.E else edges.new_zeros((0,))
    # the adjacency: both directions of every edge, sorted by (vertex, neighbour)
    src, dst = torch.cat([edges[:, 0], edges[:, 1]]), torch.cat([edges[:, 1], edges[:, 0]])
    order = torch.argsort(src * max(V, 1) + dst)
    adj_offsets = torch.searchsorted(src[order].contiguous(), torch.arange(V + 1, device=dev))
    # the wing pairs: the corners sorted stably by edge, every pair (i < j) of corners of one edge
    order_c = torch.sort(corner_edge, stable=True).indices
    positions = find_pair_positions(torch.bincount(corner_edge, minlength=t.E))
    t.P = int(positions.size(0))
    if t.P * 4 >= 2 ** 31:
        raise RuntimeError("mesh_loss_topology: 4 P must fit an int32")
    pair_edge = corner_edge[order_c][positions[:, 0]]
    wing = faces.reshape(-1)[order_c]  # the vertex of a corner is the one opposite its edge
    pairs = torch.stack([edges[pair_edge, 0], edges[pair_edge, 1], wing[positions[:, 0]], wing[positions[:, 1]]], 1)
    pair_mesh = edge_mesh[pair_edge]
    slot_vert = pairs.reshape(-1)
    slots = torch.sort(slot_vert, stable=True).indices
    pair_offsets = torch.searchsorted(slot_vert[slots].contiguous(), torch.arange(V + 1, device=dev))
    t.edges, t.edge_mesh, t.num_edges = _i32(edges), _i32(edge_mesh), _i32(torch.bincount(edge_mesh, minlength=t.N))
    t.adj_offsets, t.adj, t.vert_mesh, t.num_verts = _i32(adj_offsets), _i32(dst[order]), _i32(vert_mesh), _i32(nv)
    t.pairs, t.pair_mesh, t.num_pairs = _i32(pairs), _i32(pair_mesh), _i32(torch.bincount(pair_mesh, minlength=t.N))
    t.pair_offsets, t.pair_slots = _i32(pair_offsets), _i32(slots)
    return t


def topology_of(meshes):
    """The tables of `meshes`, built on the first call and kept in its __dict__ (key: the packed faces tensor's address, shape and
    version, and V) -- the copies that share its __dict__ entries (PackedMeshes.update_verts_packed, the patched Meshes.offset_verts)
    inherit them, so a fitting loop builds them once."""
    faces = meshes.faces_packed()
    key = (faces.data_ptr(), tuple(faces.shape), faces._version, int(meshes.verts_packed().shape[0]))
    kept = getattr(meshes, "__dict__", {}).get(_TOPOLOGY_KEY)
    if kept is None or kept[0] != key:
        kept = (key, mesh_loss_topology(faces, meshes.num_verts_per_mesh(), meshes.num_faces_per_mesh()))
        if hasattr(meshes, "__dict__"):
            meshes.__dict__[_TOPOLOGY_KEY] = kept
    return kept[1]


# ---- the torch formulation (CPU, float64, cot / cotcurv) ---------------------------------------------------------------------------
def _weights(counts, mesh):
    return 1.0 / counts.long()[mesh.long()].float()


def _torch_edge_loss(verts, t, target_length):
    e = t.edges.long()
    length = (verts[e[:, 0]] - verts[e[:, 1]]).norm(dim=1, p=2)
    return (((length - target_length) ** 2.0) * _weights(t.num_edges, t.edge_mesh)).sum() / t.N


def _neighbour_rows(t):
    off = t.adj_offsets.long()
    return torch.repeat_interleave(torch.arange(t.V, device=off.device), off[1:] - off[:-1]), t.adj.long()


def _cot_weights(verts, faces):
    """Per face and corner k: the cotangent of the angle at vertex k over 4 -- (b^2 + c^2 - a^2) / area / 4 with a the side opposite
    the corner and the area by Heron's formula, clamped at 1e-12 before the root -- and the area itself."""
    x = verts[faces]  # (F, 3, 3)
    side = torch.stack([(x[:, 1] - x[:, 2]).norm(dim=1), (x[:, 0] - x[:, 2]).norm(dim=1), (x[:, 0] - x[:, 1]).norm(dim=1)], 1)
    s = 0.5 * (side[:, 0] + side[:, 1] + side[:, 2])
    area = (s * (s - side[:, 0]) * (s - side[:, 1]) * (s - side[:, 2])).clamp(min=1e-12).sqrt()
    sq = side * side
    cot = torch.stack([sq[:, 1] + sq[:, 2] - sq[:, 0], sq[:, 0] + sq[:, 2] - sq[:, 1], sq[:, 0] + sq[:, 1] - sq[:, 2]], 1) / area[:, None]
    return cot / 4.0, area


def _torch_laplacian(verts, t, method, faces):
    w = _weights(t.num_verts, t.vert_mesh)
    if method == "uniform":
        row, col = _neighbour_rows(t)
        off = t.adj_offsets.long()
        deg = (off[1:] - off[:-1]).clamp_min(1).to(verts.dtype)  # (a vertex without a neighbour: its sum is 0)
        r = torch.zeros_like(verts).index_add(0, row, verts[col]) / deg[:, None] - verts
    else:
        # the cotangent Laplacian is a constant of the step (no gradient through its entries): L[i, j] = the sum, over the faces that
        # hold edge (i, j), of cot(angle opposite the edge) / 4, symmetric
        with torch.no_grad():
            cot, area = _cot_weights(verts, faces)
            i = torch.cat([faces[:, [1, 2, 0]].reshape(-1), faces[:, [2, 0, 1]].reshape(-1)])
            j = torch.cat([faces[:, [2, 0, 1]].reshape(-1), faces[:, [1, 2, 0]].reshape(-1)])
            val = torch.cat([cot.reshape(-1), cot.reshape(-1)])
            row_sum = torch.zeros(t.V, dtype=val.dtype, device=val.device).index_add(0, i, val)[:, None]
        lx = torch.zeros_like(verts).index_add(0, i, val[:, None].to(verts.dtype) * verts[j])
        if method == "cot":
            with torch.no_grad():
                norm_w = torch.where(row_sum > 0, 1.0 / row_sum, row_sum)
            r = lx * norm_w - verts
        else:
            with torch.no_grad():
                vert_area = torch.zeros(t.V, dtype=area.dtype, device=area.device).index_add(0, faces.reshape(-1), area.repeat_interleave(3))
                inv_area = torch.where(vert_area > 0, 1.0 / vert_area, vert_area)[:, None]
            r = (lx - row_sum * verts) * (0.25 * inv_area)
    return (r.norm(dim=1) * w).sum() / t.N


def _torch_normal_consistency(verts, t):
    p = t.pairs.long()
    x0 = verts[p[:, 0]]
    e = verts[p[:, 1]] - x0
    n0 = torch.cross(e, verts[p[:, 2]] - x0, dim=1)
    n1 = -torch.cross(e, verts[p[:, 3]] - x0, dim=1)
    return ((1 - torch.cosine_similarity(n0, n1, dim=1)) * _weights(t.num_pairs, t.pair_mesh)).sum() / t.N


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
def _fused(verts):
    return verts.is_cuda and verts.dtype == torch.float32


def _check(verts, t, who):
    if not isinstance(t, MeshLossTopology):
        raise RuntimeError(f"{who}: topology must come from mesh_loss_topology")
    if verts.dim() != 2 or verts.size(1) != 3 or verts.size(0) != t.V:
        raise RuntimeError(f"{who}: verts must have shape (V, 3) with the V = {t.V} of the topology")
    if verts.device != t.device:
        raise RuntimeError(f"{who}: verts are on {verts.device}, the topology is on {t.device}")
    if t.N == 0:
        raise RuntimeError(f"{who}: the topology holds no mesh")
    if t.repeated:
        raise ValueError(f"{who}: a face names one vertex twice; the tables do not model its self edge (use the reference's function)")


def _grad_scalar(grad_loss, dev):
    return grad_loss.to(device=dev, dtype=torch.float32).reshape(1).contiguous()


class _EdgeLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, t, target_length):
        v = _C._c(verts, torch.float32)
        lib, dev = _lib.load(), v.device
        nbytes = lib.p3d_mesh_edge_loss_forward_workspace_bytes(t.E)
        ws = _C._workspace(nbytes, dev)
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        _lib.call("p3d_mesh_edge_loss_forward", "mesh_edge_loss forward", dev, v, t.edges, t.edge_mesh, t.num_edges, t.V, t.E, t.N,
                  float(target_length), ws, nbytes, loss)
        ctx.save_for_backward(v)
        ctx.topology, ctx.target_length = t, float(target_length)
        return loss.reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        (v,), t = ctx.saved_tensors, ctx.topology
        dev = v.device
        g = _grad_scalar(grad_loss, dev)
        out = torch.empty_like(v)
        _lib.call("p3d_mesh_edge_loss_backward", "mesh_edge_loss backward", dev, g, v, t.adj_offsets, t.adj, t.vert_mesh, t.num_edges, t.V, t.E,
                  t.N, ctx.target_length, out)
        return out, None, None


class _Laplacian(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, t):
        v = _C._c(verts, torch.float32)
        lib, dev = _lib.load(), v.device
        nbytes = lib.p3d_mesh_laplacian_forward_workspace_bytes(t.V)
        ws = _C._workspace(nbytes, dev)
        q = torch.empty_like(v)
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        _lib.call("p3d_mesh_laplacian_forward", "mesh_laplacian_smoothing forward", dev, v, t.adj_offsets, t.adj, t.vert_mesh, t.num_verts, t.V,
                  t.E, t.N, q, ws, nbytes, loss)
        ctx.save_for_backward(q)
        ctx.topology = t
        return loss.reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        (q,), t = ctx.saved_tensors, ctx.topology
        dev = q.device
        g = _grad_scalar(grad_loss, dev)
        out = torch.empty_like(q)
        _lib.call("p3d_mesh_laplacian_backward", "mesh_laplacian_smoothing backward", dev, g, q, t.adj_offsets, t.adj, t.V, t.E, t.N, out)
        return out, None


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, t):
        v = _C._c(verts, torch.float32)
        lib, dev = _lib.load(), v.device
        nbytes = lib.p3d_mesh_normal_consistency_forward_workspace_bytes(t.P)
        ws = _C._workspace(nbytes, dev)
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        _lib.call("p3d_mesh_normal_consistency_forward", "mesh_normal_consistency forward", dev, v, t.pairs, t.pair_mesh, t.num_pairs, t.V, t.P,
                  t.N, ws, nbytes, loss)
        ctx.save_for_backward(v)
        ctx.topology = t
        return loss.reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        (v,), t = ctx.saved_tensors, ctx.topology
        lib, dev = _lib.load(), v.device
        g = _grad_scalar(grad_loss, dev)
        nbytes = lib.p3d_mesh_normal_consistency_backward_workspace_bytes(t.P)
        rows = _C._workspace(nbytes, dev)
        out = torch.empty_like(v)
        _lib.call("p3d_mesh_normal_consistency_backward", "mesh_normal_consistency backward", dev, g, v, t.pairs, t.pair_mesh, t.num_pairs,
                  t.pair_offsets, t.pair_slots, t.V, t.P, t.N, rows, nbytes, out)
        return out, None


# ---- on packed vertices --------------------------------------------------------------------------------------------------------------
def _empty_value(device):
    return torch.tensor([0.0], dtype=torch.float32, device=device, requires_grad=True)


def edge_loss(verts, topology, target_length=0.0):
    """verts (V, 3), topology: mesh_loss_topology(...).  A 0-dim tensor, differentiable in verts."""
    _check(verts, topology, "edge_loss")
    if _fused(verts):
        return _EdgeLoss.apply(verts, topology, target_length)
    return _torch_edge_loss(verts, topology, target_length)


def laplacian_smoothing(verts, topology, method="uniform", faces_packed=None):
    """verts (V, 3), topology: mesh_loss_topology(...).  "cot" / "cotcurv" need faces_packed and take the torch formulation."""
    if method not in ("uniform", "cot", "cotcurv"):
        raise ValueError("Method should be one of {uniform, cot, cotcurv}")
    _check(verts, topology, "laplacian_smoothing")
    if method == "uniform" and _fused(verts):
        return _Laplacian.apply(verts, topology)
    if method != "uniform" and faces_packed is None:
        raise ValueError("laplacian_smoothing: the methods cot and cotcurv need faces_packed")
    return _torch_laplacian(verts, topology, method, None if faces_packed is None else faces_packed.long())


def normal_consistency(verts, topology):
    """verts (V, 3), topology: mesh_loss_topology(...).  The empty-batch value when the topology has no wing pair."""
    _check(verts, topology, "normal_consistency")
    if topology.P == 0:
        return _empty_value(verts.device)
    if _fused(verts):
        return _NormalConsistency.apply(verts, topology)
    return _torch_normal_consistency(verts, topology)


# ---- on meshes -----------------------------------------------------------------------------------------------------------------------
def _device_of(meshes):
    dev = getattr(meshes, "device", None)
    return dev if dev is not None else meshes.verts_packed().device


def mesh_edge_loss(meshes, target_length: float = 0.0):
    """Edge-length regularisation averaged over the meshes of the batch, every mesh weighted by the inverse of its number of edges.
    Returns tensor([0.]) (requires_grad) for a batch without meshes or of empty meshes only."""
    if len(meshes) == 0:
        return _empty_value(_device_of(meshes))
    t = topology_of(meshes)
    if t.empty:
        return _empty_value(_device_of(meshes))
    return edge_loss(meshes.verts_packed(), t, target_length)


def mesh_laplacian_smoothing(meshes, method: str = "uniform"):
    """Laplacian smoothing objective |L x| averaged per mesh; method uniform (HIP kernels for float32 on the GPU), cot or cotcurv
    (torch).  Returns tensor([0.]) (requires_grad) for a batch without meshes or of empty meshes only."""
    if len(meshes) == 0:
        return _empty_value(_device_of(meshes))
    t = topology_of(meshes)
    if t.empty:
        return _empty_value(_device_of(meshes))
    return laplacian_smoothing(meshes.verts_packed(), t, method, meshes.faces_packed())


def mesh_normal_consistency(meshes):
    """1 - cos of the normals of every two faces that share an edge, averaged per mesh.  Returns tensor([0.]) (requires_grad) for a
    batch without meshes, of empty meshes only, or without two faces on one edge."""
    if len(meshes) == 0:
        return _empty_value(_device_of(meshes))
    t = topology_of(meshes)
    if t.empty:
        return _empty_value(_device_of(meshes))
    return normal_consistency(meshes.verts_packed(), t)
