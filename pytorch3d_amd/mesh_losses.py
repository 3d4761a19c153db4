"""The three mesh regularisers of a fitting loop on the HIP kernels of csrc/mesh_losses.hip and csrc/mesh_laplacian.hip.

    mesh_edge_loss(meshes, target_length=0.0)            pytorch3d/loss/mesh_edge_loss.py
    mesh_laplacian_smoothing(meshes, method="uniform")   pytorch3d/loss/mesh_laplacian_smoothing.py
    mesh_normal_consistency(meshes)                      pytorch3d/loss/mesh_normal_consistency.py
    edge_loss / laplacian_smoothing / normal_consistency (verts, topology, ...)   the same on packed vertices
    mesh_loss_topology(faces_packed, num_verts_per_mesh, num_faces_per_mesh)      the tables, once per topology
    cot_laplacian(verts, faces, eps=1e-12) -> (L, inv_areas)   pytorch3d/ops/laplacian_matrices.py
    cot_tables(faces_packed, V)                          what "cot" / "cotcurv" and cot_laplacian need beside them, on first use

Same names, defaults and return values as the reference; `meshes` is this package's PackedMeshes or the reference's Meshes (anything
with verts_packed / faces_packed / num_verts_per_mesh / num_faces_per_mesh).  The reference redoes the topology's work on every call
(unique edges, a sort and a host round trip for the wing pairs, a sparse V x V matrix) and differentiates through gathers whose
backward adds with float atomics.  Here everything that depends on the faces alone is a set of int32 tables built once
(mesh_loss_topology, kept on the mesh object and inherited by the copies offset_verts / update_verts_packed make), each loss is one
autograd node, and every sum is a gather or a fixed tree: no float atomic, the same bits on every run, stream and process, with
torch.use_deterministic_algorithms on or off (include/p3d_amd.h: the tree and its depth).

float32 vertices on the GPU take the kernels, "cot" and "cotcurv" included (csrc/mesh_laplacian.hip: the face and edge weights in
two launches, the vertex pass and its fixed-tree sum in two, the backward in one).  CPU tensors and float64 take the torch formulation
of the same arithmetic below (differentiated by autograd).  CALLS counts, for the cotangent paths, which of the two ran.
"""
import weakref

import torch

from . import _C, _lib

_TOPOLOGY_KEY = "_p3d_amd_loss_topology"
CALLS = {"cot_fused": 0, "cot_torch": 0, "cot_laplacian_fused": 0, "cot_laplacian_torch": 0}


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
        cot                                                      None, or the CotTables of "cot" / "cotcurv" (built on their first use)
    and on the host N, V, E, P, `empty` (no mesh, no vertex or no face: the reference's isempty()) and `repeated`: some face names one
    vertex twice.  Such a face has a self edge (lo == hi), which the tables would count as an edge of length 0 and a neighbour of
    itself where the reference does something else: the losses refuse such a topology and the shim hands it to the reference."""

    __slots__ = ("N", "V", "E", "P", "empty", "repeated", "device", "edges", "edge_mesh", "num_edges", "adj_offsets", "adj", "vert_mesh", "num_verts",
                 "pairs", "pair_mesh", "num_pairs", "pair_offsets", "pair_slots", "cot")


def _i32(t):
    return t.to(torch.int32).contiguous()


def _corner_edges(faces, V):
    """faces (F, 3) int64.  Corner 3 f + k of a face names the edge OPPOSITE its vertex k: (lo, hi) (F, 3) of every corner, the unique
    keys lo * V + hi ascending and the edge id of every corner (3 F,)."""
    opposite = torch.stack([faces[:, [1, 2]], faces[:, [2, 0]], faces[:, [0, 1]]], 1)  # (F, 3, 2)
    lo, hi = opposite.amin(2), opposite.amax(2)
    key, corner_edge = torch.unique((lo * max(V, 1) + hi).reshape(-1), return_inverse=True)
    return lo, hi, key, corner_edge


def _adjacency_order(edges, V):
    """Both directions of every edge sorted by (vertex, neighbour): (src, dst, order) with slot i of the adjacency = dst[order[i]]."""
    src, dst = torch.cat([edges[:, 0], edges[:, 1]]), torch.cat([edges[:, 1], edges[:, 0]])
    return src, dst, torch.argsort(src * max(V, 1) + dst)


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
    t.device, t.cot = dev, None
    t.N, F = int(nv.numel()), int(faces.size(0))
    t.V = int(nv.sum()) if t.N else 0
    if t.N and int(nf.sum()) != F:
        raise RuntimeError("mesh_loss_topology: num_faces_per_mesh does not add up to the rows of faces_packed")
    V = t.V
    t.empty = t.N == 0 or V == 0 or F == 0
    vert_mesh = torch.repeat_interleave(torch.arange(t.N, device=dev), nv)
    # the unique undirected edges, ascending by lo * V + hi; corner 3 f + k of a face names the edge OPPOSITE its vertex k
    lo, hi, key, corner_edge = _corner_edges(faces, V)
    edges = torch.stack([key // max(V, 1), key % max(V, 1)], 1)
    t.E = int(edges.size(0))
    t.repeated = bool((lo == hi).any())
    edge_mesh = vert_mesh[edges[:, 0]] if t.E else edges.new_zeros((0,))
    # the adjacency: both directions of every edge, sorted by (vertex, neighbour)
    src, dst, order = _adjacency_order(edges, V)
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


# ---- the tables of the cotangent Laplacian ---------------------------------------------------------------------------------------------
class CotTables:
    """What "cot" / "cotcurv", cot_laplacian and nothing else need, from (faces_packed, V) alone.  int32, contiguous, on the faces' device:
        adj_offsets (V + 1,), adj (2 E,)              the adjacency of MeshLossTopology (the same arrays where built from one)
        adj_edge (2 E,)                                the edge id of every slot of adj
        edge_corner_offsets (E + 1,), edge_corners (3 F,)   the corners 3 f + k sorted stably by the edge opposite them: a boundary edge
                                                       has one corner, a non-manifold edge three or more
        inc_offsets (V + 1,), inc_corners (3 F,)      the incidence list of mesh_normals.vert_incidence
    and faces (F, 3) int64 contiguous, V, E, F, `repeated`, and `coo` (2, 2 E) int64: the (row, column) of every slot, the indices
    of cot_laplacian's matrix, made on its first call."""

    __slots__ = ("V", "E", "F", "repeated", "device", "faces", "adj_offsets", "adj", "adj_edge", "edge_corner_offsets", "edge_corners",
                 "inc_offsets", "inc_corners", "coo")


def cot_tables(faces_packed, V, topology=None):
    """The CotTables of faces_packed (F, 3) integer packed vertex ids in [0, V).  Plain torch on the device of the faces; syncs with
    the host -- built once per topology (cot_tables_of).  topology: the MeshLossTopology of the same faces, whose adjacency is shared."""
    from .mesh_normals import vert_incidence

    faces = faces_packed
    if faces.dim() != 2 or faces.size(1) != 3:
        raise RuntimeError("cot_tables: faces_packed must have shape (F, 3)")
    if faces.numel() >= 2 ** 31:
        raise RuntimeError("cot_tables: 3 F must fit an int32")
    V, dev = int(V), faces.device
    faces = faces.to(torch.int64).contiguous()
    c = CotTables()
    c.V, c.F, c.device, c.faces, c.coo = V, int(faces.size(0)), dev, faces, None
    lo, hi, key, corner_edge = _corner_edges(faces, V)
    c.E = int(key.numel())
    c.repeated = bool((lo == hi).any())
    edges = torch.stack([key // max(V, 1), key % max(V, 1)], 1)
    src, dst, order = _adjacency_order(edges, V)
    if topology is not None and topology.E == c.E and topology.V == V:
        c.adj_offsets, c.adj = topology.adj_offsets, topology.adj
    else:
        c.adj_offsets = _i32(torch.searchsorted(src[order].contiguous(), torch.arange(V + 1, device=dev)))
        c.adj = _i32(dst[order])
    edge_id = torch.arange(c.E, device=dev)
    c.adj_edge = _i32(torch.cat([edge_id, edge_id])[order])
    by_edge = torch.sort(corner_edge, stable=True)
    c.edge_corners = _i32(by_edge.indices)
    c.edge_corner_offsets = _i32(torch.searchsorted(by_edge.values.contiguous(), torch.arange(c.E + 1, device=dev)))
    c.inc_offsets, c.inc_corners = vert_incidence(faces, V)
    return c


_COT_CACHE_SIZE = 8
_cot_cache = []  # [weakref of the faces tensor, data_ptr, shape, _version, V, tables], most recent last


def cot_tables_of(faces_packed, V, topology=None):
    """cot_tables(faces_packed, V) kept: in `topology.cot` where a MeshLossTopology is given (a user of "uniform" alone never pays for
    them), and in a cache of the last few faces tensors (the same tensor object with the same address, shape and _version, and V --
    the way graph_conv.topology_of_edges keeps its tables per edge tensor).  Meshes.faces_packed() hands back the same tensor on every
    call: a fitting loop builds once."""
    V = int(V)
    if topology is not None and topology.cot is not None:
        return topology.cot
    _cot_cache[:] = [c for c in _cot_cache if c[0]() is not None]
    key = (faces_packed.data_ptr(), tuple(faces_packed.shape), faces_packed._version, V)
    found = None
    for i, c in enumerate(_cot_cache):
        if c[0]() is faces_packed and tuple(c[1:5]) == key:
            _cot_cache.append(_cot_cache.pop(i))
            found = c[5]
            break
    if found is None:
        found = cot_tables(faces_packed, V, topology)
        _cot_cache[:] = [c for c in _cot_cache if c[0]() is not faces_packed]
        _cot_cache.append([weakref.ref(faces_packed), *key, found])
        del _cot_cache[:-_COT_CACHE_SIZE]
    if topology is not None:
        topology.cot = found
    return found


def clear_cot_tables_cache():
    del _cot_cache[:]


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


def _cot_weights_hip(v, c, eps=1e-12):
    """(face_cot (F, 3), face_area (F,), edge_w (E,)) of float32 GPU vertices v (V, 3) contiguous: two launches."""
    dev = v.device
    face_cot = torch.empty((c.F, 3), dtype=torch.float32, device=dev)
    face_area = torch.empty((c.F,), dtype=torch.float32, device=dev)
    edge_w = torch.empty((c.E,), dtype=torch.float32, device=dev)
    _lib.call("p3di_mesh_cot_weights", "cot_laplacian weights", dev, v, c.faces, c.edge_corner_offsets, c.edge_corners, c.V, c.F, c.E,
              float(eps), face_cot, face_area, edge_w)
    return face_cot, face_area, edge_w


class _CotLaplacian(torch.autograd.Function):
    """mesh_laplacian_smoothing "cot" / "cotcurv": five launches a step (face weights, edge weights, vertex pass, its sum; backward)."""

    @staticmethod
    def forward(ctx, verts, t, c, curvature):
        v = _C._c(verts, torch.float32)
        lib, dev = _lib.load(), v.device
        _, face_area, edge_w = _cot_weights_hip(v, c)
        nbytes = lib.p3di_mesh_cot_laplacian_forward_workspace_bytes(t.V)
        ws = _C._workspace(nbytes, dev)
        d = torch.empty_like(v)
        scale = torch.empty((t.V,), dtype=torch.float32, device=dev)
        rowsum = torch.empty((t.V,), dtype=torch.float32, device=dev)
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        _lib.call("p3di_mesh_cot_laplacian_forward", "mesh_laplacian_smoothing cot forward", dev, v, edge_w, face_area, c.adj_offsets, c.adj,
                  c.adj_edge, c.inc_offsets, c.inc_corners, t.vert_mesh, t.num_verts, t.V, c.E, c.F, t.N, int(curvature), d, scale, rowsum,
                  ws, nbytes, loss)
        ctx.save_for_backward(d, scale, rowsum, edge_w)
        ctx.tables, ctx.N, ctx.curvature = c, t.N, int(curvature)
        return loss.reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        (d, scale, rowsum, edge_w), c = ctx.saved_tensors, ctx.tables
        dev = d.device
        g = _grad_scalar(grad_loss, dev)
        out = torch.empty_like(d)
        _lib.call("p3di_mesh_cot_laplacian_backward", "mesh_laplacian_smoothing cot backward", dev, g, d, scale, rowsum, edge_w, c.adj_offsets,
                  c.adj, c.adj_edge, c.V, c.E, ctx.N, ctx.curvature, out)
        return out, None, None, None


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
    """verts (V, 3), topology: mesh_loss_topology(...).  "cot" / "cotcurv" need faces_packed -- the faces the topology was built from;
    float32 vertices on the GPU take one autograd node over csrc/mesh_laplacian.hip (the tables of cot_tables_of, built on the first
    call and kept in topology.cot), CPU tensors and float64 the torch formulation."""
    if method not in ("uniform", "cot", "cotcurv"):
        raise ValueError("Method should be one of {uniform, cot, cotcurv}")
    _check(verts, topology, "laplacian_smoothing")
    if method == "uniform" and _fused(verts):
        return _Laplacian.apply(verts, topology)
    if method != "uniform" and faces_packed is None:
        raise ValueError("laplacian_smoothing: the methods cot and cotcurv need faces_packed")
    if method != "uniform" and _fused(verts):
        if faces_packed.device != verts.device:
            raise RuntimeError(f"laplacian_smoothing: verts are on {verts.device}, faces_packed on {faces_packed.device}")
        c = cot_tables_of(faces_packed, topology.V, topology)
        if c.E != topology.E or c.F != int(faces_packed.shape[0]):
            raise RuntimeError("laplacian_smoothing: faces_packed are not the faces of the topology")
        CALLS["cot_fused"] += 1
        return _CotLaplacian.apply(verts, topology, c, method == "cotcurv")
    if method != "uniform":
        CALLS["cot_torch"] += 1
    return _torch_laplacian(verts, topology, method, None if faces_packed is None else faces_packed.long())


def cot_laplacian_torch(verts, faces, eps=1e-12):
    """The reference's chain restated (laplacian_matrices.py:91-141): an UNCOALESCED sparse (V, V) L and inv_areas (V, 1)."""
    V, F = verts.shape[0], faces.shape[0]
    face_verts = verts[faces]
    v0, v1, v2 = face_verts[:, 0], face_verts[:, 1], face_verts[:, 2]
    A, B, C = (v1 - v2).norm(dim=1), (v0 - v2).norm(dim=1), (v0 - v1).norm(dim=1)
    s = 0.5 * (A + B + C)
    area = (s * (s - A) * (s - B) * (s - C)).clamp(min=eps).sqrt()
    A2, B2, C2 = A * A, B * B, C * C
    cot = torch.stack([(B2 + C2 - A2) / area, (A2 + C2 - B2) / area, (A2 + B2 - C2) / area], dim=1) / 4.0
    idx = torch.stack([faces[:, [1, 2, 0]], faces[:, [2, 0, 1]]], dim=0).view(2, F * 3)
    L = torch.sparse_coo_tensor(idx, cot.view(-1), (V, V), dtype=torch.float32)
    L = L + L.t()
    inv_areas = torch.zeros(V, dtype=torch.float32, device=verts.device)
    inv_areas.scatter_add_(0, faces.view(-1), torch.stack([area] * 3, dim=1).view(-1))
    pos = inv_areas > 0
    inv_areas[pos] = torch.reciprocal(inv_areas[pos])
    return L, inv_areas.view(-1, 1)


def cot_laplacian_kernel_path(verts, faces):
    """Whether cot_laplacian(verts, faces) runs the kernels, the tables apart (a face that names one vertex twice: the chain)."""
    return (torch.is_tensor(verts) and torch.is_tensor(faces) and verts.is_cuda and verts.dtype == torch.float32 and verts.dim() == 2
            and verts.size(1) == 3 and faces.dim() == 2 and faces.size(1) == 3 and faces.device == verts.device
            and not faces.dtype.is_floating_point and verts.size(0) > 0 and faces.size(0) > 0
            and not (torch.is_grad_enabled() and verts.requires_grad))


def cot_laplacian(verts, faces, eps=1e-12):
    """pytorch3d.ops.cot_laplacian: (L, inv_areas) -- L a sparse float32 (V, V) with L[i, j] = the sum, over the faces that hold the
    edge (i, j), of cot(the angle opposite the edge) / 4, and inv_areas (V, 1) the reciprocal of the summed areas of the faces round
    each vertex (a sum that is not positive stays as it is).

    float32 GPU input whose result needs no gradient -- not (torch.is_grad_enabled() and verts.requires_grad) -- takes the face and
    edge kernels of csrc/mesh_laplacian.hip and the area gather: three launches and one gather of the 2 E values.  That L is COALESCED,
    with the 2 E directed entries ascending by (row, column); its indices are built once per faces tensor (cot_tables_of).  The
    reference's L is uncoalesced, one entry per corner and direction: compare `to_dense()` or `coalesce()`, not the raw values.
    Everything else (CPU tensors, inputs that want a gradient, a face that names one vertex twice) takes the reference's chain
    restated, which gives the reference's layout."""
    fused = cot_laplacian_kernel_path(verts, faces)
    c = cot_tables_of(faces, verts.shape[0]) if fused else None
    if c is None or c.repeated:
        CALLS["cot_laplacian_torch"] += 1
        return cot_laplacian_torch(verts, faces, eps)
    CALLS["cot_laplacian_fused"] += 1
    v = _C._c(verts.detach(), torch.float32)
    dev = v.device
    _, face_area, edge_w = _cot_weights_hip(v, c, eps)
    inv_areas = torch.empty((c.V,), dtype=torch.float32, device=dev)
    _lib.call("p3di_mesh_cot_inv_areas", "cot_laplacian inv_areas", dev, face_area, c.inc_offsets, c.inc_corners, c.V, c.F, inv_areas)
    if c.coo is None:
        off = c.adj_offsets.long()
        c.coo = torch.stack([torch.repeat_interleave(torch.arange(c.V, device=dev), off[1:] - off[:-1]), c.adj.long()], 0)
    L = torch.sparse_coo_tensor(c.coo, edge_w[c.adj_edge.long()], (c.V, c.V), dtype=torch.float32, is_coalesced=True)
    return L, inv_areas.view(-1, 1)


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
    """Laplacian smoothing objective |L x| averaged per mesh; method uniform, cot or cotcurv: HIP kernels for float32 on the GPU, the
    torch formulation for CPU tensors and float64.  Returns tensor([0.]) (requires_grad) for a batch without meshes or of empty meshes only."""
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
