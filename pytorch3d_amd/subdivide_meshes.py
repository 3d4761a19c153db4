"""SubdivideMeshes and the mesh edges under it, on csrc/mesh_edges.hip and csrc/subdivide.hip.

    mesh_edges(faces_packed, num_verts_per_mesh, num_faces_per_mesh) -> MeshEdges      Meshes._compute_edges_packed, kept per faces tensor
    subdivide_packed(verts, faces, num_verts_per_mesh, num_faces_per_mesh, feats=None, edges=None) -> SubdividedPacked
    SubdivideMeshes(meshes=None)                                                        pytorch3d/ops/subdivide_meshes.py, the module

The contract (structures/meshes.py:1036-1135 and ops/subdivide_meshes.py restated; checked against the reference's CPU results through
tests/golden/subdivide_ref.npz).
  edges       corner 3 f + k of face f names the edge OPPOSITE its vertex k: (v1, v2), (v2, v0), (v0, v1), as (lo, hi).  `edges` (E, 2)
              holds the unique (lo, hi) ascending by lo V + hi, `face_edges` (F, 3) the edge id of every corner, `edge_mesh` (E,) the
              mesh of lo, `first_edge` (N + 1,) the exclusive scan of `num_edges_per_mesh`.  A face that names a vertex twice has a
              self edge (v, v), which is kept.  An id outside [0, V) raises ValueError with the least and the greatest id.
  row_offsets (2 V + 1,): the edges with lo == v are the ids [row_offsets[v], row_offsets[v + 1]); the edges with hi == v are
              hi_edges[row_offsets[V + v] - E : row_offsets[V + v + 1] - E], ascending -- what the backward gathers by.
  subdivision mesh n gets V_n + E_n vertices -- its old ones, then the midpoints (x[lo] + x[hi]) / 2 of its edges in edge order, one
              rounding -- and 4 F_n faces: the block f0 = (v0, e2, e1) of its faces, then f1 = (v1, e0, e2), f2 = (v2, e1, e0),
              f3 = (e0, e1, e2), an old vertex as v - first_vert[n], an edge as V_n + e - first_edge[n].  Features (V, D) go the
              vertices' way.  SubdivideMeshes(meshes) precomputes from meshes[0]; its forward takes padded (N, V, 3) vertices and
              (N, V, D) or (N V, D) features of one topology.
  backward    grad_x[v] = g[row(v)] + 0.5 (((+0 + g[row(e_0)]) + g[row(e_1)]) + ...), e_i the vertex's edges ascending: its hi list,
              then its lo run; a self edge is in both.  A gather: the same bits on every run.

float32 vertices (and features) on a GPU with int64 faces on it, and sizes within the kernels' int32 indices (6 F and 2 V + 1), take
the kernels: `kernel_path`.  One host read per edge build (E, the edges per mesh, the flag of a bad id, the long rows); the per-mesh
vertex and face counts are best given as host sequences -- device tensors cost a read each.  One autograd node covers the forward.
Everything else -- CPU tensors, float64, oversize or empty inputs -- takes the torch formulation of the same contract in this file,
with the same bits forward.
"""
import collections
import weakref

import torch

from . import _C, _lib, structures

CALLS = {"fused": 0, "formulation": 0, "edges_fused": 0, "edges_formulation": 0}  # what ran (the shim's PATCH_CALLS and the tests read it)


class MeshEdges:
    """The tables of the module's docstring, int32, contiguous, on the faces' device; N, V, F, E, the per-mesh counts on the host
    (`num_verts`, `num_faces`, `num_edges`: lists), `vert_first` / `face_first` / `first_edge` (N + 1,) on the device, `faces` (F, 3)
    int64 contiguous and `long_rows`: how many of the 2 V sorted rows were longer than MESH_EDGES_ROW_REGISTERS and MESH_EDGES_ROW_LDS."""

    __slots__ = ("N", "V", "F", "E", "device", "faces", "edges", "face_edges", "edge_mesh", "first_edge", "vert_first", "face_first",
                 "row_offsets", "hi_edges", "num_verts", "num_faces", "num_edges", "long_rows", "_wide")

    def _int64(self, name):
        if name not in self._wide:
            self._wide[name] = getattr(self, name).to(torch.int64)
        return self._wide[name]

    def edges_packed(self):
        return self._int64("edges")

    def faces_packed_to_edges_packed(self):
        return self._int64("face_edges")

    def edges_packed_to_mesh_idx(self):
        return self._int64("edge_mesh")

    def num_edges_per_mesh(self):
        if "num_edges" not in self._wide:
            self._wide["num_edges"] = torch.tensor(self.num_edges, dtype=torch.int32, device=self.device)  # the reference's dtype
        return self._wide["num_edges"]


def _host_counts(counts):
    return [int(c) for c in (counts.tolist() if torch.is_tensor(counts) else counts)]


def _firsts(counts, device):
    first = [0]
    for c in counts:
        first.append(first[-1] + c)
    return torch.tensor(first, dtype=torch.int32, device=device)


def _bad_ids(faces, V):
    lo, hi = torch.stack([faces.min(), faces.max()]).tolist()
    return ValueError("faces_packed holds vertex indices outside [0, %d): min %d, max %d" % (V, lo, hi))


def edges_kernel_path(faces_packed, V):
    """Whether mesh_edges of these faces over V vertices runs csrc/mesh_edges.hip (else: the torch formulation)."""
    return (torch.is_tensor(faces_packed) and faces_packed.is_cuda and faces_packed.dtype == torch.int64 and faces_packed.dim() == 2
            and faces_packed.shape[1] == 3 and _C.mesh_edges_fits(int(V), faces_packed.shape[0]))


def mesh_edges_build(faces_packed, num_verts_per_mesh, num_faces_per_mesh):
    """mesh_edges without the cache."""
    faces = faces_packed
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("faces_packed must have shape (F, 3), got %s" % (tuple(faces.shape),))
    t = MeshEdges()
    t.num_verts, t.num_faces, t._wide = _host_counts(num_verts_per_mesh), _host_counts(num_faces_per_mesh), {}
    t.N, t.V, t.F, t.device = len(t.num_verts), sum(t.num_verts), faces.shape[0], faces.device
    if len(t.num_faces) != t.N or sum(t.num_faces) != t.F:
        raise ValueError("num_faces_per_mesh must have one entry per mesh and add up to the rows of faces_packed")
    if 3 * t.F > 2 ** 31 - 1 or t.V + 3 * t.F > 2 ** 31 - 1:
        raise ValueError("mesh_edges: 3 F and V + E must fit an int32")
    t.vert_first, t.face_first = _firsts(t.num_verts, t.device), _firsts(t.num_faces, t.device)
    V, F = t.V, t.F
    if edges_kernel_path(faces, V) and t.N > 0:
        CALLS["edges_fused"] += 1
        t.faces = faces.contiguous()
        edges, t.face_edges, edge_mesh, t.first_edge, t.row_offsets, hi_edges, record = _C.mesh_edges_build(t.faces, t.vert_first, V)
        record = record.tolist()  # the one host read of the build
        if record[1]:
            raise _bad_ids(faces, V)
        t.E, t.long_rows, t.num_edges = record[0], (record[2], record[3]), record[4:]
        t.edges, t.edge_mesh, t.hi_edges = edges[:t.E], edge_mesh[:t.E], hi_edges[:t.E]
        return t
    CALLS["edges_formulation"] += 1
    faces = t.faces = faces.to(torch.int64).contiguous()
    if F and (int(faces.min()) < 0 or int(faces.max()) >= V):
        raise _bad_ids(faces, V)
    i32 = lambda x: x.to(torch.int32).contiguous()  # noqa: E731
    opposite = torch.stack([faces[:, [1, 2]], faces[:, [2, 0]], faces[:, [0, 1]]], 1)  # (F, 3, 2)
    lo, hi = opposite.amin(2).reshape(-1), opposite.amax(2).reshape(-1)
    key, corner_edge = torch.unique(lo * max(V, 1) + hi, return_inverse=True)
    edges = torch.stack([key // max(V, 1), key % max(V, 1)], 1)
    t.E = edges.shape[0]
    ids = torch.arange(V + 1, device=t.device)
    lo_offsets = torch.searchsorted(edges[:, 0].contiguous(), ids)
    by_hi = torch.sort(edges[:, 1], stable=True)
    t.row_offsets = i32(torch.cat([lo_offsets, torch.searchsorted(by_hi.values.contiguous(), ids)[1:] + t.E]))
    t.edges, t.face_edges, t.hi_edges = i32(edges), i32(corner_edge.reshape(F, 3)), i32(by_hi.indices)
    t.edge_mesh = i32(torch.searchsorted(t.vert_first[1:].to(torch.int64).contiguous(), edges[:, 0].contiguous(), right=True))
    t.first_edge = i32(lo_offsets[t.vert_first.to(torch.int64)])
    t.num_edges = (t.first_edge[1:] - t.first_edge[:-1]).tolist()
    rows = torch.bincount(torch.cat([lo, V + hi]), minlength=1)
    t.long_rows = (int((rows > _lib.MESH_EDGES_ROW_REGISTERS).sum()), int((rows > _lib.MESH_EDGES_ROW_LDS).sum()))
    return t


_CACHE_SIZE = 8
_cache = []  # [weakref of the faces tensor, data_ptr, shape, _version, counts, tables], most recent last


def mesh_edges(faces_packed, num_verts_per_mesh, num_faces_per_mesh):
    """The MeshEdges of faces_packed (F, 3) packed vertex ids over meshes of num_verts_per_mesh / num_faces_per_mesh (N,), kept with
    the faces tensor the way mesh_losses.cot_tables_of keeps its tables: the same tensor object with the same address, shape and
    _version (and the same counts).  Meshes.faces_packed() hands back the same tensor on every call: a loop builds once."""
    nv, nf = _host_counts(num_verts_per_mesh), _host_counts(num_faces_per_mesh)
    _cache[:] = [c for c in _cache if c[0]() is not None]
    key = (faces_packed.data_ptr(), tuple(faces_packed.shape), faces_packed._version, (tuple(nv), tuple(nf)))
    for i, c in enumerate(_cache):
        if c[0]() is faces_packed and tuple(c[1:5]) == key:
            _cache.append(_cache.pop(i))
            return c[5]
    found = mesh_edges_build(faces_packed, nv, nf)
    _cache[:] = [c for c in _cache if c[0]() is not faces_packed]
    _cache.append([weakref.ref(faces_packed), *key, found])
    del _cache[:-_CACHE_SIZE]
    return found


def clear_mesh_edges_cache():
    del _cache[:]


# ---- the subdivision ----------------------------------------------------------------------------------------------------------------
def kernel_path(verts, feats=None, edges=None):
    """Whether the subdivision of verts (V, 3) / (N, V, 3) and feats runs csrc/subdivide.hip (else: the torch formulation)."""
    if not (torch.is_tensor(verts) and verts.is_cuda and verts.dtype == torch.float32 and verts.dim() in (2, 3) and verts.numel() > 0):
        return False
    if feats is not None and not (torch.is_tensor(feats) and feats.dtype == torch.float32 and feats.device == verts.device):
        return False
    if verts.dim() == 3 and verts.shape[0] > 65535:
        return False
    return edges is None or (edges.device == verts.device and edges.V + edges.E < 2 ** 31 - 1)


def _row_sources(t):
    """(old, edge): for every output row its source row of x (-1: a midpoint) and its edge id (-1: an old vertex), by arithmetic on the
    counts -- the reference's _create_verts_index without the argsort."""
    dev, i64 = t.device, torch.int64
    nv, ne = torch.tensor(t.num_verts, dtype=i64, device=dev), torch.tensor(t.num_edges, dtype=i64, device=dev)
    mesh = torch.repeat_interleave(torch.arange(t.N, device=dev), nv + ne)
    vf, ef = t.vert_first.to(i64), t.first_edge.to(i64)
    local = torch.arange(t.V + t.E, device=dev) - (vf + ef)[mesh]
    is_old = local < nv[mesh]
    return torch.where(is_old, vf[mesh] + local, -1), torch.where(is_old, -1, ef[mesh] + local - nv[mesh])


def _subdivide_rows_torch(x, t):
    """x (V, D) or (B, V, D) -> (V + E, D) / (B, V + E, D) in torch: the midpoints by one addition and one halving."""
    edges = t.edges.to(torch.int64)
    if t.N == 1:
        return torch.cat([x, (x[..., edges[:, 0], :] + x[..., edges[:, 1], :]) * 0.5], -2)
    old, edge = _row_sources(t)
    both = torch.cat([x, (x[edges[:, 0]] + x[edges[:, 1]]) * 0.5], 0)
    return both[torch.where(old >= 0, old, t.V + edge)]


def subdivided_faces(t, local=True, packed=True):
    """(faces_local, faces_packed) of the subdivided meshes, (4 F, 3) int64 each (None where not asked for)."""
    if t.F and edges_kernel_path(t.faces, t.V) and t.N > 0:
        return _C.subdivide_faces(t.faces, t.face_edges, t.vert_first, t.face_first, t.first_edge, local, packed)
    i64 = torch.int64
    nf = torch.tensor(t.num_faces, dtype=i64, device=t.device)
    mesh = torch.repeat_interleave(torch.arange(t.N, device=t.device), 4 * nf)
    ff, vf, ef = t.face_first.to(i64)[mesh], t.vert_first.to(i64)[mesh], t.first_edge.to(i64)[mesh]
    pos = torch.arange(4 * t.F, device=t.device) - 4 * ff
    k, f = pos // nf[mesh].clamp(min=1), ff + pos % nf[mesh].clamp(min=1)
    v = t.faces[f] - vf[:, None]
    e = t.face_edges.to(i64)[f] + (t.vert_first.to(i64)[mesh + 1] - vf - ef)[:, None]
    kk = k.clamp(max=2)[:, None]
    corner = torch.cat([v.gather(1, kk), e.gather(1, (kk + 2) % 3), e.gather(1, (kk + 1) % 3)], 1)
    faces_local = torch.where((k == 3)[:, None], e, corner)
    return (faces_local if local else None), (faces_local + (vf + ef)[:, None] if packed else None)


class _Subdivide(torch.autograd.Function):
    """verts (and feats) -> their subdivided tensors: one forward launch, one backward launch."""

    @staticmethod
    def forward(ctx, t, verts, feats):
        ctx.tables = t
        outs = _C.subdivide_forward([verts] + ([] if feats is None else [feats]), t.edges, t.vert_first, t.first_edge, t.V, t.E)
        return outs[0], (None if feats is None else outs[1])

    @staticmethod
    def backward(ctx, grad_verts, grad_feats):
        t = ctx.tables
        gs = [g.contiguous() if g is not None and need else None for g, need in zip((grad_verts, grad_feats), ctx.needs_input_grad[1:])]
        if gs[0] is None and gs[1] is None:
            return None, None, None
        outs = _C.subdivide_backward(gs, t.row_offsets, t.hi_edges, t.vert_first, t.first_edge, t.V, t.E)
        return None, outs[0], outs[1]


def subdivide_rows(verts, feats, t):
    """(new_verts, new_feats or None) of verts (V, 3) / (B, V, 3) and feats (V, D) / (B, V, D) over the tables t (for the batched form:
    the tables of ONE mesh)."""
    if kernel_path(verts, feats, t) and t.N > 0:
        CALLS["fused"] += 1
        return _Subdivide.apply(t, verts, feats)
    CALLS["formulation"] += 1
    return _subdivide_rows_torch(verts, t), (None if feats is None else _subdivide_rows_torch(feats, t))


SubdividedPacked = collections.namedtuple("SubdividedPacked", "verts faces faces_packed feats num_verts_per_mesh num_faces_per_mesh")


def subdivide_packed(verts, faces, num_verts_per_mesh, num_faces_per_mesh, feats=None, edges=None):
    """verts (V, 3), faces (F, 3) packed ids, feats (V, D) or None, edges: the MeshEdges of the faces (None: mesh_edges(...)) ->
    SubdividedPacked(verts (V + E, 3), faces (4 F, 3) with per-mesh ids, faces_packed (4 F, 3), feats (V + E, D) or None, and the
    per-mesh vertex and face counts of the result as host lists)."""
    t = edges if edges is not None else mesh_edges(faces, num_verts_per_mesh, num_faces_per_mesh)
    if verts.shape[0] != t.V or (feats is not None and (feats.dim() != 2 or feats.shape[0] != t.V)):
        raise ValueError("verts and feats must have one row per vertex of the meshes (%d)" % t.V)
    with torch.no_grad():
        faces_local, faces_packed = subdivided_faces(t)
    new_verts, new_feats = subdivide_rows(verts, feats, t)
    return SubdividedPacked(new_verts, faces_local, faces_packed, new_feats, [v + e for v, e in zip(t.num_verts, t.num_edges)],
                            [4 * f for f in t.num_faces])


# ---- the module ---------------------------------------------------------------------------------------------------------------------
def _counts_of(meshes):
    return [v.shape[0] for v in meshes.verts_list()], [f.shape[0] for f in meshes.faces_list()]


def _edges_of(meshes):
    return mesh_edges(meshes.faces_packed(), *_counts_of(meshes))


def _like(meshes, verts_list, faces_list):
    if isinstance(meshes, structures.PackedMeshes):
        return structures.PackedMeshes(verts_list, faces_list)
    return type(meshes)(verts=verts_list, faces=faces_list)


def subdivide_faces(meshes):
    """SubdivideMeshes.subdivide_faces: (4 F, 3) int64, the blocks f0 f1 f2 f3 over ALL faces with a vertex as its packed id and an edge
    as V + its id -- the subdivision of the batch taken as one mesh."""
    t = _edges_of(meshes)
    one = MeshEdges()
    for name in MeshEdges.__slots__:
        setattr(one, name, getattr(t, name))
    one.N, one.num_verts, one.num_faces, one.num_edges = 1, [t.V], [t.F], [t.E]
    one.vert_first, one.face_first, one.first_edge = (_firsts(c, t.device) for c in (one.num_verts, one.num_faces, one.num_edges))
    with torch.no_grad():
        return subdivided_faces(one, packed=False)[0]


def subdivide_heterogeneous(meshes, feats=None):
    """SubdivideMeshes.subdivide_heterogenerous: new meshes of the kind given, and the packed new feats where feats is given."""
    out = subdivide_packed(meshes.verts_packed(), meshes.faces_packed(), *_counts_of(meshes), feats=feats, edges=_edges_of(meshes))
    new_meshes = _like(meshes, list(out.verts.split(out.num_verts_per_mesh, 0)), list(out.faces.split(out.num_faces_per_mesh, 0)))
    return new_meshes if feats is None else (new_meshes, out.feats)


def subdivide_homogeneous(module, meshes, feats=None):
    """SubdivideMeshes.subdivide_homogeneous over the tables of meshes[0], kept on the module."""
    verts = meshes.verts_padded() if hasattr(meshes, "verts_padded") else torch.stack(list(meshes.verts_list()), 0)
    N = verts.shape[0]
    t = module.__dict__.get("_p3d_amd_edges")
    if t is None or t.device != verts.device or t.V != verts.shape[1]:
        t = mesh_edges_build(meshes.faces_list()[0], [verts.shape[1]], [meshes.faces_list()[0].shape[0]])
        module.__dict__["_p3d_amd_edges"] = t
    new_faces = module._subdivided_faces.view(1, -1, 3).expand(N, -1, -1)
    if feats is not None:
        if feats.dim() == 2:
            feats = feats.view(verts.size(0), verts.size(1), feats.size(1))
        if feats.dim() != 3:
            raise ValueError("features need to be of shape (N, V, D) or (N*V, D)")
    new_verts, new_feats = subdivide_rows(verts, feats, t)
    if isinstance(meshes, structures.PackedMeshes):
        new_meshes = structures.PackedMeshes(list(new_verts.unbind(0)), list(new_faces.unbind(0)))
    else:
        new_meshes = type(meshes)(verts=new_verts, faces=new_faces)
    return new_meshes if feats is None else (new_meshes, new_feats)


def _first_mesh(meshes):
    return meshes.slice(0, 1) if isinstance(meshes, structures.PackedMeshes) else meshes[0]


class SubdivideMeshes(torch.nn.Module):
    """pytorch3d.ops.SubdivideMeshes: every edge gets a vertex at its midpoint and every face becomes four, orientation kept.  With
    `meshes` the new faces of meshes[0] are precomputed and forward takes batches of that one topology.  Takes PackedMeshes or the
    reference's Meshes and returns the same kind."""

    def __init__(self, meshes=None) -> None:
        super().__init__()
        self.precomputed = False
        self._N = -1
        if meshes is not None:
            with torch.no_grad():
                subdivided_faces = self.subdivide_faces(_first_mesh(meshes))
                if subdivided_faces.shape[1] != 3:
                    raise ValueError("faces can only have three vertices")
                self.register_buffer("_subdivided_faces", subdivided_faces)
                self.precomputed = True

    def subdivide_faces(self, meshes):
        return subdivide_faces(meshes)

    def forward(self, meshes, feats=None):
        self._N = len(meshes)
        if self.precomputed:
            return self.subdivide_homogeneous(meshes, feats)
        return self.subdivide_heterogenerous(meshes, feats)

    def subdivide_homogeneous(self, meshes, feats=None):
        return subdivide_homogeneous(self, meshes, feats)

    def subdivide_heterogenerous(self, meshes, feats=None):
        return subdivide_heterogeneous(meshes, feats)
