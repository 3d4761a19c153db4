"""Distances between point clouds and meshes on the HIP kernels of csrc/point_mesh.hip (pytorch3d/loss/point_mesh_distance.py).

    point_face_distance(points, points_first_idx, tris, tris_first_idx, max_points, min_triangle_area=5e-3) -> dists (P,)
    face_point_distance(points, points_first_idx, tris, tris_first_idx, max_tris, min_triangle_area=5e-3)   -> dists (T,)
    point_edge_distance(points, points_first_idx, segms, segms_first_idx, max_points)                       -> dists (P,)
    edge_point_distance(points, points_first_idx, segms, segms_first_idx, max_segms)                        -> dists (S,)
    point_mesh_face_distance(meshes, pcls, min_triangle_area=5e-3), point_mesh_edge_distance(meshes, pcls)  -> loss

The reference's names, argument lists and values.  Each query object (a point, or a face / an edge) gets the smallest squared
distance to a target of ITS batch element -- brute force, every query against every target -- by the pair functions of
csrc/point_mesh_geom.h (the formulas of the reference's geometry_utils.h).  Among equal distances the LARGEST target index wins, an
element without targets gives FLT_MAX (and no gradient).

float32 GPU tensors take the kernels; the two losses are then ONE autograd node each: the face-vertex gather (segments from the edge
table kept with the topology, pytorch3d_amd.mesh_losses.topology_of), the two fused forward launches with their fixed-tree sums and,
in the backward, the two backward kernels and the face-gradient scatter to the vertices.  Nothing waits for the device: the grid's
maximum counts are the host integers the structures already hold (pcls._P, meshes._F, and for edges the topology's edge count capped
by 3 _F).  The backward's target side uses float atomics or, under torch.use_deterministic_algorithms(True), the ordered sum of
csrc/ordered_sum.h.

CPU tensors, float64 and everything else the kernels do not take go to the torch formulation below: the same contract and tie rule,
the (rows, targets) distances in bounded chunks, an explicit backward with the kernels' formulas.
"""
import torch

from . import _C, _lib

DEFAULT_MIN_TRIANGLE_AREA = 5e-3
EPS = 1e-8
FLT_MAX = 3.4028234663852886e38
CHUNK_ELEMENTS = 1 << 20  # the torch formulation keeps at most this many (row, target) pairs alive at a time
SPLIT = 0  # waves per workgroup in the fused losses' forwards: 0 = the library chooses (profiles/point_mesh_bench.py forces 1 for one leg)

_DIRECTIONS = ("point_face", "face_point", "point_edge", "edge_point")


def kernel_path(points, prims):
    """Whether these tensors run csrc/point_mesh.hip (else: the torch formulation)."""
    return (torch.is_tensor(points) and torch.is_tensor(prims) and points.is_cuda and prims.is_cuda and points.device == prims.device
            and points.dtype == torch.float32 and prims.dtype == torch.float32)


# ---- the torch formulation -------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _seg_dist(p, v0, v1):
    d = v1 - v0
    l2 = _dot(d, d)
    pv1 = p - v1
    tt = (_dot(d, p - v0) / l2).clamp(0.0, 1.0)
    diff = p - (v0 + tt[..., None] * d)
    return torch.where(l2 <= EPS, _dot(pv1, pv1), _dot(diff, diff))


def _tri_inside(p, v0, v1, v2, min_triangle_area):
    """(inside, t, unit normal, raw normal, |raw|) of point_mesh_geom.h: tri_inside."""
    e01, e02 = v1 - v0, v2 - v0
    raw = _cross(e02, e01)
    norm = torch.sqrt(_dot(raw, raw))
    n = raw / (norm + EPS)[..., None]
    c = _cross(e01, e02)
    area = torch.hypot(c[..., 0], torch.hypot(c[..., 1], c[..., 2])).double() / 2.0
    t = _dot(v0 - p, n)
    p2 = (p + t[..., None] * n) - v0
    d00, d01, d11, d20, d21 = _dot(e01, e01), _dot(e01, e02), _dot(e02, e02), _dot(p2, e01), _dot(p2, e02)
    denom = d00 * d11 - d01 * d01 + EPS
    w1 = (d11 * d20 - d01 * d21) / denom
    w2 = (d00 * d21 - d01 * d20) / denom
    w0 = 1.0 - w1 - w2
    inside = ~(area < min_triangle_area) & (norm > EPS)
    for w in (w0, w1, w2):
        inside = inside & (w >= 0.0) & (w <= 1.0)
    return inside, t, n, raw, norm


def _tri_dist(p, v0, v1, v2, min_triangle_area):
    inside, t, _, _, _ = _tri_inside(p, v0, v1, v2, min_triangle_area)
    e01, e02, e12 = _seg_dist(p, v0, v1), _seg_dist(p, v0, v2), _seg_dist(p, v1, v2)
    dist = torch.where(e01 > e02, e02, e01)
    dist = torch.where(dist > e12, e12, dist)
    return torch.where(inside, t * t, dist)


def _pair_dist(points, prims, min_triangle_area):
    """points (..., 3) against prims (..., 2 or 3, 3), broadcast."""
    if prims.shape[-2] == 2:
        return _seg_dist(points, prims[..., 0, :], prims[..., 1, :])
    return _tri_dist(points, prims[..., 0, :], prims[..., 1, :], prims[..., 2, :], min_triangle_area)


def _seg_backward(p, v0, v1, g):
    """(grad_p, grad_v0, grad_v1) of g * |p - segment|^2 by the four cases of point_mesh_geom.h: seg_backward."""
    d, pv0 = v1 - v0, p - v0
    t_bot, t_top = _dot(d, d), _dot(d, pv0)
    tt = t_top / t_bot
    g2 = (g * 2.0)[..., None]
    zero = torch.zeros_like(p)
    end0 = g2 * pv0
    end1 = g2 * (p - v1)
    tt3 = tt[..., None]
    base = g2 * (p - (v0 + tt3 * d))
    bd = _dot(base, d)[..., None]
    tb = t_bot[..., None]
    in_p = base - (bd * d) / tb
    in_v0 = ((-1.0 + tt3) * base) - bd * (((-1.0 * d) - pv0 + (2.0 * tt3) * d) / tb)
    in_v1 = ((-bd) * ((pv0 - (2.0 * tt3) * d) / tb)) - tt3 * base
    same, below, above = (t_bot < EPS)[..., None], (tt < 0.0)[..., None], (tt > 1.0)[..., None]
    gp = torch.where(same, end0, torch.where(below, end0, torch.where(above, end1, in_p)))
    gv0 = torch.where(same, -0.5 * end0, torch.where(below, -1.0 * end0, torch.where(above, zero, in_v0)))
    gv1 = torch.where(same, -0.5 * end0, torch.where(below, zero, torch.where(above, -1.0 * end1, in_v1)))
    return gp, gv0, gv1


def _tri_backward(p, v0, v1, v2, g, min_triangle_area):
    """(grad_p, grad_v0, grad_v1, grad_v2) by point_mesh_geom.h: tri_backward."""
    inside, t, n, raw, norm = _tri_inside(p, v0, v1, v2, min_triangle_area)
    e01, e02 = v1 - v0, v2 - v0
    gt = (g * t)[..., None]
    gn = (2.0 * gt) * ((v0 - p) + t[..., None] * n)
    an = (norm + EPS)[..., None]
    o = raw / an
    graw = (gn - o * _dot(gn, o)[..., None]) / an
    ga, gb = _cross(e01, graw), _cross(graw, e02)  # through cross(a, b): grad_a = b x g, grad_b = g x a, with a = e02, b = e01
    in_p, in_v0, in_v1, in_v2 = (-2.0 * gt) * n, (2.0 * gt) * n - (ga + gb), gb, ga
    d01, d02, d12 = _seg_dist(p, v0, v1), _seg_dist(p, v0, v2), _seg_dist(p, v1, v2)
    first = (d01 <= d02) & (d01 <= d12)
    second = ~first & (d02 <= d01) & (d02 <= d12)
    third = ~first & ~second & (d12 <= d01) & (d12 <= d02)
    zero = torch.zeros_like(p)
    a_p, a_0, a_1 = _seg_backward(p, v0, v1, g)
    b_p, b_0, b_2 = _seg_backward(p, v0, v2, g)
    c_p, c_1, c_2 = _seg_backward(p, v1, v2, g)
    out = []
    for ins, a, b, c in ((in_p, a_p, b_p, c_p), (in_v0, a_0, b_0, zero), (in_v1, a_1, zero, c_1), (in_v2, zero, b_2, c_2)):
        edge = torch.where(first[..., None], a, torch.where(second[..., None], b, torch.where(third[..., None], c, zero)))
        out.append(torch.where(inside[..., None], ins, edge))
    return out


def _element_of(first_idx, count):
    """The batch element of each of `count` packed rows: the last element whose first index is <= the row."""
    rows = torch.arange(count, device=first_idx.device)
    return (torch.searchsorted(first_idx.contiguous(), rows, right=True) - 1).clamp_(min=0)


def _ends(first_idx, total):
    return torch.cat([first_idx[1:], first_idx.new_tensor([total])])


def torch_forward(direction, points, points_first_idx, prims, prims_first_idx, min_triangle_area=DEFAULT_MIN_TRIANGLE_AREA):
    """(dists, idxs) over the query objects by the contract of the module docstring; any device and float type.  Element by element
    (the first indices are read on the host: on GPU tensors this formulation waits for the device), rows in bounded chunks."""
    point_query = direction.startswith("point")
    Q, T, N = (points if point_query else prims).shape[0], (prims if point_query else points).shape[0], points_first_idx.shape[0]
    dists = torch.full((Q,), FLT_MAX, dtype=points.dtype, device=points.device)
    idxs = torch.zeros((Q,), dtype=torch.int64, device=points.device)
    if Q == 0 or T == 0 or N == 0:
        return dists, idxs
    P, S = points.shape[0], prims.shape[0]
    pf = [min(max(int(v), 0), P) for v in points_first_idx.tolist()] + [P]
    sf = [min(max(int(v), 0), S) for v in prims_first_idx.tolist()] + [S]
    for n in range(N):
        p0, p1, s0, s1 = pf[n], max(pf[n], pf[n + 1]), sf[n], max(sf[n], sf[n + 1])
        (q0, q1), (t0, t1) = ((p0, p1), (s0, s1)) if point_query else ((s0, s1), (p0, p1))
        if q1 == q0 or t1 == t0:
            continue
        rows = max(1, CHUNK_ELEMENTS // (t1 - t0))
        for r0 in range(q0, q1, rows):
            r1 = min(q1, r0 + rows)
            if point_query:
                d = _pair_dist(points[r0:r1, None, :], prims[None, t0:t1], min_triangle_area)
            else:
                d = _pair_dist(points[None, t0:t1, :], prims[r0:r1, None], min_triangle_area)
            d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
            # the LARGEST index among equal distances: the first minimum of the reversed row
            best = (t1 - t0 - 1) - torch.argmin(d.flip(1), dim=1)
            found = torch.gather(d, 1, best[:, None])[:, 0]
            ok = found <= FLT_MAX
            dists[r0:r1] = torch.where(ok, found, dists[r0:r1])
            idxs[r0:r1] = torch.where(ok, best + t0, idxs[r0:r1])
    return dists, idxs


def torch_backward(direction, points, prims, idxs, grad_dists, min_triangle_area=DEFAULT_MIN_TRIANGLE_AREA, points_first_idx=None,
                   prims_first_idx=None):
    """(grad_points, grad_prims).  With the first-index tensors a query of an element without targets contributes nothing."""
    point_query = direction.startswith("point")
    grad_points, grad_prims = torch.zeros_like(points), torch.zeros_like(prims)
    q, t = (points, prims) if point_query else (prims, points)
    Q, T = q.shape[0], t.shape[0]
    if Q == 0 or T == 0:
        return grad_points, grad_prims
    hit = (idxs >= 0) & (idxs < T)
    if points_first_idx is not None:
        qf, tf = (points_first_idx, prims_first_idx) if point_query else (prims_first_idx, points_first_idx)
        elem = _element_of(qf, Q)
        hit = hit & (_ends(tf, T)[elem] > tf[elem])
    j = idxs.clamp(0, T - 1)
    p, s = (points, prims[j]) if point_query else (points[j], prims)
    g = grad_dists.to(points.dtype)
    if s.shape[1] == 2:
        gp, g0, g1 = _seg_backward(p, s[:, 0], s[:, 1], g)
        gs = torch.stack([g0, g1], 1)
    else:
        gp, g0, g1, g2 = _tri_backward(p, s[:, 0], s[:, 1], s[:, 2], g, min_triangle_area)
        gs = torch.stack([g0, g1, g2], 1)
    gp = torch.where(hit[:, None], gp, torch.zeros_like(gp))
    gs = torch.where(hit[:, None, None], gs, torch.zeros_like(gs))
    if point_query:
        grad_points += gp
        grad_prims.index_add_(0, j, gs)
    else:
        grad_prims += gs
        grad_points.index_add_(0, j, gp)
    return grad_points, grad_prims


# ---- the eight operators of `pytorch3d._C`: kernels where they apply, the torch formulation otherwise ------------------------------------
def _dist_forward(direction, points, points_first_idx, prims, prims_first_idx, max_queries, min_triangle_area=DEFAULT_MIN_TRIANGLE_AREA):
    if kernel_path(points, prims):
        return _C.point_mesh_forward(direction, points, points_first_idx, prims, prims_first_idx, max_queries, min_triangle_area)
    return torch_forward(direction, points, points_first_idx, prims.to(points.dtype), prims_first_idx, min_triangle_area)


def _dist_backward(direction, points, prims, idxs, grad_dists, min_triangle_area=DEFAULT_MIN_TRIANGLE_AREA, points_first_idx=None,
                   prims_first_idx=None):
    if kernel_path(points, prims):
        return _C.point_mesh_backward(direction, points, prims, idxs, grad_dists, min_triangle_area, points_first_idx, prims_first_idx)
    return torch_backward(direction, points, prims.to(points.dtype), idxs, grad_dists, min_triangle_area, points_first_idx, prims_first_idx)


def point_face_dist_forward(points, points_first_idx, tris, tris_first_idx, max_points, min_triangle_area=DEFAULT_MIN_TRIANGLE_AREA):
    return _dist_forward("point_face", points, points_first_idx, tris, tris_first_idx, max_points, min_triangle_area)


def point_face_dist_backward(points, tris, idxs, grad_dists, min_triangle_area=DEFAULT_MIN_TRIANGLE_AREA):
    return _dist_backward("point_face", points, tris, idxs, grad_dists, min_triangle_area)


def face_point_dist_forward(points, points_first_idx, tris, tris_first_idx, max_tris, min_triangle_area=DEFAULT_MIN_TRIANGLE_AREA):
    return _dist_forward("face_point", points, points_first_idx, tris, tris_first_idx, max_tris, min_triangle_area)


def face_point_dist_backward(points, tris, idxs, grad_dists, min_triangle_area=DEFAULT_MIN_TRIANGLE_AREA):
    return _dist_backward("face_point", points, tris, idxs, grad_dists, min_triangle_area)


def point_edge_dist_forward(points, points_first_idx, segms, segms_first_idx, max_points):
    return _dist_forward("point_edge", points, points_first_idx, segms, segms_first_idx, max_points)


def point_edge_dist_backward(points, segms, idxs, grad_dists):
    return _dist_backward("point_edge", points, segms, idxs, grad_dists)


def edge_point_dist_forward(points, points_first_idx, segms, segms_first_idx, max_segms):
    return _dist_forward("edge_point", points, points_first_idx, segms, segms_first_idx, max_segms)


def edge_point_dist_backward(points, segms, idxs, grad_dists):
    return _dist_backward("edge_point", points, segms, idxs, grad_dists)


# ---- the four autograd functions ---------------------------------------------------------------------------------------------------
class _Distance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, direction, points, points_first_idx, prims, prims_first_idx, max_queries, min_triangle_area):
        points, prims = points.contiguous(), prims.contiguous()
        dists, idxs = _dist_forward(direction, points, points_first_idx, prims, prims_first_idx, max_queries, min_triangle_area)
        ctx.save_for_backward(points, prims, idxs, points_first_idx, prims_first_idx)
        ctx.direction, ctx.min_triangle_area = direction, min_triangle_area
        return dists

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_dists):
        points, prims, idxs, pfirst, sfirst = ctx.saved_tensors
        grad_points, grad_prims = _dist_backward(ctx.direction, points, prims, idxs, grad_dists.contiguous(), ctx.min_triangle_area,
                                                 pfirst, sfirst)
        return None, grad_points, None, grad_prims, None, None, None


def point_face_distance(points, points_first_idx, tris, tris_first_idx, max_points, min_triangle_area=DEFAULT_MIN_TRIANGLE_AREA):
    """dists (P,): the squared distance of every point to the closest face of its element."""
    return _Distance.apply("point_face", points, points_first_idx, tris, tris_first_idx, max_points, min_triangle_area)


def face_point_distance(points, points_first_idx, tris, tris_first_idx, max_tris, min_triangle_area=DEFAULT_MIN_TRIANGLE_AREA):
    """dists (T,): the squared distance of every face to the closest point of its element."""
    return _Distance.apply("face_point", points, points_first_idx, tris, tris_first_idx, max_tris, min_triangle_area)


def point_edge_distance(points, points_first_idx, segms, segms_first_idx, max_points):
    """dists (P,): the squared distance of every point to the closest edge of its element."""
    return _Distance.apply("point_edge", points, points_first_idx, segms, segms_first_idx, max_points, DEFAULT_MIN_TRIANGLE_AREA)


def edge_point_distance(points, points_first_idx, segms, segms_first_idx, max_segms):
    """dists (S,): the squared distance of every edge to the closest point of its element."""
    return _Distance.apply("edge_point", points, points_first_idx, segms, segms_first_idx, max_segms, DEFAULT_MIN_TRIANGLE_AREA)


# ---- the two losses ----------------------------------------------------------------------------------------------------------------
class _PointMeshLoss(torch.autograd.Function):
    """verts (V, 3), points (P, 3) float32 on one GPU; index (F, 3) or (E, 2) int64 packed vertex ids of the faces / edges.  The loss
    of the reference: per direction the element means of the distances, averaged over the batch, the two directions added."""

    @staticmethod
    def forward(ctx, verts, points, index, prims_first_idx, points_first_idx, num_prims, num_points, max_prims, max_points,
                min_triangle_area):
        from .rasterize_meshes import _GatherFaceVerts

        verts, points = _C._c(verts, torch.float32), _C._c(points, torch.float32)
        faces = index.shape[1] == 3
        dev, N = verts.device, int(points_first_idx.shape[0])
        with torch.cuda.device(dev):
            if faces:
                prims = _GatherFaceVerts.forward(_Ctx(), verts, index)
            else:
                prims = verts[index]
            w_points = 1.0 / (num_points.to(torch.float32) * N)
            w_prims = 1.0 / (num_prims.to(torch.float32) * N)
            a, b = ("point_face", "face_point") if faces else ("point_edge", "edge_point")
            _, idx_p, sums_p = _C.point_mesh_forward(a, points, points_first_idx, prims, prims_first_idx, max_points, min_triangle_area,
                                                     split=SPLIT, weights=w_points, with_sums=True)
            _, idx_s, sums_s = _C.point_mesh_forward(b, points, points_first_idx, prims, prims_first_idx, max_prims, min_triangle_area,
                                                     split=SPLIT, weights=w_prims, with_sums=True)
            loss = sums_p.sum() + sums_s.sum()
        ctx.save_for_backward(verts, points, index, prims, idx_p, idx_s, points_first_idx, prims_first_idx, w_points, w_prims)
        ctx.directions, ctx.min_triangle_area = (a, b), min_triangle_area
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        verts, points, index, prims, idx_p, idx_s, pfirst, sfirst, w_points, w_prims = ctx.saved_tensors
        a, b = ctx.directions
        dev = verts.device
        with torch.cuda.device(dev):
            up = grad_loss.to(device=dev, dtype=torch.float32).reshape(())
            grad_points, grad_prims = _C.point_mesh_backward(a, points, prims, idx_p, None, ctx.min_triangle_area, pfirst, sfirst,
                                                             elem_scale=up * w_points)
            _C.point_mesh_backward(b, points, prims, idx_s, None, ctx.min_triangle_area, pfirst, sfirst, elem_scale=up * w_prims,
                                   grad_points=grad_points, grad_prims=grad_prims, accumulate=True)
            grad_verts = None
            if ctx.needs_input_grad[0]:
                V = verts.shape[0]
                if index.shape[1] == 3:
                    grad_verts = _C.scatter_face_grads(grad_prims, index, V)
                else:
                    grad_verts = _scatter_corner_grads(grad_prims, index, V)
        return grad_verts, (grad_points if ctx.needs_input_grad[1] else None), None, None, None, None, None, None, None, None


class _Ctx:
    """Stands in for an autograd context where a Function's forward is used as a plain function."""

    def save_for_backward(self, *tensors):
        pass


def _scatter_corner_grads(grad_segms, edges, V):
    """The backward of verts[edges] through the face scatter (p3d_scatter_face_grads, ordered under the strict flag): the 2 E corners
    are padded to a multiple of three with zero rows that go to vertex 0."""
    corners = edges.reshape(-1)
    pad = (-corners.numel()) % 3
    g = grad_segms.reshape(-1, 3)
    if pad:
        corners = torch.cat([corners, corners.new_zeros((pad,))])
        g = torch.cat([g, g.new_zeros((pad, 3))])
    return _C.scatter_face_grads(g.reshape(-1, 3, 3).contiguous(), corners.reshape(-1, 3).contiguous(), V)


_EDGE_KEY = "_p3d_amd_point_mesh_edges"


def _edge_tables(meshes):
    """(edges (E, 2) int64, first index (N,) int64, edges per mesh (N,) int64, host bound of the edges per mesh) of `meshes`: the set
    and order of edges_packed(), from the topology kept with the object (built once, with host syncs; then none)."""
    from . import mesh_losses

    t = mesh_losses.topology_of(meshes)
    kept = getattr(meshes, "__dict__", {}).get(_EDGE_KEY)
    if kept is None or kept[0] is not t:
        num = t.num_edges.long()
        first = torch.cumsum(num, 0) - num
        bound = t.E
        F = getattr(meshes, "_F", None)
        if isinstance(F, int):
            bound = min(bound, 3 * F)
        kept = (t, t.edges.long().contiguous(), first.contiguous(), num, int(bound))
        if hasattr(meshes, "__dict__"):
            meshes.__dict__[_EDGE_KEY] = kept
    return kept[1:]


def _host_max(obj, attr, total):
    v = getattr(obj, attr, None)
    return int(v) if isinstance(v, int) and 0 <= v <= total else int(total)


def fused_path(meshes, pcls):
    """Whether the losses on these batches are the single autograd node over the kernels."""
    verts, points = meshes.verts_packed(), pcls.points_packed()
    return kernel_path(points, verts) and verts.dim() == 2 and verts.shape[1] == 3 and points.dim() == 2 and points.shape[1] == 3


def _loss(meshes, pcls, faces, min_triangle_area):
    if len(meshes) != len(pcls):
        raise ValueError("meshes and pointclouds must be equal sized batches")
    N = len(meshes)
    points = pcls.points_packed()
    points_first_idx = pcls.cloud_to_packed_first_idx()
    num_points = pcls.num_points_per_cloud()
    max_points = _host_max(pcls, "_P", points.shape[0])
    verts = meshes.verts_packed()
    if faces:
        index = meshes.faces_packed()
        prims_first_idx = meshes.mesh_to_faces_packed_first_idx()
        num_prims = meshes.num_faces_per_mesh()
        max_prims = _host_max(meshes, "_F", index.shape[0])
    else:
        index, prims_first_idx, num_prims, max_prims = _edge_tables(meshes)
    if fused_path(meshes, pcls):
        dev = verts.device
        return _PointMeshLoss.apply(verts, points, index.to(device=dev, dtype=torch.int64).contiguous(),
                                    prims_first_idx.to(device=dev, dtype=torch.int64).contiguous(),
                                    points_first_idx.to(device=dev, dtype=torch.int64).contiguous(), num_prims.to(dev), num_points.to(dev),
                                    max_prims, max_points, float(min_triangle_area))
    # the reference's expression over the autograd functions above (torch formulation, or kernels for what only they take)
    prims = verts[index.to(verts.device)]
    a, b = ("point_face", "face_point") if faces else ("point_edge", "edge_point")
    to_prim = _Distance.apply(a, points, points_first_idx, prims, prims_first_idx, max_points, min_triangle_area)
    w = torch.reciprocal(num_points.gather(0, _element_of(points_first_idx, points.shape[0])).to(torch.float32)) if points.shape[0] \
        else to_prim
    point_dist = (to_prim * w).sum() / N
    to_point = _Distance.apply(b, points, points_first_idx, prims, prims_first_idx, max_prims, min_triangle_area)
    w = 1.0 / num_prims.gather(0, _element_of(prims_first_idx, prims.shape[0])).to(torch.float32) if prims.shape[0] else to_point
    prim_dist = (to_point * w).sum() / N
    return point_dist + prim_dist


def point_mesh_face_distance(meshes, pcls, min_triangle_area: float = DEFAULT_MIN_TRIANGLE_AREA):
    """point_face(mesh, pcl) + face_point(mesh, pcl), each the mean over an element's points / faces, averaged over the batch."""
    return _loss(meshes, pcls, True, min_triangle_area)


def point_mesh_edge_distance(meshes, pcls):
    """point_edge(mesh, pcl) + edge_point(mesh, pcl), each the mean over an element's points / edges, averaged over the batch."""
    return _loss(meshes, pcls, False, DEFAULT_MIN_TRIANGLE_AREA)
