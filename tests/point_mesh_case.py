"""The cases of the point-mesh distance tests, shared by tests/golden/make_golden_point_mesh.py (which records the reference's results
into tests/golden/point_mesh_ref.npz), tests/test_cpu_point_mesh.py, tests/test_gpu_point_mesh.py and tests/shim_point_mesh_case.py;
at the end the generated batch of tests/test_cpu_loss_kernel_edges.py / tests/test_gpu_loss_kernel_edges.py.

The fixture holds the inputs too.  Independent of the package: a float64 restatement of the pair distances (differentiated by
autograd), the rule that admits a query to the index comparison, exact-tie soups and the star.

A case is a BATCH: a list of (points, primitives) counts per element.  Every case exists for triangles ("tri") and for segments
("seg") and is used in both directions -- the points query the primitives and the primitives query the points -- so a count pair
(a, b) puts a queries against b targets and b queries against a targets.  An error budget (E of a case and direction: the largest
absolute error of the reference's float32 minima against float64; the same for each gradient) belongs to a whole batch, which keeps it
from resting on one or two queries.
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "point_mesh_ref.npz")

TILE = 64                  # targets the kernel stages per wave and step (include/p3d_amd.h: P3D_POINT_MESH_TILE); it reads them four at a time
MIN_AREA = 5e-3            # the reference's default min_triangle_area
FLT_MAX = 3.4028234663852886e38
GAP_FACTOR = 16.0          # a query enters the index comparison when its two smallest float64 distances differ by >= 16 E
MAX_DROPPED = 0.05         # of a soup case's queries
KINDS = ("tri", "seg")
DIRECTIONS = {"tri": ("point_face", "face_point"), "seg": ("point_edge", "edge_point")}

# name -> [(points, primitives) per element].  Soups: independent uniform vertices in the unit cube.
OP_CASES = {
    # targets T - 1, T, T + 1, 2 T + 3 and 1; queries 1, 63, 64, 65, 130 (and 131) -- in both directions
    "tiles": [(65, TILE - 1), (TILE, TILE), (63, TILE + 1), (130, 2 * TILE + 3), (1, 1), (2 * TILE + 3, 130)],
    "ragged": [(70, 40), (1, TILE + 1), (130, 1)],
    "empty_cloud": [(0, 10), (20, 15), (5, 3)],
    "empty_mesh": [(12, 0), (20, 15), (5, 3)],
    "degenerate": None,  # built by degenerate_case(): one element
}
SOUP_CASES = ("tiles", "ragged", "empty_cloud", "empty_mesh")
MESH_CASES = ("ico2", "ragged", "small_faces_a", "small_faces_b")  # mesh-level losses: verts + faces + clouds


def key(kind, name, what, direction=None):
    return "%s/%s/%s" % (kind, name, what) if direction is None else "%s/%s/%s/%s" % (kind, name, direction, what)


_LOADED = {}


def fixture():
    if "z" not in _LOADED:
        with np.load(FIXTURE) as z:
            _LOADED["z"] = {k: torch.from_numpy(z[k]) for k in z.files}
    return _LOADED["z"]


def first_idx(counts):
    c = torch.tensor(counts, dtype=torch.int64)
    return torch.cumsum(c, 0) - c


def counts_of(z, kind, name):
    return [int(v) for v in z[key(kind, name, "num_points")]], [int(v) for v in z[key(kind, name, "num_prims")]]


def op_inputs(z, kind, name, device="cpu", dtype=torch.float32, requires_grad=False):
    """(points, points_first_idx, prims, prims_first_idx, max_points, max_prims) of an operator-level case."""
    np_, ns = counts_of(z, kind, name)
    points = z[key(kind, name, "points")].detach().clone().to(device=device, dtype=dtype).requires_grad_(requires_grad)
    prims = z[key(kind, name, "prims")].detach().clone().to(device=device, dtype=dtype).requires_grad_(requires_grad)
    return points, first_idx(np_).to(device), prims, first_idx(ns).to(device), max(np_ + [0]), max(ns + [0])


def upstream(n, shift=0):
    """The upstream gradient of n distances: every entry weighted differently."""
    return torch.cos(torch.arange(n, dtype=torch.float64) + shift).to(torch.float32)


def degenerate_case(kind, gen):
    """One element, everything inside the unit cube like the soups (the budgets are absolute errors): hand-built primitives followed
    by 12 soup primitives, and points: special[k] meets primitive target[k] in a chosen way, then 60 uniform ones around both.  Returns (points,
    prims, target); the generator asserts that the reference sends special point k to primitive target[k]."""
    a = (2 * 0.5 * MIN_AREA) ** 0.5  # legs of a right triangle of HALF the minimum area
    b = (2 * 2.0 * MIN_AREA) ** 0.5  # ... of TWICE the minimum area
    if kind == "seg":
        built = torch.tensor([[[0.2, 0.2, 0.2], [0.2, 0.2, 0.2]],      # zero length
                              [[0.25, 0.5, 0.5], [0.75, 0.5, 0.5]]])
        special = torch.tensor([[0.22, 0.21, 0.19],   # nearest to the zero-length segment
                                [0.5, 0.5, 0.5],      # ON a segment (exactly, in float32): distance 0, gradient 0
                                [0.19, 0.51, 0.52],   # before an end (t < 0)
                                [0.8, 0.49, 0.52]])   # past an end (t > 1)
        target = [0, 1, 1, 1]
    else:
        built = torch.tensor([[[0.1, 0.1, 0.1], [0.3, 0.1, 0.1], [0.5, 0.1, 0.1]],                  # collinear
                              [[0.3, 0.8, 0.1], [0.3, 0.8, 0.1], [0.6, 0.9, 0.4]],                  # two equal vertices
                              [[0.7, 0.1, 0.8], [0.7 + a, 0.1, 0.8], [0.7, 0.1 + a, 0.8]],          # half the minimum area
                              [[0.1, 0.6, 0.8], [0.1 + b, 0.6, 0.8], [0.1, 0.6 + b, 0.8]],          # twice the minimum area
                              [[0.6, 0.5, 0.5], [0.9, 0.5, 0.5], [0.6, 0.8, 0.5]]])                 # a plain face in the plane z = 0.5
        special = torch.tensor([[0.28, 0.12, 0.11],                       # near the collinear face
                                [0.32, 0.83, 0.12],                       # near the face with two equal vertices
                                [0.7 + a / 4, 0.1 + a / 4, 0.85],         # above the interior of the small face: edge branch
                                [0.1 + b / 4, 0.6 + b / 4, 0.85],         # above the interior of the large face: plane branch
                                [0.68, 0.58, 0.5]])                       # IN the plain face's plane, inside: distance 0, gradient 0
        target = [0, 1, 2, 3, 4]
    # the soup lies below the built primitives (z in [-0.6, -0.1]; the special points stay within 0.1 of their targets)
    below = torch.rand(12, built.shape[1], 3, generator=gen) * torch.tensor([1.0, 1.0, 0.5]) - torch.tensor([0.0, 0.0, 0.6])
    prims = torch.cat([built, below], 0)
    points = torch.cat([special, torch.rand(60, 3, generator=gen) * torch.tensor([1.0, 1.0, 1.6]) - torch.tensor([0.0, 0.0, 0.6])], 0)
    return points.contiguous(), prims.contiguous(), target


# ---- float64 restatement (vectorised, differentiable) -------------------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum(-1)


def seg_dist64(p, s0, s1):
    d = s1 - s0
    l2 = _dot(d, d)
    same = l2 < 1e-8
    safe = torch.where(same, torch.ones_like(l2), l2)
    t = (_dot(d, p - s0) / safe).clamp(0.0, 1.0)
    x = s0 + t[..., None] * d
    on = _dot(x - p, x - p)
    ends = 0.5 * _dot(p - s0, p - s0) + 0.5 * _dot(p - s1, p - s1)
    return torch.where(same, ends, on)


def tri_dist64(p, a, b, c, min_area=MIN_AREA):
    cross = torch.cross(b - a, c - a, dim=-1)
    norm = cross.norm(dim=-1)
    normal = cross / norm.clamp_min(1e-30)[..., None]
    tt = _dot(normal, a) - _dot(normal, p)
    p0 = p + tt[..., None] * normal
    v0, v1, v2 = b - a, c - a, p0 - a
    d00, d01, d11, d20, d21 = _dot(v0, v0), _dot(v0, v1), _dot(v1, v1), _dot(v2, v0), _dot(v2, v1)
    denom = d00 * d11 - d01 * d01 + 1e-8
    s2 = (d11 * d20 - d01 * d21) / denom
    s3 = (d00 * d21 - d01 * d20) / denom
    s1 = 1.0 - s2 - s3
    inside = (norm / 2.0 >= min_area) & (norm > 1e-8)
    for s in (s1, s2, s3):
        inside = inside & (s >= 0.0) & (s <= 1.0)
    e01, e02, e12 = seg_dist64(p, a, b), seg_dist64(p, a, c), seg_dist64(p, b, c)
    # the reference's cascade (an exact tie between two edges, as on a collinear face, goes to the first; no gradient is split)
    first, second = (e01 <= e02) & (e01 <= e12), (e02 <= e01) & (e02 <= e12)
    e = torch.where(first, e01, torch.where(second, e02, e12))
    return torch.where(inside, tt * tt, e)


def pair_dist64(points, prims, min_area=MIN_AREA):
    """points (..., 3) against prims (..., 2 or 3, 3), broadcast; in the dtype given (float64 for the budgets)."""
    if prims.shape[-2] == 2:
        return seg_dist64(points, prims[..., 0, :], prims[..., 1, :])
    return tri_dist64(points, prims[..., 0, :], prims[..., 1, :], prims[..., 2, :], min_area)


def matrix64(points, prims, min_area=MIN_AREA):
    """(P, T) float64 distances of the float32 VALUES."""
    return pair_dist64(points.double()[:, None, :], prims.double()[None], min_area)


def element_slices(counts):
    out, at = [], 0
    for c in counts:
        out.append((at, at + c))
        at += c
    return out


def minima64(points, prims, num_points, num_prims, point_query, min_area=MIN_AREA):
    """Per query of the direction: (smallest float64 distance or FLT_MAX, the gap to the second smallest or +inf, how many targets)."""
    Q = points.shape[0] if point_query else prims.shape[0]
    best = torch.full((Q,), FLT_MAX, dtype=torch.float64, device=points.device)
    gap = torch.full((Q,), float("inf"), dtype=torch.float64, device=points.device)
    for (p0, p1), (s0, s1) in zip(element_slices(num_points), element_slices(num_prims)):
        if p1 == p0 or s1 == s0:
            continue
        d = matrix64(points[p0:p1], prims[s0:s1], min_area)
        d = d if point_query else d.t()
        sd = torch.sort(d, dim=1).values
        q0, q1 = (p0, p1) if point_query else (s0, s1)
        best[q0:q1] = sd[:, 0]
        if sd.shape[1] > 1:
            gap[q0:q1] = sd[:, 1] - sd[:, 0]
    return best, gap


def admitted(gap, E):
    return gap >= GAP_FACTOR * E


def grads64(points, prims, idxs, up, has_target, point_query, min_area=MIN_AREA):
    """float64 (grad_points, grad_prims) of sum(up * distance(query, target idxs[query])) over the queries that have a target."""
    a, b = points.detach().double().requires_grad_(True), prims.detach().double().requires_grad_(True)
    if not bool(has_target.any()):
        return torch.zeros_like(a), torch.zeros_like(b)
    q = torch.nonzero(has_target).squeeze(1)
    d = pair_dist64(a[q], b[idxs[q]], min_area) if point_query else pair_dist64(a[idxs[q]], b[q], min_area)
    ga, gb = torch.autograd.grad((d * up.double()[q]).sum(), (a, b), allow_unused=True)
    return (torch.zeros_like(a) if ga is None else ga), (torch.zeros_like(b) if gb is None else gb)


# ---- exact ties and the star -------------------------------------------------------------------------------------------------------
def tie_case(kind, seed=7):
    """A soup in which every third primitive appears AGAIN further down (bit-equal distances by construction): (points, prims,
    twin), twin[j] = the index of the later copy of primitive j, or j itself."""
    gen = torch.Generator().manual_seed(seed)
    corners = 3 if kind == "tri" else 2
    base = torch.rand(90, corners, 3, generator=gen)
    prims = torch.cat([base, base[::3]], 0).contiguous()
    twin = torch.arange(prims.shape[0])
    twin[0:90:3] = 90 + torch.arange(30)
    points = torch.rand(100, 3, generator=gen)
    return points, prims, twin


def star_case(kind, seed=5, P=300):
    """Every point is nearest to ONE primitive (the worst case of the scatter): a small primitive near the origin's corner and a far
    decoy, the points spread around the near one."""
    gen = torch.Generator().manual_seed(seed)
    if kind == "tri":
        near = torch.tensor([[0.0, 0.0, 0.0], [0.3, 0.0, 0.0], [0.0, 0.3, 0.0]])
        far = near + 50.0
    else:
        near = torch.tensor([[0.0, 0.0, 0.0], [0.3, 0.0, 0.0]])
        far = near + 50.0
    points = torch.randn(P, 3, generator=gen) * 0.5
    return points, torch.stack([near, far], 0).contiguous()


# ---- mesh-level cases -----------------------------------------------------------------------------------------------------------------
def mesh_inputs(z, name, device="cpu", dtype=torch.float32):
    """(verts list, faces list, points list) of a mesh-level case; the leaves require grad."""
    n = int(z["mesh/%s/N" % name])
    verts = [z["mesh/%s/verts%d" % (name, i)].detach().clone().to(device=device, dtype=dtype).requires_grad_(True) for i in range(n)]
    faces = [z["mesh/%s/faces%d" % (name, i)].to(device) for i in range(n)]
    points = [z["mesh/%s/points%d" % (name, i)].detach().clone().to(device=device, dtype=dtype).requires_grad_(True) for i in range(n)]
    return verts, faces, points


# ---- the comparisons every implementation has to pass (CPU and GPU tests) ---------------------------------------------------------------
def check_direction(z, kind, name, direction, dists, idxs, grad_points, grad_prims, who=""):
    """The comparisons every implementation has to pass on an operator-level case (also used by the GPU tests)."""
    def rec(what):
        return z[key(kind, name, what, direction)]

    E, Egp, Egs = float(rec("E")), float(rec("E_grad_points")), float(rec("E_grad_prims"))
    want_d, want_i, ok = rec("dists"), rec("idxs"), rec("admitted")
    none = want_d == FLT_MAX
    dists, idxs = dists.detach().cpu(), idxs.cpu()
    err = float((dists.double() - want_d.double())[~none].abs().max()) if bool((~none).any()) else 0.0
    gerr_p = float((grad_points.cpu().double() - rec("grad_points").double()).abs().max())
    gerr_s = float((grad_prims.cpu().double() - rec("grad_prims").double()).abs().max())
    print("%s %s %s %s: dist error %.3g (4 E = %.3g), grad_points %.3g (%.3g), grad_prims %.3g (%.3g), admitted %d of %d"
          % (who, kind, name, direction, err, 4 * E, gerr_p, 4 * Egp, gerr_s, 4 * Egs, int(ok.sum()), ok.numel()))
    assert torch.equal(dists[none], want_d[none]) and bool((idxs[none] == 0).all()), "an element without targets: FLT_MAX, index 0"
    assert torch.equal(idxs[ok], want_i[ok]), "indices differ on admitted queries"
    assert err <= 4 * E
    assert gerr_p <= 4 * Egp and gerr_s <= 4 * Egs


def run_direction(pm, z, kind, name, direction, device="cpu"):
    points, pfirst, prims, sfirst, max_p, max_s = op_inputs(z, kind, name, device=device, requires_grad=True)
    fn = getattr(pm, direction + "_distance")
    point_query = direction.startswith("point")
    args = (points, pfirst, prims, sfirst, max_p if point_query else max_s)
    dists = fn(*args)
    assert dists.shape == ((points if point_query else prims).shape[0],)
    idxs = getattr(pm, direction + "_dist_forward")(points.detach(), pfirst, prims.detach(), sfirst, args[4])[1]
    up = upstream(dists.shape[0]).to(device)
    gp, gs = torch.autograd.grad((dists * up).sum(), (points, prims), allow_unused=True)
    gp = torch.zeros_like(points) if gp is None else gp
    gs = torch.zeros_like(prims) if gs is None else gs
    return dists, idxs, gp, gs


def check_mesh_loss(z, name, tag, loss, grad_verts, grad_points, who=""):
    """Loss: every distance carries at most the recorded error of the minima (E_minima sums the two directions' largest), the loss is
    two weighted means of them; 4 x that plus 32 roundings of the sum itself.  Gradients, per entry: 4 x the recorded error plus
    4 x 2^-24 of the entry -- the fused node multiplies by ONE rounded weight 1 / (count N) where the reference rounds 1 / count, the
    product and the division by N (three roundings against one), and the entry itself is rounded once more; an absolute bound alone
    would lie below the float32 spacing of the largest entries (an element with a single point has gradients of order 1)."""
    want = float(z["mesh/%s/%s_loss" % (name, tag)])
    E, Eg = float(z["mesh/%s/%s_E_minima" % (name, tag)]), float(z["mesh/%s/%s_E_grad" % (name, tag)])
    tol = 4 * E + 32 * 2.0 ** -24 * abs(want)
    gerr, excess = 0.0, 0.0
    for i, (gv, gp) in enumerate(zip(grad_verts, grad_points)):
        for got, ref in ((gv, z["mesh/%s/%s_grad_verts%d" % (name, tag, i)]), (gp, z["mesh/%s/%s_grad_points%d" % (name, tag, i)])):
            if not ref.numel():
                continue
            err = (got.detach().cpu().double() - ref.double()).abs()
            gerr = max(gerr, float(err.max()))
            excess = max(excess, float((err - (4 * Eg + 4 * 2.0 ** -24 * ref.double().abs())).max()))
    print("%s mesh %s %s: loss %.8g, reference %.8g (tolerance %.3g); gradient error %.3g (4 E_grad = %.3g), largest excess over the "
          "per-entry bound %.3g" % (who, name, tag, float(loss), want, tol, gerr, 4 * Eg, excess))
    assert abs(float(loss) - want) <= tol
    assert excess <= 0.0


# ---- the second round of the element sums (tests/test_*_loss_kernel_edges.py) ---------------------------------------------------------------
def sum_depth(n):
    """Additions a term passes through in a fused loss whose largest element has n queries: 6 butterfly rounds in the wave, lane t of
    one block adding the wave partials t, t + 256, ..., 8 more rounds (csrc/fixed_sum.h: segment_sum_kernel), then the
    elements and the two directions added."""
    import math

    return 6 + math.ceil(math.ceil(n / 64) / 256) + 8 + 2


def second_round_batch():
    """(verts list, faces list, points list, edges (E, 2) packed) of two elements, each direction with one element beyond the 16 384
    queries = 256 wave partials of the first round while every distance matrix stays 16.5 k x a few dozen:
      0. a jittered 92 x 92 vertex grid, 0.1 apart (16 562 faces of 5e-3 area and more on average -- both branches of the triangle
         distance --, 25 025 edges), under a cloud of 30 points;
      1. ico_sphere(0) around a cloud of 16 500 points INSIDE it (radius 0.3 .. 0.7 of the unit sphere's, the inscribed sphere has
         0.79): a point inside a convex body is nearest to the interior of a face, so the nearest face is not a tie of the two faces
         on an edge."""
    import _util as U
    import mesh_losses_case as ML

    gen = torch.Generator().manual_seed(41)
    gv, gf = ML.jittered_grid(92, gen)
    above = torch.rand(30, 3, generator=gen) * torch.tensor([9.1, 9.1, 0.4]) + torch.tensor([0.0, 0.0, 0.05])
    iv, iface = U.ico_sphere(0)
    d = torch.randn(16500, 3, generator=gen)
    inside = d / d.norm(dim=1, keepdim=True) * (0.3 + 0.4 * torch.rand(16500, 1, generator=gen))
    verts, faces, points = [gv, iv.contiguous()], [gf, iface.contiguous()], [above.contiguous(), inside.float().contiguous()]
    return verts, faces, points, ML.tensor_tables(verts, faces)["edges"]


_SECOND = {}


def second_round_truth(tag):
    """Everything tests judge the fused loss `tag` ("face" / "edge") on second_round_batch() by, computed once and never modified:
    per direction the float64 minima and gaps (minima64), the package's float32 torch formulation's distances and indices on the
    CPU, its error E and the admission; the float64 loss on the minima, S (the same sum: every term is >= 0), the float64 gradients on
    the formulation's indices, and the formulation's own loss and gradients through the package's loss on CPU tensors with their
    largest error."""
    if tag in _SECOND:
        return _SECOND[tag]
    import pytorch3d_amd as p3d
    from pytorch3d_amd import point_mesh as pm

    verts, faces, points, edges = second_round_batch()
    N = len(verts)
    nv = [v.shape[0] for v in verts]
    packed_v, packed_p = torch.cat(verts, 0), torch.cat(points, 0)
    if tag == "face":
        index = torch.cat([f + b for f, b in zip(faces, first_idx(nv).tolist())], 0)
        num_prims = [f.shape[0] for f in faces]
    else:
        index = edges
        num_prims = torch.bincount(torch.searchsorted(first_idx(nv), edges[:, 0].contiguous(), right=True) - 1, minlength=N).tolist()
    num_points = [p.shape[0] for p in points]
    prims = packed_v[index]
    pfirst, sfirst = first_idx(num_points), first_idx(num_prims)
    out = {"index": index, "num_points": num_points, "num_prims": num_prims, "pfirst": pfirst, "sfirst": sfirst, "points": packed_p,
           "prims": prims, "directions": {}}
    loss64, e_minima = 0.0, 0.0
    gp64, gs64 = torch.zeros(packed_p.shape, dtype=torch.float64), torch.zeros(prims.shape, dtype=torch.float64)
    for direction in DIRECTIONS["tri" if tag == "face" else "seg"]:
        point_query = direction.startswith("point")
        best64, gap = minima64(packed_p, prims, num_points, num_prims, point_query)
        want_d, want_i = pm.torch_forward(direction, packed_p, pfirst, prims, sfirst)
        E = float((want_d.double() - best64).abs().max())
        counts = num_points if point_query else num_prims
        w = torch.cat([torch.full((c,), 1.0 / (c * N), dtype=torch.float64) for c in counts])
        loss64 += float((best64 * w).sum())
        e_minima += E
        a, b = grads64(packed_p, prims, want_i, w, torch.ones_like(gap, dtype=torch.bool), point_query)
        gp64, gs64 = gp64 + a, gs64 + b
        out["directions"][direction] = dict(best64=best64, gap=gap, want_i=want_i, E=E, ok=admitted(gap, E), max_queries=max(counts))
    gv64 = torch.zeros(packed_v.shape, dtype=torch.float64).index_add(0, index.reshape(-1), gs64.reshape(-1, 3))
    v32, p32 = [v.clone().requires_grad_(True) for v in verts], [p.clone().requires_grad_(True) for p in points]
    meshes, pcls = p3d.PackedMeshes(v32, faces), p3d.PackedPointclouds(p32)
    f_loss = p3d.point_mesh_face_distance(meshes, pcls) if tag == "face" else p3d.point_mesh_edge_distance(meshes, pcls)
    f_grads = torch.autograd.grad(f_loss, v32 + p32)
    f_gv, f_gp = torch.cat(f_grads[:N], 0), torch.cat(f_grads[N:], 0)
    out.update(loss64=loss64, S=loss64, E_minima=e_minima, grad_verts64=gv64, grad_points64=gp64, f32_loss=float(f_loss.detach()),
               f32_grad_verts=f_gv, f32_grad_points=f_gp,
               E_grad=max(float((f_gv.double() - gv64).abs().max()), float((f_gp.double() - gp64).abs().max())),
               n=max(max(num_points), max(num_prims)))
    _SECOND[tag] = out
    return out


def check_second_round_loss(who, t, loss, grad_verts, grad_points):
    """The loss within 4 E + sum_depth(n) 2^-24 S (E: the two directions' largest errors of the minima, added -- the loss is two
    weighted means of them); the gradients per entry within 4 x the formulation's largest error + 4 x 2^-24 of the entry
    (check_mesh_loss).  Returns (loss ok, gradients ok)."""
    tol = 4 * t["E_minima"] + sum_depth(t["n"]) * 2.0 ** -24 * t["S"]
    loss = float(loss.detach()) if torch.is_tensor(loss) else float(loss)
    err = abs(loss - t["loss64"])
    gerr, excess = 0.0, -1.0
    for got, ref in ((grad_verts, t["grad_verts64"]), (grad_points, t["grad_points64"])):
        e = (got.detach().cpu().double() - ref).abs()
        gerr = max(gerr, float(e.max()))
        excess = max(excess, float((e - (4 * t["E_grad"] + 4 * 2.0 ** -24 * ref.abs())).max()))
    print("%s: loss %.9g, float64 %.9g, error %.3g (tolerance %.3g = 4 x %.3g + %d x 2^-24 x %.3g); gradient error %.3g (4 E_grad = %.3g), "
          "largest excess over the per-entry bound %.3g" % (who, float(loss), t["loss64"], err, tol, t["E_minima"], sum_depth(t["n"]), t["S"],
                                                           gerr, 4 * t["E_grad"], excess))
    return err <= tol, excess <= 0.0
