"""The inputs and the yardsticks of the cotangent-Laplacian tests (tests/test_cpu_mesh_laplacian.py, tests/test_gpu_mesh_laplacian.py,
tests/shim_mesh_laplacian_case.py, tests/golden/make_golden_mesh_laplacian.py): mesh_laplacian_smoothing "cot" / "cotcurv",
cot_laplacian and taubin_smoothing.

Cases (cases()): batches of float32 vertices and int64 faces, the smallest that reach each structure --
  batch      tests/mesh_losses_case.build_batch(): closed, open, non-manifold with three faces on an edge, a vertex without a face
             (packed id LONE_VERTEX: "cot" gives r = -x there and a non-zero gradient, "cotcurv" r = 0 and a zero gradient, Taubin a
             NaN row, the reference's), an empty mesh and a doubled face;
  collinear  a jittered ico_sphere(1) and a mesh whose face (0, 1, 2) has the side lengths 1, 2, 1 on integers: Heron's product is
             exactly 0 in both precisions, the clamp gives the area 1e-6, cot / 4 = +-1e6 / 4;
  coincident a jittered ico_sphere(1) and one triangle with two vertices at one position: the third vertex's row sum is exactly 0, so
             nw stays 0 and r = -x;
  fan200     200 separate petals (every angle near 60 degrees) round one vertex: a row of 400 neighbours, longer than a wave;
  grid20     a 20 x 20 jittered grid: 400 vertices, more than one block;
  grid257    a 257 x 257 jittered grid: 66 049 terms, the second round of the fixed tree (mesh_losses_case.SUM_CAP).
No kernel of csrc/mesh_laplacian.hip loops over the grid, so there is no second-pass case.

The truth is this file's restatement of the formulas in float64, differentiated by autograd: the reference hard-codes float32 in
cot_laplacian, norm_laplacian and the loss, so a float64 call of it raises.  laplacian_dense builds the same L as a dense V x V matrix
by Python loops over the faces (small cases; the CPU test holds the vectorised form to it).  The fixture tests/golden/
mesh_laplacian_ref.npz records the reference's own float32 results on the CPU and their errors against this truth; every gate is
four times that error, per case and per quantity (gates below), a loss additionally D(n) 2^-24 S.
"""
import math
import os

import numpy as np
import torch

import _util as U
import mesh_losses_case as M

GOLDEN = os.path.join(U.ROOT, "tests", "golden", "mesh_laplacian_ref.npz")
METHODS = ("cot", "cotcurv")
GRAD_OUTPUTS = (1.0, 0.37)
TAUBIN_ITERS = (1, 10)
LAMBD, MU = 0.53, -0.53
EPS = 1e-12
SMALL = ("batch", "collinear", "coincident", "fan200", "grid20")  # the cases whose arrays the fixture holds (the others: errors only)
LONE_VERTEX = 162 + 16 + 5  # the vertex of build_batch()'s "book" that no face uses
MIN_ANGLE = 15.0


def _jittered_ico(level, gen, jitter=0.03):
    v, f = U.ico_sphere(level)
    return (v + jitter * torch.randn(v.shape, generator=gen)).float().contiguous(), f.contiguous()


def _fan(petals, gen):
    """`petals` triangles that share vertex 0 and nothing else: petal i is (0, 1 + 2 i, 2 + 2 i), near equilateral, in a random plane."""
    d = torch.randn(petals, 3, generator=gen, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    e = torch.cross(d, torch.randn(petals, 3, generator=gen, dtype=torch.float64), dim=1)
    e = e / e.norm(dim=1, keepdim=True)
    a = d * math.cos(math.pi / 6) + e * math.sin(math.pi / 6)
    b = d * math.cos(math.pi / 6) - e * math.sin(math.pi / 6)
    rim = torch.stack([a, b], 1).reshape(-1, 3) * (1.0 + 0.1 * torch.rand(2 * petals, 1, generator=gen, dtype=torch.float64))
    verts = torch.cat([torch.tensor([[0.1, -0.2, 0.05]], dtype=torch.float64), rim + torch.tensor([0.1, -0.2, 0.05])], 0)
    i = torch.arange(petals)
    return verts.float().contiguous(), torch.stack([torch.zeros_like(i), 1 + 2 * i, 2 + 2 * i], 1).contiguous()


_CASES = {}


def cases():
    """{name: (verts_list, faces_list)}, built once and never modified."""
    if not _CASES:
        gen = torch.Generator().manual_seed(91)
        _CASES["batch"] = M.build_batch()
        ico = _jittered_ico(1, gen)
        line = torch.tensor([[0.0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [2, 1, 0]])
        _CASES["collinear"] = ([ico[0], line], [ico[1], torch.tensor([[0, 1, 2], [0, 1, 3], [1, 2, 4]])])
        twin = torch.tensor([[0.5, 0.25, 1.0], [0.5, 0.25, 1.0], [1.5, 0.25, 1.0]])
        _CASES["coincident"] = ([ico[0], twin], [ico[1], torch.tensor([[0, 1, 2]])])
        _CASES["fan200"] = tuple([x] for x in _fan(200, gen))
        _CASES["grid20"] = tuple([x] for x in M.jittered_grid(20, gen))
        _CASES["grid257"] = tuple([x] for x in M.jittered_grid(257, gen))
    return _CASES


def packed(verts_list, faces_list):
    """(verts (V, 3) float32, faces (F, 3) int64 in packed ids, [V_n], vert_mesh (V,) int64)."""
    nv = [int(v.shape[0]) for v in verts_list]
    base = np.cumsum([0] + nv[:-1]).tolist()
    faces = torch.cat([f.to(torch.int64) + b for f, b in zip(faces_list, base)], 0)
    vert_mesh = torch.repeat_interleave(torch.arange(len(nv)), torch.tensor(nv, dtype=torch.int64))
    return torch.cat(list(verts_list), 0), faces, nv, vert_mesh


def edges_of(faces, V):
    """The unique undirected edges (E, 2) int64, ascending by (lo, hi): the set of Meshes.edges_packed()."""
    a = torch.cat([faces[:, [1, 2]], faces[:, [2, 0]], faces[:, [0, 1]]], 0)
    key = torch.unique(a.amin(1) * max(V, 1) + a.amax(1))
    return torch.stack([key // max(V, 1), key % max(V, 1)], 1)


def depth(n):
    return M.depth(n)


# ---- the formulas ----------------------------------------------------------------------------------------------------------------------
def face_weights(x, faces, eps=EPS, over=4.0):
    """(cot (F, 3), area (F,)) in the dtype of x: per corner k (b^2 + c^2 - a^2) / area / 4 with a the side opposite the corner, the
    area by Heron's formula clamped at eps before the root."""
    v0, v1, v2 = x[faces[:, 0]], x[faces[:, 1]], x[faces[:, 2]]
    A, B, C = (v1 - v2).norm(dim=1), (v0 - v2).norm(dim=1), (v0 - v1).norm(dim=1)
    s = 0.5 * (A + B + C)
    area = (s * (s - A) * (s - B) * (s - C)).clamp(min=eps).sqrt()
    A2, B2, C2 = A * A, B * B, C * C
    return torch.stack([B2 + C2 - A2, A2 + C2 - B2, A2 + B2 - C2], 1) / area[:, None] / over, area


def _directed(faces):
    """Corner 3 f + k gives L[i, j] and L[j, i] with (i, j) the edge opposite it: rows i, columns j, the corner of every entry."""
    i, j = faces[:, [1, 2, 0]].reshape(-1), faces[:, [2, 0, 1]].reshape(-1)
    corner = torch.arange(faces.numel())
    return torch.cat([i, j]), torch.cat([j, i]), torch.cat([corner, corner])


def residual(method, x, faces, variant=None):
    """r (V, 3) of the loss in the dtype of x; L is a constant of the step.  variant: a deliberately WRONG formulation that the gates
    must refuse -- "cot_not_over_4", "plain_reciprocal", "cotcurv_without_rowsum"."""
    V = x.shape[0]
    with torch.no_grad():
        cot, area = face_weights(x, faces, over=1.0 if variant == "cot_not_over_4" else 4.0)
        row, col, corner = _directed(faces)
        val = cot.reshape(-1)[corner]
        rowsum = torch.zeros(V, dtype=x.dtype).index_add(0, row, val)[:, None]
    lx = torch.zeros_like(x).index_add(0, row, val[:, None] * x[col])
    if method == "cot":
        nw = 1.0 / rowsum if variant == "plain_reciprocal" else torch.where(rowsum > 0, 1.0 / rowsum, rowsum)
        return lx * nw - x
    with torch.no_grad():
        va = torch.zeros(V, dtype=x.dtype).index_add(0, faces.reshape(-1), area.repeat_interleave(3))[:, None]
        ia = torch.where(va > 0, 1.0 / va, va)
    if variant == "cotcurv_without_rowsum":
        return lx * (0.25 * ia)
    return (lx - rowsum * x) * (0.25 * ia)


def loss_terms(method, x, faces, nv, vert_mesh, variant=None):
    count = torch.tensor(nv, dtype=x.dtype)[vert_mesh]
    return residual(method, x, faces, variant).norm(dim=1) / count


def evaluate(method, verts, faces, nv, vert_mesh, grad_output=1.0, dtype=torch.float64, variant=None):
    """(loss, grad_verts of loss * grad_output, S = the sum of the absolute terms / N, the number of terms) by autograd in `dtype`."""
    x = verts.to(dtype).clone().requires_grad_(True)
    t = loss_terms(method, x, faces, nv, vert_mesh, variant)
    loss = t.sum() / len(nv)
    (g,) = torch.autograd.grad(loss * grad_output, x)
    return float(loss.detach()), g, float(t.detach().abs().sum()) / len(nv), int(t.numel())


def laplacian_entries(verts, faces, dtype=torch.float64):
    """cot_laplacian by the formulas: (row, col, val, mag, inv_areas) -- the coalesced directed entries ascending by (row, col), the
    sum of the absolute terms of each entry -- per corner (a^2 + b^2 + c^2) / area / 4: every term that is added or subtracted on the
    way to the entry, taken positive (a cotangent near 0 is a difference of squares that cancel) -- and inv_areas (V,)."""
    x = verts.to(dtype)
    V = x.shape[0]
    cot, area = face_weights(x, faces)
    row, col, corner = _directed(faces)
    key, inverse = torch.unique(row * max(V, 1) + col, return_inverse=True)
    term = cot.reshape(-1)[corner]
    val = torch.zeros(key.numel(), dtype=dtype).index_add(0, inverse, term)
    v0, v1, v2 = x[faces[:, 0]], x[faces[:, 1]], x[faces[:, 2]]
    squares = ((v1 - v2) ** 2).sum(1) + ((v0 - v2) ** 2).sum(1) + ((v0 - v1) ** 2).sum(1)
    mag = torch.zeros(key.numel(), dtype=dtype).index_add(0, inverse, (squares / area / 4.0).repeat_interleave(3)[corner])
    va = torch.zeros(V, dtype=dtype).index_add(0, faces.reshape(-1), area.repeat_interleave(3))
    return key // max(V, 1), key % max(V, 1), val, mag, torch.where(va > 0, 1.0 / va, va)


def laplacian_dense(verts, faces):
    """(L (V, V), inv_areas (V,)) in float64 by Python loops over the faces, straight from the definition."""
    x = verts.double()
    V = x.shape[0]
    L, va = torch.zeros((V, V), dtype=torch.float64), torch.zeros(V, dtype=torch.float64)
    for f in faces.tolist():
        p = [x[f[0]], x[f[1]], x[f[2]]]
        side = [float((p[1] - p[2]).norm()), float((p[0] - p[2]).norm()), float((p[0] - p[1]).norm())]
        s = 0.5 * (side[0] + side[1] + side[2])
        area = math.sqrt(max(s * (s - side[0]) * (s - side[1]) * (s - side[2]), EPS))
        for k in range(3):
            a, b, c = side[k], side[(k + 1) % 3], side[(k + 2) % 3]
            i, j = f[(k + 1) % 3], f[(k + 2) % 3]
            L[i, j] += (b * b + c * c - a * a) / area / 4.0
            L[j, i] += (b * b + c * c - a * a) / area / 4.0
            va[f[k]] += area
    return L, torch.where(va > 0, 1.0 / va, va)


def taubin(verts, edges, num_iter, lambd=LAMBD, mu=MU, dtype=torch.float64, variant=None):
    """taubin_smoothing by the formulas in `dtype`: per half-step w = 1 / (|x_i - x_j| + 1e-12) on every edge, both directions,
    x := (1 - c) x + (c L x) / (L 1).  variant "taubin_grouping": the WRONG grouping c (L x / L 1)."""
    x = verts.to(dtype)
    row, col = torch.cat([edges[:, 0], edges[:, 1]]), torch.cat([edges[:, 1], edges[:, 0]])
    for _ in range(num_iter):
        for c in (lambd, mu):
            w = 1.0 / ((x[row] - x[col]).norm(dim=1) + EPS)
            lx = torch.zeros_like(x).index_add(0, row, w[:, None] * x[col])
            tw = torch.zeros(x.shape[0], dtype=dtype).index_add(0, row, w)[:, None]
            x = (1 - c) * x + (c * (lx / tw) if variant == "taubin_grouping" else c * lx / tw)
    return x


def min_angles(verts, faces):
    """The smallest angle of every face in degrees, float64."""
    x = verts.double()
    out = []
    for k in range(3):
        a, b = x[faces[:, (k + 1) % 3]] - x[faces[:, k]], x[faces[:, (k + 2) % 3]] - x[faces[:, k]]
        out.append(torch.atan2(torch.cross(a, b, dim=1).norm(dim=1), (a * b).sum(1)))
    return torch.rad2deg(torch.stack(out, 1).amin(1))


def exact_degenerate(verts, faces):
    """Per face: Heron's product is exactly 0 in float32 and float64 and the coordinates lie on the lattice of multiples of 1 / 4."""
    out = []
    for dtype in (torch.float32, torch.float64):
        x = verts.to(dtype)
        v0, v1, v2 = x[faces[:, 0]], x[faces[:, 1]], x[faces[:, 2]]
        A, B, C = (v1 - v2).norm(dim=1), (v0 - v2).norm(dim=1), (v0 - v1).norm(dim=1)
        s = 0.5 * (A + B + C)
        out.append(s * (s - A) * (s - B) * (s - C) == 0)
    lattice = (verts[faces] * 4 == (verts[faces] * 4).round()).all(2).all(1)
    return out[0] & out[1] & lattice


# ---- the fixture and the gates ---------------------------------------------------------------------------------------------------------
_FIXTURE = {}


def fixture():
    if "z" not in _FIXTURE:
        _FIXTURE["z"] = dict(np.load(GOLDEN))
    return _FIXTURE["z"]


def e32(case, quantity):
    """The reference's own float32 error against the truth, recorded by the generator: quantity in loss_<method>, grad_<method>_<g>,
    L, inv_areas, taubin_<num_iter>."""
    return float(fixture()[f"{case}/e32_{quantity}"])


def nan_aware_error(got, want):
    """The largest |got - want| over the entries where `want` is a number; inf where the NaN patterns differ."""
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    if not torch.equal(torch.isnan(got), torch.isnan(want)):
        return float("inf")
    keep = ~torch.isnan(want)
    return float((got[keep] - want[keep]).abs().max()) if bool(keep.any()) else 0.0


_TRUTH = {}


def truth(case, method, grad_output=1.0):
    """evaluate(...) of a case in float64, computed once."""
    key = (case, method, grad_output)
    if key not in _TRUTH:
        verts, faces, nv, vert_mesh = packed(*cases()[case])
        _TRUTH[key] = evaluate(method, verts, faces, nv, vert_mesh, grad_output)
    return _TRUTH[key]


def loss_gates(case, method, grad_output=1.0):
    """(truth loss, truth grad, loss gate, grad gate, record): the gradient within 4 x the reference's float32 error, the loss within
    4 x its error plus D(n) 2^-24 S."""
    t_loss, t_grad, S, n = truth(case, method, grad_output)
    el, eg = e32(case, f"loss_{method}"), e32(case, f"grad_{method}_{grad_output:g}")
    rec = {"E32_loss": el, "E32_grad": eg, "S": S, "n": n, "D": depth(n)}
    return t_loss, t_grad, 4 * el + depth(n) * 2.0 ** -24 * S, 4 * eg, rec
