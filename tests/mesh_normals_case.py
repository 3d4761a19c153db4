"""The input and the float64 yardsticks of the vertex / face normal tests (tests/test_cpu_mesh_normals.py, tests/test_gpu_mesh_normals.py).

Input: one packed batch of four pieces --
  * ico_sphere(2) with 0.05 noise (162 vertices, 320 faces, valence 5 - 6),
  * torus(0.5, 1.0, 7, 9) (63 vertices, 126 faces),
  * a fan whose apex has valence 200 (201 vertices, 200 faces): one lane of the per-vertex kernel sums 200 rows,
  * an "eps group" of 7 vertices and 3 faces: two coincident faces of opposite winding, one collinear face, one isolated vertex.
    Its coordinates are small integers, so every difference and product is exact in float32 and every vertex sum is EXACTLY zero in
    any order: the max(|s|, 1e-6) branch, forward (normal 0) and backward (gradient g / 1e-6, a million times the others').
"""
import math

import torch

import _util as U

EPS = 1e-6


def build_input():
    """(verts (V, 3) float32, faces (F, 3) int64, eps (V,) bool: the vertices of the eps group)."""
    gen = torch.Generator().manual_seed(20)
    pieces = []
    v, f = U.ico_sphere(2)
    pieces.append((v + 0.05 * torch.randn(v.shape, generator=gen), f))
    v, f = U.torus(0.5, 1.0, 7, 9)
    pieces.append((v + torch.tensor([3.0, 0.0, 0.0]), f))
    n = 200
    ang = torch.arange(n, dtype=torch.float64) * (2 * math.pi / n)
    rim = torch.stack([torch.cos(ang), torch.sin(ang), torch.zeros(n, dtype=torch.float64)], 1).float()
    rim = rim * (1.0 + 0.2 * torch.rand(n, 1, generator=gen)) + 0.02 * torch.randn(n, 3, generator=gen)
    fan_v = torch.cat([torch.tensor([[0.0, 0.0, 0.6]]), rim], 0) + torch.tensor([0.0, 3.0, 0.0])
    k = torch.arange(n)
    fan_f = torch.stack([torch.zeros(n, dtype=torch.int64), 1 + k, 1 + (k + 1) % n], 1)
    pieces.append((fan_v, fan_f))
    eps_v = torch.tensor([[4.0, 4, 4], [5, 4, 4], [4, 6, 5],      # the two coincident faces
                          [8.0, 2, 2], [9, 2, 2], [11, 2, 2],     # collinear
                          [7.0, 7, 7]])                           # isolated
    eps_f = torch.tensor([[0, 1, 2], [0, 2, 1], [3, 4, 5]], dtype=torch.int64)
    pieces.append((eps_v, eps_f))
    verts, faces, base = [], [], 0
    for v, f in pieces:
        verts.append(v.float())
        faces.append(f + base)
        base += v.shape[0]
    verts, faces = torch.cat(verts, 0).contiguous(), torch.cat(faces, 0).contiguous()
    eps = torch.zeros(verts.shape[0], dtype=torch.bool)
    eps[-7:] = True
    return verts, faces, eps


def reference_verts_normals(verts, faces):
    """The reference's formulation (structures/meshes.py:899-926) in torch, any dtype: what autograd differentiates for the truth
    and what, in float32 on the CPU, sets the scale of the gates."""
    fv = verts[faces]
    fn = torch.cross(fv[:, 2] - fv[:, 1], fv[:, 0] - fv[:, 1], dim=1)
    s = torch.zeros_like(verts)
    for j in range(3):
        s = s.index_add(0, faces[:, j], fn)
    return torch.nn.functional.normalize(s, eps=EPS, dim=1)


def brute_incidence(faces, V):
    """(offsets, corners) as Python lists by the definition: per vertex, ascending, the corners 3 f + j that name it (a negative id
    wraps once, an id still out of range is dropped)."""
    per_vertex = [[] for _ in range(V)]
    for c, v in enumerate(faces.reshape(-1).tolist()):
        if v < 0:
            v += V
        if 0 <= v < V:
            per_vertex[v].append(c)
    offsets, corners = [0], []
    for lst in per_vertex:
        corners += lst
        offsets.append(len(corners))
    return offsets, corners


def restated_forward(verts, faces):
    """The kernels' forward formulas in the dtype of verts (float64 for the truth): face_raw = (v2 - v1) x (v0 - v1) per face, per
    vertex the sum over its corners in list order, normals = sums / max(|sums|, 1e-6).  Returns (normals, sums)."""
    V = verts.shape[0]
    offsets, corners = brute_incidence(faces, V)
    fv = verts[faces]
    raw = torch.cross(fv[:, 2] - fv[:, 1], fv[:, 0] - fv[:, 1], dim=1)
    sums = torch.zeros_like(verts)
    for v in range(V):
        for c in corners[offsets[v]:offsets[v + 1]]:
            sums[v] = sums[v] + raw[c // 3]
    norm = sums.norm(dim=1, keepdim=True)
    return sums / norm.clamp_min(EPS), sums


def restated_backward(grad_normals, verts, faces, sums):
    """The kernels' backward formulas: per vertex g_s = (g - n (n . g)) / |s| where |s| > 1e-6 and g / 1e-6 where not; per face G = the
    sum of its three g_s in corner order, a = v2 - v1, b = v0 - v1, grad_v2 = b x G, grad_v0 = G x a, grad_v1 = -(grad_v0 + grad_v2);
    per vertex the sum of its corners' rows in list order."""
    V = verts.shape[0]
    offsets, corners = brute_incidence(faces, V)
    norm = sums.norm(dim=1, keepdim=True)
    n = sums / norm.clamp_min(EPS)
    g_s = torch.where(norm > EPS, (grad_normals - n * (n * grad_normals).sum(1, keepdim=True)) / norm.clamp_min(EPS), grad_normals / EPS)
    G = g_s[faces[:, 0]] + g_s[faces[:, 1]] + g_s[faces[:, 2]]
    fv = verts[faces]
    a, b = fv[:, 2] - fv[:, 1], fv[:, 0] - fv[:, 1]
    g2, g0 = torch.cross(b, G, dim=1), torch.cross(G, a, dim=1)
    rows = torch.stack([g0, -(g0 + g2), g2], 1).reshape(-1, 3)
    out = torch.zeros_like(verts)
    for v in range(V):
        for c in corners[offsets[v]:offsets[v + 1]]:
            out[v] = out[v] + rows[c]
    return out


def autograd_truth(verts, faces, grad_normals):
    """float64: (normals, grad_verts) of the reference's formulation by torch autograd."""
    v = verts.double().clone().requires_grad_(True)
    n = reference_verts_normals(v, faces)
    (g,) = torch.autograd.grad(n, v, grad_normals.double())
    return n.detach(), g


# ---- vectorised restatements for meshes too large for the Python loops above (tests/test_*_loss_kernel_edges.py) -------------------------
def restated_forward_vectorised(verts, faces):
    """restated_forward without the loops, on the device of verts: the rows raw[c // 3] added per vertex by one index_add over the
    corners c = 3 f + j ascending (on the CPU that IS the list order, bit for bit; on the GPU the order is open, in float64)."""
    fv = verts[faces]
    raw = torch.cross(fv[:, 2] - fv[:, 1], fv[:, 0] - fv[:, 1], dim=1)
    sums = torch.zeros_like(verts).index_add(0, faces.reshape(-1), raw.repeat_interleave(3, 0))
    norm = sums.norm(dim=1, keepdim=True)
    return sums / norm.clamp_min(EPS), sums


def restated_backward_vectorised(grad_normals, verts, faces, sums):
    """restated_backward without the loops (the same remark on the order)."""
    norm = sums.norm(dim=1, keepdim=True)
    n = sums / norm.clamp_min(EPS)
    g_s = torch.where(norm > EPS, (grad_normals - n * (n * grad_normals).sum(1, keepdim=True)) / norm.clamp_min(EPS), grad_normals / EPS)
    G = g_s[faces[:, 0]] + g_s[faces[:, 1]] + g_s[faces[:, 2]]
    fv = verts[faces]
    a, b = fv[:, 2] - fv[:, 1], fv[:, 0] - fv[:, 1]
    g2, g0 = torch.cross(b, G, dim=1), torch.cross(G, a, dim=1)
    rows = torch.stack([g0, -(g0 + g2), g2], 1).reshape(-1, 3)
    return torch.zeros_like(verts).index_add(0, faces.reshape(-1), rows)


def face_areas_normals_restated(verts, faces):
    """(areas, normals) of the faces in the dtype of verts: c = (v1 - v0) x (v2 - v0), |c| / 2 and c / max(|c|, 1e-6)."""
    fv = verts[faces]
    c = torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1)
    norm = c.norm(dim=1)
    return norm / 2.0, c / norm.clamp_min(EPS)[:, None]


def face_areas_normals_backward_restated(grad_areas, grad_normals, verts, faces):
    """What the reference's backward returns on faces with |c| > 1e-6, in the dtype of verts: the derivative of
    face_areas_normals_restated by autograd, plus the ONE deviation the reference has (and a drop-in keeps): in d / d(v1.z) the term of
    grad_normal_y is multiplied by c_x where the derivative has c_y.  With s = d(c)/d(v1.z) . c = (e_z x b) . c, b = v2 - v0, that
    adds -grad_normal_y (c_x - c_y) s / |c|^3 to the z entry of the face's vertex 1."""
    v = verts.detach().clone().requires_grad_(True)
    areas, normals = face_areas_normals_restated(v, faces)
    (g,) = torch.autograd.grad([areas, normals], v, [grad_areas.to(v.dtype), grad_normals.to(v.dtype)])
    fv = verts[faces]
    b = fv[:, 2] - fv[:, 0]
    c = torch.cross(fv[:, 1] - fv[:, 0], b, dim=1)
    norm = c.norm(dim=1)
    ez = torch.zeros_like(b)
    ez[:, 2] = 1.0
    s = (torch.cross(ez, b, dim=1) * c).sum(1)
    extra = -grad_normals[:, 1].to(v.dtype) * (c[:, 0] - c[:, 1]) * s / norm ** 3
    return g.index_add(0, faces[:, 1], torch.stack([torch.zeros_like(extra), torch.zeros_like(extra), extra], 1))
