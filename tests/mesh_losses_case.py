"""The input and the yardsticks of the mesh-regulariser tests (tests/test_cpu_mesh_losses.py, tests/test_gpu_mesh_losses.py,
tests/shim_mesh_losses_case.py).

Input: one batch of five meshes, small and through every branch of pytorch3d_amd/mesh_losses.py and csrc/mesh_losses.hip --
  1. ico_sphere(2): 162 vertices, 320 faces, 480 edges, 480 wing pairs; closed; more than one block of 256 terms and more than one wave;
  2. an open 4 x 4 vertex grid of 18 triangles: 33 edges, the 12 on the boundary lie in one face and give no pair: 21 pairs;
  3. a "book": three triangles on one edge (that edge gives 3 pairs, the six others none) and one vertex that no face uses (deg = 0);
  4. an empty mesh, 0 vertices and 0 faces;
  5. ico_sphere(0) with its first face listed twice: 30 edges; the doubled face's three edges lie in 3 faces each: 27 + 3 * 3 = 36 pairs.
Vertices are jittered with a seeded generator.

Yardsticks: the tables by Python loops from the definition (brute_tables), each loss restated from the formulas of include/p3d_amd.h
in plain torch and differentiated by autograd in float64 on the CPU (truth), and the float32 formulation on the CPU whose own error
against that truth scales every gate (float32_formulation: the reference's Python where oracle/_ref/reference_py is staged -- run
once in a child process, the shim replaces sys.modules entries -- else the package's torch formulation).
"""
import json
import math
import os
import subprocess
import sys

import torch

import _util as U

STAGE = os.path.join(U.ROOT, "oracle", "_ref", "reference_py")
LOSSES = ("edge", "edge_target", "laplacian", "normal")
TARGET = 0.3  # the target length of the "edge_target" case
PAIRS_BY_HAND = {1: 21, 2: 3, 4: 36}  # meshes 2, 3 and 5 of the docstring (0-based index)
EDGES_BY_HAND = {0: 480, 1: 33, 2: 7, 3: 0, 4: 30}


def build_batch():
    """(verts_list, faces_list): float32 (V_n, 3) and int64 (F_n, 3) per mesh."""
    gen = torch.Generator().manual_seed(77)
    verts, faces = [], []
    v, f = U.ico_sphere(2)
    verts.append(v + 0.04 * torch.randn(v.shape, generator=gen))
    faces.append(f)
    g = torch.arange(4, dtype=torch.float32)
    grid = torch.stack([g.repeat_interleave(4), g.repeat(4), torch.zeros(16)], 1) * 0.5
    quads = [(4 * i + j, 4 * i + j + 1, 4 * (i + 1) + j, 4 * (i + 1) + j + 1) for i in range(3) for j in range(3)]
    verts.append(grid + 0.05 * torch.randn(grid.shape, generator=gen) + torch.tensor([3.0, 0.0, 0.0]))
    faces.append(torch.tensor([t for a, b, c, d in quads for t in ((a, b, c), (b, d, c))], dtype=torch.int64))
    book = torch.tensor([[0.0, 0, 0], [0, 1, 0], [1, 0.4, 0.1], [-0.6, 0.5, 0.8], [-0.5, 0.6, -0.9], [2.0, 2, 2]])
    verts.append(book + 0.03 * torch.randn(book.shape, generator=gen) + torch.tensor([0.0, 3.0, 0.0]))
    faces.append(torch.tensor([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=torch.int64))
    verts.append(torch.zeros((0, 3)))
    faces.append(torch.zeros((0, 3), dtype=torch.int64))
    v, f = U.ico_sphere(0)
    verts.append(0.7 * v + 0.05 * torch.randn(v.shape, generator=gen) + torch.tensor([0.0, 0.0, 3.0]))
    faces.append(torch.cat([f, f[:1]], 0))
    return [x.float().contiguous() for x in verts], [x.contiguous() for x in faces]


def build_with_a_mesh_of_vertices_alone():
    """(verts_list, faces_list): three vertices without a face (0 edges: the weight of that mesh is 1 / 0) in front of a jittered
    ico_sphere(0)."""
    gen = torch.Generator().manual_seed(78)
    v, f = U.ico_sphere(0)
    return [torch.rand(3, 3, generator=gen), (v + 0.05 * torch.randn(v.shape, generator=gen)).float()], [torch.zeros((0, 3), dtype=torch.int64), f]


def brute_tables(verts_list, faces_list):
    """The tables by the definition, as Python lists in packed vertex ids: edges [(lo, hi)] ascending with edge_mesh, adjacency
    (per vertex the ascending neighbours), pairs [(v0, v1, a, b)] -- edges ascending, then j, then i over the faces that hold the
    edge in the order of their corners 3 f + k -- with pair_mesh, and vert_mesh."""
    edges, edge_mesh, pairs, pair_mesh, vert_mesh, base = [], [], [], [], [], 0
    for n, (v, f) in enumerate(zip(verts_list, faces_list)):
        wings = {}
        for face in f.tolist():
            for k in range(3):
                a, b = face[(k + 1) % 3] + base, face[(k + 2) % 3] + base
                wings.setdefault((min(a, b), max(a, b)), []).append(face[k] + base)
        for lo, hi in sorted(wings):
            edges.append((lo, hi))
            edge_mesh.append(n)
            opp = wings[(lo, hi)]
            for j in range(len(opp)):
                for i in range(j):
                    pairs.append((lo, hi, opp[i], opp[j]))
                    pair_mesh.append(n)
        vert_mesh += [n] * v.shape[0]
        base += v.shape[0]
    adjacency = [[] for _ in range(base)]
    for lo, hi in edges:
        adjacency[lo].append(hi)
        adjacency[hi].append(lo)
    return {"edges": edges, "edge_mesh": edge_mesh, "pairs": pairs, "pair_mesh": pair_mesh, "vert_mesh": vert_mesh,
            "adjacency": [sorted(a) for a in adjacency], "N": len(verts_list), "V": base}


def depth(n):
    """D(n) of include/p3d_amd.h: the additions a term passes through in the kernels' sum of n terms."""
    return 8 + math.ceil(math.ceil(n / 256) / 256) + 8


def terms(name, verts, tables):
    """The per-element terms of a loss (already weighted by 1 / count of the element's mesh) from the formulas, in the dtype of verts."""
    N = tables["N"]
    long = lambda x: torch.tensor(x, dtype=torch.int64)  # noqa: E731
    count = lambda mesh: torch.bincount(long(mesh), minlength=N)[long(mesh)].to(verts.dtype)  # noqa: E731
    if name in ("edge", "edge_target"):
        e = long(tables["edges"]).reshape(-1, 2)
        d = verts[e[:, 0]] - verts[e[:, 1]]
        return ((d * d).sum(1).sqrt() - (TARGET if name == "edge_target" else 0.0)) ** 2 / count(tables["edge_mesh"])
    if name == "laplacian":
        row = long([v for v, a in enumerate(tables["adjacency"]) for _ in a])
        col = long([u for a in tables["adjacency"] for u in a])
        deg = torch.tensor([max(len(a), 1) for a in tables["adjacency"]], dtype=verts.dtype)
        r = torch.zeros_like(verts).index_add(0, row, verts[col]) / deg[:, None] - verts
        return r.norm(dim=1) / count(tables["vert_mesh"])
    p = long(tables["pairs"]).reshape(-1, 4)
    x0 = verts[p[:, 0]]
    e = verts[p[:, 1]] - x0
    n0 = torch.cross(e, verts[p[:, 2]] - x0, dim=1)
    n1 = -torch.cross(e, verts[p[:, 3]] - x0, dim=1)
    cos = ((n0 / n0.norm(dim=1, keepdim=True).clamp_min(1e-8)) * (n1 / n1.norm(dim=1, keepdim=True).clamp_min(1e-8))).sum(1)
    return (1 - cos) / count(tables["pair_mesh"])


def truth(name, verts, tables, grad_output=1.0):
    """float64 on the CPU: (loss, grad_verts of loss * grad_output, S = the sum of the absolute terms / N, the number of terms)."""
    v = verts.double().clone().requires_grad_(True)
    t = terms(name, v, tables)
    loss = t.sum() / tables["N"]
    (g,) = torch.autograd.grad(loss * grad_output, v)
    return float(loss.detach()), g, float(t.detach().abs().sum()) / tables["N"], int(t.numel())


def package_formulation(verts_list, faces_list, dtype=torch.float32, names=LOSSES + ("cot", "cotcurv")):
    """{loss name: (loss, grad)} of the package's torch formulation on the CPU (pytorch3d_amd/mesh_losses.py below its kernels)."""
    import pytorch3d_amd as p3d

    out = {}
    for name in names:
        v = [x.to(dtype).clone().requires_grad_(True) for x in verts_list]
        m = p3d.PackedMeshes(v, faces_list)
        if name in ("edge", "edge_target"):
            loss = p3d.mesh_edge_loss(m, TARGET if name == "edge_target" else 0.0)
        elif name == "normal":
            loss = p3d.mesh_normal_consistency(m)
        else:
            loss = p3d.mesh_laplacian_smoothing(m, "uniform" if name == "laplacian" else name)
        grads = torch.autograd.grad(loss, v)
        out[name] = (float(loss.detach()), torch.cat(list(grads), 0))
    return out


_REFERENCE = {}


def reference_formulation():
    """{loss name: (loss, grad)} of the reference's own Python in float32 on the CPU, its `edges_packed()` under "edges_packed"; None
    where oracle/_ref/reference_py is not staged.  One child process per test session."""
    if "got" not in _REFERENCE:
        got = None
        if os.path.isdir(os.path.join(STAGE, "pytorch3d", "loss")):
            res = subprocess.run([sys.executable, os.path.join(U.ROOT, "tests", "shim_mesh_losses_case.py"), "--cpu-reference"],
                                 capture_output=True, text=True, timeout=300)
            assert res.returncode == 0, res.stderr[-3000:]
            rec = json.loads(res.stdout.strip().splitlines()[-1])
            if "skipped" not in rec:
                got = {k: (v["loss"], torch.tensor(v["grad"], dtype=torch.float32).reshape(-1, 3)) for k, v in rec["losses"].items()}
                got["edges_packed"] = rec["edges_packed"]
        _REFERENCE["got"] = got
    return _REFERENCE["got"]


def float32_formulation(verts_list, faces_list):
    """The float32 formulation on the CPU that scales the gates: the reference's where it is staged, else the package's."""
    ref = reference_formulation()
    return ref if ref is not None else package_formulation(verts_list, faces_list)


def gates(name, verts_list, faces_list, tables, grad_output=1.0, f32=None):
    """(truth loss, truth grad, loss gate, grad gate, record) of one loss on a batch: the gradient within 4 x the float32
    formulation's own largest error, the loss within 4 x its error plus D(n) 2^-24 S.  f32: the float32 formulation's results when
    the batch is not build_batch()'s (package_formulation(verts_list, faces_list))."""
    verts = torch.cat(verts_list, 0)
    t_loss, t_grad, S, n = truth(name, verts, tables, grad_output)
    f_loss, f_grad = (f32 if f32 is not None else float32_formulation(verts_list, faces_list))[name]
    e32_loss = abs(f_loss - t_loss)
    e32_grad = float((f_grad.double() * grad_output - t_grad).abs().max())
    rec = {"E32_loss": e32_loss, "E32_grad": e32_grad, "S": S, "n": n, "D": depth(n)}
    return t_loss, t_grad, 4 * e32_loss + depth(n) * 2.0 ** -24 * S, 4 * e32_grad, rec


# ---- larger generated meshes and the vectorised restatements they need (tests/test_*_loss_kernel_edges.py) --------------------------------
SUM_CAP = 256 * 256          # terms the first round of segment_sum_kernel (csrc/fixed_sum.h) covers: one partial per 256 terms, 256 lanes
STREAM_CAP = 256 * 16 * 256  # items one pass of a grid-stride loop covers (csrc/p3d_common.h: stream_blocks, 4 096 blocks of 256 threads)


def jittered_grid(n, gen, spacing=0.1, jitter=0.2):
    """An open n x n vertex grid in the plane z = 0, `spacing` apart, every coordinate moved by up to jitter / 2 of the spacing:
    (verts (n n, 3) float32, faces (2 (n - 1)^2, 3) int64).  n^2 vertices, 2 (n - 1)^2 faces, 3 (n - 1)^2 + 2 (n - 1) edges,
    3 (n - 1)^2 - 2 (n - 1) wing pairs."""
    g = torch.arange(n, dtype=torch.float32)
    verts = torch.stack([g.repeat_interleave(n), g.repeat(n), torch.zeros(n * n)], 1)
    verts = (verts + jitter * (torch.rand(n * n, 3, generator=gen) - 0.5)) * spacing
    i, j = torch.arange(n - 1).repeat_interleave(n - 1), torch.arange(n - 1).repeat(n - 1)
    a = i * n + j
    b, c, d = a + 1, a + n, a + n + 1
    faces = torch.stack([torch.stack([a, b, c], 1), torch.stack([b, d, c], 1)], 1).reshape(-1, 3)
    return verts.float().contiguous(), faces.contiguous()


def second_round_batch():
    """ico_sphere(1) and a 257 x 257 grid: 66 049 + 42 vertices, 197 120 + 120 edges, 196 096 + 120 pairs -- each count beyond the
    65 536 terms of the first round of the partial sums."""
    gen = torch.Generator().manual_seed(79)
    v, f = U.ico_sphere(1)
    gv, gf = jittered_grid(257, gen)
    return [(v + 0.03 * torch.randn(v.shape, generator=gen)).float().contiguous(), gv], [f.contiguous(), gf]


def second_pass_mesh(n=1025):
    """One n x n grid; at 1025: 1 050 625 vertices, 2 097 152 faces, 3 147 776 edges, 3 143 680 pairs -- the smallest at which the loops
    over faces, vertices, edges and pairs all take a second pass."""
    return jittered_grid(n, torch.Generator().manual_seed(80))


def tensor_tables(verts_list, faces_list, device="cpu"):
    """brute_tables as int64 tensors on `device`, by sorting instead of Python loops: edges (E, 2), edge_mesh, pairs (P, 4), pair_mesh,
    vert_mesh, the adjacency as (adj_row, adj_col) ascending by (vertex, neighbour), N, V."""
    nv = torch.tensor([v.shape[0] for v in verts_list], dtype=torch.int64)
    base = torch.cumsum(nv, 0) - nv
    faces = torch.cat([f.to(torch.int64) + int(b) for f, b in zip(faces_list, base)], 0).to(device)
    V, N = int(nv.sum()), len(verts_list)
    vert_mesh = torch.repeat_interleave(torch.arange(N), nv).to(device)
    # corner 3 f + k: the edge opposite vertex k of face f and that vertex as its wing
    lo = torch.minimum(faces[:, [1, 2, 0]], faces[:, [2, 0, 1]]).reshape(-1)
    hi = torch.maximum(faces[:, [1, 2, 0]], faces[:, [2, 0, 1]]).reshape(-1)
    wing = faces.reshape(-1)
    order = torch.sort(lo * V + hi, stable=True).indices  # the corners by edge, 3 f + k ascending inside an edge
    lo, hi, wing = lo[order], hi[order], wing[order]
    first = torch.ones_like(lo, dtype=torch.bool)
    first[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    start = torch.nonzero(first).squeeze(1)               # where each edge's corners begin
    count = torch.cat([start[1:], start.new_tensor([lo.numel()])]) - start
    edges = torch.stack([lo[start], hi[start]], 1)
    edge_mesh = vert_mesh[edges[:, 0]]
    # pairs (i < j) of an edge's corners: edges ascending, then j, then i
    rows = []
    for j in range(1, int(count.max()) if count.numel() else 0):
        has = torch.nonzero(count > j).squeeze(1)
        for i in range(j):
            rows.append(torch.stack([has, torch.full_like(has, j), torch.full_like(has, i)], 1))
    if rows:
        r = torch.cat(rows, 0)
        r = r[torch.sort((r[:, 0] * 64 + r[:, 1]) * 64 + r[:, 2]).indices]
        e = r[:, 0]
        pairs = torch.stack([edges[e, 0], edges[e, 1], wing[start[e] + r[:, 2]], wing[start[e] + r[:, 1]]], 1)
    else:
        e, pairs = start.new_zeros((0,)), start.new_zeros((0, 4))
    src, dst = torch.cat([edges[:, 0], edges[:, 1]]), torch.cat([edges[:, 1], edges[:, 0]])
    by_vertex = torch.sort(src * V + dst).indices
    return {"edges": edges, "edge_mesh": edge_mesh, "pairs": pairs, "pair_mesh": edge_mesh[e], "vert_mesh": vert_mesh,
            "adj_row": src[by_vertex], "adj_col": dst[by_vertex], "N": N, "V": V}


def terms_vectorised(name, verts, tt):
    """terms() from tensor_tables, on the device of verts: the same formulas, the same order of the operations."""
    N, V = tt["N"], tt["V"]
    count = lambda mesh: torch.bincount(mesh, minlength=N)[mesh].to(verts.dtype)  # noqa: E731
    if name in ("edge", "edge_target"):
        e = tt["edges"]
        d = verts[e[:, 0]] - verts[e[:, 1]]
        return ((d * d).sum(1).sqrt() - (TARGET if name == "edge_target" else 0.0)) ** 2 / count(tt["edge_mesh"])
    if name == "laplacian":
        deg = torch.bincount(tt["adj_row"], minlength=V).clamp_min(1).to(verts.dtype)
        r = torch.zeros_like(verts).index_add(0, tt["adj_row"], verts[tt["adj_col"]]) / deg[:, None] - verts
        return r.norm(dim=1) / count(tt["vert_mesh"])
    p = tt["pairs"]
    x0 = verts[p[:, 0]]
    e = verts[p[:, 1]] - x0
    n0 = torch.cross(e, verts[p[:, 2]] - x0, dim=1)
    n1 = -torch.cross(e, verts[p[:, 3]] - x0, dim=1)
    cos = ((n0 / n0.norm(dim=1, keepdim=True).clamp_min(1e-8)) * (n1 / n1.norm(dim=1, keepdim=True).clamp_min(1e-8))).sum(1)
    return (1 - cos) / count(tt["pair_mesh"])


def truth_vectorised(name, verts, tt, grad_output=1.0):
    """truth() from tensor_tables, float64 on the device of the tables."""
    v = verts.to(tt["edges"].device).double().clone().requires_grad_(True)
    t = terms_vectorised(name, v, tt)
    loss = t.sum() / tt["N"]
    (g,) = torch.autograd.grad(loss * grad_output, v)
    return float(loss.detach()), g.cpu(), float(t.detach().abs().sum()) / tt["N"], int(t.numel())


def gates_vectorised(name, verts_list, tt, f32, grad_output=1.0):
    """gates() with truth_vectorised; f32: package_formulation(verts_list, faces_list) of the batch."""
    t_loss, t_grad, S, n = truth_vectorised(name, torch.cat(verts_list, 0), tt, grad_output)
    f_loss, f_grad = f32[name]
    e32_loss = abs(f_loss - t_loss)
    e32_grad = float((f_grad.double() * grad_output - t_grad).abs().max())
    rec = {"E32_loss": e32_loss, "E32_grad": e32_grad, "S": S, "n": n, "D": depth(n)}
    return t_loss, t_grad, 4 * e32_loss + depth(n) * 2.0 ** -24 * S, 4 * e32_grad, rec
