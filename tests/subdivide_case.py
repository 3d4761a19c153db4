"""The inputs and the yardstick of the subdivision tests: named batches of meshes at the smallest shapes at which csrc/mesh_edges.hip
and csrc/subdivide.hip can go wrong (the fans and the scan case sized from the header's constants), and `restate`, the contract in
plain loops.  tests/golden/subdivide_ref.npz records the reference's CPU results for the same batches."""
import os

import numpy as np
import torch

import _util as U
from pytorch3d_amd import _lib

GOLDEN = os.path.join(U.ROOT, "tests", "golden", "subdivide_ref.npz")
REGS, LDS, ITEMS = _lib.MESH_EDGES_ROW_REGISTERS, _lib.MESH_EDGES_ROW_LDS, _lib.MESH_EDGES_ITEMS
FEATS_D = 5
TETRA = [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]


def _fan(entries):
    """A fan around vertex 0 whose row of corners with lo == 0 has `entries` entries: two per face, and three from one face that names
    the hub twice where the number is odd."""
    k = (entries - 3) // 2 if entries % 2 else entries // 2
    faces = [[0, i, i + 1] for i in range(1, k + 1)] + ([[0, 0, k + 1]] if entries % 2 else [])
    return k + 2, faces


def _strip(V):
    """A triangle strip over V vertices: E = 2 V - 3."""
    return V, [[i, i + 1, i + 2] if i % 2 == 0 else [i + 1, i, i + 2] for i in range(V - 2)]


def _topologies():
    ico_v, ico_f = U.ico_sphere(2)
    strip = _strip(ITEMS // 2 + 6)  # 2 V rows: just past two scan blocks' boundary, so the carry is used, and E past one block
    return {
        "triangle": [(3, [[0, 1, 2]])],
        "tetrahedron": [(4, TETRA)],
        "tetrahedron_flipped": [(4, TETRA[:3] + [[1, 2, 3]])],
        "three_on_an_edge": [(5, [[0, 1, 2], [1, 0, 3], [0, 1, 4]])],
        "vertex_twice": [(4, [[0, 1, 2], [2, 2, 3], [3, 1, 1]])],
        "vertex_in_no_face": [(6, [[0, 1, 3], [3, 1, 5]])],
        "batch_of_4": [(4, TETRA), (5, [[0, 1, 2], [2, 1, 4]]), (0, []), _strip(9)],
        "ico_sphere_2": [(ico_v.shape[0], ico_f.tolist())],
        "fan_regs": [_fan(REGS)],
        "fan_regs_plus_1": [_fan(REGS + 1)],
        "fan_lds": [_fan(LDS)],
        "fan_lds_plus_1": [_fan(LDS + 1)],
        "scan_carry": [strip, (4, TETRA)],
    }


LONG_ROWS = {"fan_regs": (0, 0), "fan_regs_plus_1": (1, 0), "fan_lds": (1, 0), "fan_lds_plus_1": (1, 1)}  # what the build must report


def cases():
    return list(_topologies())


def inputs(name, device="cpu", dtype=torch.float32):
    """(verts_list, faces_list, feats (V, FEATS_D)) of a case: seeded vertices and features, int64 faces."""
    gen = torch.Generator().manual_seed(cases().index(name) + 11)
    meshes = _topologies()[name]
    verts = [torch.randn((V, 3), generator=gen).to(device=device, dtype=dtype) for V, _ in meshes]
    faces = [torch.tensor(f, dtype=torch.int64).reshape(-1, 3).to(device) for _, f in meshes]
    feats = torch.randn((sum(V for V, _ in meshes), FEATS_D), generator=gen).to(device=device, dtype=dtype)
    return verts, faces, feats


def restate(verts, faces, feats=None):
    """The contract in loops -> dict of edges (E, 2), face_edges (F, 3), num_edges (N,), new_verts [per mesh], new_faces [per mesh, local
    ids], new_feats (V + E, D) or None.  Floats stay in the dtype given: a midpoint is one addition and one halving."""
    first, packed = [0], []
    for v, f in zip(verts, faces):
        packed += [[int(i) + first[-1] for i in row] for row in f.tolist()]
        first.append(first[-1] + v.shape[0])
    V = first[-1]
    opposite = lambda row, k: tuple(sorted((row[(k + 1) % 3], row[(k + 2) % 3])))  # noqa: E731
    edges = sorted({opposite(row, k) for row in packed for k in range(3)}, key=lambda e: e[0] * V + e[1])
    ids = {e: i for i, e in enumerate(edges)}
    face_edges = [[ids[opposite(row, k)] for k in range(3)] for row in packed]
    mesh_of = lambda v: max(n for n in range(len(verts)) if first[n] <= v)  # noqa: E731
    num_edges = [0] * len(verts)
    for lo, _ in edges:
        num_edges[mesh_of(lo)] += 1
    x = torch.cat(list(verts), 0) if verts else torch.zeros((0, 3))
    new_verts, new_faces, new_feats, e0, f0 = [], [], [], 0, 0
    for n, (v, f) in enumerate(zip(verts, faces)):
        mine = edges[e0:e0 + num_edges[n]]
        mid = lambda t: [(t[lo] + t[hi]) * 0.5 for lo, hi in mine]  # noqa: E731
        new_verts.append(torch.stack(list(v) + mid(x), 0) if v.shape[0] else v)
        if feats is not None:
            new_feats += list(feats[first[n]:first[n + 1]]) + mid(feats)
        Vn, blocks = v.shape[0], [[], [], [], []]
        for j, row in enumerate(f.tolist()):
            e = [Vn + face_edges[f0 + j][k] - e0 for k in range(3)]
            for k, block in enumerate(([row[0], e[2], e[1]], [row[1], e[0], e[2]], [row[2], e[1], e[0]], e)):
                blocks[k].append(block)
        new_faces.append(torch.tensor(sum(blocks, []), dtype=torch.int64).reshape(-1, 3))
        e0, f0 = e0 + num_edges[n], f0 + f.shape[0]
    return {"edges": torch.tensor(edges, dtype=torch.int64).reshape(-1, 2), "face_edges": torch.tensor(face_edges, dtype=torch.int64).reshape(-1, 3),
            "num_edges": torch.tensor(num_edges, dtype=torch.int64), "new_verts": new_verts, "new_faces": new_faces,
            "new_feats": None if feats is None else (torch.stack(new_feats, 0) if new_feats else feats[:0])}


def expected(name):
    """The reference's recorded CPU results of a case, in the layout of `restate`."""
    with np.load(GOLDEN) as z:
        get = lambda key: torch.from_numpy(z[f"{name}/{key}"])  # noqa: E731
        nv, nf = get("new_num_verts").tolist(), get("new_num_faces").tolist()
        return {"edges": get("edges"), "face_edges": get("face_edges"), "num_edges": get("num_edges"),
                "new_verts": list(get("new_verts").split(nv, 0)), "new_faces": list(get("new_faces").split(nf, 0)), "new_feats": get("new_feats")}


def misses(got, want, tag=""):
    """The keys at which two results in the layout of `restate` differ (torch.equal and the dtype)."""
    def same(a, b):
        return (a is None and b is None) or (a is not None and b is not None and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu()))

    out = []
    for key, w in want.items():
        g = got[key]
        ok = len(g) == len(w) and all(same(a, b) for a, b in zip(g, w)) if isinstance(w, list) else same(g, w)
        out += [] if ok else [f"{tag}:{key}"]
    return out


def backward_truth(verts, faces, g):
    """(grad (V, D) float64, bound (V, D)) of the subdivision's backward for the output gradient g (V + E, D): grad_x[v] = g[row(v)] +
    0.5 sum g[row(e)] over the edges that name v (a self edge twice), and the bound (deg + 1) 2^-24 (|g_v| + 0.5 sum |g_e|): one rounding
    per addition of deg + 1 terms."""
    r = restate(verts, faces)
    V, D, g = sum(v.shape[0] for v in verts), g.shape[1], g.double().cpu()
    grad, mag, deg = torch.zeros((V, D), dtype=torch.float64), torch.zeros((V, D), dtype=torch.float64), torch.zeros((V, 1), dtype=torch.float64)
    v0 = e0 = row = 0
    for n, v in enumerate(verts):
        Vn, En = v.shape[0], int(r["num_edges"][n])
        grad[v0:v0 + Vn] += g[row:row + Vn]
        mag[v0:v0 + Vn] += g[row:row + Vn].abs()
        for j, (lo, hi) in enumerate(r["edges"][e0:e0 + En].tolist()):
            for end in (lo, hi):
                grad[end] += 0.5 * g[row + Vn + j]
                mag[end] += 0.5 * g[row + Vn + j].abs()
                deg[end] += 1
        v0, e0, row = v0 + Vn, e0 + En, row + Vn + En
    return grad, (deg + 1) * 2.0 ** -24 * mag
