"""Shared cases of the sample_points_from_meshes tests (tests/test_cpu_sample_points.py, tests/test_gpu_sample_points.py and
tests/golden/make_golden_sample_points.py): the inputs, and the contract of pytorch3d_amd/sample_points.py restated in float64 numpy
-- areas from the float32 vertices, the per-mesh cumulative table, the upper-bound choice, the barycentric weights, samples, normals,
and the gradients on GIVEN indices and weights.  Nothing of the package is imported here.
"""
import math
import os
import sys

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_points_ref.npz")
EPS = sys.float_info.epsilon  # the sampler normal's clamp (sample_points_from_meshes.py:120-122), not face_areas_normals' 1e-6
SAMPLE_COUNTS = (1, 63, 64, 65, 257)
SCAN_BLOCK = 256  # csrc/sample_points.hip: kScanBlock -- faces per block of level 1, block records per round of level 2


def scan_depth(F):
    """D(F) of csrc/sample_points.hip / include/p3d_amd.h: the additions a term of the table passes through at most."""
    return 19 + 4 * math.ceil(math.ceil(max(F, 1) / SCAN_BLOCK) / SCAN_BLOCK)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _soup(gen, V, F):
    """F faces over V random vertices, every face three different vertices."""
    verts = (torch.rand(V, 3, generator=gen) * 2 - 1).float()
    a = torch.randint(0, V, (F,), generator=gen)
    b = (a + 1 + torch.randint(0, V - 2, (F,), generator=gen)) % V
    c = torch.where((a + 1) % V == b, (a + 2) % V, (a + 1) % V)
    return verts, torch.stack([a, b, c], 1).long()


def ragged_batch(seed=11):
    """Five meshes (lists of verts (V_i, 3) f32 and faces (F_i, 3) i64 with local ids): one face; 70 faces; an EMPTY mesh in the middle;
    300 faces with faces of exactly zero area (a vertex named twice) at the start, in the middle and at the END of its range; a mesh
    whose faces are all degenerate."""
    gen = torch.Generator().manual_seed(seed)
    v0 = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.25, 0.0], [0.25, 1.5, 0.5]])
    f0 = torch.tensor([[0, 1, 2]])
    v1, f1 = _soup(gen, 40, 70)
    v2, f2 = torch.rand(3, 3, generator=gen), torch.zeros((0, 3), dtype=torch.int64)
    v3, f3 = _soup(gen, 120, 300)
    for f in (0, 1, 2, 140, 141, 150, 297, 298, 299):
        f3[f, 1] = f3[f, 0]
    v4 = torch.rand(6, 3, generator=gen)
    f4 = torch.tensor([[0, 0, 1], [2, 3, 2], [4, 4, 4], [5, 1, 5], [1, 1, 2]])  # (an edge is the zero vector: area 0 in any arithmetic)
    return [v0, v1, v2, v3, v4], [f0, f1, f2, f3, f4]


def pack(verts_list, faces_list):
    """-> (verts_packed, faces_packed, first_idx (N,), num_faces (N,)) as a packed batch has them."""
    nv = torch.tensor([v.shape[0] for v in verts_list], dtype=torch.int64)
    nf = torch.tensor([f.shape[0] for f in faces_list], dtype=torch.int64)
    v_first, f_first = torch.cumsum(nv, 0) - nv, torch.cumsum(nf, 0) - nf
    return (torch.cat(verts_list, 0).float(), torch.cat([f + int(o) for f, o in zip(faces_list, v_first)], 0).long(), f_first, nf)


def areas_mesh(ratio=1000.0, seed=3):
    """One mesh of 12 separate right triangles whose areas span 1 : ratio geometrically, in shuffled order."""
    gen = torch.Generator().manual_seed(seed)
    areas = torch.tensor([ratio ** (k / 11.0) for k in range(12)], dtype=torch.float64)[torch.randperm(12, generator=gen)]
    verts, faces = [], []
    for k, a in enumerate(areas.tolist()):
        s = math.sqrt(2.0 * a) * 0.05
        o = torch.tensor([float(k), 0.5 * k, -0.25 * k])
        verts += [o, o + torch.tensor([s, 0.0, 0.0]), o + torch.tensor([0.0, s, 0.0])]
        faces.append([3 * k, 3 * k + 1, 3 * k + 2])
    return torch.stack(verts).float(), torch.tensor(faces, dtype=torch.int64)


def uniforms(N, S, seed):
    """(N, S, 3) float32 in [0, 1) from a seeded CPU generator."""
    return torch.rand((N, S, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


# ---- the contract in float64 -------------------------------------------------------------------------------------------------------
def areas64(verts, faces):
    v = verts.double().numpy()[faces.numpy()]
    return np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1) / 2.0


def tables64(areas, first, nf):
    """[the inclusive prefix sum of mesh n's areas] for every mesh (an empty array for an empty mesh)."""
    return [np.cumsum(np.asarray(areas, dtype=np.float64)[int(a):int(a) + int(n)]) for a, n in zip(first.tolist(), nf.tolist())]


def last_positive(row):
    """Position of the last face of non-zero area of a table row (-1 for none): the last place where the table steps up."""
    step = np.diff(np.concatenate([[0.0], np.asarray(row, dtype=np.float64)])) > 0
    return int(np.nonzero(step)[0][-1]) if step.any() else -1


def choose(rows, first, u0, lower_bound=False, dtype=np.float64):
    """sample_face_idxs (N, S): per mesh the first face whose table entry is ABOVE t = u0 * total (the upper bound: a face of zero area
    is never taken), clamped to the last face of non-zero area; -1 for an empty mesh and for a total that is zero or not finite.
    dtype: the precision of the product t (np.float32 to re-do a float32 table's choice exactly).  lower_bound: the WRONG rule (the
    first entry at or above t), for the tests that show the gates reject it."""
    u0 = np.asarray(u0)
    out = np.full(u0.shape, -1, dtype=np.int64)
    for n, row in enumerate(rows):
        row = np.asarray(row)
        if row.size == 0 or not np.isfinite(row[-1]) or not row[-1] > 0:
            continue
        t = (u0[n].astype(dtype) * dtype(row[-1])).astype(row.dtype)
        local = np.searchsorted(row, t, side="left" if lower_bound else "right")
        out[n] = int(first[n]) + np.minimum(local, last_positive(row))
    return out


def weights64(u):
    u = np.asarray(u, dtype=np.float64)
    r = np.sqrt(u[..., 1])
    return np.stack([1.0 - r, r * (1.0 - u[..., 2]), r * u[..., 2]], -1)


def samples64(verts, faces, idx, w):
    """(N, S, 3): sum_k w_k v_k of the chosen face; zeros where idx is -1."""
    fv = verts.double().numpy()[faces.numpy()[np.maximum(idx, 0)]]  # (N, S, 3, 3)
    return np.where((idx >= 0)[..., None], (np.asarray(w, dtype=np.float64)[..., None] * fv).sum(-2), 0.0)


def face_normals64(verts, faces, eps=EPS):
    v = verts.double().numpy()[faces.numpy()]
    c = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 1])
    return c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), eps)


def normals64(verts, faces, idx, eps=EPS):
    return np.where((idx >= 0)[..., None], face_normals64(verts, faces, eps)[np.maximum(idx, 0)], 0.0)


def textures64(features, faces, idx, w):
    """(N, S, C): the per-vertex features (V, C) interpolated with the weights."""
    fa = features.double().numpy()[faces.numpy()[np.maximum(idx, 0)]]  # (N, S, 3, C)
    return np.where((idx >= 0)[..., None], (np.asarray(w, dtype=np.float64)[..., None] * fa).sum(-2), 0.0)


def grads64(verts, faces, idx, w, grad_samples=None, grad_normals=None, eps=EPS):
    """grad_verts (V, 3) float64 with the face choice and the weights held fixed.  Returns (grad, scale): scale (V, 3) is the sum of
    the absolute per-sample terms (with the Jacobian's entries taken absolute for the normals)."""
    V, fc = verts.shape[0], faces.numpy()
    v = verts.double().numpy()[fc]
    idx, w = np.asarray(idx).reshape(-1), np.asarray(w, dtype=np.float64).reshape(-1, 3)
    hit = idx >= 0
    per_face = np.zeros((fc.shape[0], 3, 3))
    per_face_abs = np.zeros((fc.shape[0], 3, 3))
    if grad_samples is not None:
        gs = np.asarray(grad_samples, dtype=np.float64).reshape(-1, 3)
        terms = w[hit][:, :, None] * gs[hit][:, None, :]  # (hits, 3 corners, 3)
        np.add.at(per_face, idx[hit], terms)
        np.add.at(per_face_abs, idx[hit], np.abs(terms))
    if grad_normals is not None:
        gn = np.asarray(grad_normals, dtype=np.float64).reshape(-1, 3)
        G, Gabs = np.zeros((fc.shape[0], 3)), np.zeros((fc.shape[0], 3))
        np.add.at(G, idx[hit], gn[hit])
        np.add.at(Gabs, idx[hit], np.abs(gn[hit]))
        a, b = v[:, 1] - v[:, 0], v[:, 2] - v[:, 1]
        c = np.cross(a, b)
        norm = np.linalg.norm(c, axis=1, keepdims=True)
        clamped = norm < eps
        n = c / np.maximum(norm, eps)
        safe = np.maximum(norm, eps)
        gc = np.where(clamped, G / eps, (G - n * (n * G).sum(1, keepdims=True)) / safe)
        ga, gb = np.cross(b, gc), np.cross(gc, a)
        per_face += np.stack([-ga, ga - gb, gb], 1)
        # the scale: |dL/dc| <= 2 |G|_1 / |c| per entry, crossed with the edges' absolute values
        gca = np.where(clamped, Gabs / eps, 2.0 * Gabs.sum(1, keepdims=True) / safe)
        edge = np.abs(a).sum(1, keepdims=True) + np.abs(b).sum(1, keepdims=True)
        per_face_abs += (edge * gca.sum(1, keepdims=True))[:, None, :] * np.ones((1, 3, 1))
    grad, scale = np.zeros((V, 3)), np.zeros((V, 3))
    np.add.at(grad, fc.reshape(-1), per_face.reshape(-1, 3))
    np.add.at(scale, fc.reshape(-1), per_face_abs.reshape(-1, 3))
    return grad, scale


def formulation_grads32(verts, faces, idx, w, grad_samples=None, grad_normals=None, eps=EPS):
    """The same gradient by the float32 torch chain on the CPU (gathers, the reference's normal expression, autograd's index_put):
    the formulation whose own error against grads64 sets the tolerance of a gradient test (four times it)."""
    x = verts.float().clone().requires_grad_(True)
    idx_t = torch.as_tensor(np.asarray(idx)).long()
    hit = (idx_t >= 0)[..., None]
    f = faces[idx_t.clamp_min(0)]
    wt = torch.as_tensor(np.asarray(w)).float()
    total = x.sum() * 0
    if grad_samples is not None:
        s = (wt[..., 0:1] * x[f[..., 0]] + wt[..., 1:2] * x[f[..., 1]]) + wt[..., 2:3] * x[f[..., 2]]
        total = total + (torch.where(hit, s, s.new_zeros(())) * torch.as_tensor(np.asarray(grad_samples)).float()).sum()
    if grad_normals is not None:
        fv = x[faces]
        n = torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 1], dim=1)
        n = n / n.norm(dim=1, p=2, keepdim=True).clamp(min=eps)
        total = total + (torch.where(hit, n[idx_t.clamp_min(0)], n.new_zeros(())) * torch.as_tensor(np.asarray(grad_normals)).float()).sum()
    total.backward()
    return x.grad.double().numpy()


def formulation_normals32(verts, faces, idx, eps=EPS):
    """The reference's float32 expression of the sampler normal on the CPU (sample_points_from_meshes.py:119-123), on given indices."""
    fv = verts.float()[faces]
    n = torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 1], dim=1)
    n = n / n.norm(dim=1, p=2, keepdim=True).clamp(min=eps)
    idx_t = torch.as_tensor(np.asarray(idx)).long()
    return torch.where((idx_t >= 0)[..., None], n[idx_t.clamp_min(0)], n.new_zeros(())).numpy()


def formulation_weights32(u):
    """The reference's _rand_barycentric_coords in IEEE float32, one operation each: what the torch formulation computes.  The root is
    taken in float64 and rounded, which IS the correctly rounded float32 root (53 >= 2 x 24 + 2 bits): torch's own float32 sqrt on the
    CPU returns a neighbour of it for about one input in a hundred (seen: 1 ulp either way, other inputs on other hosts), so it cannot
    pin bits."""
    u = np.asarray(u, dtype=np.float32)
    r = np.sqrt(u[..., 1].astype(np.float64)).astype(np.float32)
    one = np.float32(1.0)
    return np.stack([one - r, r * (one - u[..., 2]), r * u[..., 2]], -1).astype(np.float32)


def formulation_textures32(features, faces, idx, w):
    fa = features.float()[faces[torch.as_tensor(np.asarray(idx)).long().clamp_min(0)]]
    t = (torch.as_tensor(np.asarray(w)).float()[..., None] * fa).sum(-2)
    return np.where((np.asarray(idx) >= 0)[..., None], t.numpy(), 0.0)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def measure(formulation, truth):
    """The project's measure: four times the largest error the float32 torch formulation makes on the CPU against the float64 truth."""
    return 4.0 * float(np.abs(np.asarray(formulation, dtype=np.float64) - truth).max())


# ---- the gates: the CPU and the GPU tests call the same ones, and the tests of wrong answers show that they bite ------------------------
def golden_inputs(g=None):
    g = golden() if g is None else g
    return (torch.from_numpy(g["verts"]), torch.from_numpy(g["faces"]), torch.from_numpy(g["first_idx"]), torch.from_numpy(g["num_faces"]))


def gate_ragged(S, samples, normals, idx, bary, textures=None, g=None):
    """Case 1 on numpy outputs of the five-mesh batch for the golden uniforms of S."""
    g = golden() if g is None else g
    verts, faces, first, nf = golden_inputs(g)
    u = g["uniforms_%d" % S]
    for name, t in (("samples", samples), ("normals", normals), ("bary", bary)):
        assert t.shape == (5, S, 3) and np.isfinite(t).all(), name + ": an entry was not written"
    assert idx.shape == (5, S) and idx.dtype == np.int64 and (idx != -7).all(), "sample_face_idxs: an entry was not written"
    for n in (2, 4):  # the empty mesh and the mesh of zero total area
        assert (idx[n] == -1).all() and not samples[n].any() and not normals[n].any() and not bary[n].any(), n
    assert np.array_equal(idx[:4], g["idx_%d" % S]), "sample_face_idxs differ from the golden"
    assert bits_equal(samples[:4], g["samples_%d" % S]), "samples differ from the golden in some bit"
    w32 = np.where((idx >= 0)[..., None], formulation_weights32(u), 0.0)
    if not bits_equal(bary, w32):
        bad = np.argwhere(bary != w32)
        print("bary != formulation at", [(tuple(i), float(bary[tuple(i)]).hex(), float(w32[tuple(i)]).hex(), u[tuple(i[:2])].tolist()) for i in bad[:6]])
    assert bits_equal(bary, w32), "bary differs from the torch formulation in some bit"
    truth = normals64(verts, faces, idx)
    tol = measure(formulation_normals32(verts, faces, idx), truth)
    err = float(np.abs(normals - truth).max())
    print("ragged S=%d normals: error %.3g, gate %.3g; golden's own %.3g" % (S, err, tol, float(np.abs(g["normals_%d" % S] - truth[:4]).max())))
    assert err <= tol and float(np.abs(g["normals_%d" % S] - truth[:4]).max()) <= tol
    if textures is not None:
        rows = g["texture_meshes"]
        feats = torch.from_numpy(g["features"])
        truth_t = textures64(feats, faces, idx, weights64(u))
        tol_t = measure(formulation_textures32(feats, faces, idx, w32), truth_t)
        err_t = float(np.abs(textures - truth_t).max())
        print("ragged S=%d textures: error %.3g, gate %.3g" % (S, err_t, tol_t))
        assert textures.shape == (5, S, 3) and err_t <= tol_t
        assert float(np.abs(g["textures_%d" % S] - truth_t[rows]).max()) <= tol_t


def edge_mesh():
    """One mesh near the origin whose faces are all far below 1e-6 in |c|: [zero area, tiny, zero area, tiny, tiny, zero area] -- a normal
    clamped at 1e-6 instead of sys.float_info.epsilon is wrong on every one of them."""
    verts = torch.tensor([[0.0, 0.0, 0.0], [1e-4, 0.0, 0.0], [0.0, 1e-4, 0.0], [2e-4, 1e-4, 5e-5], [1e-4, 3e-4, 0.0], [0.0, 0.0, 2e-4],
                          [3e-4, 3e-4, 3e-4]])
    faces = torch.tensor([[0, 0, 1], [0, 1, 2], [3, 4, 3], [1, 3, 4], [2, 5, 6], [6, 6, 5]])
    return verts, faces


def edge_uniforms(S=192, seed=5):
    """(1, S, 3): thirds of the samples with u0 = 0, u0 = nextafter(1, 0) and random u0; every fourth sample has u1 = 0."""
    u = uniforms(1, S, seed)
    u[0, : S // 3, 0] = 0.0
    u[0, S // 3: 2 * (S // 3), 0] = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    u[0, ::4, 1] = 0.0
    return u


def gate_edges(u, samples, normals, idx, eps=EPS):
    """Case 2 on numpy outputs for edge_mesh() / edge_uniforms()."""
    verts, faces = edge_mesh()
    S = u.shape[1]
    area = areas64(verts, faces)
    positive = np.nonzero(area > 0)[0]
    assert ((idx[0] >= 0) & (idx[0] < faces.shape[0])).all(), "an index outside the mesh's range"
    assert (area[idx[0]] > 0).all(), "a face of zero area was chosen"
    assert (idx[0, : S // 3] == positive[0]).all(), "u0 = 0 must pick the first face of non-zero area"
    assert (idx[0, S // 3: 2 * (S // 3)] == positive[-1]).all(), "u0 = nextafter(1, 0) must pick the last face of non-zero area"
    v0 = verts.numpy()[faces.numpy()[idx[0, ::4], 0]]
    assert bits_equal(samples[0, ::4], v0), "u1 = 0 must put the sample on v0"
    truth = normals64(verts, faces, idx)
    tol = measure(formulation_normals32(verts, faces, idx), truth)
    err = float(np.abs(normals - truth).max())
    print("edges normals: error %.3g, gate %.3g" % (err, tol))
    assert err <= tol, "normals beyond the measure (the clamp is sys.float_info.epsilon)"


def gate_distribution(idx, areas, first=0):
    """Case 5: every face's count within 5 binomial standard deviations of S * area / total."""
    S = idx.size
    counts = np.bincount(idx.reshape(-1) - first, minlength=len(areas))
    want, allowed = binomial_bounds(areas, S)
    worst = float((np.abs(counts - want) / allowed).max())
    print("distribution: worst deviation %.2f of the allowed 5 sigma band" % worst)
    assert counts.sum() == S and worst <= 1.0, (counts, want)


def grads_gate(verts, faces, idx, w, grad_samples=None, grad_normals=None):
    """(truth, tolerance) of gate_grads: the float64 restatement and four times the float32 torch formulation's error against it."""
    truth, _ = grads64(verts, faces, idx, w, grad_samples, grad_normals)
    return truth, measure(formulation_grads32(verts, faces, idx, w, grad_samples, grad_normals), truth)


def gate_grads(verts, faces, idx, w, got, grad_samples=None, grad_normals=None, what="", known=None):
    """Case 6: grad_verts against the float64 restatement on the given indices and weights, within the project's measure.
    known: grads_gate(...) of the same arguments, where several answers are judged on one input."""
    truth, tol = grads_gate(verts, faces, idx, w, grad_samples, grad_normals) if known is None else known
    err = float(np.abs(np.asarray(got, dtype=np.float64) - truth).max())
    print("grads %s: error %.3g, gate %.3g, largest |gradient| %.3g" % (what, err, tol, float(np.abs(truth).max())))
    assert np.isfinite(np.asarray(got)).all() and err <= tol, what
    return err, tol


def star():
    """One face, 300 samples: every sample adds to the same three vertices."""
    verts = torch.tensor([[0.5, -0.25, 0.125], [1.5, 0.75, -0.5], [-0.75, 1.25, 0.25]])
    faces = torch.tensor([[0, 1, 2]])
    gs = torch.cos(torch.arange(900, dtype=torch.float64)).reshape(1, 300, 3).float()
    return verts, faces, uniforms(1, 300, 9), gs


def gate_star(idx, w, got):
    verts, faces, _, gs = star()
    terms = np.asarray(w, dtype=np.float64).reshape(300, 3, 1) * gs.double().numpy().reshape(300, 1, 3)
    truth = terms.sum(0)
    bound = 300 * 2.0 ** -23 * float(np.abs(terms).max())
    err = float(np.abs(np.asarray(got, dtype=np.float64) - truth).max())
    print("star: error %.3g, bound %.3g" % (err, bound))
    assert (np.asarray(idx) == 0).all() and err <= bound


def gate_table(areas32, faces, first, nf, u, idx, table):
    """The cumulative table (F,) float32 of an implementation whose float32 face areas are areas32: non-decreasing inside a mesh,
    restarting at each mesh, a face of zero area repeating its predecessor, within D(F) 2^-24 total of the float64 prefix sums of
    those areas; and the choice idx exactly the host's searchsorted on that table."""
    F = faces.shape[0]
    rows64 = tables64(areas32, first, nf)
    assert table.shape == (F,) and table.dtype == np.float32
    rows32 = [table[int(a):int(a) + int(n)] for a, n in zip(first.tolist(), nf.tolist())]
    depth, worst = scan_depth(F), 0.0
    for n, (r32, r64) in enumerate(zip(rows32, rows64)):
        if r32.size == 0:
            continue
        assert (np.diff(r32) >= 0).all(), "the table steps down inside mesh %d" % n
        assert r32[0] == areas32[int(first[n])], "the table does not restart at mesh %d" % n
        zero = np.nonzero(areas32[int(first[n]):int(first[n]) + r32.size] == 0)[0]
        assert all(r32[k] == (r32[k - 1] if k else 0.0) for k in zero), "a face of zero area does not repeat its predecessor"
        bound = depth * 2.0 ** -24 * float(r64[-1])
        err = float(np.abs(r32.astype(np.float64) - r64).max())
        worst = max(worst, err / bound if bound > 0 else err)
        assert err <= bound, (n, err, bound)
    print("table: F = %d, D(F) = %d, worst error / bound %.3g" % (F, depth, worst))
    assert np.array_equal(idx, choose(rows32, first.tolist(), u[:, :, 0].numpy(), dtype=np.float32)), "the choice is not the host's on this table"


# ---- long runs of the backward (tests/test_*_cloud_kernel_edges.py, section A) -----------------------------------------------------------
WAVE_STEP = 64     # csrc/sample_points.hip: face_sums_kernel -- samples a wave adds per step
FLUSH_AT = 128     # csrc/wave_table.h: WaveTable<9 | 12, 192>::kFlushAt = SLOTS - 64
LONG_S = 180010    # samples per mesh of long_run_batch(): 3 x 180 010 = 540 030 > 2048 x 64 x 4


def backward_plan(num_samples):
    """(waves, span) of backward_rows_atomic (csrc/sample_points.hip): wave w adds the samples [w span, (w + 1) span), 64 per step."""
    waves = -(-num_samples // 64)
    if waves > 2048:
        waves = max(-(-num_samples // 1024), 2048)
    waves = min(waves, 4 * 4096)
    blocks = -(-waves // 4)
    span = -(-(-(-num_samples // (blocks * 4))) // 64) * 64
    return -(-num_samples // span), span


def long_run_batch(seed=71):
    """Three meshes for ONE launch over long runs: the single face of star(); a soup of 6 000 faces over 1 500 vertices; the 300-face
    mesh of ragged_batch() with its faces of zero area.  -> (verts, faces, first, nf) packed."""
    v0, f0 = star()[:2]
    v1, f1 = _soup(torch.Generator().manual_seed(seed), 1500, 6000)
    verts_list, faces_list = ragged_batch()
    return pack([v0, v1, verts_list[3]], [f0, f1, faces_list[3]])


def long_run_grads(which, seed=72):
    """(uniforms, grad_samples, grad_normals or None) of the long-run case."""
    gen = torch.Generator().manual_seed(seed)
    gs = torch.randn(3, LONG_S, 3, generator=gen)
    gn = torch.randn(3, LONG_S, 3, generator=gen) if which == "both" else None
    return uniforms(3, LONG_S, seed + 1), gs, gn


def long_run_reach(idx, nf):
    """What the long-run case is for, from the host's plan and the face indices (3, LONG_S) of a forward: asserts every condition and
    returns the waves that show them {"one_key", "flush", "straddle", "last"}."""
    flat = np.asarray(idx).reshape(-1)
    num_samples, S = flat.size, np.asarray(idx).shape[1]
    waves, span = backward_plan(num_samples)
    assert num_samples > 2048 * 64 * 4 and span >= 256 and span % WAVE_STEP == 0, (num_samples, span)
    assert (flat >= 0).all()
    steps = span // WAVE_STEP
    # a wave wholly inside mesh 0 (one face): the same key in every step, found in the slot an earlier step left
    one_key = [w for w in range(waves) if (w + 1) * span <= S]
    assert one_key and all((flat[w * span:(w + 1) * span] == flat[0]).all() for w in one_key[:3]) and int(nf[0]) == 1
    # a wave inside mesh 1 with more than kFlushAt distinct faces in its first three steps: step four begins with the flush
    flush = [w for w in range(-(-S // span), 2 * S // span)
             if np.unique(flat[w * span:w * span + 3 * WAVE_STEP]).size > FLUSH_AT]
    assert steps >= 4 and flush, "no wave fills its table"
    # a wave across each mesh boundary, and a last wave that the clamp of `end` cuts short
    straddle = [b // span for b in (S, 2 * S) if b % span != 0]
    assert len(straddle) == 2, "a mesh boundary falls on a wave border"
    assert num_samples % span != 0 and (waves - 1) * span < num_samples
    return {"one_key": one_key[0], "flush": flush[0], "straddle": straddle, "last": waves - 1, "span": span, "waves": waves}


def drop_fourth_step(idx, wave):
    """idx with every sample of the fourth step of `wave` set to -1: what the rows hold when a flush loses that step."""
    flat = np.array(idx).reshape(-1)
    _, span = backward_plan(flat.size)
    assert span >= 4 * WAVE_STEP
    flat[wave * span + 3 * WAVE_STEP:wave * span + 4 * WAVE_STEP] = -1
    return flat.reshape(np.asarray(idx).shape)


# ---- many small meshes (section B) -----------------------------------------------------------------------------------------------------
def many_small_meshes(seed=81, N=700):
    """700 meshes with face counts drawn from {0, 0, 1, 2, 3, 70}; three EMPTY meshes at the start, a run of five in the middle and two
    at the end.  -> (verts, faces, first, nf) packed."""
    gen = torch.Generator().manual_seed(seed)
    counts = torch.tensor([0, 0, 1, 2, 3, 70])[torch.randint(0, 6, (N,), generator=gen)].tolist()
    for n in (0, 1, 2, N // 2, N // 2 + 1, N // 2 + 2, N // 2 + 3, N // 2 + 4, N - 2, N - 1):
        counts[n] = 0
    verts_list, faces_list = [], []
    for c in counts:
        if c == 0:
            verts_list.append(torch.rand(3, 3, generator=gen) * 2 - 1), faces_list.append(torch.zeros((0, 3), dtype=torch.int64))
        else:
            v, f = _soup(gen, 3 + c // 2, c)
            verts_list.append(v), faces_list.append(f)
    return pack(verts_list, faces_list)


def small_meshes_reach(first, nf, F):
    """Asserts what the batch is for: more than one block of level 1, several heads in most waves of 64 faces, runs of empty meshes
    at the start, in the middle and at the end (first_idx == F there)."""
    first, nf = np.asarray(first), np.asarray(nf)
    N = nf.size
    assert F > 4 * SCAN_BLOCK and not nf[:3].any() and not nf[N // 2:N // 2 + 5].any() and not nf[-2:].any()
    assert (first[:4] == 0).all() and (first[-2:] == F).all() and len(set(first[N // 2:N // 2 + 6].tolist())) == 1
    heads = np.bincount(np.unique(first[nf > 0]) // 64, minlength=-(-F // 64))
    print("small meshes: F = %d, heads per wave: median %d, largest %d" % (F, int(np.median(heads)), int(heads.max())))
    assert np.median(heads) >= 2 and heads.max() >= 16
    return heads


def gate_small_meshes(verts, faces, first, nf, u, areas32, table, samples, normals, idx, bary):
    """Section B on numpy outputs: gate_table; -1 and zero rows for the empty meshes; bary the formulation's bits; samples within
    12 x 2^-24 of the float64 restatement (|v| <= 1: the bound of the second-round test of the scan)."""
    gate_table(areas32, faces, first, nf, u, idx, table)
    empty = np.asarray(nf) == 0
    assert (idx[empty] == -1).all() and (idx[~empty] >= 0).all()
    for name, t in (("samples", samples), ("normals", normals), ("bary", bary)):
        assert np.isfinite(t).all() and not t[empty].any(), name
    w32 = np.where((idx >= 0)[..., None], formulation_weights32(u.numpy()), 0.0)
    assert bits_equal(bary, w32), "bary differs from the torch formulation in some bit"
    assert float(verts.abs().max()) <= 1.0
    err = float(np.abs(samples - samples64(verts, faces, idx, weights64(u.numpy()))).max())
    print("small meshes: samples error %.3g, bound %.3g" % (err, 12 * 2.0 ** -24))
    assert err <= 12 * 2.0 ** -24


def binomial_bounds(areas, S, sigmas=5.0):
    """(expected count, allowed deviation) per face for S draws with probability area / total."""
    p = np.asarray(areas, dtype=np.float64) / float(np.sum(areas))
    return S * p, sigmas * np.sqrt(S * p * (1.0 - p))


def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}
