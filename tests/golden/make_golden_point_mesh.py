"""Golden fixture for the point-mesh distances, generated FROM THE REFERENCE's own Python on the CPU (build container only).

    python tests/golden/make_golden_point_mesh.py   ->  tests/golden/point_mesh_ref.npz

* Operator level (tests/point_mesh_case.py: OP_CASES, triangles and segments, both directions): every (point, primitive) pair of an
  element is evaluated by the reference's tests/test_point_mesh_distance.py: TestPointMeshDistance._point_to_tri_distance /
  _point_to_edge_distance in float32; the minimum is taken by the tie rule (the LARGEST index among equal distances), an element
  without targets gives FLT_MAX / index 0; the gradients are autograd's through those functions on the chosen pairs, of
  sum(dists * upstream(Q)).  Nothing of pytorch3d_amd is in the loop, and no compiled reference code either.
* Error budgets: the same minima and gradients from the float64 restatement of point_mesh_case.py (on the reference's pairs) give,
  per case and direction, E = max |float32 - float64| of the minima and the same for either gradient.  They set the tests' tolerances.
* Mesh level (MESH_CASES): the value of the reference's point_mesh_face_distance / point_mesh_edge_distance EXPRESSION built from
  those minima, on the reference's Meshes (edges_packed() order), with gradients to vertices and points, and the budgets again.

The generator asserts that in every soup case at most 5 % of a direction's queries miss the gap rule (second smallest float64
distance >= smallest + 16 E) and that no soup face has an area within a factor 2 of min_triangle_area.  SEED was picked so.
"""
import importlib
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 2


def soup(n, corners, gen):
    """n primitives with independent uniform vertices in the unit cube; triangles are redrawn while their area lies within a factor
    2 of the minimum area."""
    import point_mesh_case as C

    prims = torch.rand(n, corners, 3, generator=gen)
    if corners == 3:
        for _ in range(100):
            area = torch.cross(prims[:, 1] - prims[:, 0], prims[:, 2] - prims[:, 0], dim=1).norm(dim=1) / 2
            bad = (area > C.MIN_AREA / 2) & (area < C.MIN_AREA * 2)
            if not bool(bad.any()):
                break
            prims[bad] = torch.rand(int(bad.sum()), 3, 3, generator=gen)
        assert not bool(bad.any())
    return prims


def draw(seed):
    import _util as U
    import point_mesh_case as C

    gen = torch.Generator().manual_seed(seed)
    out = {}
    for kind in C.KINDS:
        corners = 3 if kind == "tri" else 2
        for name in C.SOUP_CASES:
            counts = C.OP_CASES[name]
            out[C.key(kind, name, "points")] = torch.rand(sum(c[0] for c in counts), 3, generator=gen)
            out[C.key(kind, name, "prims")] = soup(sum(c[1] for c in counts), corners, gen)
            out[C.key(kind, name, "num_points")] = torch.tensor([c[0] for c in counts])
            out[C.key(kind, name, "num_prims")] = torch.tensor([c[1] for c in counts])
        points, prims, _ = C.degenerate_case(kind, gen)
        out[C.key(kind, "degenerate", "points")], out[C.key(kind, "degenerate", "prims")] = points, prims
        out[C.key(kind, "degenerate", "num_points")] = torch.tensor([points.shape[0]])
        out[C.key(kind, "degenerate", "num_prims")] = torch.tensor([prims.shape[0]])
    # mesh level
    iv, jf = U.ico_sphere(2)
    direction = torch.randn(150, 3, generator=gen)
    meshes = {"ico2": ([iv.float()], [jf.long()], [direction / direction.norm(dim=1, keepdim=True) * (1.0 + 0.1 * torch.randn(150, 1, generator=gen))])}
    tris, pts = out[C.key("tri", "ragged", "prims")], out[C.key("tri", "ragged", "points")]
    counts = C.OP_CASES["ragged"]
    ps, ts = C.element_slices([c[0] for c in counts]), C.element_slices([c[1] for c in counts])
    meshes["ragged"] = ([tris[a:b].reshape(-1, 3).clone() for a, b in ts], [torch.arange(3 * (b - a)).reshape(-1, 3) for a, b in ts],
                        [pts[a:b].clone() for a, b in ps])
    small = torch.tensor([[-0.0021, -0.3769, 0.7146], [-0.0161, -0.3771, 0.7146], [-0.0021, -0.3771, 0.7147]])
    cloud = torch.tensor([[-0.3623, -0.5340, 0.7727]])
    meshes["small_faces_a"] = ([small], [torch.tensor([[0, 2, 1]])], [cloud])
    meshes["small_faces_b"] = ([small], [torch.tensor([[2, 0, 1]])], [cloud])
    for name, (verts, faces, clouds) in meshes.items():
        out["mesh/%s/N" % name] = torch.tensor(len(verts))
        for i, (v, f, p) in enumerate(zip(verts, faces, clouds)):
            out["mesh/%s/verts%d" % (name, i)], out["mesh/%s/faces%d" % (name, i)], out["mesh/%s/points%d" % (name, i)] = v, f, p
    return out


def pair_fn(T, kind):
    return T._point_to_tri_distance if kind == "tri" else T._point_to_edge_distance


def reference_matrix(fn, points, prims):
    """(P, T) float32: the reference's function on every pair."""
    out = torch.empty((points.shape[0], prims.shape[0]), dtype=torch.float32)
    with torch.no_grad():
        for i in range(points.shape[0]):
            for j in range(prims.shape[0]):
                out[i, j] = fn(points[i], prims[j])
    return out


def reference_minima(fn, points, prims, num_points, num_prims):
    """For both directions (points query, prims query): dists, packed idxs, has-target mask."""
    import point_mesh_case as C

    res = []
    P, S = points.shape[0], prims.shape[0]
    dp, ip, hp = torch.full((P,), C.FLT_MAX), torch.zeros(P, dtype=torch.int64), torch.zeros(P, dtype=torch.bool)
    ds, is_, hs = torch.full((S,), C.FLT_MAX), torch.zeros(S, dtype=torch.int64), torch.zeros(S, dtype=torch.bool)
    for (p0, p1), (s0, s1) in zip(C.element_slices(num_points), C.element_slices(num_prims)):
        if p1 == p0 or s1 == s0:
            continue
        d = reference_matrix(fn, points[p0:p1], prims[s0:s1])
        n = d.shape[1]
        j = (n - 1) - torch.argmin(d.flip(1), dim=1)  # the largest index among equal minima
        dp[p0:p1], ip[p0:p1], hp[p0:p1] = d.gather(1, j[:, None])[:, 0], s0 + j, True
        n = d.shape[0]
        i = (n - 1) - torch.argmin(d.t().flip(1), dim=1)
        ds[s0:s1], is_[s0:s1], hs[s0:s1] = d.t().gather(1, i[:, None])[:, 0], p0 + i, True
    res.append((dp, ip, hp))
    res.append((ds, is_, hs))
    return res


def reference_grads(fn, points, prims, idxs, up, has, point_query):
    a, b = points.clone().requires_grad_(True), prims.clone().requires_grad_(True)
    total = None
    for q in torch.nonzero(has).squeeze(1).tolist():
        t = int(idxs[q])
        d = fn(a[q], b[t]) if point_query else fn(a[t], b[q])
        total = d * up[q] if total is None else total + d * up[q]
    if total is None:
        return torch.zeros_like(points), torch.zeros_like(prims)
    ga, gb = torch.autograd.grad(total, (a, b), allow_unused=True)
    return (torch.zeros_like(points) if ga is None else ga), (torch.zeros_like(prims) if gb is None else gb)


def record_op_case(T, out, kind, name):
    import point_mesh_case as C

    points, prims = out[C.key(kind, name, "points")], out[C.key(kind, name, "prims")]
    num_points, num_prims = C.counts_of(out, kind, name)
    fn = pair_fn(T, kind)
    both = reference_minima(fn, points, prims, num_points, num_prims)
    for direction, (dists, idxs, has), point_query in zip(C.DIRECTIONS[kind], both, (True, False)):
        up = C.upstream(dists.shape[0])
        gp, gs = reference_grads(fn, points, prims, idxs, up, has, point_query)
        best64, gap = C.minima64(points, prims, num_points, num_prims, point_query)
        E = float((dists.double() - best64)[has].abs().max()) if bool(has.any()) else 0.0
        gp64, gs64 = C.grads64(points, prims, idxs, up, has, point_query)
        Egp, Egs = float((gp.double() - gp64).abs().max()), float((gs.double() - gs64).abs().max())
        ok = C.admitted(gap, E) | ~has
        dropped = 1.0 - float(ok.double().mean()) if ok.numel() else 0.0
        print("%s %-12s %-11s Q=%4d  E=%.3g  E_grad_points=%.3g  E_grad_prims=%.3g  dropped=%.2f%%"
              % (kind, name, direction, dists.shape[0], E, Egp, Egs, 100 * dropped))
        if name in C.SOUP_CASES:
            assert dropped <= C.MAX_DROPPED, "pick another SEED"
        elif point_query:  # the hand-built meetings happen: special point k goes to the primitive built for it, in the chosen branch
            target = C.degenerate_case(kind, torch.Generator().manual_seed(0))[2]
            assert idxs[:len(target)].tolist() == target, idxs[:len(target)].tolist()
            on = 1 if kind == "seg" else 4
            assert float(dists[on]) == 0.0 and float(gp[on].abs().max()) == 0.0 and float(gs.abs().max()) > 0.0
        for what, v in (("dists", dists), ("idxs", idxs), ("grad_points", gp), ("grad_prims", gs), ("E", torch.tensor(E)),
                        ("E_grad_points", torch.tensor(Egp)), ("E_grad_prims", torch.tensor(Egs)), ("admitted", ok)):
            out[C.key(kind, name, what, direction)] = v


def loss_expression(pair, verts, index, points, num_points, num_prims, idx_p, idx_s, N):
    """The reference's loss (point_mesh_distance.py) from the distances of the chosen pairs: pair(points (Q, 3), prims (Q, c, 3))."""
    prims = verts[index]
    to_prim = pair(points, prims[idx_p], True)
    w = torch.repeat_interleave(1.0 / torch.tensor(num_points, dtype=to_prim.dtype), torch.tensor(num_points))
    point_dist = (to_prim * w).sum() / N
    to_point = pair(points[idx_s], prims, False)
    w = torch.repeat_interleave(1.0 / torch.tensor(num_prims, dtype=to_point.dtype), torch.tensor(num_prims))
    return point_dist + (to_point * w).sum() / N


def record_mesh_case(T, out, name):
    import point_mesh_case as C
    from pytorch3d.structures import Meshes

    verts, faces, clouds = C.mesh_inputs(out, name)
    meshes = Meshes(verts=[v.detach() for v in verts], faces=faces)
    N = len(verts)
    num_points = [int(p.shape[0]) for p in clouds]
    points = torch.cat(clouds, 0)
    vp = torch.cat(verts, 0)
    for kind, index, num_prims in (("tri", meshes.faces_packed(), meshes.num_faces_per_mesh().tolist()),
                                   ("seg", meshes.edges_packed(), meshes.num_edges_per_mesh().tolist())):
        fn = pair_fn(T, kind)
        (dp, ip, hp), (ds, is_, hs) = reference_minima(fn, points.detach(), vp.detach()[index], num_points, num_prims)
        assert bool(hp.all()) and bool(hs.all())

        def by_reference(a, b, _point_query):
            return torch.stack([fn(a[i], b[i]) for i in range(a.shape[0])])

        loss = loss_expression(by_reference, vp, index, points, num_points, num_prims, ip, is_, N)
        grads = torch.autograd.grad(loss, verts + clouds)
        v64 = [v.detach().double().requires_grad_(True) for v in verts]
        p64 = [p.detach().double().requires_grad_(True) for p in clouds]
        loss64 = loss_expression(lambda a, b, _pq: C.pair_dist64(a, b), torch.cat(v64, 0), index, torch.cat(p64, 0), num_points, num_prims,
                                 ip, is_, N)
        grads64 = torch.autograd.grad(loss64, v64 + p64)
        b64p, _ = C.minima64(points.detach(), vp.detach()[index], num_points, num_prims, True)
        b64s, _ = C.minima64(points.detach(), vp.detach()[index], num_points, num_prims, False)
        E = float((dp.double() - b64p).abs().max()) + float((ds.double() - b64s).abs().max())
        Eg = max(float((g.double() - g64).abs().max()) for g, g64 in zip(grads, grads64))
        tag = "face" if kind == "tri" else "edge"
        print("mesh %-14s %s loss=%.8g (float64 %.8g)  E_minima=%.3g  E_grad=%.3g" % (name, tag, float(loss), float(loss64), E, Eg))
        out["mesh/%s/%s_loss" % (name, tag)] = loss.detach()
        out["mesh/%s/%s_E_minima" % (name, tag)] = torch.tensor(E)
        out["mesh/%s/%s_E_grad" % (name, tag)] = torch.tensor(Eg)
        for i in range(N):
            out["mesh/%s/%s_grad_verts%d" % (name, tag, i)] = grads[i]
            out["mesh/%s/%s_grad_points%d" % (name, tag, i)] = grads[N + i]


def main():
    import make_golden as mg
    import point_mesh_case as C

    mg.bind_reference()
    # the reference's tests are a package of their own (relative imports): loaded under a name that cannot meet this repository's tests/
    ref_tests = os.path.join(mg.REFERENCE, "tests")
    spec = importlib.util.spec_from_file_location("p3d_reference_tests", os.path.join(ref_tests, "__init__.py"),
                                                  submodule_search_locations=[ref_tests])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules["p3d_reference_tests"] = pkg
    spec.loader.exec_module(pkg)
    T = importlib.import_module("p3d_reference_tests.test_point_mesh_distance").TestPointMeshDistance

    out = draw(SEED)
    for kind in C.KINDS:
        for name in C.OP_CASES:
            record_op_case(T, out, kind, name)
    for name in C.MESH_CASES:
        record_mesh_case(T, out, name)
    arrays = {k: v.detach().cpu().numpy() for k, v in out.items()}
    np.savez_compressed(C.FIXTURE, **arrays)
    print("wrote", C.FIXTURE, os.path.getsize(C.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
