"""csrc/point_mesh_grid.hip on the MI355X: the grid search must return what the scan of all pairs returns, bit for bit.

Every case is a batch of four elements -- the case's own cloud and mesh, an empty mesh, an empty cloud, a small soup -- for triangles
and for segments (the faces' three edges each, so every edge occurs twice), at occupancy 1 and 3 (many cells, several rings), and asserts
  torch.equal of dists and idxs with _C.point_mesh_forward (all pairs) on the same tensors, and
  |dists - float64 minimum| <= 4 E, E the worst such error of the package's float32 torch formulation (the gate of
  tests/test_gpu_point_mesh.py).
Then the public route with point_mesh.GRID_MIN_TARGETS = 1.
"""
import pytest
import torch

import _util as U
import point_mesh_case as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = ("surface", "outside", "spanning", "duplicates", "small_area", "far", "nan", "one_cell")
OCCUPANCIES = (1, 3)


def _prims(verts, faces, kind):
    tris = verts[faces]
    return tris if kind == "tri" else torch.cat([tris[:, [0, 1]], tris[:, [0, 2]], tris[:, [1, 2]]], 0)


def _case(name, kind):
    """(points, prims, num_points, num_prims) on the CPU, seeded; element 0 is the case."""
    gen = torch.Generator().manual_seed(CASES.index(name) * 7 + len(kind))
    rand = lambda *shape: torch.rand(*shape, generator=gen)  # noqa: E731
    verts, faces = U.ico_sphere(3)  # 1280 faces of area 0.0098: above the default min_triangle_area
    prims = _prims(verts, faces, kind)
    d = torch.randn(450, 3, generator=gen)
    points = d / d.norm(dim=1, keepdim=True) * (1.0 + 0.03 * torch.randn(450, 1, generator=gen))  # near the surface: rings, then a stop
    if name == "outside":  # far outside the box, and astride it (uniform in twice the box)
        points = torch.cat([points[:150] + torch.tensor([10.0, 0.0, 0.0]), rand(300, 3) * 4.0 - 2.0], 0)
    elif name == "spanning":  # one primitive across the whole box: the large list
        big = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [1.0, -1.0, 1.0]])[None, :prims.shape[1]]
        prims = torch.cat([prims[:600], big, prims[600:]], 0)
    elif name == "duplicates":  # every third primitive again further down: bit-equal distances, the larger index wins
        prims = torch.cat([prims, prims[::3]], 0)
    elif name == "small_area":  # faces of area 0.0048 +- : both sides of min_triangle_area
        prims, points = prims * 0.7, points * 0.7
    elif name == "far":  # coordinates near 1000: the bound's slack exceeds the box, nobody stops
        prims, points = prims + 1000.0, points + 1000.0
    elif name == "nan":
        points[77, 1] = float("nan")
    elif name == "one_cell":  # 600 primitives inside one cell of a grid that a single far primitive stretches
        prims = torch.cat([prims[:600] * 1e-3, prims[:1] + 3.0], 0)
        points = torch.cat([points[:300] * 1e-3, points[300:]], 0)
    soup = (rand(300, prims.shape[1], 3) - 0.5) * 0.1 + rand(300, 1, 3)
    num_points, num_prims = [points.shape[0], 20, 0, 130], [prims.shape[0], 0, 15, 300]
    points = torch.cat([points, rand(20, 3), rand(130, 3)], 0)
    prims = torch.cat([prims, soup[:15], soup], 0)
    return points.contiguous(), prims.contiguous(), num_points, num_prims


@pytest.mark.parametrize("occupancy", OCCUPANCIES)
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("name", CASES)
def test_grid_search_is_the_scan_of_all_pairs_bit_for_bit(name, kind, occupancy):
    from pytorch3d_amd import _C, _lib
    from pytorch3d_amd import point_mesh as pm

    points, prims, num_points, num_prims = _case(name, kind)
    # the path the case is for, from the host-side constants: several waves, more than 27 cells wanted (so the grid has more than
    # one cell and the primitive across the box more than three cells an axis: the large list is not empty)
    assert num_points[0] > 2 * 64 and num_prims[0] / occupancy > 27 and _lib.POINT_MESH_GRID_MAX_REFS < 27
    direction = C.DIRECTIONS[kind][0]
    points, prims = points.to(DEV), prims.to(DEV)
    pfirst, sfirst = C.first_idx(num_points).to(DEV), C.first_idx(num_prims).to(DEV)
    want_d, want_i = _C.point_mesh_forward(direction, points, pfirst, prims, sfirst, max(num_points))
    dists, idxs = _C.point_mesh_grid_forward(direction, points, pfirst, prims, sfirst, max(num_points), 5e-3, occupancy)
    assert torch.equal(idxs, want_i)
    assert torch.equal(dists, want_d)
    assert bool((dists[num_points[0]:num_points[0] + 20] == C.FLT_MAX).all())  # the element without a mesh
    if name == "duplicates":  # the order inside a cell differs from run to run; the result may not
        again = _C.point_mesh_grid_forward(direction, points, pfirst, prims, sfirst, max(num_points), 5e-3, occupancy)
        assert torch.equal(again[0], dists) and torch.equal(again[1], idxs)
    best64, _ = C.minima64(points, prims, num_points, num_prims, True)
    f32, _ = pm.torch_forward(direction, points, pfirst, prims, sfirst)
    judged = torch.isfinite(best64) & (best64 < C.FLT_MAX)
    E = float((f32.double() - best64)[judged].abs().max())
    err = float((dists.double() - best64)[judged].abs().max())
    print(f"{name} {kind} occupancy {occupancy}: error against float64 {err:.3e}, 4 E = {4 * E:.3e}")
    assert err <= 4 * E


@pytest.mark.parametrize("strict", [False, True])
def test_public_route_and_the_backward_from_its_indices(monkeypatch, strict):
    import pytorch3d_amd as p3d
    from pytorch3d_amd import _C
    from pytorch3d_amd import point_mesh as pm

    gen = torch.Generator().manual_seed(3)
    meshes = [U.ico_sphere(2), U.ico_sphere(1)]
    clouds = [torch.randn(300, 3, generator=gen) * 0.7, torch.randn(90, 3, generator=gen) * 0.7]
    calls = []
    monkeypatch.setattr(_C, "point_mesh_grid_forward", lambda *a, _f=_C.point_mesh_grid_forward, **k: calls.append(a[0]) or _f(*a, **k))

    def run(threshold, loss_fn):
        monkeypatch.setattr(pm, "GRID_MIN_TARGETS", threshold)
        verts = [v.to(DEV).requires_grad_(True) for v, _ in meshes]
        points = [c.to(DEV).requires_grad_(True) for c in clouds]
        loss = loss_fn(p3d.PackedMeshes(verts, [f.to(DEV) for _, f in meshes]), p3d.PackedPointclouds(points))
        return [loss.detach()] + list(torch.autograd.grad(loss, verts + points))

    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(strict)
    try:
        for loss_fn, direction in ((pm.point_mesh_face_distance, "point_face"), (pm.point_mesh_edge_distance, "point_edge")):
            del calls[:]
            brute = run(None, loss_fn)
            assert not calls
            grid = run(1, loss_fn)
            assert calls == [direction]  # the point-query forward alone
            assert torch.equal(grid[0], brute[0])  # the loss: the same tree over the same bits
            for g, b in zip(grid[1:], brute[1:]):
                if strict:
                    assert torch.equal(g, b)  # the ordered sums, from equal indices
                else:  # float atomics in any order on both sides: the two differ by rounding alone
                    assert bool(((g - b).abs() <= 64 * 2.0 ** -24 * b.abs().max()).all())
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])
    # what the predicate says is what ran
    p, t = clouds[0].to(DEV), meshes[0][0][meshes[0][1]].to(DEV)
    assert pm.GRID_MIN_TARGETS == 1 and pm.grid_kernel_path("point_face", p, t) and not pm.grid_kernel_path("face_point", p, t)
    del calls[:]
    first = torch.zeros(1, dtype=torch.int64, device=DEV)
    pm.point_face_distance(p, first, t, first, 300)
    pm.face_point_distance(p, first, t, first, 320)
    assert calls == ["point_face"]
