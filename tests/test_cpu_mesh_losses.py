"""The host side of the mesh regularisers (no GPU): `_C.mesh_normal_consistency_find_verts`, the topology tables of
pytorch3d_amd.mesh_losses and its torch formulation (CPU tensors, float64, cot / cotcurv).

Input and yardsticks: tests/mesh_losses_case.py.  Gates: a gradient within FOUR times the largest error the float32 formulation on the
CPU makes against the float64 truth on this input, a loss within four times its error plus D(n) 2^-24 S (D(n) the documented depth of
the kernels' sum tree, S the float64 sum of the absolute terms): the measure of tests/test_gpu_mesh_normals.py.
"""
import random

import pytest
import torch

import mesh_losses_case as C

EXAMPLES = {  # the five examples of the reference's source comment -> the rows in the documented order (edges, then j, then i)
    (1, 0, 1, 1, 0): [],
    (3,): [(0, 1), (0, 2), (1, 2)],
    (0, 3): [(0, 1), (0, 2), (1, 2)],
    (1, 3): [(1, 2), (1, 3), (2, 3)],
    (1, 0, 2, 1, 0, 2): [(1, 2), (4, 5)],
}


def _brute_find_verts(edge_num):
    rows, offset = [], 0
    for k in edge_num:
        rows += [(offset + i, offset + j) for j in range(k) for i in range(j)]
        offset += k
    return rows


@pytest.fixture(scope="module")
def batch():
    verts, faces = C.build_batch()
    return {"verts": verts, "faces": faces, "tables": C.brute_tables(verts, faces)}


@pytest.fixture(scope="module")
def topology(batch):
    import pytorch3d_amd as p3d

    m = p3d.PackedMeshes(batch["verts"], batch["faces"])
    return p3d.mesh_loss_topology(m.faces_packed(), m.num_verts_per_mesh(), m.num_faces_per_mesh())


def test_find_verts_on_the_examples_of_the_references_source_comment():
    from pytorch3d_amd import _aux_ops

    for edge_num, want in EXAMPLES.items():
        got = _aux_ops.mesh_normal_consistency_find_verts(torch.tensor(edge_num, dtype=torch.int64))
        assert got.dtype == torch.int64 and got.device.type == "cpu" and tuple(got.shape) == (len(want), 2)
        assert {tuple(r) for r in got.tolist()} == set(want), edge_num
        assert torch.equal(got, torch.tensor(want, dtype=torch.int64).reshape(-1, 2)), edge_num
    empty = _aux_ops.mesh_normal_consistency_find_verts(torch.zeros((0,), dtype=torch.int64))
    assert tuple(empty.shape) == (0, 2) and empty.dtype == torch.int64


def test_find_verts_against_a_python_double_loop():
    from pytorch3d_amd import _aux_ops

    rng = random.Random(11)
    edge_num = [rng.randint(0, 4) for _ in range(200)]
    got = _aux_ops.mesh_normal_consistency_find_verts(torch.tensor(edge_num, dtype=torch.int64))
    want = _brute_find_verts(edge_num)
    assert len(want) == sum(k * (k - 1) // 2 for k in edge_num) > 100
    assert got.tolist() == [list(r) for r in want]


def test_find_verts_is_served_by_the_shim_module_and_the_rest_still_raises():
    from pytorch3d_amd import shim

    mod = shim.make_module()
    got = mod.mesh_normal_consistency_find_verts(torch.tensor([1, 3], dtype=torch.int64))
    assert got.tolist() == [[1, 2], [1, 3], [2, 3]]
    with pytest.raises(NotImplementedError):
        mod.knn_points_idx(None)
    with pytest.raises(RuntimeError, match="int64 vector"):
        mod.mesh_normal_consistency_find_verts(torch.tensor([1.0, 3.0]))


def test_topology_tables_of_the_case_batch(batch, topology):
    t, b = topology, batch["tables"]
    for name in ("edges", "edge_mesh", "num_edges", "adj_offsets", "adj", "vert_mesh", "num_verts", "pairs", "pair_mesh", "num_pairs",
                 "pair_offsets", "pair_slots"):
        x = getattr(t, name)
        assert x.dtype == torch.int32 and x.is_contiguous() and x.device.type == "cpu", name
    assert (t.N, t.V, t.E, t.P, t.empty) == (5, 162 + 16 + 6 + 0 + 12, len(b["edges"]), len(b["pairs"]), False)
    # edges: the definition, the counts by hand, and the reference's Meshes.edges_packed() where it is staged
    assert t.edges.tolist() == [list(e) for e in b["edges"]] and t.edge_mesh.tolist() == b["edge_mesh"]
    assert t.num_edges.tolist() == [C.EDGES_BY_HAND[n] for n in range(5)]
    key = t.edges[:, 0].long() * t.V + t.edges[:, 1].long()
    assert bool((key[1:] > key[:-1]).all()) and bool((t.edges[:, 0] < t.edges[:, 1]).all())
    ref = C.reference_formulation()
    if ref is not None:
        assert t.edges.tolist() == ref["edges_packed"]
    # the adjacency: symmetric, 2 E entries, ascending per vertex
    off, adj = t.adj_offsets.tolist(), t.adj.tolist()
    assert len(adj) == 2 * t.E and off[0] == 0 and off[-1] == 2 * t.E and len(off) == t.V + 1
    rows = [adj[off[v]:off[v + 1]] for v in range(t.V)]
    assert rows == b["adjacency"]
    assert all(v in rows[u] for v in range(t.V) for u in rows[v])
    assert rows[162 + 16 + 5] == [], "the book's sixth vertex has no neighbour"
    # the wing pairs: the definition (rows and order), P per mesh by hand
    assert t.pairs.tolist() == [list(p) for p in b["pairs"]] and t.pair_mesh.tolist() == b["pair_mesh"]
    assert t.num_pairs.tolist() == [480, C.PAIRS_BY_HAND[1], C.PAIRS_BY_HAND[2], 0, C.PAIRS_BY_HAND[4]]
    assert t.num_verts.tolist() == [162, 16, 6, 0, 12] and t.vert_mesh.tolist() == b["vert_mesh"]
    # every incidence slot points back to its vertex; stable: ascending slots inside a vertex; every slot exactly once
    poff, slots = t.pair_offsets.tolist(), t.pair_slots.tolist()
    flat = t.pairs.reshape(-1).tolist()
    assert len(slots) == 4 * t.P and poff[0] == 0 and poff[-1] == 4 * t.P and sorted(slots) == list(range(4 * t.P))
    for v in range(t.V):
        mine = slots[poff[v]:poff[v + 1]]
        assert all(flat[s] == v for s in mine) and mine == sorted(mine)


def test_topology_refuses_what_it_cannot_index_and_marks_empty_batches():
    import pytorch3d_amd as p3d

    class Huge:  # 3 F = 2^31 without the memory
        def dim(self):
            return 2

        def size(self, i):
            return (2 ** 31 // 3 + 1, 3)[i]

        def numel(self):
            return 3 * (2 ** 31 // 3 + 1)

    with pytest.raises(RuntimeError, match="int32"):
        p3d.mesh_loss_topology(Huge(), torch.tensor([4]), torch.tensor([2 ** 31 // 3 + 1]))
    with pytest.raises(RuntimeError, match=r"\(F, 3\)"):
        p3d.mesh_loss_topology(torch.zeros((4, 2), dtype=torch.int64), torch.tensor([4]), torch.tensor([4]))
    t = p3d.mesh_loss_topology(torch.zeros((0, 3), dtype=torch.int64), torch.tensor([0, 0]), torch.tensor([0, 0]))
    assert t.empty and (t.N, t.V, t.E, t.P) == (2, 0, 0, 0)
    for fn in (p3d.mesh_edge_loss, p3d.mesh_laplacian_smoothing, p3d.mesh_normal_consistency):
        for m in (p3d.PackedMeshes([], []), p3d.PackedMeshes([torch.zeros((0, 3))] * 2, [torch.zeros((0, 3), dtype=torch.int64)] * 2)):
            out = fn(m)
            assert out.tolist() == [0.0] and out.requires_grad and out.dtype == torch.float32
    one = p3d.PackedMeshes([torch.rand(3, 3)], [torch.tensor([[0, 1, 2]])])  # one triangle: 3 edges, no pair
    assert p3d.mesh_normal_consistency(one).tolist() == [0.0] and p3d.mesh_normal_consistency(one).requires_grad
    assert p3d.mesh_edge_loss(one).dim() == 0
    with pytest.raises(ValueError, match="Method should be one of {uniform, cot, cotcurv}"):
        p3d.mesh_laplacian_smoothing(one, "cotangent")


def test_the_topology_is_kept_on_the_mesh_and_handed_on_by_update_verts_packed(batch):
    import pytorch3d_amd as p3d
    from pytorch3d_amd import mesh_losses

    m = p3d.PackedMeshes(batch["verts"], batch["faces"])
    p3d.mesh_edge_loss(m)
    kept = m.__dict__[mesh_losses._TOPOLOGY_KEY]
    p3d.mesh_normal_consistency(m)
    assert m.__dict__[mesh_losses._TOPOLOGY_KEY] is kept
    m2 = m.update_verts_packed(m.verts_packed() + 0.01)
    assert mesh_losses.topology_of(m2) is kept[1]
    other = p3d.PackedMeshes(batch["verts"][:1], batch["faces"][:1])
    assert mesh_losses.topology_of(other) is not kept[1]


@pytest.mark.parametrize("name", C.LOSSES)
def test_torch_formulation_on_the_cpu_within_the_gates(batch, name):
    verts, faces, tables = batch["verts"], batch["faces"], batch["tables"]
    t_loss, t_grad, gate_l, gate_g, rec = C.gates(name, verts, faces, tables)
    loss, grad = C.package_formulation(verts, faces)[name]
    err_l, err_g = abs(loss - t_loss), float((grad.double() - t_grad).abs().max())
    print(f"{name}: loss {loss:.9g} (truth {t_loss:.9g}) error {err_l:.2e}, gate {gate_l:.2e} = 4 x {rec['E32_loss']:.2e} + {rec['D']} x 2^-24 x "
          f"{rec['S']:.3g}; gradient error {err_g:.2e}, gate {gate_g:.2e} = 4 x {rec['E32_grad']:.2e} (n = {rec['n']})")
    assert rec["E32_grad"] > 0 and t_loss > 0
    assert err_l <= gate_l and err_g <= gate_g
    # float64 input: everything in float64 but the weights, which are 1.0 / count.float() as in the reference -- float32, half an ulp
    # (2^-24 = 6e-8, relative) from the truth's exact quotient
    loss64, grad64 = C.package_formulation(verts, faces, torch.float64)[name]
    assert abs(loss64 - t_loss) <= 1e-7 * abs(t_loss) and float((grad64 - t_grad).abs().max()) <= 1e-7 * float(t_grad.abs().max())


def test_the_book_vertex_without_a_face_and_the_weights(batch):
    """The package's torch formulation: the Laplacian gradient of a vertex without a neighbour is x / |x| / V_mesh / N (r = -x), and every
    mesh weighs 1 / N whatever its size -- the loss of the batch is the mean of the losses of its meshes taken alone."""
    import pytorch3d_amd as p3d

    verts, faces = batch["verts"], batch["faces"]
    whole = C.package_formulation(verts, faces)
    lone = 162 + 16 + 5
    x = torch.cat(verts, 0)[lone].double()
    assert torch.allclose(whole["laplacian"][1][lone].double(), x / x.norm() / 6 / 5, rtol=1e-6, atol=0)
    for name, fn in (("edge", p3d.mesh_edge_loss), ("laplacian", p3d.mesh_laplacian_smoothing), ("normal", p3d.mesh_normal_consistency)):
        alone = [float(fn(p3d.PackedMeshes([v], [f])).detach().sum()) for v, f in zip(verts, faces)]
        assert alone[3] == 0.0 and all(a > 0 for k, a in enumerate(alone) if k != 3), (name, alone)
        assert abs(whole[name][0] - sum(alone) / 5) <= 1e-6 * whole[name][0], (name, whole[name][0], alone)


def test_a_mesh_of_vertices_alone_inside_a_batch_gets_zero_rows():
    """A mesh with vertices and no face in a non-empty batch: 0 edges, so its weight 1 / 0 is infinite and must never meet its
    vertices' zero sums.  The torch formulation (what the kernels are held to on the GPU) against the float64 truth."""
    import pytorch3d_amd as p3d
    from pytorch3d_amd import mesh_losses

    verts, faces = C.build_with_a_mesh_of_vertices_alone()
    tables = C.brute_tables(verts, faces)
    t = mesh_losses.topology_of(p3d.PackedMeshes(verts, faces))
    assert not t.empty and t.num_edges.tolist() == [0, 30] and t.num_verts.tolist() == [3, 12] and t.vert_mesh.tolist()[:3] == [0, 0, 0]
    got = C.package_formulation(verts, faces)
    for name in C.LOSSES:
        t_loss, t_grad, gate_l, gate_g, _ = C.gates(name, verts, faces, tables, f32=got)
        assert bool(torch.isfinite(got[name][1]).all()) and abs(got[name][0] - t_loss) <= gate_l, name
        if name != "laplacian":
            assert torch.equal(got[name][1][:3], torch.zeros(3, 3)) and float(t_grad[:3].abs().max()) == 0.0, name


def test_a_face_that_names_a_vertex_twice_is_flagged_and_refused():
    import pytorch3d_amd as p3d
    from pytorch3d_amd import mesh_losses

    v = torch.rand(4, 3)
    m = p3d.PackedMeshes([v], [torch.tensor([[0, 1, 2], [1, 3, 3]])])
    assert mesh_losses.topology_of(m).repeated
    assert not mesh_losses.topology_of(p3d.PackedMeshes([v], [torch.tensor([[0, 1, 2], [1, 3, 2]])])).repeated
    for fn in (p3d.mesh_edge_loss, p3d.mesh_laplacian_smoothing, p3d.mesh_normal_consistency):
        with pytest.raises(ValueError, match="names one vertex twice"):
            fn(m)


def test_the_cosine_the_kernels_restate_is_the_installed_torchs():
    """csrc/mesh_losses.hip restates torch.cosine_similarity(eps=1e-8) as (x1 / max(|x1|, eps)) . (x2 / max(|x2|, eps)) and its
    gradient with the clamp applied to the norm's VALUE only (under no_grad).  Pinned here against the installed torch: the same bits
    forward on 100 000 float32 rows, rows below the clamp and zero rows included, and the same gradient through the explicit form."""
    gen = torch.Generator().manual_seed(4)
    a, b = torch.randn(100_000, 3, generator=gen), torch.randn(100_000, 3, generator=gen)
    a[:10] *= 1e-9
    b[5:20] *= 1e-10
    a[20:25] = 0.0

    def explicit(x1, x2):
        n1 = torch.linalg.vector_norm(x1, 2, dim=1, keepdim=True)
        n2 = torch.linalg.vector_norm(x2, 2, dim=1, keepdim=True)
        c1 = n1 + (n1.detach().clamp_min(1e-8) - n1.detach())  # the clamp moves the value, not the graph
        c2 = n2 + (n2.detach().clamp_min(1e-8) - n2.detach())
        return ((x1 / c1) * (x2 / c2)).sum(1)

    assert torch.equal(explicit(a, b), torch.cosine_similarity(a, b, dim=1, eps=1e-8))
    g = torch.randn(100_000, generator=gen)
    grads = []
    for fn in (explicit, lambda x1, x2: torch.cosine_similarity(x1, x2, dim=1, eps=1e-8)):
        x1, x2 = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        grads.append(torch.autograd.grad(fn(x1, x2), (x1, x2), g))
    for mine, theirs in zip(grads[0], grads[1]):
        assert bool(torch.isfinite(theirs).all())
        assert torch.allclose(mine, theirs, rtol=1e-5, atol=0)
    # at a zero row the gradient is up / eps: the norm's own backward is masked there
    up = (b[20:25] / b[20:25].norm(dim=1, keepdim=True)) * g[20:25, None]
    assert torch.allclose(grads[1][0][20:25], up / 1e-8, rtol=1e-5, atol=0)


@pytest.mark.parametrize("method", ["cot", "cotcurv"])
def test_cot_and_cotcurv_on_the_cpu_match_the_reference(batch, method):
    ref = C.reference_formulation()
    if ref is None:
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    loss, grad = C.package_formulation(batch["verts"], batch["faces"])[method]
    want_loss, want_grad = ref[method]
    # two float32 evaluations of one formula that differ in the order of their row sums (sparse mm there, index_add here)
    print(f"{method}: {loss:.9g} against the reference's {want_loss:.9g}; gradient difference {float((grad - want_grad).abs().max()):.2e} of "
          f"{float(want_grad.abs().max()):.2e}")
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss)
    assert float((grad - want_grad).abs().max()) <= 1e-4 * float(want_grad.abs().max())
