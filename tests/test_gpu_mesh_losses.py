"""csrc/mesh_losses.hip on the MI355X: mesh_edge_loss, mesh_laplacian_smoothing ("uniform") and mesh_normal_consistency, forward and
backward, and the three patches of pytorch3d_amd.shim.

Input and yardsticks: tests/mesh_losses_case.py -- a batch of five small meshes through every branch (closed, open, non-manifold, a
vertex without a face, an empty mesh, a doubled face), each loss restated in float64 and differentiated by autograd.
Gates, the measure of tests/test_gpu_mesh_normals.py: a gradient within FOUR times the largest error the float32 formulation makes on
the CPU against the same truth; a loss within four times its error plus D(n) 2^-24 S, D(n) = 8 + ceil(ceil(n / 256) / 256) + 8 the
depth of the kernels' sum tree (include/p3d_amd.h) and S the float64 sum of the absolute terms (the float32 formulation's own error on
one scalar can be zero by luck).
"""
import contextlib
import json
import os
import subprocess
import sys

import pytest
import torch

import _util as U
import mesh_losses_case as C

pytestmark = pytest.mark.gpu

ROOT = U.ROOT
KERNELS = {"edge": "mesh_edge_loss", "edge_target": "mesh_edge_loss", "laplacian": "mesh_laplacian", "normal": "mesh_normal_consistency"}


def _dev():
    return torch.device("cuda:0")


@contextlib.contextmanager
def _flag(on):
    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])


@pytest.fixture(scope="module")
def batch():
    """The input, its tables by the definition and the float32 formulation's results -- computed once, never modified."""
    verts, faces = C.build_batch()
    C.float32_formulation(verts, faces)
    return {"verts": verts, "faces": faces, "tables": C.brute_tables(verts, faces)}


def _call(name, meshes):
    import pytorch3d_amd as p3d

    if name in ("edge", "edge_target"):
        return p3d.mesh_edge_loss(meshes, C.TARGET if name == "edge_target" else 0.0)
    if name == "normal":
        return p3d.mesh_normal_consistency(meshes)
    return p3d.mesh_laplacian_smoothing(meshes)


def _run(name, verts, faces, grad_output=1.0):
    """(loss, grad (V, 3), the PackedMeshes) of one loss on the GPU (the tables are built by the call)."""
    import pytorch3d_amd as p3d

    d = _dev()
    v = [x.to(d).requires_grad_(True) for x in verts]
    m = p3d.PackedMeshes(v, [x.to(d) for x in faces])
    loss = _call(name, m)
    grads = torch.autograd.grad(loss * grad_output if grad_output != 1.0 else loss, v)
    return loss.detach(), torch.cat(list(grads), 0), m


@pytest.mark.parametrize("name", C.LOSSES)
def test_loss_and_gradient_within_the_gates(batch, name):
    from pytorch3d_amd import _lib

    t_loss, t_grad, gate_l, gate_g, rec = C.gates(name, batch["verts"], batch["faces"], batch["tables"])
    _lib.load().p3d_profile_reset()
    _lib.load().p3d_profile_enable(1)
    try:
        loss, grad, _ = _run(name, batch["verts"], batch["faces"])
        ran = _lib.profile_snapshot()
    finally:
        _lib.load().p3d_profile_enable(0)
    assert KERNELS[name] + "_forward" in ran and KERNELS[name] + "_backward" in ran, f"the HIP kernels did not run: {sorted(ran)}"
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    err_l, err_g = abs(float(loss) - t_loss), float((grad.cpu().double() - t_grad).abs().max())
    print(f"{name}: loss {float(loss):.9g} (truth {t_loss:.9g}) error {err_l:.2e}, gate {gate_l:.2e} = 4 x {rec['E32_loss']:.2e} + {rec['D']} x "
          f"2^-24 x {rec['S']:.3g}; gradient error {err_g:.2e}, gate {gate_g:.2e} = 4 x {rec['E32_grad']:.2e} (n = {rec['n']}, largest "
          f"gradient {float(t_grad.abs().max()):.2e})")
    assert rec["E32_grad"] > 0
    assert err_l <= gate_l, (err_l, gate_l)
    assert err_g <= gate_g, (err_g, gate_g)


@pytest.mark.parametrize("name", C.LOSSES)
def test_a_grad_output_other_than_one(batch, name):
    _, t_grad, _, gate_g, rec = C.gates(name, batch["verts"], batch["faces"], batch["tables"], grad_output=0.37)
    _, grad, _ = _run(name, batch["verts"], batch["faces"], grad_output=0.37)
    err_g = float((grad.cpu().double() - t_grad).abs().max())
    print(f"{name} x 0.37: gradient error {err_g:.2e}, gate {gate_g:.2e} = 4 x {rec['E32_grad']:.2e}")
    assert err_g <= gate_g, (err_g, gate_g)


@pytest.mark.parametrize("name", C.LOSSES)
def test_the_same_bits_on_two_runs_two_streams_and_under_the_strict_flag(batch, name):
    first = _run(name, batch["verts"], batch["faces"])
    torch.cuda.synchronize()
    runs = {"a second call": _run(name, batch["verts"], batch["faces"])}
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):
        runs["another stream"] = _run(name, batch["verts"], batch["faces"])
    side.synchronize()
    with _flag(True):  # nothing to refuse: no atomic in either direction; the tables are rebuilt under the flag too
        runs["the strict flag"] = _run(name, batch["verts"], batch["faces"])
    torch.cuda.synchronize()
    for how, (loss, grad, _) in runs.items():
        assert torch.equal(loss, first[0]), f"the loss differs with {how}"
        assert torch.equal(grad, first[1]), f"the gradient differs with {how}"


def test_the_tables_on_the_gpu_equal_the_definition(batch):
    import pytorch3d_amd as p3d
    from pytorch3d_amd import mesh_losses

    d = _dev()
    m = p3d.PackedMeshes([x.to(d) for x in batch["verts"]], [x.to(d) for x in batch["faces"]])
    t, b = mesh_losses.topology_of(m), batch["tables"]
    assert t.edges.is_cuda and t.edges.dtype == torch.int32
    assert t.edges.tolist() == [list(e) for e in b["edges"]] and t.pairs.tolist() == [list(p) for p in b["pairs"]]
    off, adj = t.adj_offsets.tolist(), t.adj.tolist()
    assert [adj[off[v]:off[v + 1]] for v in range(t.V)] == b["adjacency"]
    cpu = p3d.PackedMeshes(batch["verts"], batch["faces"])
    t_cpu = mesh_losses.topology_of(cpu)
    assert torch.equal(t.pair_slots.cpu(), t_cpu.pair_slots) and torch.equal(t.pair_offsets.cpu(), t_cpu.pair_offsets)


def test_trivial_sizes(batch):
    import pytorch3d_amd as p3d

    d = _dev()
    e_v, e_f = torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int64)
    # an all-empty batch: the reference's value
    for name in C.LOSSES:
        out = _call(name, p3d.PackedMeshes([e_v.to(d)] * 2, [e_f.to(d)] * 2))
        assert out.tolist() == [0.0] and out.requires_grad and out.is_cuda
    # one triangle: 3 edges, no pair
    tri_v, tri_f = [torch.tensor([[0.0, 0, 0], [2, 0, 0], [0, 3, 0]])], [torch.tensor([[0, 1, 2]])]
    tables = C.brute_tables(tri_v, tri_f)
    assert len(tables["edges"]) == 3 and not tables["pairs"]
    none = _call("normal", p3d.PackedMeshes([tri_v[0].to(d)], [tri_f[0].to(d)]))
    assert none.tolist() == [0.0] and none.requires_grad
    loss, grad, _ = _run("edge", tri_v, tri_f)
    assert abs(float(loss) - (4 + 9 + 13) / 3) < 1e-6  # lengths 2, 3, sqrt(13)
    assert torch.allclose(grad.cpu().double(), C.truth("edge", tri_v[0], tables)[1], atol=1e-6)
    loss, grad, _ = _run("laplacian", tri_v, tri_f)
    t_loss, t_grad, _, _ = C.truth("laplacian", tri_v[0], tables)
    assert abs(float(loss) - t_loss) < 1e-6 and torch.allclose(grad.cpu().double(), t_grad, atol=1e-6)
    # N = 1, and the batch with the empty mesh in front: (N - 1) / N of the value without it
    one_v, one_f = [batch["verts"][0]], [batch["faces"][0]]
    tables1 = C.brute_tables(one_v, one_f)
    tables2 = C.brute_tables([e_v] + one_v, [e_f] + one_f)
    f32 = C.package_formulation(one_v, one_f)  # the gates of this input: the package's torch formulation in float32 on the CPU
    for name in C.LOSSES:
        t_loss, t_grad, gate_l, gate_g, _ = C.gates(name, one_v, one_f, tables1, f32=f32)
        loss, grad, _ = _run(name, one_v, one_f)
        assert abs(float(loss) - t_loss) <= gate_l, (name, float(loss), t_loss, gate_l)
        assert float((grad.cpu().double() - t_grad).abs().max()) <= gate_g, (name, gate_g)
        loss2, grad2, _ = _run(name, [e_v] + one_v, [e_f] + one_f)
        assert tables2["N"] == 2 and float(loss2) == float(loss) / 2  # a division by 2 instead of 1: exact
        assert torch.allclose(grad2 * 2, grad, rtol=1e-6, atol=0)
    # what is not float32 on the GPU takes the torch formulation; the lower-level forms refuse a topology of another size
    from pytorch3d_amd import mesh_losses

    m = p3d.PackedMeshes([one_v[0].to(d)], [one_f[0].to(d)])
    with pytest.raises(RuntimeError, match="topology"):
        mesh_losses.edge_loss(m.verts_packed()[:10], mesh_losses.topology_of(m))
    m64 = p3d.PackedMeshes([one_v[0].to(d).double()], [one_f[0].to(d)])
    assert abs(float(p3d.mesh_edge_loss(m64)) - C.truth("edge", one_v[0], tables1)[0]) < 1e-7


def test_degenerate_input_gives_finite_numbers():
    """Two coincident vertices joined by an edge (0 and 1), a wing pair whose opposite vertex lies on v0 (the pair on edge (0, 2):
    a = vertex 1, so n0 = e x 0 = 0), and a triangle collapsed to one point.  The normal-consistency gradient at the zero normal is
    what autograd gives torch's cosine_similarity there -- up / eps, the clamp being applied under no_grad: about 1e8 times a
    regular one -- printed, not gated."""
    import pytorch3d_amd as p3d

    verts = [torch.tensor([[0.0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]]), torch.tensor([[2.0, 2, 2]] * 3)]
    faces = [torch.tensor([[0, 1, 2], [0, 2, 3], [2, 4, 3]]), torch.tensor([[0, 1, 2]])]
    tables = C.brute_tables(verts, faces)
    assert (0, 1) in tables["edges"] and (0, 2, 1, 3) in tables["pairs"]
    want = C.package_formulation(verts, faces)  # the installed torch's formulation, float32 on the CPU
    for name in ("edge", "laplacian", "normal"):
        loss, grad, _ = _run(name, verts, faces)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()), name
        print(f"{name}: {float(loss):.9g} against torch's {want[name][0]:.9g}; largest gradient {float(grad.abs().max()):.3g} "
              f"(torch autograd: {float(want[name][1].abs().max()):.3g})")
        assert abs(float(loss) - want[name][0]) <= 1e-6, name
        if name == "edge":
            # vertex 1 has the edges (0, 1), of length 0, and (1, 2): its row is the second edge's alone; the collapsed triangle's
            # rows are exactly zero
            e_count = len([m for m in tables["edge_mesh"] if m == 0])
            assert torch.equal(grad[5:8].cpu(), torch.zeros(3, 3))
            assert torch.allclose(grad[1].cpu(), torch.tensor([-2.0, 0.0, 0.0]) / e_count / 2, rtol=1e-6, atol=0)
        if name == "laplacian":
            assert torch.equal(grad[5:8].cpu(), torch.zeros(3, 3))  # r = 0 there: q = 0, as torch's norm backward


def test_a_mesh_of_vertices_alone_inside_a_batch():
    """Three vertices without a face in front of an icosahedron: that mesh has 0 edges, its weight is 1 / 0, and the edge backward
    must give its vertices exact zeros (not 0 x inf); every gradient against the float64 truth within the gates of this input."""
    verts, faces = C.build_with_a_mesh_of_vertices_alone()
    tables = C.brute_tables(verts, faces)
    f32 = C.package_formulation(verts, faces)
    for name in C.LOSSES:
        t_loss, t_grad, gate_l, gate_g, _ = C.gates(name, verts, faces, tables, f32=f32)
        loss, grad, _ = _run(name, verts, faces)
        err_g = float((grad.cpu().double() - t_grad).abs().max())
        print(f"{name}: loss error {abs(float(loss) - t_loss):.2e} (gate {gate_l:.2e}), gradient error {err_g:.2e} (gate {gate_g:.2e})")
        assert bool(torch.isfinite(grad).all()), name
        assert abs(float(loss) - t_loss) <= gate_l and err_g <= gate_g, name
        if name != "laplacian":
            assert torch.equal(grad[:3].cpu(), torch.zeros(3, 3)), name
        else:
            assert float(grad[:3].abs().min()) > 0  # r = -x there


# ---- the shim ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim_report():
    if not os.path.isdir(os.path.join(C.STAGE, "pytorch3d", "loss")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_mesh_losses_case.py")], capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    print(json.dumps(rec))
    return rec


def test_install_alone_runs_the_references_normal_consistency(shim_report):
    """pytorch3d.loss.mesh_normal_consistency, unpatched, on a GPU Meshes: `_C.mesh_normal_consistency_find_verts` on the host."""
    r = shim_report["install_alone"]
    assert r["error"] <= r["gate"], r


def test_patched_losses_are_fused_and_agree_with_the_originals(shim_report):
    r = shim_report
    assert r["patched_everywhere"]
    assert r["fused_calls"] == {"mesh_edge_loss": 2, "mesh_laplacian_smoothing": 1, "mesh_normal_consistency": 1}
    assert r["fallback_calls"] == {"mesh_edge_loss": 0, "mesh_laplacian_smoothing": 0, "mesh_normal_consistency": 0}
    for name, c in r["cases"].items():
        assert c["patched_loss_error"] <= c["loss_gate"] and c["patched_grad_error"] <= c["grad_gate"], (name, c)
        # against the original itself (the reference's function on the GPU): ours is within one gate of the truth and the original
        # lies where this run measured it, so the two are no further apart than the gate plus the original's own error
        assert c["loss_difference"] <= c["loss_gate"] + c["original_loss_error"], (name, c)
        assert c["grad_difference"] <= c["grad_gate"] + c["original_grad_error"], (name, c)


def test_offset_verts_hands_the_topology_on(shim_report):
    assert shim_report["offset_hands_topology_on"]


def test_a_cpu_mesh_and_cot_take_the_references_functions_and_uninstall_restores_them(shim_report):
    r = shim_report
    assert r["cpu_fallback_calls"] == {"mesh_edge_loss": 1, "mesh_laplacian_smoothing": 2, "mesh_normal_consistency": 1}
    assert r["cpu_fused_calls"] == {"mesh_edge_loss": 0, "mesh_laplacian_smoothing": 0, "mesh_normal_consistency": 0}
    assert r["restored"]


def test_a_mesh_of_vertices_alone_and_a_repeated_vertex_through_the_patches(shim_report):
    r = shim_report
    assert r["vertices_alone_fused_calls"] == 4
    for name, c in r["vertices_alone"].items():
        assert c["finite"] and c["grad_error"] <= c["grad_gate"], (name, c)
        if name != "laplacian":
            assert c["rows_of_the_lone_vertices"] == 0.0, (name, c)
    assert r["repeated_vertex_fallback_calls"] == {"mesh_edge_loss": 1, "mesh_laplacian_smoothing": 1, "mesh_normal_consistency": 1}
    assert r["repeated_vertex_fused_calls"] == 0


def test_a_fitting_step_with_the_three_regularisers(shim_report):
    r = shim_report["step"]
    assert r["fused_calls"] == 3 and r["fused_calls_when_restored"] == 0 and r["finite"] and r["largest"] > 0
    # The two steps differ in three things.  (1) The regularisers: each side's gradient is within its gate of the truth (four times the
    # float32 formulation's error on this mesh), weighted 1, 1 and 0.01 as in the loss: twice the weighted gates.  (2) The image term's
    # backward adds with float atomics: what two runs of the SAME restored step differ by, taken twice (the patched step is a third
    # draw).  (3) autograd adds the four terms' gradients into one float32 row: four roundings of half an ulp of the largest entry.
    gate = 2 * r["regulariser_gates"] + 2 * r["same_code_twice"] + 4 * 2.0 ** -24 * r["largest"]
    print(f"fitting step: difference {r['max_diff']:.2e}, gate {gate:.2e} = 2 x {r['regulariser_gates']:.2e} + 2 x {r['same_code_twice']:.2e} + "
          f"4 x 2^-24 x {r['largest']:.2e}")
    assert r["max_diff"] <= gate, r
