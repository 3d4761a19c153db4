"""csrc/mesh_edges.hip and csrc/subdivide.hip on the MI355X: integers and forward floats torch.equal to the reference's recording and
the loop restatement (tests/subdivide_case.py); the backward within its derived bound of float64, the same bits on every run."""
import json
import os
import subprocess
import sys

import pytest
import torch

import subdivide_case as C

import pytorch3d_amd as p3d
from pytorch3d_amd import subdivide_meshes as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _packed(verts, faces):
    meshes = p3d.PackedMeshes(verts, faces)
    return meshes, [v.shape[0] for v in verts], [f.shape[0] for f in faces]


def _kernels(verts, faces, feats):
    """A case through the kernels, in the layout of subdivide_case.restate; asserts that the kernels ran."""
    M.clear_mesh_edges_cache()
    meshes, nv, nf = _packed(verts, faces)
    before = dict(M.CALLS)
    out = p3d.subdivide_packed(meshes.verts_packed(), meshes.faces_packed(), nv, nf, feats=feats)
    assert M.CALLS["fused"] == before["fused"] + 1 and M.CALLS["edges_fused"] == before["edges_fused"] + 1
    assert M.CALLS["formulation"] == before["formulation"] and M.CALLS["edges_formulation"] == before["edges_formulation"]
    first = torch.tensor([0] + out.num_verts_per_mesh[:-1]).cumsum(0).repeat_interleave(torch.tensor(out.num_faces_per_mesh)).to(DEV)
    assert torch.equal(out.faces_packed, out.faces + first[:, None])
    return {"edges": meshes.edges_packed(), "face_edges": meshes.faces_packed_to_edges_packed(),
            "num_edges": meshes.num_edges_per_mesh().to(torch.int64), "new_verts": list(out.verts.split(out.num_verts_per_mesh, 0)),
            "new_faces": list(out.faces.split(out.num_faces_per_mesh, 0)), "new_feats": out.feats}, M.mesh_edges(meshes.faces_packed(), nv, nf)


@pytest.mark.parametrize("name", C.cases())
def test_cases_on_the_kernels(name):
    verts, faces, feats = C.inputs(name, DEV)
    got, tables = _kernels(verts, faces, feats)
    cpu = C.inputs(name)
    assert C.misses(got, C.expected(name), name) == [] and C.misses(got, C.restate(*cpu), name) == []
    assert tables.long_rows == C.LONG_ROWS.get(name, (0, 0))
    host = M.mesh_edges_build(p3d.PackedMeshes(cpu[0], cpu[1]).faces_packed(), tables.num_verts, tables.num_faces)  # the torch formulation
    for key in ("edge_mesh", "first_edge", "row_offsets", "hi_edges"):
        assert torch.equal(getattr(tables, key).cpu(), getattr(host, key)), key


@pytest.mark.parametrize("D,view", [(1, "plain"), (3, "plain"), (4, "plain"), (4, "unaligned"), (5, "strided"), (132, "plain"), (132, "strided")])
def test_feature_widths_and_views(D, view):
    verts, faces, _ = C.inputs("batch_of_4", DEV)
    V = sum(v.shape[0] for v in verts)
    base = torch.randn((V, 2 * D + 1), generator=torch.Generator().manual_seed(D)).to(DEV)
    feats = {"plain": base[:, :D].contiguous(), "unaligned": base.reshape(-1)[1:1 + V * D].view(V, D), "strided": base[:, 1::2][:, :D]}[view]
    assert feats.is_contiguous() == (view != "strided") and (view == "strided" or (feats.data_ptr() % 16 != 0) == (view == "unaligned"))
    got, _ = _kernels(verts, faces, feats)
    want = C.restate([v.cpu() for v in verts], [f.cpu() for f in faces], feats.cpu())
    assert C.misses(got, want, f"D{D}") == []


@pytest.mark.parametrize("name", ["vertex_twice", "batch_of_4", "fan_regs_plus_1", "ico_sphere_2"])
def test_backward_within_the_bound_and_the_same_bits(name):
    verts, faces, feats = C.inputs(name, DEV)
    meshes, nv, nf = _packed(verts, faces)
    gen = torch.Generator().manual_seed(5)
    grads = []
    for strict in (False, False, True):
        torch.use_deterministic_algorithms(strict)
        try:
            x, f = meshes.verts_packed().clone().requires_grad_(True), feats.clone().requires_grad_(True)
            out = p3d.subdivide_packed(x, meshes.faces_packed(), nv, nf, feats=f)
            if not grads:
                gv, gf = (torch.randn(t.shape, generator=gen).to(DEV) for t in (out.verts, out.feats))
            torch.autograd.backward([out.verts, out.feats], [gv, gf])
            grads.append((x.grad, f.grad))
        finally:
            torch.use_deterministic_algorithms(False)
    cpu = C.inputs(name)
    for got, g in zip(grads[0], (gv, gf)):
        want, bound = C.backward_truth(cpu[0], cpu[1], g)
        assert bool(((got.double().cpu() - want).abs() <= bound).all())
    assert all(torch.equal(a, b) for later in grads[1:] for a, b in zip(grads[0], later))


@pytest.mark.parametrize("packed_feats", [False, True])
def test_homogeneous_path(packed_feats):
    gen = torch.Generator().manual_seed(7)
    verts = [torch.randn((4, 3), generator=gen) for _ in range(3)]
    faces = [torch.tensor(C.TETRA)] * 3
    feats = torch.randn((3, 4, 5), generator=gen)
    meshes = p3d.PackedMeshes([v.to(DEV) for v in verts], [f.to(DEV) for f in faces])
    module = p3d.SubdivideMeshes(meshes)
    x = feats.to(DEV).requires_grad_(True)
    before = dict(M.CALLS)
    new_meshes, new_feats = module(meshes, x.reshape(12, 5) if packed_feats else x)
    assert M.CALLS["fused"] == before["fused"] + 1 and M.CALLS["formulation"] == before["formulation"]
    want = C.restate(verts, faces, feats.reshape(12, 5))
    assert C.misses({"new_verts": new_meshes.verts_list(), "new_faces": new_meshes.faces_list(), "new_feats": new_feats.detach().reshape(-1, 5)},
                    {k: want[k] for k in ("new_verts", "new_faces", "new_feats")}) == []
    g = torch.randn(new_feats.shape, generator=gen)
    new_feats.backward(g.to(DEV))
    for n in range(3):
        truth, bound = C.backward_truth(verts[n:n + 1], faces[n:n + 1], g[n])
        assert bool(((x.grad[n].double().cpu() - truth).abs() <= bound).all())


def test_a_bad_id_raises_and_an_empty_batch_is_empty():
    faces = torch.tensor([[0, 1, 2], [1, 2, 7], [-3, 0, 1]], device=DEV)
    with pytest.raises(ValueError, match=r"outside \[0, 4\): min -3, max 7"):
        M.mesh_edges(faces, [4], [3])
    new_meshes, new_feats = p3d.SubdivideMeshes()(p3d.PackedMeshes([], []), torch.zeros((0, 4), device=DEV))
    assert len(new_meshes) == 0 and new_feats.shape == (0, 4)


def test_the_shim_on_the_gpu():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.isdir(os.path.join(root, "oracle", "_ref", "reference_py", "pytorch3d", "ops")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(root, "tests", "shim_subdivide_case.py")], capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    print(json.dumps(rec))
    assert rec["misses"] == [] and rec["ico_sphere_equal"] and rec["ico_sphere_cpu_close"] and rec["forward_calls"] == [rec["forwards"], 0] and rec["faces_calls"][1] == 0
    assert rec["ico_sphere_calls"] == [3, 0]
    assert rec["cpu_forward_calls"] == [0, 1] and rec["restored"]
