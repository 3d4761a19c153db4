"""sample_points_from_meshes (pytorch3d_amd/sample_points.py) on the CPU: the torch formulation of the contract against
tests/golden/sample_points_ref.npz (the reference's own code on recorded uniforms) and the float64 restatement of
tests/sample_points_case.py, through the SAME gates the GPU tests use (sample_points_case.gate_*) -- and three deliberately wrong
answers that those gates reject.  The public function's errors, tuple orders and generator; the drop-in patch in a process of its own.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sample_points_case as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p3d():
    import pytorch3d_amd as p3d

    return p3d


def _run(verts, faces, first, nf, S, u, return_normals=True, dtype=torch.float32):
    out = _p3d().sample_points_packed(verts.to(dtype), faces, first, nf, S, u, return_normals)
    return tuple(None if t is None else t.detach().numpy() for t in out)


class DuckMeshes:
    """What sample_points_from_meshes reads of a batch, with per-vertex features as textures."""

    def __init__(self, verts, faces, first, nf, features=None):
        self.v, self.f, self.first, self.nf = verts, faces, first, nf
        self.textures = features

    def __len__(self):
        return int(self.nf.numel())

    def verts_packed(self):
        return self.v

    def faces_packed(self):
        return self.f

    def mesh_to_faces_packed_first_idx(self):
        return self.first

    def num_faces_per_mesh(self):
        return self.nf

    def sample_textures(self, fragments):
        p2f, w = fragments.pix_to_face, fragments.bary_coords
        fa = self.textures[self.f[p2f.clamp_min(0)]]  # (N, S, 1, 1, 3, C)
        return torch.where((p2f >= 0)[..., None], (w[..., None] * fa).sum(-2), fa.new_zeros(()))


# ---- 1. the ragged batch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", C.SAMPLE_COUNTS)
def test_ragged_batch_matches_the_golden(S):
    g = C.golden()
    verts, faces, first, nf = C.golden_inputs(g)
    u = torch.from_numpy(g["uniforms_%d" % S])
    samples, normals, idx, bary = _run(verts, faces, first, nf, S, u)
    meshes = DuckMeshes(verts, faces, first, nf, torch.from_numpy(g["features"]))
    textures = _p3d().sample_points_from_meshes(meshes, S, return_textures=True, uniforms=u)[1].numpy()
    C.gate_ragged(S, samples, normals, idx, bary, textures, g)


# ---- 2. edge uniforms --------------------------------------------------------------------------------------------------------------
def _edge_outputs():
    verts, faces = C.edge_mesh()
    u = C.edge_uniforms()
    first, nf = torch.tensor([0]), torch.tensor([faces.shape[0]])
    return u, _run(verts, faces, first, nf, u.shape[1], u)


def test_edge_uniforms():
    u, (samples, normals, idx, _) = _edge_outputs()
    C.gate_edges(u, samples, normals, idx)


# ---- 5. the distribution -------------------------------------------------------------------------------------------------------------
def test_distribution_follows_the_areas():
    verts, faces = C.areas_mesh()
    S = 200000
    u = C.uniforms(1, S, 21)
    _, _, idx, _ = _run(verts, faces, torch.tensor([0]), torch.tensor([12]), S, u, return_normals=False)
    C.gate_distribution(idx, C.areas64(verts, faces))


# ---- 6. gradients ------------------------------------------------------------------------------------------------------------------
def _grad(verts, faces, first, nf, u, gs, gn, dtype=torch.float32):
    x = verts.to(dtype).clone().requires_grad_(True)
    samples, normals, idx, bary = _p3d().sample_points_packed(x, faces, first, nf, u.shape[1], u, gn is not None)
    outs, grads = [], []
    if gs is not None:
        outs.append(samples), grads.append(gs.to(dtype))
    if gn is not None:
        outs.append(normals), grads.append(gn.to(dtype))
    torch.autograd.backward(outs, grads)
    return x.grad.numpy(), idx.numpy(), bary.detach().numpy()


@pytest.mark.parametrize("which", ["samples", "normals", "both"])
def test_gradients_against_the_float64_restatement(which):
    g = C.golden()
    verts, faces, first, nf = C.golden_inputs(g)
    u = torch.from_numpy(g["uniforms_257"])
    gen = torch.Generator().manual_seed(5)
    gs = torch.randn(5, 257, 3, generator=gen) if which != "normals" else None
    gn = torch.randn(5, 257, 3, generator=gen) if which != "samples" else None
    got, idx, w = _grad(verts, faces, first, nf, u, gs, gn)
    C.gate_grads(verts, faces, idx, w, got, gs, gn, which)


def test_star_gradient_within_its_bound():
    verts, faces, u, gs = C.star()
    got, idx, w = _grad(verts, faces, torch.tensor([0]), torch.tensor([1]), u, gs, None)
    C.gate_star(idx, w, got)


# ---- wrong answers, rejected by the same gates -----------------------------------------------------------------------------------------
def test_the_gates_reject_a_lower_bound_choice():
    verts, faces = C.edge_mesh()
    u, (samples, normals, idx, _) = _edge_outputs()
    rows = C.tables64(C.areas64(verts, faces), torch.tensor([0]), torch.tensor([faces.shape[0]]))
    wrong = C.choose(rows, [0], u[:, :, 0].numpy(), lower_bound=True)  # u0 = 0 lands on the zero-area face in front
    assert not np.array_equal(wrong, idx)
    w = C.weights64(u.numpy())
    with pytest.raises(AssertionError):
        C.gate_edges(u, C.samples64(verts, faces, wrong, w).astype(np.float32), C.normals64(verts, faces, wrong).astype(np.float32), wrong)


def test_the_gates_reject_the_face_normals_clamp():
    verts, faces = C.edge_mesh()
    u, (samples, normals, idx, _) = _edge_outputs()
    wrong = C.normals64(verts, faces, idx, eps=1e-6).astype(np.float32)
    with pytest.raises(AssertionError):
        C.gate_edges(u, samples, wrong, idx)


def test_the_gates_reject_weights_in_the_wrong_order():
    g = C.golden()
    verts, faces, first, nf = C.golden_inputs(g)
    S = 65
    u = torch.from_numpy(g["uniforms_%d" % S])
    samples, normals, idx, bary = _run(verts, faces, first, nf, S, u)
    swapped = bary[..., [1, 0, 2]]
    wrong = C.samples64(verts, faces, idx, swapped).astype(np.float32)
    with pytest.raises(AssertionError):
        C.gate_ragged(S, wrong, normals, idx, bary, None, g)
    with pytest.raises(AssertionError):
        C.gate_ragged(S, samples, normals, idx, swapped, None, g)
    # and the gradient gate: the corners' gradients follow the weights
    gs = torch.randn(5, S, 3, generator=torch.Generator().manual_seed(2))
    wrong_grad, _ = C.grads64(verts, faces, idx, swapped, gs)
    with pytest.raises(AssertionError):
        C.gate_grads(verts, faces, idx, bary, wrong_grad, gs, None, "swapped weights")


# ---- 7. the public function --------------------------------------------------------------------------------------------------------
def _meshes(dtype=torch.float32, features=True):
    g = C.golden()
    verts, faces, first, nf = C.golden_inputs(g)
    return DuckMeshes(verts.to(dtype), faces, first, nf, torch.from_numpy(g["features"]).to(dtype) if features else None)


def test_value_errors():
    p3d = _p3d()
    with pytest.raises(ValueError, match="Meshes are empty."):
        p3d.sample_points_from_meshes(p3d.PackedMeshes([], []))
    empty = p3d.PackedMeshes([torch.rand(3, 3), torch.rand(4, 3)], [torch.zeros((0, 3), dtype=torch.int64)] * 2)
    with pytest.raises(ValueError, match="Meshes are empty."):
        p3d.sample_points_from_meshes(empty, 5)
    with pytest.raises(ValueError, match="Meshes do not contain textures."):
        p3d.sample_points_from_meshes(_meshes(features=False), 5, return_textures=True)
    bad = _meshes()
    bad.v = bad.v.clone()
    bad.v[7, 1] = float("nan")
    with pytest.raises(ValueError, match="Meshes contain nan or inf."):
        p3d.sample_points_from_meshes(bad, 5)
    out = p3d.sample_points_from_meshes(bad, 5, check_finite=False)  # no check: the call goes through
    assert out.shape == (5, 5, 3)


def test_tuple_orders_shapes_and_generator():
    p3d, m, S = _p3d(), _meshes(), 33
    u = C.uniforms(5, S, 1)
    s = p3d.sample_points_from_meshes(m, S, uniforms=u)
    assert torch.is_tensor(s) and s.shape == (5, S, 3)
    s1, n1 = p3d.sample_points_from_meshes(m, S, True, uniforms=u)
    s2, t2 = p3d.sample_points_from_meshes(m, S, False, True, uniforms=u)
    s3, n3, t3 = p3d.sample_points_from_meshes(m, S, return_normals=True, return_textures=True, uniforms=u)
    s4, n4, t4, i4 = p3d.sample_points_from_meshes(m, S, True, True, uniforms=u, return_face_idxs=True)
    for x in (s1, s2, s3, s4):
        assert torch.equal(x, s)
    assert torch.equal(n1, n3) and torch.equal(n1, n4) and torch.equal(t2, t3) and torch.equal(t2, t4)
    assert n1.shape == (5, S, 3) and t2.shape == (5, S, 3) and i4.shape == (5, S) and i4.dtype == torch.int64
    # unit normals where a face was hit, zero rows elsewhere; textures are convex combinations of features in [0, 1)
    hit = i4 >= 0
    assert torch.allclose(n1[hit].norm(dim=1), torch.ones(int(hit.sum())), atol=1e-5) and not n1[~hit].any()
    assert float(t2.min()) >= 0 and float(t2.max()) <= 1 and not t2[~hit].any()
    a = p3d.sample_points_from_meshes(m, S, generator=torch.Generator().manual_seed(7))
    b = p3d.sample_points_from_meshes(m, S, generator=torch.Generator().manual_seed(7))
    c = p3d.sample_points_from_meshes(m, S, generator=torch.Generator().manual_seed(8))
    assert torch.equal(a, b) and not torch.equal(a, c)
    torch.manual_seed(3)
    d = p3d.sample_points_from_meshes(m, S)
    torch.manual_seed(3)
    assert torch.equal(d, p3d.sample_points_from_meshes(m, S))
    # PackedMeshes is taken as well
    verts_list, faces_list = C.ragged_batch()
    pm = p3d.PackedMeshes(verts_list, faces_list)
    assert torch.equal(p3d.sample_points_from_meshes(pm, S, uniforms=u), s)


def test_float64_takes_the_formulation_and_agrees_with_the_restatement():
    g = C.golden()
    verts, faces, first, nf = C.golden_inputs(g)
    S = 257
    u = torch.from_numpy(g["uniforms_%d" % S])
    samples, normals, idx, bary = _run(verts, faces, first, nf, S, u, dtype=torch.float64)
    assert samples.dtype == np.float64
    rows = C.tables64(C.areas64(verts, faces), first, nf)
    assert np.array_equal(idx, C.choose(rows, first.tolist(), u[:, :, 0].numpy()))
    w = C.weights64(u.numpy()) * (idx >= 0)[..., None]
    assert np.abs(bary - w).max() <= 1e-15
    assert np.abs(samples - C.samples64(verts, faces, idx, w)).max() <= 1e-14
    assert np.abs(normals - C.normals64(verts, faces, idx)).max() <= 1e-13
    gs = torch.randn(5, S, 3, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    got, idx2, w2 = _grad(verts, faces, first, nf, u, gs, gs.flip(1), dtype=torch.float64)
    truth, scale = C.grads64(verts, faces, idx2, w2, gs.numpy(), gs.flip(1).numpy())
    assert np.abs(got - truth).max() <= 1e-12 * max(1.0, float(scale.max()))


def test_shim_patch_on_the_cpu():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    if not os.path.isdir(os.path.join(stage, "pytorch3d", "ops")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_sample_points_case.py"), "cpu"], capture_output=True, text=True,
                         timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    print(json.dumps(rec))
    assert rec["unpatched_is_the_reference"] and rec["patched_everywhere"] and rec["restored"]
    assert rec["golden_ok"], rec.get("golden_error")
    assert rec["fallback_calls"] >= 1 and rec["fused_calls"] == 0  # CPU tensors: the package's torch formulation
