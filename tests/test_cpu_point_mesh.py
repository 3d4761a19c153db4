"""Point-mesh distances without a GPU: the package's torch formulation against the reference's recorded results
(tests/golden/point_mesh_ref.npz, made by tests/golden/make_golden_point_mesh.py from the reference's own Python), the C entries'
validation, the shim's module, and the UNMODIFIED reference loss through the shim on CPU tensors.

Tolerances come from the fixture: a case and direction records E, the largest absolute error of the reference's float32 minima
against float64, and the same for either gradient; distances must lie within 4 E, gradients within 4 x their recorded error, indices
must be exact for the queries whose two smallest float64 distances differ by at least 16 E.
"""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import _util as U
import point_mesh_case as C


def _op_params():
    return [(kind, name, direction) for kind in C.KINDS for name in C.OP_CASES for direction in C.DIRECTIONS[kind]]


@pytest.mark.parametrize("kind,name,direction", _op_params())
def test_torch_formulation_matches_the_reference(kind, name, direction):
    from pytorch3d_amd import point_mesh as pm

    z = C.fixture()
    C.check_direction(z, kind, name, direction, *C.run_direction(pm, z, kind, name, direction), who="torch")


def test_chunked_formulation_equals_the_unchunked_one(monkeypatch):
    from pytorch3d_amd import point_mesh as pm

    z = C.fixture()
    points, pfirst, prims, sfirst, _, _ = C.op_inputs(z, "tri", "tiles")
    whole = [pm.torch_forward(d, points, pfirst, prims, sfirst) for d in C.DIRECTIONS["tri"]]
    monkeypatch.setattr(pm, "CHUNK_ELEMENTS", 1000)
    for d, (wd, wi) in zip(C.DIRECTIONS["tri"], whole):
        gd, gi = pm.torch_forward(d, points, pfirst, prims, sfirst)
        assert torch.equal(gd, wd) and torch.equal(gi, wi)


@pytest.mark.parametrize("kind", C.KINDS)
def test_exact_ties_go_to_the_larger_index(kind):
    from pytorch3d_amd import point_mesh as pm

    points, prims, twin = C.tie_case(kind)
    z1 = torch.zeros(1, dtype=torch.int64)
    _, idxs = pm.torch_forward(C.DIRECTIONS[kind][0], points, z1, prims, z1)
    assert torch.equal(twin[idxs], idxs), "the earlier copy of a duplicated primitive was returned"
    assert int((idxs >= 90).sum()) >= 10
    # points twice: a primitive's nearest point is the later copy
    _, idxs = pm.torch_forward(C.DIRECTIONS[kind][1], torch.cat([points, points], 0), z1, prims, z1)
    assert bool((idxs >= points.shape[0]).all())


def test_float64_inputs_take_the_formulation_in_float64():
    from pytorch3d_amd import point_mesh as pm

    z = C.fixture()
    points, pfirst, prims, sfirst, max_p, _ = C.op_inputs(z, "tri", "ragged", dtype=torch.float64)
    d = pm.point_face_distance(points, pfirst, prims, sfirst, max_p)
    best, _ = C.minima64(points, prims, *C.counts_of(z, "tri", "ragged"), True)
    # the formulation keeps the kernels' 1e-8 beside |n| (>= 2e-2 on these faces: their areas are >= 2 x the minimum), the restatement
    # divides by |n| alone: t differs by up to 5e-7 of itself, t^2 by 1e-6
    assert d.dtype == torch.float64 and bool(((d - best).abs() <= 1e-6 * best + 1e-12).all())


def _mesh_objects(z, name, device="cpu"):
    import pytorch3d_amd as p3d

    verts, faces, points = C.mesh_inputs(z, name, device=device)
    return verts, points, p3d.PackedMeshes(verts, faces), p3d.PackedPointclouds(points)


@pytest.mark.parametrize("name", ["ico2", "ragged"])
@pytest.mark.parametrize("tag", ["face", "edge"])
def test_mesh_level_losses_match_the_reference(name, tag):
    import pytorch3d_amd as p3d

    z = C.fixture()
    verts, points, meshes, pcls = _mesh_objects(z, name)
    loss = p3d.point_mesh_face_distance(meshes, pcls) if tag == "face" else p3d.point_mesh_edge_distance(meshes, pcls)
    grads = torch.autograd.grad(loss, verts + points)
    C.check_mesh_loss(z, name, tag, loss, grads[:len(verts)], grads[len(verts):], who="torch")


def test_small_faces_case_gives_the_same_loss_in_both_vertex_orders():
    """The reference's test_small_faces_case and its own criterion (assertClose: rtol 1e-5, atol 1e-8)."""
    import pytorch3d_amd as p3d

    z = C.fixture()
    got = []
    for name in ("small_faces_a", "small_faces_b"):
        _, _, meshes, pcls = _mesh_objects(z, name)
        got.append(float(p3d.point_mesh_face_distance(meshes, pcls)))
        want = float(z["mesh/%s/face_loss" % name])
        assert abs(got[-1] - want) <= 1e-5 * abs(want) + 1e-8
    assert abs(got[0] - got[1]) <= 1e-5 * abs(got[1]) + 1e-8


def test_unequal_batches_raise_the_reference_error():
    import pytorch3d_amd as p3d

    z = C.fixture()
    verts, points, meshes, _ = _mesh_objects(z, "ragged")
    with pytest.raises(ValueError, match="meshes and pointclouds must be equal sized batches"):
        p3d.point_mesh_face_distance(meshes, p3d.PackedPointclouds(points[:2]))
    with pytest.raises(ValueError, match="meshes and pointclouds must be equal sized batches"):
        p3d.point_mesh_edge_distance(meshes, p3d.PackedPointclouds(points[:2]))


def test_operator_wrappers_refuse_cpu_tensors_and_the_shim_serves_the_eight_names():
    from pytorch3d_amd import _C, point_mesh, shim

    z1 = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        _C.point_face_dist_forward(torch.rand(4, 3), z1, torch.rand(2, 3, 3), z1, 4, 5e-3)
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        _C.edge_point_dist_backward(torch.rand(4, 3), torch.rand(2, 2, 3), torch.zeros(2, dtype=torch.int64), torch.rand(2))
    assert len(_C.POINT_MESH_EXPORTS) == 8 and not set(_C.POINT_MESH_EXPORTS) & set(_C.HOT_PATH_EXPORTS)
    mod = shim.make_module()
    for name in _C.POINT_MESH_EXPORTS:
        assert getattr(mod, name) is getattr(point_mesh, name)
    for name in ("knn_points_idx", "point_face_array_dist_forward", "point_edge_array_dist_backward"):
        with pytest.raises(NotImplementedError):
            getattr(mod, name)(None)
    # on CPU tensors the operators answer with the torch formulation
    d, i = mod.point_edge_dist_forward(torch.zeros(1, 3), z1, torch.tensor([[[1.0, 0, 0], [1.0, 1, 0]]]), z1, 1)
    assert float(d) == 1.0 and int(i) == 0


def test_header_declares_the_entries_and_they_validate_before_any_launch():
    from pytorch3d_amd import _lib

    src = open(os.path.join(U.ROOT, "include", "p3d_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = ("p3d_point_mesh_forward_workspace_bytes", "p3d_point_mesh_forward", "p3d_point_mesh_backward_workspace_bytes",
             "p3d_point_mesh_backward")
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert not name.endswith("_ordered") and not name.endswith("_ordered_workspace_bytes")
    assert int(re.search(r"#define P3D_POINT_MESH_TILE (\d+)", src).group(1)) == C.TILE == _lib.POINT_MESH_TILE
    lib = _lib.load()
    assert lib.p3d_point_mesh_forward_workspace_bytes(3, 130) == 3 * 3 * 4  # one float per 64 queries of an element
    assert lib.p3d_point_mesh_forward_workspace_bytes(0, 130) == 0
    assert 0 < lib.p3d_point_mesh_backward_workspace_bytes(2, 100) <= lib.p3d_point_mesh_backward_workspace_bytes(2, 1000)
    assert lib.p3d_point_mesh_backward_workspace_bytes(0, 10000) < lib.p3d_point_mesh_backward_workspace_bytes(2, 10000)

    def fwd(qk, tk, N=1, Q=4, T=4, max_q=4, split=0, fake=None):
        p = fake
        return lib.p3d_point_mesh_forward(qk, tk, p, p, p, p, N, Q, T, max_q, 5e-3, split, None, p, p, None, None, 0, None)

    # arguments are checked before anything is launched: no device needed for these answers
    assert fwd(0, 0) == -1 and fwd(2, 1) == -1 and fwd(1, 2) == -1 and fwd(3, 0) == -1  # not a direction
    assert fwd(0, 2) == -1                                                            # null pointers
    assert fwd(0, 2, Q=-1) == -1
    assert fwd(0, 2, N=0, Q=0) == 0                                                   # nothing to do
    buf = (torch.zeros(64, dtype=torch.int64)).data_ptr()
    assert fwd(0, 2, split=3, fake=buf) == -1                                         # split is 0, 1, 2, 4 or 8
    assert fwd(0, 2, Q=4, max_q=0, fake=buf) == -1                                    # rows nobody would write
    assert lib.p3d_point_mesh_forward(0, 2, buf, buf, buf, buf, 1, 4, 4, 4, 5e-3, 0, None, buf, buf, buf, None, 0, None) == -4  # sums need the workspace

    def bwd(qk, tk, Q=4, T=4, first=(None, None), scale=None, sorted_hits=None, fake=None, ws=0):
        p = fake
        return lib.p3d_point_mesh_backward(qk, tk, p, p, p, None, scale, first[0], first[1], 1, Q, T, 5e-3, 0, sorted_hits, p, p, None, ws, None)

    assert bwd(0, 0) == -1 and bwd(0, 2) == -1
    assert bwd(2, 0, fake=buf, first=(buf, None)) == -1       # both first-index arrays or neither
    assert bwd(2, 0, fake=buf, scale=buf) == -1               # the element scale needs them
    assert bwd(0, 1, fake=buf, sorted_hits=buf) == -4         # the ordered sum needs its workspace
    assert bwd(0, 1, Q=2 ** 31, fake=buf) == -1


def _reference_root():
    stage = os.path.join(U.ROOT, "oracle", "_ref", "reference_py")
    return next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "loss"))), None)


def test_unmodified_reference_losses_run_through_the_shim_on_the_cpu():
    """`shim.install()` alone: the reference's point_mesh_face_distance / point_mesh_edge_distance end in the eight operators."""
    if _reference_root() is None:
        pytest.skip("the reference's Python package is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(U.ROOT, "tests", "shim_point_mesh_case.py"), "--cpu"], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    z = C.fixture()
    for name in ("ico2", "ragged"):
        for tag in ("face", "edge"):
            r = rec["plain"][name][tag]
            grads = [torch.tensor(g) for g in r["grads"]]
            n = len(grads) // 2
            C.check_mesh_loss(z, name, tag, r["loss"], grads[:n], grads[n:], who="reference through the shim (cpu)")
