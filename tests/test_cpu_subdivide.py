"""SubdivideMeshes and mesh_edges without a GPU: the torch formulation of pytorch3d_amd/subdivide_meshes.py against the reference's
recorded results and the loop restatement of tests/subdivide_case.py, bit for bit; the host logic and the wiring."""
import re

import pytest
import torch

import subdivide_case as C

import pytorch3d_amd as p3d
from pytorch3d_amd import _lib, build, shim
from pytorch3d_amd import subdivide_meshes as M


def result_of(verts, faces, feats):
    """A case through the public interface, in the layout of subdivide_case.restate."""
    meshes = p3d.PackedMeshes(verts, faces)
    new_meshes, new_feats = p3d.SubdivideMeshes()(meshes, feats)
    return {"edges": meshes.edges_packed(), "face_edges": meshes.faces_packed_to_edges_packed(),
            "num_edges": meshes.num_edges_per_mesh().to(torch.int64), "new_verts": new_meshes.verts_list(),
            "new_faces": new_meshes.faces_list(), "new_feats": new_feats}


@pytest.mark.parametrize("name", C.cases())
def test_formulation_equals_the_reference_and_the_restatement(name):
    verts, faces, feats = C.inputs(name)
    got = result_of(verts, faces, feats)
    assert C.misses(got, C.expected(name), name) == [] and C.misses(got, C.restate(verts, faces, feats), name) == []
    t = M.mesh_edges(p3d.PackedMeshes(verts, faces).faces_packed(), [v.shape[0] for v in verts], [f.shape[0] for f in faces])
    assert t.long_rows == C.LONG_ROWS.get(name, t.long_rows)
    assert torch.equal(t.edges_packed_to_mesh_idx(), torch.repeat_interleave(torch.arange(t.N), torch.tensor(t.num_edges, dtype=torch.int64)))


def test_empty_batch_and_float64():
    new_meshes, new_feats = p3d.SubdivideMeshes()(p3d.PackedMeshes([], []), torch.zeros((0, 4)))
    assert len(new_meshes) == 0 and new_feats.shape == (0, 4) and new_meshes.faces_packed().shape == (0, 3)
    verts, faces, feats = C.inputs("batch_of_4", dtype=torch.float64)
    assert C.misses(result_of(verts, faces, feats), C.restate(verts, faces, feats), "float64") == []


@pytest.mark.parametrize("packed_feats", [False, True])
def test_homogeneous_path(packed_feats):
    gen = torch.Generator().manual_seed(7)
    verts = [torch.randn((4, 3), generator=gen) for _ in range(3)]
    faces = [torch.tensor(C.TETRA)] * 3
    feats = torch.randn((3, 4, 5), generator=gen)
    meshes = p3d.PackedMeshes(verts, faces)
    module = p3d.SubdivideMeshes(meshes)
    assert module.precomputed and torch.equal(module._subdivided_faces, C.restate(verts[:1], faces[:1])["new_faces"][0])
    new_meshes, new_feats = module(meshes, feats.reshape(12, 5) if packed_feats else feats)
    want = C.restate(verts, faces, feats.reshape(12, 5))
    assert C.misses({"new_verts": new_meshes.verts_list(), "new_faces": new_meshes.faces_list(), "new_feats": new_feats.reshape(-1, 5)},
                    {k: want[k] for k in ("new_verts", "new_faces", "new_feats")}) == []
    assert new_feats.shape == (3, 10, 5)
    with pytest.raises(ValueError, match=re.escape("features need to be of shape (N, V, D) or (N*V, D)")):
        module(meshes, feats[None])


def test_errors_and_the_cache():
    faces = torch.tensor([[0, 1, 2], [1, 2, 7], [-3, 0, 1]])
    with pytest.raises(ValueError, match=re.escape("outside [0, 4): min -3, max 7")):
        M.mesh_edges(faces, [4], [3])
    with pytest.raises(ValueError, match="add up"):
        M.mesh_edges(faces, [4], [2])
    faces = torch.tensor(C.TETRA)
    a = M.mesh_edges(faces, [4], [4])
    assert M.mesh_edges(faces, [4], [4]) is a and M.mesh_edges(faces.clone(), [4], [4]) is not a and M.mesh_edges(faces, [5], [4]) is not a
    faces[0, 0] = 0  # an in-place write: the version moves
    assert M.mesh_edges(faces, [4], [4]) is not a


def test_wiring():
    header = open(_lib.EXTENSION_HEADER_PATH).read()
    for name in ("p3di_mesh_edges_workspace_bytes", "p3di_mesh_edges_build", "p3di_subdivide_faces", "p3di_subdivide_forward", "p3di_subdivide_backward"):
        assert re.search(r"\b%s\(" % name, header) and name in _lib.EXTENSION_SYMBOLS and name not in _lib.EXPORTED_SYMBOLS
    for const in ("MESH_EDGES_BLOCK", "MESH_EDGES_ITEMS", "MESH_EDGES_CARRY_BLOCK", "MESH_EDGES_ROW_REGISTERS", "MESH_EDGES_ROW_LDS",
                  "MESH_EDGES_LONG_GROUPS", "SUBDIVIDE_MAX_GROUPS"):
        assert const in _lib.EXTENSION_CONSTANTS and getattr(_lib, const) == _lib.EXTENSION_CONSTANTS[const] > 0
    assert "mesh_edges.hip" in build.SOURCES and "subdivide.hip" in build.SOURCES
    assert ("pytorch3d.ops.subdivide_meshes", ("pytorch3d.ops",), shim._subdivide_meshes) in shim._FUNCTION_PATCHES
    assert p3d.SubdivideMeshes is M.SubdivideMeshes and p3d.mesh_edges is M.mesh_edges and p3d.subdivide_packed is M.subdivide_packed
    assert not M.kernel_path(torch.zeros((4, 3))) and not M.edges_kernel_path(torch.zeros((4, 3), dtype=torch.int64), 4)
