"""pytorch3d_amd/mesh_normals.py without a GPU: the incidence list against a brute-force loop, the float64 restatement of the
vertex-normal kernels' formulas (the yardstick of tests/test_gpu_mesh_normals.py) against torch autograd of the reference's
formulation, and the new entries in the header and in the built library."""
import os
import re
import subprocess

import pytest
import torch

import _util as U
import mesh_normals_case as C


def _check_incidence(faces, V):
    from pytorch3d_amd import vert_incidence

    offsets, corners = vert_incidence(faces, V)
    want_off, want_corners = C.brute_incidence(faces, V)
    assert offsets.dtype == torch.int32 and corners.dtype == torch.int32
    assert offsets.tolist() == want_off
    assert corners.tolist() == want_corners
    return offsets, corners


def test_vert_incidence_two_mesh_packed_batch():
    v0, f0 = U.ico_sphere(1)
    v1, f1 = U.torus(0.5, 1.0, 5, 6)
    faces = torch.cat([f0, f1 + v0.shape[0]], 0)
    offsets, corners = _check_incidence(faces, v0.shape[0] + v1.shape[0])
    assert int(offsets[-1]) == corners.numel() == faces.numel()


def test_vert_incidence_vertex_without_a_face_repeated_vertex_and_negative_id():
    # vertex 2 has no face; face 1 names vertex 3 twice; -1 is vertex 5 (wraps once); 6 and -7 are out of range and dropped
    faces = torch.tensor([[0, 1, 4], [3, 3, 5], [-1, 0, 1], [6, 4, -7]], dtype=torch.int64)
    offsets, corners = _check_incidence(faces, 6)
    assert int(offsets[3]) - int(offsets[2]) == 0
    assert corners[int(offsets[3]):int(offsets[4])].tolist() == [3, 4]
    assert corners[int(offsets[5]):int(offsets[6])].tolist() == [5, 6]
    assert corners.numel() == 10
    # the trivial sizes
    o, c = _check_incidence(torch.zeros((0, 3), dtype=torch.int64), 4)
    assert o.tolist() == [0] * 5 and c.numel() == 0
    o, c = _check_incidence(torch.zeros((0, 3), dtype=torch.int64), 0)
    assert o.tolist() == [0] and c.numel() == 0


def test_float64_restatement_of_the_vertex_normal_formulas_matches_autograd_of_the_reference_formulation():
    verts, faces, eps = C.build_input()
    assert 420 <= verts.shape[0] <= 440 and 640 <= faces.shape[0] <= 660
    gen = torch.Generator().manual_seed(5)
    g = torch.randn(verts.shape, generator=gen, dtype=torch.float64)
    want_n, want_g = C.autograd_truth(verts, faces, g)
    got_n, sums = C.restated_forward(verts.double(), faces)
    got_g = C.restated_backward(g, verts.double(), faces, sums)
    assert float((got_n - want_n).abs().max()) < 1e-13
    # the eps group: sums exactly zero (in float32 as well), normals zero, gradients g / 1e-6 through the faces
    assert float(sums[eps].abs().max()) == 0.0 and float(got_n[eps].abs().max()) == 0.0
    assert float(C.restated_forward(verts, faces)[1][eps].abs().max()) == 0.0
    for group in (eps, ~eps):
        scale = float(want_g[group].abs().max())
        assert scale > 0 and float((got_g[group] - want_g[group]).abs().max()) < 1e-12 * scale
    assert float(want_g[eps].abs().max()) > 1e5 * float(want_g[~eps].abs().max())
    # the apex of the fan sums 200 faces
    assert int(torch.bincount(faces.reshape(-1)).max()) == 200


def test_cpu_and_float64_inputs_keep_the_torch_formulation_and_the_node_refuses_them():
    import pytorch3d_amd as p3d
    from pytorch3d_amd import _aux_ops as A

    v, f = U.ico_sphere(0)
    assert not A.fused_face_areas_normals(v, f) and not A.fused_face_areas_normals(v.double(), f)
    a, n = A.face_areas_normals_forward(v.double(), f)
    assert a.dtype == torch.float64 and n.shape == (20, 3)
    with pytest.raises(RuntimeError):
        p3d.verts_normals(v, f)
    with pytest.raises(RuntimeError):
        p3d.face_areas_normals(v, f)
    assert "not HIP kernels" not in A.__doc__


def test_new_entries_are_declared_and_exported():
    from pytorch3d_amd import _lib

    names = ("p3d_face_areas_normals_forward", "p3d_face_areas_normals_backward", "p3d_verts_normals_forward",
             "p3d_verts_normals_backward", "p3d_verts_normals_forward_workspace_bytes", "p3d_verts_normals_backward_workspace_bytes")
    header = open(os.path.join(U.ROOT, "include", "p3d_amd.h")).read()
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS
    assert os.path.exists(_lib.LIB_PATH), "run `python -m pytorch3d_amd.build` (hipcc --offload-arch=gfx950)"
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in names:
        assert re.search(r"\bT %s\b" % name, dyn), name
    lib = _lib.load()
    assert lib.p3d_verts_normals_forward_workspace_bytes(10) == 120 and lib.p3d_verts_normals_backward_workspace_bytes(10) == 360
    # argument checks and empty problems answer before anything is launched
    import ctypes

    null = ctypes.c_void_p(None)
    assert lib.p3d_face_areas_normals_forward(null, null, 5, 0, null, null, null) == 0
    assert lib.p3d_face_areas_normals_forward(null, null, -1, 3, null, null, null) == -1
    assert lib.p3d_face_areas_normals_forward(null, null, 5, 3, null, null, null) == -1
    assert lib.p3d_face_areas_normals_backward(null, null, null, null, 5, 3, null, null) == -1
    assert lib.p3d_verts_normals_forward(null, null, null, null, 0, 3, null, null, null, null) == 0
    assert lib.p3d_verts_normals_forward(null, null, null, null, 4, 3, null, null, null, null) == -1
    assert lib.p3d_verts_normals_backward(null, null, null, null, null, null, 0, 0, null, null, null) == 0
    assert lib.p3d_verts_normals_backward(null, null, null, null, null, null, 4, 2, null, null, null) == -1
    assert lib.p3d_verts_normals_forward(null, null, null, null, 4, 1 << 30, null, null, null, null) == -1  # 3 F beyond int32
