"""csrc/point_mesh_grid.hip without a device: the two entries, the workspace function, the checks in front of any launch, the routing
predicate."""
import ctypes

import pytest
import torch

import _util as U  # noqa: F401  (puts the repository on the path)


def test_grid_entries_validate_before_any_launch_and_the_predicate_routes():
    from pytorch3d_amd import _C, _lib
    from pytorch3d_amd import point_mesh as pm

    for name in ("p3di_point_mesh_grid_forward_workspace_bytes", "p3di_point_mesh_grid_forward"):
        assert name in _lib.EXTENSION_DECLARATIONS and name not in _lib.DECLARATIONS
    lib = _lib.load()
    size = lib.p3di_point_mesh_grid_forward_workspace_bytes
    assert size(0, 100, 100) == 0 and size(-1, 100, 100) == 0 and size(2, -1, 5) == 0
    assert 0 < size(2, 500, 100) < size(2, 500, 1000) < size(2, 500, 100000) and size(2, 500, 100) < size(2, 50000, 100)

    null, some = ctypes.c_void_p(None), ctypes.c_void_p(4096)  # never dereferenced: every call below returns before a launch
    POINT, SEG, TRI = _lib.POINT_MESH_POINT, _lib.POINT_MESH_SEGMENT, _lib.POINT_MESH_TRIANGLE

    def fwd(qk=POINT, tk=TRI, N=2, Q=100, T=50, max_queries=60, occupancy=0, ptr=some, ws=some, nbytes=1 << 40):
        return lib.p3di_point_mesh_grid_forward(qk, tk, ptr, ptr, ptr, ptr, N, Q, T, max_queries, 5e-3, occupancy, null, ptr, ptr, null,
                                                ws, nbytes, null)

    bad = _lib.ERR_INVALID_ARG
    assert fwd(qk=POINT, tk=POINT) == bad and fwd(qk=TRI, tk=SEG) == bad and fwd(tk=7) == bad
    assert fwd(N=-1) == bad and fwd(Q=-1) == bad and fwd(T=-1) == bad and fwd(max_queries=-1) == bad and fwd(occupancy=-1) == bad
    assert fwd(Q=2 ** 31) == bad and fwd(T=2 ** 31 // 24 + 1) == bad
    assert fwd(ptr=null) == bad and fwd(N=0) == bad and fwd(max_queries=0) == bad  # rows nobody would write
    assert fwd(qk=TRI, tk=POINT) == _lib.ERR_UNSUPPORTED and fwd(qk=SEG, tk=POINT) == _lib.ERR_UNSUPPORTED
    assert fwd(ws=null) == _lib.ERR_WORKSPACE and fwd(nbytes=size(2, 100, 50) - 1) == _lib.ERR_WORKSPACE
    assert fwd(N=0, Q=0, ptr=null, ws=null, nbytes=0) == _lib.OK

    points, tris = torch.rand(10, 3), torch.rand(4, 3, 3)
    first = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        _C.point_mesh_grid_forward("point_face", points, first, tris, first, 10)
    prev = pm.GRID_MIN_TARGETS
    pm.GRID_MIN_TARGETS = 1
    try:
        assert not pm.grid_kernel_path("point_face", points, tris)  # CPU tensors
        assert not pm.grid_kernel_path("point_face", points.double(), tris.double())
        assert not pm.grid_kernel_path("face_point", points, tris) and not pm.grid_kernel_path("edge_point", points, tris[:, :2])
    finally:
        pm.GRID_MIN_TARGETS = prev
    assert prev is None or isinstance(prev, int)
