"""csrc/knn_tree.hip without a device: the two entries, the workspace function, the checks in front of any launch, the routing
predicate."""
import ctypes

import pytest
import torch

import _util as U  # noqa: F401  (puts the repository on the path)


def test_tree_entries_validate_before_any_launch_and_small_clouds_keep_their_route():
    from pytorch3d_amd import _C, _lib, knn

    for name in ("p3di_knn_tree_forward_workspace_bytes", "p3di_knn_tree_forward"):
        assert name in _lib.EXTENSION_DECLARATIONS and name not in _lib.DECLARATIONS
    assert _lib.KNN_TREE_LEAF == 64 and _lib.KNN_TREE_FANOUT == 8
    lib = _lib.load()
    size = lib.p3di_knn_tree_forward_workspace_bytes
    assert size(0, 100, 100) == 0 and size(-1, 100, 100) == 0 and size(2, 0, 100) == 0 and size(2, 5, -1) == 0
    sizes = [size(2, 500, P2) for P2 in (0, 1, 64, 65, 2048, 2049, 5000, 100000, 1 << 20)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0] and size(2, 500, 100) < size(2, 50000, 100)

    null, some = ctypes.c_void_p(None), ctypes.c_void_p(4096)  # never dereferenced: every call below returns before a launch

    def fwd(N=2, P1=100, P2=50, D=3, K=8, ptr=some, ws=some, nbytes=1 << 40):
        return lib.p3di_knn_tree_forward(ptr, ptr, null, null, N, P1, P2, D, K, ptr, ptr, ws, nbytes, null)

    bad = _lib.ERR_INVALID_ARG
    assert fwd(N=-1) == bad and fwd(P1=-1) == bad and fwd(P2=-1) == bad and fwd(K=0) == bad and fwd(D=0) == bad
    assert fwd(P2=2 ** 30 + 1) == bad and fwd(ptr=null) == bad
    assert fwd(D=2) == _lib.ERR_UNSUPPORTED and fwd(D=4) == _lib.ERR_UNSUPPORTED and fwd(K=_lib.KNN_MAX_K + 1) == _lib.ERR_UNSUPPORTED
    assert fwd(ws=null) == _lib.ERR_WORKSPACE and fwd(nbytes=size(2, 100, 50) - 1) == _lib.ERR_WORKSPACE
    assert fwd(N=0, ptr=null, ws=null, nbytes=0) == _lib.OK and fwd(P1=0, ptr=null, ws=null, nbytes=0) == _lib.OK

    p1, p2 = torch.rand(1, 10, 3), torch.rand(1, 300, 3)
    with pytest.raises(RuntimeError):
        _C.knn_tree_idx(p1, p2, None, None, 4)
    # what the rule of DESIGN 8.33 gave: the smallest size from which the sweep saw the tree win everywhere
    prev = knn.TREE_MIN_P2
    assert prev == 262144 and knn.TREE_MAX_P == 2 ** 30 and not knn.tree_kernel_path(p1, p2, 4)
    knn.TREE_MIN_P2 = 1
    try:
        assert not knn.tree_kernel_path(p1, p2, 4) and not knn.tree_kernel_path(p1.double(), p2.double(), 4)  # CPU tensors
    finally:
        knn.TREE_MIN_P2 = prev
