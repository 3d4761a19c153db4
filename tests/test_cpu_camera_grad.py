"""CPU suite: the C ABI of the camera gradients (include/p3d_amd.h: p3d_transform_backward_workspace_bytes,
p3d_transform_backward_cameras) is declared, bound and exported -- no GPU, no compute calls."""
import ctypes
import os
import re
import subprocess

import _util as U

HEADER = os.path.join(U.ROOT, "include", "p3d_amd.h")
ENTRIES = ("p3d_transform_backward_workspace_bytes", "p3d_transform_backward_cameras")


def _header_without_comments():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_two_entries_and_abi_version_stays_3():
    src = _header_without_comments()
    flat = " ".join(src.split())
    assert "size_t p3d_transform_backward_workspace_bytes(int64_t V, int N, int num_matrices);" in flat
    m = re.search(r"\bint p3d_transform_backward_cameras\((.*?)\);", flat)
    assert m, "p3d_transform_backward_cameras is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.rsplit(" ", 1)[0] for a in args] == ["const float*", "const int64_t*", "const float*", "const float*", "int64_t", "int", "int",
                                                   "float*", "float*", "void*", "size_t", "p3d_stream_t"], args
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+3\b", src)


def test_lib_carries_their_signatures():
    from pytorch3d_amd import _lib

    assert _lib.ABI_VERSION == 3
    p, i64, i, sz = _lib.c_ptr, _lib.c_i64, _lib.c_int, _lib.c_size
    assert _lib._SIGNATURES["p3d_transform_backward_workspace_bytes"] == (sz, [i64, i, i])
    assert _lib._SIGNATURES["p3d_transform_backward_cameras"] == (i, [p, p, p, p, i64, i, i, p, p, p, sz, p])
    for name in ENTRIES:
        assert name in _lib.EXPORTED_SYMBOLS


def test_built_library_exports_the_symbols_and_sizes_the_workspace_on_the_host():
    from pytorch3d_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "run `python -m pytorch3d_amd.build` (hipcc --offload-arch=gfx950)"
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (p3d_[a-z0-9_]+)", dyn))
    for name in ENTRIES:
        assert name in exported, name
    lib = _lib.load()
    assert lib.p3d_abi_version() == 3
    size = lib.p3d_transform_backward_workspace_bytes
    # one row of 32 floats per wave of 64 vertices, plus one per mesh when every mesh has matrices of its own
    assert size(0, 1, 1) == 0
    assert size(64, 1, 1) >= 128 and size(65, 1, 1) >= 2 * 128 and size(64, 1, 1) % 16 == 0
    assert size(1000, 3, 1) >= 16 * 128 and size(1000, 3, 3) >= 19 * 128
    assert size(1_000_000, 1, 1) <= 3 * 2 ** 20  # config 4: 15 625 waves, 2 MB
    # validation that precedes any launch
    null = ctypes.c_void_p(None)
    assert lib.p3d_transform_backward_cameras(null, null, null, null, 10, 2, 3, null, null, null, 0, null) == -1  # num_matrices
    assert lib.p3d_transform_backward_cameras(null, null, null, null, -1, 1, 1, null, null, null, 0, null) == -1


def test_tree_depth_restatement():
    from pytorch3d_amd.rasterize_meshes import camera_grad_tree_depth as depth

    assert depth(1) == 13 and depth(64 * 63) == 13  # up to 64 partial rows: one addition per lane in stage 2
    assert depth(64 * 63 + 1) == 14
    assert depth(64 * 300 + 7) == 12 + 5
    assert depth(1_000_000) == 257
