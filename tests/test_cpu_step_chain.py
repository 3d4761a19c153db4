"""Host side of the shortened step chain: the new entry p3d_rasterize_meshes_verts_ex and the flag
P3D_BWD_GRAD_OUT_ZEROED exist in the header and in the ctypes table, and what the entry refuses it refuses before it touches
a device (null and never-dereferenced pointers, on a machine without a GPU)."""
import ctypes
import os
import re

import _util as U

HEADER = os.path.join(U.ROOT, "include", "p3d_amd.h")


def test_header_and_ctypes_table_carry_the_entry_and_the_flag():
    from pytorch3d_amd import _C, _lib

    src = open(HEADER).read()
    assert re.search(r"\bint\s+p3d_rasterize_meshes_verts_ex\s*\(", src)
    m = re.search(r"#define\s+P3D_BWD_GRAD_OUT_ZEROED\s+(\d+)u", src)
    assert m and int(m.group(1)) == _lib.BWD_GRAD_OUT_ZEROED
    # a bit of its own, beside the two older flags
    assert _lib.BWD_GRAD_OUT_ZEROED & (_lib.BWD_COVER_HAS_LIST | _lib.BWD_MAKE_FACE_PRE) == 0
    assert bin(_lib.BWD_GRAD_OUT_ZEROED).count("1") == 1
    res, args = _lib._SIGNATURES["p3d_rasterize_meshes_verts_ex"]
    p, i, i64 = _lib.c_ptr, _lib.c_int, _lib.c_i64
    # verts, faces, V, face_verts, face_pre, zero_verts, then the arguments of p3d_rasterize_meshes_ex without its face_verts
    assert res is i and args[:6] == [p, p, i64, p, p, p]
    assert args[6:] == _lib._SIGNATURES["p3d_rasterize_meshes_ex"][1][1:]
    assert callable(getattr(_lib.load(), "p3d_rasterize_meshes_verts_ex"))
    # the switches of the call path, one per item
    assert _C.NULL_NEIGHBOR and _C.FUSED_GATHER and _C.PRECLEARED_GRAD


def test_verts_entry_validates_before_any_launch():
    from pytorch3d_amd import _lib

    lib = _lib.load()
    null = ctypes.c_void_p(None)
    some = ctypes.c_void_p(4096)  # never dereferenced: every call below returns before it would touch the device
    odd = ctypes.c_void_p(4096 + 4)
    INVALID = -1

    def call(verts=some, faces=some, V=10, face_verts=some, face_pre=null, zero=null, F=5, N=1, K=4, cover=null, flags=0, outs=some):
        return lib.p3d_rasterize_meshes_verts_ex(verts, faces, V, face_verts, face_pre, zero, some, some, null, F, N, 8, 8, 0.0, K, 0, 0,
                                                 0, 0, 0, outs, outs, outs, outs, cover, flags, null, 0, null)

    assert call(flags=4) == INVALID and call(flags=1 << 31) == INVALID  # unknown flag bits
    assert call(flags=_lib.RASTER_COVER_LIST) == INVALID  # a list needs its buffer
    assert call(cover=some, flags=_lib.RASTER_COVER_LIST | _lib.RASTER_CUDA_TIE_ORDER) == INVALID
    assert call(verts=null) == INVALID  # F > 0 and no vertices
    assert call(faces=null) == INVALID and call(face_verts=null) == INVALID
    assert call(face_verts=null, face_pre=some, F=0) == INVALID  # records without the faces they belong to, whatever F
    assert call(face_pre=odd) == INVALID  # records are read 16 bytes at a time
    assert call(V=-1) == INVALID and call(F=-1) == INVALID and call(N=-1) == INVALID
    assert call(K=151) == -2
    assert call(outs=null) == INVALID  # an output is missing
    # empty problems: nothing to gather, nothing to clear, nothing to write
    assert call(verts=null, faces=null, face_verts=null, V=0, F=0, N=0, outs=null) == 0
    assert call(verts=null, faces=null, face_verts=null, V=0, F=0, K=0, outs=null) == 0


def test_backward_flag_is_accepted_and_its_neighbour_bit_is_not():
    from pytorch3d_amd import _lib

    lib = _lib.load()
    null = ctypes.c_void_p(None)
    some = ctypes.c_void_p(4096)

    def bwd(F, V, faces, flags):
        return lib.p3d_rasterize_meshes_backward_ex(null, faces, null, null, null, null, null, null, F, V, 1, 8, 8, 4, 1, 1, flags, null,
                                                    null, 0, null)

    Z = _lib.BWD_GRAD_OUT_ZEROED
    assert bwd(0, 0, null, Z) == 0 and bwd(10, 0, some, Z | _lib.BWD_COVER_HAS_LIST) == 0  # empty outputs
    assert bwd(0, 0, null, Z | 4) == -1 and bwd(0, 0, null, 16) == -1  # unknown bits
    assert bwd(10, 5, some, Z) == -1  # grad_out is missing: refused before anything is cleared or launched
