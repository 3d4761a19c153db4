"""CPU suite, part 3: the C-ABI library and the host logic (no GPU, no compute calls).

* libp3d_amd.so loads and exports every function include/p3d_amd.h declares (and nothing in the
  header is missing from the ctypes table);
* entry points that can answer without a device (version, error strings, workspace sizing, argument
  validation that precedes any launch) behave;
* the `pytorch3d._C` surface mirrors the reference's pybind names / error behaviour and REFUSES CPU
  tensors (no fallback);
* host-side heuristics of the L2 mirror (bin size, max bins) follow the reference.
"""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import _util as U

HEADER = os.path.join(U.ROOT, "include", "p3d_amd.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(p3d_[a-z0-9_]+)\s*\(", src)))


def test_abi_v3_header_declares_the_operator_surface():
    names = _declared()
    for want in ("p3d_rasterize_meshes", "p3d_rasterize_meshes_naive", "p3d_rasterize_meshes_coarse",
                 "p3d_rasterize_meshes_fine", "p3d_rasterize_meshes_backward", "p3d_rasterize_points",
                 "p3d_rasterize_points_naive", "p3d_rasterize_points_coarse", "p3d_rasterize_points_fine",
                 "p3d_rasterize_points_ex", "p3d_rasterize_points_backward", "p3d_composite_forward", "p3d_composite_backward",
                 "p3d_interp_face_attrs_forward", "p3d_interp_face_attrs_backward", "p3d_sigmoid_alpha_blend_forward",
                 "p3d_sigmoid_alpha_blend_backward", "p3d_softmax_rgb_blend_forward", "p3d_softmax_rgb_blend_backward",
                 "p3d_gather_face_verts", "p3d_scatter_face_grads", "p3d_clip_faces_plan", "p3d_clip_faces_emit",
                 "p3d_clip_faces_backward", "p3d_convert_clipped_forward", "p3d_convert_clipped_backward"):
        assert want in names
    # ABI 3 folded these into p3d_rasterize_points_ex and into the compositors' feature strides
    for gone in ("p3d_rasterize_points_cuda_order", "p3d_rasterize_points_composite", "p3d_composite_forward_strided",
                 "p3d_composite_backward_strided"):
        assert gone not in names


def test_library_exports_every_declared_symbol():
    from pytorch3d_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "run `python -m pytorch3d_amd.build` (hipcc --offload-arch=gfx950)"
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (p3d_[a-z0-9_]+)", dyn))
    declared = set(_declared())
    assert declared <= exported, f"declared but not exported: {sorted(declared - exported)}"
    assert exported <= declared, f"exported but not declared in include/p3d_amd.h: {sorted(exported - declared)}"
    assert set(_lib.EXPORTED_SYMBOLS) == declared, "ctypes table out of sync with the header"


def test_library_contains_gfx950_code_object():
    from pytorch3d_amd import _lib

    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"mesh_raster_kernel" in blob


def test_abi_v3_library_loads_and_answers_without_a_device():
    from pytorch3d_amd import _lib

    lib = _lib.load()
    assert lib.p3d_abi_version() == 3
    assert b"150" in lib.p3d_error_string(-2) or b"K" in lib.p3d_error_string(-2)
    assert lib.p3d_error_string(0)
    # workspace sizing is pure host arithmetic
    a = lib.p3d_rasterize_meshes_workspace_bytes(10000, 4, 128, 128, 16, 1000)
    b = lib.p3d_rasterize_meshes_workspace_bytes(20000, 4, 128, 128, 16, 1000)
    assert 0 < a <= b
    assert lib.p3d_rasterize_meshes_workspace_bytes(10000, 4, 128, 128, 0, 0) == 0
    # short workspaces: the fixed arrays + the list entries asked for, never above the worst case; the needed-entries word
    # lies inside the fixed part, 8-byte aligned
    bench = (321_000, 64, 512, 512, 32, 64_200)
    worst = lib.p3d_rasterize_meshes_workspace_bytes(*bench)
    s0 = lib.p3d_rasterize_meshes_short_workspace_bytes(*bench, 0)
    s1 = lib.p3d_rasterize_meshes_short_workspace_bytes(*bench, 2_100_000)
    assert 0 < s0 < s1 < worst and s1 - s0 == pytest.approx(4 * 2_100_000, abs=512)
    assert worst > 1.2e9 and s1 < 12e6  # the bench batch: 1.3 GB -> 11 MB
    assert lib.p3d_rasterize_meshes_short_workspace_bytes(*bench, 1 << 40) <= worst
    at = lib.p3d_rasterize_meshes_workspace_need_offset(*bench)
    assert 0 < at < s0 and at % 8 == 0
    assert lib.p3d_rasterize_meshes_short_workspace_bytes(10000, 4, 128, 128, 0, 0, 100) == 0
    # round 5: the worst-case size counts the marks of the CUDA tie order in (one 64-bit lane mask per 8 x 8 sub-tile, taken off
    # the END of the workspace); the short size does not -- a caller of it adds them (_C._mesh_workspace(extra=...))
    marks = 64 * (512 // 8) * (512 // 8) * 8
    assert lib.p3d_rasterize_meshes_short_workspace_bytes(*bench, 1 << 40) + marks <= worst
    assert lib.p3d_rasterize_points_workspace_bytes(10000, 2, 64, 64, 8, 100) > 0
    # ... and a point list entry is (id, depth bits): 8 bytes
    pts = (1_000_000, 1, 512, 512, 32, 20_000)
    p0 = lib.p3d_rasterize_points_short_workspace_bytes(*pts, 0)
    p1 = lib.p3d_rasterize_points_short_workspace_bytes(*pts, 2_000_000)
    assert p1 - p0 == pytest.approx(8 * 2_000_000, abs=512) and p1 <= lib.p3d_rasterize_points_workspace_bytes(*pts)
    assert lib.p3d_rasterize_fine_workspace_bytes(2, 4, 4, 10) >= 2 * 16 * 10 * 4
    # validation that precedes any launch: K > 150, too many bins, null outputs
    null = ctypes.c_void_p(None)
    rc = lib.p3d_rasterize_meshes_naive(null, null, null, null, 0, 1, 8, 8, 0.0, 151, 0, 0, 0, null, null, null, null, null)
    assert rc == -2
    rc = lib.p3d_rasterize_meshes(null, null, null, null, 0, 1, 64, 64, 0.0, 4, 2, 10, 0, 0, 0, null, null, null, null,
                                  null, 0, null)
    assert rc in (-1, -3)
    rc = lib.p3d_rasterize_meshes_coarse(null, null, null, 0, 1, 64, 64, 0.0, 2, 10, null, null, 0, null)
    assert rc == -3
    # empty problems return OK before touching the device
    rc = lib.p3d_rasterize_meshes_naive(null, null, null, null, 0, 0, 8, 8, 0.0, 4, 0, 0, 0, null, null, null, null, null)
    assert rc == 0


def test_mesh_ex_entries_validate_before_any_launch():
    """p3d_rasterize_meshes_ex / p3d_rasterize_meshes_backward_ex: the checks that precede any device work, with null pointers."""
    from pytorch3d_amd import _lib

    lib = _lib.load()
    null = ctypes.c_void_p(None)
    some = ctypes.c_void_p(4096)  # never dereferenced: every call below returns before it would touch the device
    odd = ctypes.c_void_p(4096 + 4)  # not 16-byte aligned
    COVER_LIST, TIE = _lib.RASTER_COVER_LIST, _lib.RASTER_CUDA_TIE_ORDER

    def fwd(N, H, W, K, cover, flags):
        return lib.p3d_rasterize_meshes_ex(null, null, null, null, 0, N, H, W, 0.0, K, 0, 0, 0, 0, 0, null, null, null, null,
                                           cover, flags, null, 0, null)

    assert fwd(1, 8, 8, 151, null, 0) == -2  # K > 150
    assert fwd(-1, 8, 8, 4, null, 0) == -1 and fwd(1, -8, 8, 4, null, 0) == -1 and fwd(1, 8, 8, -4, null, 0) == -1
    assert fwd(1, 8, 8, 4, some, 4) == -1  # unknown flag bit
    assert fwd(1, 8, 8, 4, some, COVER_LIST | TIE) == -1
    assert fwd(1, 8, 8, 4, null, COVER_LIST) == -1  # a list needs its buffer
    assert fwd(0, 8, 8, 4, null, TIE) == 0 and fwd(1, 8, 8, 0, null, 0) == 0  # empty problems: OK

    def bwd(F, V, faces, face_pre, flags, N=1, K=4):
        return lib.p3d_rasterize_meshes_backward_ex(null, faces, face_pre, null, null, null, null, null, F, V, N, 8, 8, K, 1, 1,
                                                    flags, null, null, 0, null)

    for neg in ((-1, 0, 1, 4), (1, -1, 1, 4), (1, 0, -1, 4), (1, 0, 1, -4)):
        F, V, N, K = neg
        assert bwd(F, V, some, null, 0, N=N, K=K) == -1
    assert bwd(0, 0, null, null, 4) == -1  # unknown flag bit
    assert bwd(0, 0, null, odd, _lib.BWD_MAKE_FACE_PRE) == -1 and bwd(0, 5, some, odd, 0) == -1  # misaligned face_pre
    assert bwd(0, 0, null, some, _lib.BWD_MAKE_FACE_PRE | _lib.BWD_COVER_HAS_LIST) == 0  # F == 0: grad_face_verts is empty
    assert bwd(10, 0, some, some, 0) == 0  # V == 0: grad_verts is empty
    assert bwd(10, 0, null, null, 0) == -1  # F > 0 per face: the output is missing


def test_points_ex_entry_validates_before_any_launch():
    """p3d_rasterize_points_ex and the compositors: the checks that precede any device work, with null pointers."""
    from pytorch3d_amd import _lib

    lib = _lib.load()
    null = ctypes.c_void_p(None)
    some = ctypes.c_void_p(4096)  # never dereferenced: every call below returns before it would touch the device
    COVER_LIST, TIE = _lib.RASTER_COVER_LIST, _lib.RASTER_CUDA_TIE_ORDER

    def fwd(N, H, W, K, flags=0, images=null, C=3, mode=0, P=0, features=null, ptr=null, bins=(0, 0)):
        return lib.p3d_rasterize_points_ex(ptr, ptr, ptr, ptr, P, N, H, W, K, *bins, ptr, ptr, ptr, mode, features, C, 1.0, images, flags,
                                           null, 0, null)

    assert fwd(1, 8, 8, 151) == -2 and fwd(1, 8, 8, 151, images=some) == -2  # K > 150
    assert fwd(-1, 8, 8, 4) == -1 and fwd(1, -8, 8, 4) == -1 and fwd(1, 8, -8, 4) == -1 and fwd(1, 8, 8, -4) == -1
    assert fwd(1, 8, 8, 4, flags=4) == -1  # unknown flag bit
    assert fwd(0, 8, 8, 4, flags=COVER_LIST) == -1  # the meshes' flag
    assert fwd(0, 8, 8, 4, flags=TIE, images=some) == -1  # no caller reaches this combination
    # with images: C outside 1..4 or a bad mode, checked before the sizes; without images C and the mode are ignored
    for C, mode in ((0, 0), (5, 0), (3, 2), (3, -1)):
        assert fwd(0, 8, 8, 4, images=some, C=C, mode=mode) == -1 and fwd(1, 8, 8, 151, images=some, C=C, mode=mode) == -1
        assert fwd(0, 8, 8, 4, C=C, mode=mode) == 0
    assert fwd(1, 8, 8, 4, images=some, P=10) == -1  # points but no features
    # empty problems return OK; null outputs of a non-empty one do not
    assert fwd(0, 8, 8, 4) == 0 and fwd(1, 0, 8, 4) == 0 and fwd(1, 8, 8, 0) == 0 and fwd(0, 8, 8, 4, flags=TIE) == 0
    assert fwd(0, 8, 8, 4, images=some, P=10, features=some) == 0 and fwd(1, 8, 0, 4, images=some) == 0
    assert fwd(1, 8, 8, 4) == -1 and fwd(1, 8, 8, 4, flags=TIE) == -1 and fwd(1, 8, 8, 4, images=some) == -1
    # binned: too many bins, then the workspace
    assert fwd(1, 64, 64, 4, ptr=some, bins=(2, 10)) == -3 and fwd(1, 64, 64, 4, ptr=some, bins=(16, 10)) == -4
    # the reference-signature entries check the same way
    assert lib.p3d_rasterize_points(null, null, null, null, 0, 1, 8, 8, 151, 0, 0, null, null, null, null, 0, null) == -2
    assert lib.p3d_rasterize_points_naive(null, null, null, null, 0, 1, 8, 8, 151, null, null, null, null) == -2
    assert lib.p3d_rasterize_points_naive(null, null, null, null, 0, 0, 8, 8, 4, null, null, null, null) == 0

    # the compositors take (P, 1) planes, (1, C) rows or null (planes) as feature strides, nothing else
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
    st4 = i64(0, 0, 0, 0)
    for bad in (i64(20, 2), i64(1, 1), i64(10, 3)):  # C = 3, P = 10
        assert lib.p3d_composite_forward(0, some, bad, some, some, 1, 3, 10, 2, 4, 4, st4, st4, some, null) == -1
        assert lib.p3d_composite_backward(0, some, some, bad, some, some, 1, 3, 10, 2, 4, 4, st4, st4, some, None, some, null) == -1
        assert lib.p3d_composite_backward(0, some, some, None, some, some, 1, 3, 10, 2, 4, 4, st4, st4, some, bad, some, null) == -1


def test_stale_library_fails_in_load(monkeypatch):
    """A library of another ABI version is refused by _lib.load() before any symbol of this one is looked up."""
    from pytorch3d_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "ABI_VERSION", _lib.ABI_VERSION + 1)
    with pytest.raises(_lib.ExtensionMissing, match="ABI version"):
        _lib.load()


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    from pytorch3d_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libp3d_amd.so"))
    with pytest.raises(_lib.ExtensionMissing, match="no CPU/eager fallback"):
        _lib.load()


def test_operator_surface_names_match_the_reference_pybind_module():
    """pytorch3d/csrc/ext.cpp:38-73 (hot-path subset) + the constants read at import (ext.cpp:180-185)."""
    from pytorch3d_amd import _C, shim

    ref_names = ["rasterize_meshes", "rasterize_meshes_backward", "_rasterize_meshes_naive", "_rasterize_meshes_coarse",
                 "_rasterize_meshes_fine", "rasterize_points", "rasterize_points_backward", "_rasterize_points_naive",
                 "_rasterize_points_coarse", "_rasterize_points_fine", "accum_alphacomposite",
                 "accum_alphacomposite_backward", "accum_weightedsumnorm", "accum_weightedsumnorm_backward",
                 "accum_weightedsum", "accum_weightedsum_backward", "interp_face_attrs_forward",
                 "interp_face_attrs_backward", "sigmoid_alpha_blend", "sigmoid_alpha_blend_backward"]
    mod = shim.make_module()
    for n in ref_names:
        assert callable(getattr(_C, n)) and callable(getattr(mod, n))
    assert (mod.EPS, mod.MAX_INT, mod.MAX_UINT, mod.MAX_USHORT, mod.PULSAR_MAX_GRAD_SPHERES) == (
        1e-6, 2147483647, 4294967295, 65535, 128)
    with pytest.raises(NotImplementedError):
        mod.knn_points_idx(None)


def test_cpu_tensors_are_refused_not_emulated():
    from pytorch3d_amd import _C

    fv = torch.rand(4, 3, 3)
    z = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU path only"):
        _C.rasterize_meshes(fv, z, z + 4, torch.full((4,), -1, dtype=torch.int64), (8, 8), 0.0, 2, 0, 0, False, False,
                            False)
    with pytest.raises(RuntimeError, match="GPU path only"):
        _C.accum_alphacomposite(torch.rand(3, 5), torch.rand(1, 2, 4, 4), torch.zeros(1, 2, 4, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU path only"):
        _C.interp_face_attrs_forward(torch.zeros(5, dtype=torch.int64), torch.rand(5, 3), torch.rand(2, 3, 4))


def test_l2_mirror_heuristics_follow_the_reference():
    """rasterize_meshes.py:195-222 / rasterize_points.py:104-126."""
    import importlib

    rm = importlib.import_module("pytorch3d_amd.rasterize_meshes")

    assert rm.default_bin_size(64) == 8
    assert rm.default_bin_size(65) == 16
    assert rm.default_bin_size(256) == 16
    assert rm.default_bin_size(512) == 32
    assert rm.default_bin_size(1024) == 64
    assert rm.parse_image_size(32) == (32, 32)
    assert rm.parse_image_size((20, 48)) == (20, 48)
    with pytest.raises(ValueError):
        rm.parse_image_size((0, 4))

    class M:
        _F = 10

        def verts_packed(self):
            return torch.rand(6, 3)

        def faces_packed(self):
            return torch.tensor([[0, 1, 2], [3, 4, 5]])

        def mesh_to_faces_packed_first_idx(self):
            return torch.tensor([0])

        def num_faces_per_mesh(self):
            return torch.tensor([2])

    with pytest.raises(ValueError, match="bin_size too small"):
        rm.rasterize_meshes(M(), image_size=512, bin_size=8)  # tests/test_rasterize_meshes.py:461-466
    with pytest.raises(RuntimeError, match="GPU path only"):  # clipping is implemented: it reaches the GPU check
        rm.rasterize_meshes(M(), image_size=32, z_clip_value=0.1)


def test_packed_containers_match_reference_accessors():
    import pytorch3d_amd as p3d

    v = [torch.rand(5, 3), torch.rand(7, 3)]
    f = [torch.tensor([[0, 1, 2], [2, 3, 4]]), torch.tensor([[0, 5, 6]])]
    m = p3d.PackedMeshes(v, f)
    assert len(m) == 2
    assert m.verts_packed().shape == (12, 3)
    assert m.faces_packed().tolist() == [[0, 1, 2], [2, 3, 4], [5, 10, 11]]
    assert m.mesh_to_faces_packed_first_idx().tolist() == [0, 2]
    assert m.num_faces_per_mesh().tolist() == [2, 1]
    assert m._F == 2


def test_shading_host_logic_packs_broadcasts_and_refuses():
    """pytorch3d_amd/shading.py host side (no GPU): the (N, 25) parameter block of p3d_phong_shade_*, light-kind
    detection, (1,3)/(N,3) broadcasting, loud refusals."""
    from collections import namedtuple

    import pytorch3d_amd as p3d
    import pytorch3d_amd.shading as sh

    class Cam:
        def get_camera_center(self):
            return torch.tensor([[0.0, 0.0, -3.0]])

    M = sh.Materials(torch.ones(1, 3), torch.full((1, 3), 0.5), torch.full((1, 3), 0.25), torch.tensor([64.0]))
    point = sh.Lights(torch.tensor([[0.1, 0.2, 0.3]]), torch.rand(3, 3), torch.rand(1, 3), location=torch.rand(3, 3))
    params, kind = sh.pack_shade_params(point, Cam(), M, 3, torch.device("cpu"))
    assert params.shape == (3, sh.PARAM_FLOATS) and params.is_contiguous() and kind == sh.LIGHT_POINT
    assert torch.equal(params[:, 0:3], torch.tensor([[0.1, 0.2, 0.3]]).expand(3, 3))
    assert torch.equal(params[:, 3:6], point.diffuse_color) and torch.equal(params[:, 9:12], point.location)
    assert torch.equal(params[:, 21], torch.full((3,), 64.0)) and torch.equal(params[:, 22:25], torch.tensor([[0.0, 0.0, -3.0]]).expand(3, 3))
    direc = sh.Lights(torch.ones(1, 3), torch.ones(1, 3), torch.ones(1, 3), direction=torch.tensor([[0.0, 1.0, 0.0]]))
    assert sh.pack_shade_params(direc, Cam(), M, 2, torch.device("cpu"))[1] == sh.LIGHT_DIRECTIONAL
    amb = sh.Lights(torch.full((1, 3), 0.7), diffuse_color=torch.ones(1, 3))  # ambient-only: diffuse / specular ignored
    pa, ka = sh.pack_shade_params(amb, Cam(), M, 2, torch.device("cpu"))
    assert ka == sh.LIGHT_DIRECTIONAL and pa[:, 3:12].abs().max() == 0 and torch.all(pa[:, 0:3] == 0.7)
    with pytest.raises(ValueError, match="must have shape"):
        sh.pack_shade_params(point, Cam(), M, 2, torch.device("cpu"))  # (3,3) lights against a batch of 2
    # the packing is differentiable: a light / material / camera tensor that requires grad gets its gradient through it
    loc = torch.rand(3, 3, requires_grad=True)
    pg, _ = sh.pack_shade_params(point._replace(location=loc), Cam(), M, 3, torch.device("cpu"))
    pg[:, 9:12].sum().backward()
    assert torch.equal(loc.grad, torch.ones(3, 3))
    # no CPU emulation of the fused kernels
    Frag = namedtuple("Frag", "pix_to_face bary_coords")
    m = p3d.PackedMeshes([torch.rand(4, 3)], [torch.tensor([[0, 1, 2], [1, 2, 3]])])
    frag = Frag(torch.zeros(1, 2, 2, 1, dtype=torch.int64), torch.rand(1, 2, 2, 1, 3))
    with pytest.raises(RuntimeError, match="GPU path only"):
        p3d.phong_shading(m, frag, direc, Cam(), M, torch.rand(1, 2, 2, 1, 3))
    # the container's normals follow Meshes._compute_vertex_normals / mesh_face_areas_normals
    assert torch.allclose(m.verts_normals_packed().norm(dim=1), torch.ones(4), atol=1e-6)
    assert torch.allclose(m.faces_normals_packed().norm(dim=1), torch.ones(2), atol=1e-6)
    assert m.verts_packed_to_mesh_idx().tolist() == [0, 0, 0, 0]


def test_uv_sampling_host_logic_refuses_loudly():
    """pytorch3d_amd/textures.py host side (no GPU): argument checks, no CPU emulation."""
    from collections import namedtuple

    import pytorch3d_amd as p3d

    Frag = namedtuple("Frag", "pix_to_face bary_coords")
    frag = Frag(torch.zeros(1, 2, 2, 1, dtype=torch.int64), torch.rand(1, 2, 2, 1, 3))
    fu, maps = torch.rand(3, 3, 2), torch.rand(1, 4, 4, 3)
    with pytest.raises(NotImplementedError, match="padding_mode"):
        p3d.sample_textures_uv(frag, fu, maps, padding_mode="reflection")
    with pytest.raises(ValueError, match="sampling_mode"):
        p3d.sample_textures_uv(frag, fu, maps, sampling_mode="bicubic")
    with pytest.raises(RuntimeError, match="GPU path only"):
        p3d.sample_textures_uv(frag, fu, maps)


def test_shared_reciprocal_division_is_exact_and_fast_path_equals_plain_path():
    """csrc/p3d_geom.h, compiled for the host: (1) exact_div -- (float)((double)n * rd) -- equals IEEE n / d for every rd
    within one double ulp of 1/d (30M triples); (2) the fine kernel's fast path (rectangle prune + face_hit_rec on
    FaceRecs) produces bit-identical rasterizations to the plain reference-order path on random soups, with and without
    blur, all flag combinations, including degenerate and tiny faces."""
    import ctypes

    import _util as U

    hg = U.hostgeom()
    hg.hg_exact_div_check.restype = ctypes.c_int64
    hg.hg_exact_div_check.argtypes = [ctypes.c_int64, ctypes.c_uint64]
    assert hg.hg_exact_div_check(10_000_000, 12345) == 0
    gen = torch.Generator().manual_seed(5)
    for case, (blur, persp, clip, cull) in enumerate([(0.0, False, False, False), (1e-4, True, True, False),
                                                     (9.2e-4, True, True, False), (0.01, True, False, True),
                                                     (0.003, False, True, False)]):
        F = 160
        fv = U.triangle_soup(F, gen, size=0.6 if case % 2 else 0.15, behind_every=13)
        fv[5::17, 2] = fv[5::17, 1] + 1e-5  # slivers with a near-degenerate edge
        fv[3::29, 1, :2] = fv[3::29, 0, :2]  # exactly degenerate edge
        fv[7::31] *= torch.tensor([1e-3, 1e-3, 1.0])  # tiny faces near the image centre
        first, count = U.split_counts(F, 2)
        nbr = torch.full((F,), -1, dtype=torch.int64)
        for size in ((40, 40), (24, 56)):
            plain = U.hg_rasterize_meshes(fv, first, count, nbr, size, blur, 8, persp, clip, cull, use_mem=0)
            fast = U.hg_rasterize_meshes(fv, first, count, nbr, size, blur, 8, persp, clip, cull, use_mem=2)
            for a, b in zip(plain, fast):
                assert torch.equal(a, b), (case, size)


def test_pixel_masks_equal_the_per_pixel_bbox_test():
    """csrc/p3d_geom.h: range_mask16 / block_mask_8x8 -- the fine rasterizer takes a face's bounding-box test once per
    (face, tile column) and (face, tile row) and hands the pixels inside to a visit as a 64-bit lane mask; the reference
    tests every pixel (rasterize_meshes.cu:94-97, strict comparisons).  Host build of the header: 128M (pixel, box) pairs on
    random image sizes, partial tiles, edges exactly on pixel centres, NaN edges -- the mask bit equals the per-pixel test."""
    import ctypes

    import _util as U

    hg = U.hostgeom()
    hg.hg_pixel_mask_check.restype = ctypes.c_int64
    hg.hg_pixel_mask_check.argtypes = [ctypes.c_int64, ctypes.c_uint64]
    assert hg.hg_pixel_mask_check(500_000, 3) == 0


def test_point_rasterizer_host_logic():
    """pytorch3d_amd/rasterize_points.py: radius forms, the reference's bin-size heuristic (rasterize_points.py:104-113, no
    "<= 64 -> 8" special case as meshes have) and its error; the kernels themselves refuse CPU tensors."""
    import importlib

    import pytorch3d_amd as p3d

    rp = importlib.import_module("pytorch3d_amd.rasterize_points")  # the package re-exports the function under this name

    assert [rp.default_bin_size(s) for s in (16, 64, 256, 257, 512, 1024)] == [16, 16, 16, 32, 32, 64]
    pts = [torch.rand(5, 3), torch.rand(3, 3)]
    pc = p3d.PackedPointclouds(pts)
    r = rp.radius_per_packed_point(0.25, pc)
    assert r.shape == (8,) and r.dtype == torch.float32 and bool((r == 0.25).all())
    packed = torch.arange(8, dtype=torch.float32)
    assert torch.equal(rp.radius_per_packed_point(packed, pc), packed)
    padded = torch.arange(10, dtype=torch.float32).reshape(2, 5)
    assert torch.equal(rp.radius_per_packed_point(padded, pc), torch.tensor([0., 1., 2., 3., 4., 5., 6., 7.]))
    one = p3d.PackedPointclouds([torch.rand(4, 3)])
    assert torch.equal(rp.radius_per_packed_point([1.0, 2.0, 3.0, 4.0], one), torch.tensor([1., 2., 3., 4.]))
    with pytest.raises(ValueError, match="shape"):
        rp.radius_per_packed_point(torch.rand(2, 4), pc)
    with pytest.raises(ValueError, match="float, list, tuple or tensor"):
        rp.radius_per_packed_point("0.1", pc)
    with pytest.raises(ValueError, match="bin_size too small"):
        p3d.rasterize_points(pc, image_size=512, bin_size=8)
    with pytest.raises(RuntimeError, match="GPU path only"):
        p3d.rasterize_points(pc, image_size=32, radius=0.1)


def test_bench_jobs_partition_and_fast_path_on_the_cow():
    """(1) bench.py --jobs (BASELINE configs[4]): 512 jobs = 8 sub-batches of 64 dealt to 1 / 2 / 4 / 8 ranks, every sub-batch
    exactly once.  (2) The fine kernel's fast path (csrc/p3d_geom.h compiled for the host: rectangle prune + FaceRec
    evaluation) on REAL geometry: the reference's cow at 96x96, K=8, blur 1e-4 -- bit-identical to the plain reference-order
    path and to the C oracle."""
    import importlib.util

    import numpy as np

    import _util as U
    from oracle import oracle as orc

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(U.ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for world in (1, 2, 4, 8):
        got = sorted(s for r in range(world) for s in bench.sub_batches_of_rank(512, 64, r, world))
        assert got == list(range(8))
        assert all(len(bench.sub_batches_of_rank(512, 64, r, world)) == 8 // world for r in range(world))
    # an uneven deal (round 6): 8 sub-batches over 3 ranks = 3 + 3 + 2, every sub-batch exactly once; rank 0 never has fewer than another
    deal = [bench.sub_batches_of_rank(512, 64, r, 3) for r in range(3)]
    assert [len(d) for d in deal] == [3, 3, 2] and sorted(s for d in deal for s in d) == list(range(8))
    with pytest.raises(SystemExit):
        bench.sub_batches_of_rank(512, 64, 0, 9)  # a rank would have nothing to run
    with pytest.raises(SystemExit):
        bench.sub_batches_of_rank(500, 64, 0, 1)

    g = np.load(os.path.join(U.GOLDEN, "cow_ref.npz"))
    fv = torch.from_numpy(g["verts_ndc"])[torch.from_numpy(g["faces"]).long()].contiguous()
    F = fv.shape[0]
    first = torch.zeros(1, dtype=torch.int64)
    count = torch.tensor([F], dtype=torch.int64)
    nbr = torch.full((F,), -1, dtype=torch.int64)
    size, blur, K = (96, 96), 1e-4, 8
    plain = U.hg_rasterize_meshes(fv, first, count, nbr, size, blur, K, True, True, False, use_mem=0)
    fast = U.hg_rasterize_meshes(fv, first, count, nbr, size, blur, K, True, True, False, use_mem=2)
    ref = orc.rasterize_meshes_naive(fv, first, count, nbr, size, blur, K, True, True, False)
    for a, b, c in zip(plain, fast, ref):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert int((ref[0] >= 0).sum()) > 1000


def test_pair_register_queue_scheme_matches_the_register_queue():
    """csrc/topk.h: TopKPairs (entries in 64-bit register pairs, insertion = two masked pair moves per entry; the queue of
    the K = 4, 8, 16 mesh kernels and of the common point capacities since round 3) against TopKReg on 200k random
    operation sequences with depth ties, repeated indices, find and erase.  On the host the masked moves are plain ifs:
    this pins the scheme; the v_pk_mov_b32 / exec sequence itself is what the whole GPU suite runs."""
    import ctypes

    hg = U.hostgeom()
    hg.hg_queue_pairs_check.restype = ctypes.c_int64
    hg.hg_queue_pairs_check.argtypes = [ctypes.c_int64, ctypes.c_uint64]
    assert hg.hg_queue_pairs_check(200_000, 99) == 0
    # the payload-free form of the point queues, with and without the 64-bit key compare
    hg.hg_queue_pairs0_check.restype = ctypes.c_int64
    hg.hg_queue_pairs0_check.argtypes = [ctypes.c_int64, ctypes.c_uint64]
    assert hg.hg_queue_pairs0_check(200_000, 7) == 0


def test_no_kernel_of_the_library_spills_vgprs():
    """pytorch3d_amd/build.py records the compiler's per-kernel resource usage next to the library and refuses a build in which
    a kernel spills VGPRs: in round 4 every kernel of raster_mesh.hip that did lost queue entries on the GPU, bit-exact again as
    soon as it fitted its registers (profiles/r04/spill_miscompile.md).  Scratch itself is fine where it is the design (the
    private-memory queue TopKMem for K > 64 / > 100; the replay of the reference's 150-entry array in the *_cuda_order kernels)."""
    import json

    from pytorch3d_amd import build as B

    path = B.LIB + ".resources.json"
    assert os.path.exists(path), "build the library with `python -m pytorch3d_amd.build` (conftest does)"
    res = json.load(open(path))
    assert len(res) > 150
    spilled = {B.demangle(k): v["vgpr_spill"] for k, v in res.items() if v["vgpr_spill"] != 0}
    assert not spilled, spilled
    scratch = sorted(B.demangle(k) for k, v in res.items() if v["scratch"] > 0)
    assert all("TopKMem" in k or "_cuda_order_kernel" in k for k in scratch), scratch
    # round 5: registers kept in AGPRs only in kernels that name the GPU test which fills every register row
    agpr = sorted(B.demangle(k) for k, v in res.items() if v["agprs"] > 0)
    assert all(any(t + "(" in k for t in B.AGPR_KERNELS_TESTED) for k in agpr), agpr


def test_short_workspace_sizing_follows_a_running_maximum_and_reports_while_tight():
    """pytorch3d_amd/_C.py: _Need: the list size of a call shape is the running maximum (slow decay) of what its
    calls reported, and a call whose last report used more than 80 % of its lists asks for a report again at once -- not the last
    report alone, read back every 8th call (up to seven calls in a row could then run the naive stand-by on a growing scene)."""
    from pytorch3d_amd import _C

    class Done:
        def query(self):
            return True

    need = _C._Need()

    def report(v, capacity):
        need.pinned = torch.tensor([v], dtype=torch.int64)
        need.event = Done()
        need.capacity = capacity
        need.collect()

    report(1000, 5000)
    assert need.entries == 1000 and need.last == 1000 and not need.tight()
    report(4000, 5000)  # growth is taken at once
    assert need.entries == 4000 and not need.tight()
    report(4100, 5000)
    assert need.entries == 4100 and need.tight()  # 82 % of the lists: the next call reports again whatever its number
    report(2000, 5000)  # a smaller report pulls the size down slowly
    assert need.entries == 4100 - (4100 - 2000) // 8 and not need.tight()
    report(9000, 5000)  # overflow (the stand-by kernel ran): tight, and the size jumps
    assert need.entries == 9000 and need.tight()
    need.calls, need.event = 100, None  # far from the first four calls, not a multiple of 8
    need.calls = 101
    asked = []

    class FakeWs:
        def __getitem__(self, sl):
            asked.append(sl)
            raise RuntimeError("stop here")  # the copy itself needs a device

    try:
        need.report_later(FakeWs(), 0, 5000)
    except RuntimeError:
        pass
    assert asked, "a tight shape did not ask for a report"
    report(1000, 50000)
    need.calls = 101
    asked.clear()
    need.report_later(FakeWs(), 0, 50000)
    assert not asked, "a roomy shape asked for a report on a call that is not its eighth"


def test_bench_jobs_mode_deals_every_sub_batch_to_exactly_one_rank():
    """BASELINE configs[4]: 512 jobs = 8 sub-batches of 64 (generator seeds 0..7); on G in
    {1, 2, 4, 8} GPUs rank r runs sub-batches r, r + G, ...: every seed exactly once, the same number per rank.  A G that does
    not divide deals unevenly (round 6: the gather pads the shards to the largest, bench.py: `own`); a G with an idle rank is refused."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(U.ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for world in (1, 2, 4, 8):
        dealt = [bench.sub_batches_of_rank(512, 64, r, world) for r in range(world)]
        assert sorted(s for d in dealt for s in d) == list(range(8))
        assert len({len(d) for d in dealt}) == 1 and len(dealt[0]) == 8 // world
        assert all(d == sorted(d) and d[0] == r for r, d in enumerate(dealt))
    for world in (3, 5):
        dealt = [bench.sub_batches_of_rank(512, 64, r, world) for r in range(world)]
        assert sorted(s for d in dealt for s in d) == list(range(8)) and max(len(d) for d in dealt) == len(dealt[0]) == -(-8 // world)
    with pytest.raises(SystemExit):
        bench.sub_batches_of_rank(512, 64, 0, 16)
    with pytest.raises(SystemExit):
        bench.sub_batches_of_rank(500, 64, 0, 2)


def test_bench_dump_outputs_writes_a_fixed_sample_within_its_budget(tmp_path, monkeypatch):
    """bench.py --dump-outputs (bench.py: dump_outputs) on CPU tensors shaped like the step's outputs: outputs that fit are written
    whole; past the byte budget a fixed seeded sample of pixels (every K slot of each, the same pixels in every array, ascending) and
    of vertex rows; float64 pix_to_face, float32 for the rest; the same files from two calls."""
    import importlib.util

    import numpy as np

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(U.ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    N, H, W, K, V = 2, 16, 16, 4, 100
    pix = torch.arange(N * H * W * K, dtype=torch.int64).view(N, H, W, K)  # entry = pixel * K + slot
    out = {"pix_to_face": pix, "zbuf": pix.float(), "dists": -pix.float(), "bary_coords": pix.float()[..., None].expand(-1, -1, -1, -1, 3),
           "verts_packed_grad": torch.arange(V * 3, dtype=torch.float32).view(V, 3)}
    whole = bench.dump_outputs(out, str(tmp_path / "whole"))
    assert whole == {"pix_to_face": [N * H * W, K], "zbuf": [N * H * W, K], "bary_coords": [N * H * W, K, 3], "dists": [N * H * W, K],
                     "verts_packed_grad": [V, 3]}
    assert np.array_equal(np.load(tmp_path / "whole" / "pix_to_face.npy"), pix.view(-1, K).double().numpy())

    monkeypatch.setattr(bench, "DUMP_FRAGMENT_BYTES", 10_000)  # K * (8 + 4 + 12 + 4) = 112 bytes per pixel -> 89 of 512 pixels
    monkeypatch.setattr(bench, "DUMP_VERTS_BYTES", 600)        # 12 bytes per vertex -> 50 of 100 rows
    runs = [bench.dump_outputs(out, str(tmp_path / r)) for r in ("a", "b")]
    assert runs[0] == runs[1] and runs[0]["pix_to_face"] == [89, K] and runs[0]["verts_packed_grad"] == [50, 3]
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in runs[0]}
    b = {n: np.load(tmp_path / "b" / (n + ".npy")) for n in runs[0]}
    assert all(np.array_equal(a[n], b[n]) for n in a)
    assert a["pix_to_face"].dtype == np.float64 and all(a[n].dtype == np.float32 for n in a if n != "pix_to_face")
    assert sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in a) <= 10_000 + 600 + 5 * 128  # + the .npy headers
    px = a["pix_to_face"][:, 0] / K
    assert np.all(np.diff(px) > 0) and np.array_equal(a["pix_to_face"], px[:, None] * K + np.arange(K))  # whole pixels, ascending
    assert np.array_equal(a["zbuf"], a["pix_to_face"]) and np.array_equal(a["dists"], -a["pix_to_face"])
    assert np.array_equal(a["bary_coords"], np.repeat(a["pix_to_face"][..., None], 3, -1))
    rows = a["verts_packed_grad"][:, 0] / 3
    assert np.all(np.diff(rows) > 0) and np.array_equal(a["verts_packed_grad"], rows[:, None] * 3 + np.arange(3))


def test_pybind_flavour_builds_and_exports_the_operator_set():
    """pytorch3d_amd/csrc/bind.cpp (INTEGRATION.md section B compiled): the torch extension builds against include/p3d_amd.h, links
    libp3d_amd.so and exports every hot-path operator of `pytorch3d._C` under the reference's names (no compute call without a GPU)."""
    from pytorch3d_amd import _C, build_bind

    try:
        mod = build_bind.load()
    except Exception as e:  # noqa: BLE001
        pytest.skip("no host toolchain for the pybind flavour here: %r" % (e,))
    missing = [n for n in _C.HOT_PATH_EXPORTS if not callable(getattr(mod, n, None))]
    assert not missing, missing
    assert mod.MAX_INT == 2147483647 and mod.__p3d_amd_flavour__ == "pybind"
    with pytest.raises(RuntimeError, match="GPU tensor"):  # CPU tensors are refused, as in the ctypes flavour
        z = torch.zeros(1, dtype=torch.int64)
        mod.rasterize_meshes(torch.rand(4, 3, 3), z, z + 4, torch.full((4,), -1, dtype=torch.int64), (8, 8), 0.0, 2, 0, 0, False, False, False)


# ---- the header as the one description of the ABI: pytorch3d_amd/_lib.py reads its signatures and constants from it ----

def _host_compiler():
    """The clang++ of the toolchain build._hipcc() resolves to (host compilation only, no offload arch), or hipcc itself as a C++ driver."""
    import shutil

    from pytorch3d_amd import build

    hipcc = shutil.which(build._hipcc())
    assert hipcc, "no hipcc"
    root = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for clang in (os.path.join(root, "llvm", "bin", "clang++"), os.path.join(root, "lib", "llvm", "bin", "clang++")):
        if os.path.exists(clang):
            return [clang]
    return [hipcc, "-x", "c++"]


def test_compiler_confirms_the_parsed_signatures_and_constants(tmp_path):
    """The C types pytorch3d_amd._lib.parse_header read, restated as function-pointer types, are the types the compiler sees in
    include/p3d_amd.h -- for EVERY entry: a dropped parameter, an int for an int64_t or a missed entry fails.  The ctypes table is
    those same C types through the parser's dictionary, and the constants are the values the preprocessor sees."""
    from pytorch3d_amd import _lib

    assert set(_lib.DECLARATIONS) == set(_declared()) and len(_lib.DECLARATIONS) >= 136
    lines = ["#include <type_traits>", '#include "p3d_amd.h"']
    for name, (ret, params) in _lib.DECLARATIONS.items():
        lines.append(f"static_assert(std::is_same_v<decltype(&{name}), {ret} (*)({', '.join(params)})>, \"{name}\");")
    for name, value in _lib.CONSTANTS.items():
        lines.append(f"static_assert(P3D_{name} == {value}, \"P3D_{name}\");")
    src = tmp_path / "abi_check.cpp"
    src.write_text("\n".join(lines) + "\n")
    res = subprocess.run(_host_compiler() + ["-std=c++17", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]

    assert _lib._SIGNATURES == {name: _lib.ctypes_signature(ret, params) for name, (ret, params) in _lib.DECLARATIONS.items()}
    assert _lib.EXPORTED_SYMBOLS == tuple(_lib._SIGNATURES)
    S, P = _lib._SIGNATURES, ctypes.POINTER
    # hand-written expectations, one of each kind (the types are the aliases of _lib themselves: what load() assigns)
    assert S["p3d_abi_version"] == (_lib.c_int, []) and S["p3d_profile_collect"] == (None, [])
    assert S["p3d_error_string"] == (ctypes.c_char_p, [_lib.c_int])
    assert S["p3d_profile_entry"] == (ctypes.c_char_p, [_lib.c_int, _lib.c_ptr, _lib.c_ptr])
    assert S["p3d_rasterize_meshes_short_workspace_bytes"] == (_lib.c_size, [_lib.c_i64] + [_lib.c_int] * 5 + [_lib.c_i64])
    assert S["p3d_point_frames_workgroups"] == (_lib.c_i64, [_lib.c_i64, _lib.c_i64])
    assert S["p3d_clip_faces_plan"] == (_lib.c_int, [_lib.c_ptr, _lib.c_i64, P(_lib.c_f32), _lib.c_int, _lib.c_int, _lib.c_int, _lib.c_f32,
                                                     _lib.c_ptr, _lib.c_size, _lib.c_ptr])
    assert S["p3d_composite_forward"][1][:3] == [_lib.c_int, _lib.c_ptr, P(_lib.c_i64)]
    assert S["p3d_point_mesh_forward"][1][10] is _lib.c_f64 and S["p3d_vert_align_keys"][1][10] is _lib.c_uint


_SYNTHETIC_HEADER = """
/* a block comment with a declaration inside: int p3d_fake(int); and
   #define P3D_NOT_A_MACRO 7 on its second line */
#ifndef FAKE_H_
#define FAKE_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define P3D_A 3
#define P3D_B (-2)   /* negative */
#define P3D_C 8u     // unsigned; int p3d_fake(int);
#define P3D_NAME_ONLY
typedef void* p3d_stream_t; /* hipStream_t */
// int p3d_fake(int);
int p3d_scalars(int a, unsigned b, int64_t c, size_t d, float e, double f);
size_t p3d_pointers(const int* a, unsigned* b, const int64_t* c, size_t* d, float* e, const double* f, void* g, const void* h,
                    int32_t* i, p3d_stream_t stream);
void p3d_arrays(const int64_t strides[2], const float background[3],
                const double planes[6],
                float *spaced);
const char* p3d_nothing(void);
int64_t p3d_wide(void); double p3d_real(int n); float p3d_single(int n); unsigned p3d_bits(void);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_header_parser_on_synthetic_text():
    from pytorch3d_amd import _lib

    decls, constants = _lib.parse_header(_SYNTHETIC_HEADER)
    assert constants == {"A": 3, "B": -2, "C": 8}
    assert decls == {
        "p3d_scalars": ("int", ["int", "unsigned", "int64_t", "size_t", "float", "double"]),
        "p3d_pointers": ("size_t", ["const int*", "unsigned*", "const int64_t*", "size_t*", "float*", "const double*", "void*", "const void*",
                                    "int32_t*", "p3d_stream_t"]),
        "p3d_arrays": ("void", ["const int64_t[2]", "const float[3]", "const double[6]", "float*"]),
        "p3d_nothing": ("const char*", []),
        "p3d_wide": ("int64_t", []), "p3d_real": ("double", ["int"]), "p3d_single": ("float", ["int"]), "p3d_bits": ("unsigned", []),
    }
    P, sig = ctypes.POINTER, lambda name: _lib.ctypes_signature(*decls[name])
    assert sig("p3d_scalars") == (ctypes.c_int, [ctypes.c_int, ctypes.c_uint, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float, ctypes.c_double])
    assert sig("p3d_pointers") == (ctypes.c_size_t, [ctypes.c_void_p] * 10)
    assert sig("p3d_arrays") == (None, [P(ctypes.c_int64), P(ctypes.c_float), P(ctypes.c_double), ctypes.c_void_p])
    assert sig("p3d_nothing") == (ctypes.c_char_p, [])
    assert [sig(n)[0] for n in ("p3d_wide", "p3d_real", "p3d_single", "p3d_bits")] == [ctypes.c_int64, ctypes.c_double, ctypes.c_float, ctypes.c_uint]

    # what the dictionary does not hold is refused with the declaration's text, never guessed
    for bad in ("int p3d_bad(long double x);", "int p3d_bad(int n, long double);", "long double p3d_bad(void);", "int p3d_bad(unsigned int n);",
                "int p3d_bad(struct thing* t);", "int* p3d_bad(void);", "int p3d_bad(char c);", "int p3d_bad(const int64_t* strides[2]);"):
        with pytest.raises(ValueError, match=re.escape(bad[:-1])):
            _lib.parse_header(bad)
    with pytest.raises(ValueError, match="long double"):
        _lib.parse_header("int p3d_good(int n);\nint p3d_bad(long double x);")
    with pytest.raises(ValueError, match=re.escape("struct p3d_options { int k")):  # not a declaration of an entry
        _lib.parse_header("struct p3d_options { int k; };")
    with pytest.raises(ValueError, match="p3d_twice"):
        _lib.parse_header("int p3d_twice(void); int p3d_twice(int n);")


def test_a_marshaller_builds_for_every_declaration():
    """_lib.marshaller: one converter per parameter without the stream; the status entries are the 91 that take a stream and the
    host entry, and those are what load() binds for _lib.call."""
    from pytorch3d_amd import _lib

    assert len(_lib.DECLARATIONS) == 136
    status, streamed = [], []
    for name, (ret, params) in _lib.DECLARATIONS.items():
        converters, stream, is_status = _lib.marshaller(name, ret, params)
        assert len(converters) == len(params) - int(stream), name
        assert all((c is None) == (p in _lib._SCALARS) for c, p in zip(converters, params)), name
        status += [name] if is_status else []
        streamed += [name] if stream else []
    assert len(status) == 92 and len(streamed) == 91
    assert sorted(set(status) - set(streamed)) == ["p3d_iou_box3d_host"] and set(streamed) <= set(status)
    _lib.load()
    assert sorted(_lib._CALLS) == sorted(status)
    with pytest.raises(ValueError, match="p3d_stream_t"):  # anywhere but last
        _lib.marshaller("p3d_x", "int", ["p3d_stream_t", "int"])
    with pytest.raises(ValueError, match=re.escape("size_t*")):  # no torch dtype stands for it: never guessed
        _lib.marshaller("p3d_x", "int", ["size_t*"])


_CALL_HEADER = """
typedef void* p3d_stream_t;
int p3d_host(const float* a, float* out, const int64_t* idx, int32_t* small, const uint8_t* mask, void* ws, const int64_t strides[4],
             int n, float x);
int p3d_launch(const float* a, int n, p3d_stream_t stream);
"""


def _stand_in(entry, code=0):
    """(invoke of _lib.bind over a Python callable that records what arrives, the list of recorded argument tuples)"""
    from pytorch3d_amd import _lib

    seen = []

    def fn(*args):
        seen.append(args)
        return code

    return _lib.bind(fn, entry, *_lib.parse_header(_CALL_HEADER)[0][entry]), seen


def test_call_marshals_by_the_declaration():
    invoke, seen = _stand_in("p3d_host")
    t = torch.arange(15, dtype=torch.float32).reshape(3, 5)
    idx, small = torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    invoke("where", None, t[:, 2:], None, torch.empty(0, dtype=torch.int64), small, None, idx, (20, 1, 5, 4), 7, 0.5)
    (a, out, empty, sm, mask, ws, strides, n, x), = seen
    assert a == t.data_ptr() + 8 and out is None and empty is None and sm == small.data_ptr() and mask is None and ws == idx.data_ptr()
    assert isinstance(strides, ctypes.c_int64 * 4) and list(strides) == [20, 1, 5, 4]
    assert (n, x) == (7, 0.5) and type(n) is int and type(x) is float
    invoke("where", None, 4096, None, None, None, None, None, [0, 0, 0, 0], 0, 0.0)  # a plain int is an address
    assert seen[1][0] == 4096
    del seen[:]
    with pytest.raises(ValueError, match=re.escape("p3d_host: argument 6 is declared `const int64_t[4]`; got 3 numbers")):
        invoke("where", None, t, None, None, None, None, None, (1, 2, 3), 7, 0.5)
    for args in ((t, None, None, None, None, None, (1, 2, 3, 4), 7), (t, None, None, None, None, None, (1, 2, 3, 4), 7, 0.5, 1)):
        with pytest.raises(TypeError, match=re.escape("p3d_host takes 9 arguments (const float*, float*, const int64_t*, int32_t*, "
                                                      "const uint8_t*, void*, const int64_t[4], int, float), got %d" % len(args))):
            invoke("where", None, *args)
    # the stream slot is not an argument: handing one over is one argument too many
    launch, launched = _stand_in("p3d_launch")
    with pytest.raises(TypeError, match=re.escape("p3d_launch takes 2 arguments (const float*, int), got 3")):
        launch("where", None, t, 3, None)
    assert seen == [] and launched == []
    # a status other than P3D_OK goes through check(code, where)
    failing, _ = _stand_in("p3d_host", code=-1)
    with pytest.raises(RuntimeError, match=r"^where: .* \(p3d error -1\)$"):
        failing("where", None, t, None, None, None, None, None, (1, 2, 3, 4), 7, 0.5)


def test_call_rejects_a_tensor_of_another_dtype_or_device():
    invoke, seen = _stand_in("p3d_host")
    ok = [torch.zeros(2), torch.zeros(2), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32),
          torch.zeros(2, dtype=torch.uint8), torch.zeros(2, dtype=torch.uint8), (0, 0, 0, 0), 0, 0.0]
    for pos, ctype, bad in ((0, "const float*", torch.float64), (2, "const int64_t*", torch.int32), (3, "int32_t*", torch.int64),
                            (4, "const uint8_t*", torch.int8)):
        args = list(ok)
        args[pos] = torch.zeros(2, dtype=bad)
        with pytest.raises(RuntimeError, match=re.escape(f"p3d_host: argument {pos} is declared `{ctype}`") + ".*" + re.escape(str(bad))):
            invoke("where", None, *args)
    assert seen == []
    for pos, dtype in ((4, torch.bool), (5, torch.float64), (5, torch.int16), (5, torch.bool)):  # bool for uint8_t, anything for void
        args = list(ok)
        args[pos] = torch.zeros(2, dtype=dtype)
        invoke("where", None, *args)
        assert seen.pop()[pos] == args[pos].data_ptr()
    meta = torch.zeros(2, device="meta")  # not the host's memory
    with pytest.raises(RuntimeError, match=re.escape("p3d_host: argument 0 is declared `const float*` and the call is for the host") + ".*meta"):
        invoke("where", None, meta, *ok[1:])
    assert seen == []


def test_call_on_the_host_entry_of_the_library():
    import box3d_case
    from pytorch3d_amd import _C, _lib

    gen = torch.Generator().manual_seed(5)
    b1, b2 = (box3d_case.random_boxes(2, gen).to(torch.float32) for _ in range(2))
    want = _C.iou_box3d_host(b1, b2)
    vol, iou = torch.full((2, 2), -7.0), torch.full((2, 2), -7.0)
    _lib.call("p3d_iou_box3d_host", "iou_box3d_host", None, b1, b2, 2, 2, vol, iou)
    assert torch.equal(vol, want[0]) and torch.equal(iou, want[1]) and bool((want[0] >= 0).all())
    vol.fill_(-7.0), iou.fill_(-7.0)
    with pytest.raises(RuntimeError, match=re.escape("p3d_iou_box3d_host: argument 0 is declared `const float*`") + ".*float64"):
        _lib.call("p3d_iou_box3d_host", "iou_box3d_host", None, b1.double(), b2.double(), 2, 2, vol, iou)
    assert bool((vol == -7.0).all()) and bool((iou == -7.0).all())  # the library was not entered


def test_the_package_marshals_through_call_alone():
    """No module of the package builds a pointer, a stream or a status check by hand: _lib.py does, and _C.py keeps _ptr, _stream and
    cover_ptr for the raw calls of the tests and the profile scripts."""
    import ast

    pkg = os.path.join(U.ROOT, "pytorch3d_amd")
    for f in sorted(os.listdir(pkg)):
        if not f.endswith(".py") or f == "_lib.py":
            continue
        src = open(os.path.join(pkg, f)).read()
        if f == "_C.py":
            helpers = [ast.get_source_segment(src, n) for n in ast.parse(src).body
                       if isinstance(n, ast.FunctionDef) and n.name in ("_ptr", "_stream", "cover_ptr")]
            assert len(helpers) == 3
            for text in helpers:
                src = src.replace(text, "")
        found = re.findall(r"(?<![A-Za-z0-9])_ptr\(|(?<![A-Za-z0-9])_stream\(|_lib\.check\(|c_void_p", src)  # (data_ptr() is not meant)
        assert found == [], (f, found)


def test_every_integer_macro_of_the_header_is_a_constant_of_lib():
    from pytorch3d_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    macros = dict(re.findall(r"^#define (P3D_\w+)[ \t]+(\S.*?)\s*$", text, re.M))  # every macro that has a value (not the include guard)
    assert len(macros) >= 47 and "P3D_AMD_H_" not in macros
    for macro, value in macros.items():
        assert re.fullmatch(r"\(?-?\d+u?\)?", value), (macro, value)  # the header holds integer macros only
        assert getattr(_lib, macro[len("P3D_"):]) == int(value.strip("()u")) == _lib.CONSTANTS[macro[len("P3D_"):]], macro
    # the names the package and the tests used before the header was read, with the values they had
    before = {"ABI_VERSION": 3, "RASTER_COVER_LIST": 1, "RASTER_CUDA_TIE_ORDER": 2, "BWD_COVER_HAS_LIST": 1, "BWD_MAKE_FACE_PRE": 2,
              "BWD_GRAD_OUT_ZEROED": 8, "KNN_MAX_K": 32, "KNN_TILE": 512, "KNN_ACCUMULATE_P2": 1, "FRAMES_MAX_K": 64, "FRAMES_DISAMBIGUATE": 1,
              "FRAMES_ROWS_PER_GROUP": 64, "BOX3D_LDS_CAPACITY": 64, "BOX3D_WAVES_PER_GROUP": 4, "BOX3D_MAX_GROUPS": 4096,
              "NEIGHBOR_SUM_MAX_GROUPS": 2048, "VERT_ALIGN_NEAREST": 1, "VERT_ALIGN_BORDER": 2, "VERT_ALIGN_CORNERS": 4,
              "VERT_ALIGN_MAX_GROUPS": 4096, "FPS_REGISTER_POINTS": 16384, "POINT_MESH_POINT": 0, "POINT_MESH_SEGMENT": 1,
              "POINT_MESH_TRIANGLE": 2, "POINT_MESH_TILE": 64, "POINT_MESH_ACCUMULATE_QUERIES": 1, "POINT_MESH_ACCUMULATE_TARGETS": 2}
    assert len(before) == 27 and all(_lib.CONSTANTS[name] == value == getattr(_lib, name) for name, value in before.items())
    assert _lib.NEIGHBOR_SUM_GROUP_LANES == 256 and "NEIGHBOR_SUM_GROUP_LANES" not in _lib.CONSTANTS  # the one written by hand
    # the copies elsewhere in the package are these
    from pytorch3d_amd import _C, shading, textures

    assert (_C.kMaxPointsPerPixel, _C.kMaxItemsPerBin) == (150, 22) == (_lib.MAX_K, _lib.MAX_BINS_PER_SIDE + 1)
    assert (_C._ALPHA, _C._NORM, _C._SUM) == (0, 1, 2) == (_lib.COMPOSITE_ALPHA, _lib.COMPOSITE_NORM_SUM, _lib.COMPOSITE_SUM)
    assert (shading.PARAM_FLOATS, shading.LIGHT_DIRECTIONAL, shading.LIGHT_POINT) == (25, 0, 1)
    assert textures._PAD == {"zeros": 0, "border": 1} and textures._MODE == {"bilinear": 0, "nearest": 1}


def test_missing_header_is_an_extension_missing_error(tmp_path):
    """The header travels with the package (<package>/../include/p3d_amd.h); without it the import names the path."""
    import importlib.util

    from pytorch3d_amd import _lib

    os.makedirs(tmp_path / "pkg")
    copy = tmp_path / "pkg" / "_lib.py"
    copy.write_text(open(_lib.__file__).read())
    spec = importlib.util.spec_from_file_location("_lib_without_header", str(copy))
    with pytest.raises(Exception, match=re.escape(str(tmp_path / "include" / "p3d_amd.h"))) as info:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(info.value).__name__ == "ExtensionMissing" and isinstance(info.value, RuntimeError)


def test_profile_snapshot_without_a_device():
    """p3d_profile_entry's out-parameters are plain pointers in the header, so c_void_p in the table: byref() results pass."""
    from pytorch3d_amd import _lib

    snap = _lib.profile_snapshot()  # nothing was launched: no entry with a launch
    assert isinstance(snap, dict) and all(n > 0 and ms >= 0.0 for n, ms in snap.values())
    lib, n, ms = _lib.load(), _lib.c_i64(-7), _lib.c_f64(-7.0)
    assert lib.p3d_profile_entry(lib.p3d_profile_num_entries(), ctypes.byref(n), ctypes.byref(ms)) is None  # past the end: untouched
    assert (n.value, ms.value) == (-7, -7.0)


def test_build_dependency_lists_are_what_is_on_disk():
    """needs_build() compares the library with SOURCES + HEADERS: a kernel file that is not compiled, or a header that is included and
    not listed, would leave a stale library in place."""
    from pytorch3d_amd import build

    on_disk = sorted(os.listdir(build.CSRC))
    assert [f for f in on_disk if f.endswith(".hip")] == sorted(s for s in build.SOURCES if s.endswith(".hip"))
    assert len(set(build.SOURCES)) == len(build.SOURCES) and "bind.cpp" not in build.SOURCES
    assert all(os.path.isfile(os.path.join(build.CSRC, f)) for f in build.SOURCES + build.HEADERS)
    headers = {os.path.normpath(h) for h in build.HEADERS}
    assert headers == {f for f in on_disk if f.endswith(".h")} | {os.path.normpath("../../include/p3d_amd.h")}
    for f in build.SOURCES + build.HEADERS:
        here = os.path.dirname(f)  # quoted includes are relative to the including file
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(build.CSRC, f)).read(), re.M):
            assert os.path.normpath(os.path.join(here, inc)) in headers, (f, inc)
