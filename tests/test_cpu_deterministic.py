"""The deterministic backwards without a GPU: the new kernels hold no float atomic (gfx950 assembly of their translation unit), the
new C entries check their arguments before anything is launched, and the host picks the ordered entries exactly under
torch.use_deterministic_algorithms(True) without warn_only (include/p3d_amd.h: *_ordered)."""
import contextlib
import ctypes
import os
import re
import subprocess
import types

import pytest
import torch

from pytorch3d_amd import _C, _lib
from pytorch3d_amd import build as hip_build

INVALID, WORKSPACE = -1, -4  # P3D_ERR_INVALID_ARG, P3D_ERR_WORKSPACE

ORDERED = [n for n in _lib.EXPORTED_SYMBOLS if n.endswith("_ordered")]
ORDERED_SIZES = [n for n in _lib.EXPORTED_SYMBOLS if n.endswith("_ordered_workspace_bytes")]


def test_the_ordered_entries_are_declared_and_exported():
    assert len(ORDERED) == 6 and len(ORDERED_SIZES) == 6
    header = open(os.path.join(os.path.dirname(hip_build.HERE), "include", "p3d_amd.h")).read()
    for name in ORDERED + ORDERED_SIZES:
        assert re.search(r"\b" + name + r"\(", header), name
    assert "#define P3D_ABI_VERSION 3" in header  # additive: the version existing callers pin stays


def test_no_float_atomic_in_the_ordered_kernels():
    """Device-only assembly of ordered_bwd.hip with the library's flags: no add / packed add on f32 or 16-bit floats through the global,
    flat or buffer atomic path or in LDS, in any kernel.  (The mnemonics are put together from pieces here.)"""
    src = os.path.join(hip_build.CSRC, "ordered_bwd.hip")
    cmd = [hip_build._hipcc()] + hip_build.FLAGS + ["-x", "hip", "--cuda-device-only", "-S", src, "-o", "-"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    asm = res.stdout
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M)
    assert len(kernels) >= 20 and any("pass1_kernel" in k for k in kernels) and any("pass2_kernel" in k for k in kernels), kernels
    memory = "(?:" + "|".join(["global", "flat", "buffer"]) + ")_" + "atomic" + "_(?:pk_)?(?:add|fadd)_(?:f|bf)(?:16|32|64)"
    lds = "d" + "s_(?:pk_)?add_(?:rtn_)?(?:f|bf)(?:16|32|64)"
    hits = [line.strip() for line in asm.splitlines() if re.search(r"^\s*(?:" + memory + "|" + lds + r")\b", line)]
    assert not hits, hits[:10]
    # the pattern is live: the same search finds the float atomics of an atomic translation unit
    res = subprocess.run(cmd[:-3] + [os.path.join(hip_build.CSRC, "gather.hip"), "-o", "-"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    assert any(re.search(r"^\s*(?:" + memory + "|" + lds + r")\b", line) for line in res.stdout.splitlines())


def _buf(n=64):
    b = (ctypes.c_char * n)()
    return b, ctypes.c_void_p(ctypes.addressof(b))


def test_ordered_entries_validate_before_any_launch():
    """Every call here returns from the argument checks: no device is needed (and none is touched)."""
    lib = _lib.load()
    keep, p = _buf()
    null = ctypes.c_void_p(None)
    st2 = (ctypes.c_int64 * 2)(1, 4)
    st4 = (ctypes.c_int64 * 4)(40, 1, 20, 5)

    # the sizes: something for a non-empty list, more for more, nothing for nonsense
    assert lib.p3d_rasterize_meshes_backward_ordered_workspace_bytes(100, 0, 0) == 0
    a = lib.p3d_rasterize_meshes_backward_ordered_workspace_bytes(100, 0, 1000)
    b = lib.p3d_rasterize_meshes_backward_ordered_workspace_bytes(100, 1, 1000)
    assert 0 < a < b and b >= a + 100 * 9 * 4
    assert lib.p3d_rasterize_meshes_backward_ordered_workspace_bytes(100, 0, 100000) > a
    assert lib.p3d_rasterize_meshes_backward_ordered_workspace_bytes(-1, 0, 10) == 0
    assert lib.p3d_scatter_face_grads_ordered_workspace_bytes(1000) > 0
    assert lib.p3d_rasterize_points_backward_ordered_workspace_bytes(1000) > 0
    assert lib.p3d_rasterize_points_composite_backward_ordered_workspace_bytes(1, 8, 8, 4, 3, 100) >= 2 * 8 * 8 * 4 * 4
    assert lib.p3d_rasterize_points_composite_backward_ordered_workspace_bytes(1, 8, 8, 4, 5, 100) == 0  # C > 4
    assert lib.p3d_composite_backward_ordered_workspace_bytes(1, 4, 8, 8, 9, 100) >= 8 * 8 * 4 * 4
    assert lib.p3d_interp_face_attrs_backward_ordered_workspace_bytes(5, 100) > 0

    def mesh(fv=p, faces=null, p2f=p, g=p, sorted_=p, S=10, corners=null, nc=0, F=5, V=0, N=1, H=4, W=4, K=2, out=p, ws=p, wsb=1 << 20):
        return lib.p3d_rasterize_meshes_backward_ordered(fv, faces, p2f, g, g, g, sorted_, S, corners, nc, F, V, N, H, W, K, 1, 1, out, ws, wsb, null)

    assert mesh(out=null) == INVALID and mesh(fv=null) == INVALID and mesh(p2f=null) == INVALID and mesh(sorted_=null) == INVALID
    assert mesh(F=-1) == INVALID and mesh(S=-1) == INVALID and mesh(S=33) == INVALID  # more hits than samples
    assert mesh(faces=p, V=4, corners=null, nc=3) == INVALID and mesh(faces=p, V=4, corners=p, nc=16) == INVALID
    assert mesh(wsb=0) == WORKSPACE and mesh(ws=null) == WORKSPACE
    assert mesh(faces=p, V=4, corners=p, nc=3, wsb=lib.p3d_rasterize_meshes_backward_ordered_workspace_bytes(5, 0, 10)) == WORKSPACE
    assert mesh(F=0) == 0  # nothing to write

    def scatter(g=p, faces=p, corners=p, nc=6, V=4, F=2, out=p, ws=p, wsb=1 << 20):
        return lib.p3d_scatter_face_grads_ordered(g, faces, corners, nc, V, F, out, ws, wsb, null)

    assert scatter(out=null) == INVALID and scatter(corners=null) == INVALID and scatter(nc=7) == INVALID and scatter(V=-1) == INVALID
    assert scatter(wsb=0) == WORKSPACE and scatter(V=0) == 0

    def points(pts=p, idx=p, g=p, sorted_=p, S=10, P=5, N=1, H=4, W=4, K=2, out=p, ws=p, wsb=1 << 20):
        return lib.p3d_rasterize_points_backward_ordered(pts, idx, g, g, sorted_, S, P, N, H, W, K, out, ws, wsb, null)

    assert points(out=null) == INVALID and points(idx=null) == INVALID and points(sorted_=null) == INVALID and points(S=33) == INVALID
    assert points(wsb=0) == WORKSPACE and points(P=0) == 0

    def fused(mode=0, pts=p, sorted_=p, S=10, P=5, C=3, K=2, gp=p, gf=p, ws=p, wsb=1 << 20):
        return lib.p3d_rasterize_points_composite_backward_ordered(mode, pts, p, p, p, p, sorted_, S, P, C, 1, 4, 4, K, 1.0, gp, gf, ws, wsb, null)

    assert fused(mode=2) == INVALID and fused(C=5) == INVALID and fused(gp=null) == INVALID and fused(pts=null) == INVALID
    assert fused(sorted_=null) == INVALID and fused(K=151) == -2 and fused(wsb=0) == WORKSPACE and fused(P=0) == 0

    def comp(mode=0, go=p, feats=p, fst=st2, sorted_=p, S=10, C=4, P=6, gf=p, ga=p, ws=p, wsb=1 << 20):
        return lib.p3d_composite_backward_ordered(mode, go, feats, fst, p, p, sorted_, S, 1, C, P, 2, 4, 5, st4, st4, gf, fst, ga, ws, wsb, null)

    assert comp(mode=3) == INVALID and comp(gf=null) == INVALID and comp(ga=null) == INVALID and comp(go=null) == INVALID
    assert comp(fst=(ctypes.c_int64 * 2)(3, 2)) == INVALID and comp(sorted_=null) == INVALID and comp(S=41) == INVALID
    assert comp(wsb=0) == WORKSPACE

    def interp(p2f=p, g=p, sorted_=p, S=10, P=20, F=3, D=4, gb=p, gf=p, ws=p, wsb=1 << 20):
        return lib.p3d_interp_face_attrs_backward_ordered(p2f, p, p, g, sorted_, S, P, F, D, gb, gf, ws, wsb, null)

    assert interp(p2f=null) == INVALID and interp(gf=null) == INVALID and interp(gb=null) == INVALID and interp(S=21) == INVALID
    assert interp(sorted_=null) == INVALID and interp(D=-1) == INVALID and interp(wsb=0) == WORKSPACE
    del keep


# ---- the host switch ------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for the loaded library: every entry returns 0 (P3D_OK, or a size of 0) and leaves its name."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("p3d_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append(name)
            return 0

        return entry

    def launched(self):
        return [c for c in self.calls if not c.endswith("_bytes")]


@contextlib.contextmanager
def _mode(on, warn_only=False):
    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(on, warn_only=warn_only)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])


def _host_calls():
    """name -> (a call of the host layer on CPU stand-ins, its atomic entry, its ordered entry)."""
    N, H, W, K, F, V, P, C, D = 1, 4, 5, 2, 6, 9, 7, 3, 2
    p2f = torch.randint(-1, F, (N, H, W, K))
    idx = torch.randint(-1, P, (N, H, W, K), dtype=torch.int32)
    fv, faces = torch.rand(F, 3, 3), torch.randint(0, V, (F, 3))
    g1, g3 = torch.rand(N, H, W, K), torch.rand(N, H, W, K, 3)
    pts, feats = torch.rand(P, 3), torch.rand(P, C)
    cidx, alphas = torch.randint(-1, P, (N, K, H, W)), torch.rand(N, K, H, W)
    flat = p2f.reshape(-1)
    S = flat.shape[0]
    comp = lambda name: (lambda: getattr(_C, name)(torch.rand(N, C, H, W), feats.t(), alphas, cidx))
    calls = {
        "mesh": (lambda: _C.rasterize_meshes_backward(fv, p2f, g1, g3, g1, True, True), "p3d_rasterize_meshes_backward_ex",
                 "p3d_rasterize_meshes_backward_ordered"),
        "mesh through faces": (lambda: _C._mesh_backward(fv, faces, V, p2f, g1, g3, g1, True, True, None), "p3d_rasterize_meshes_backward_ex",
                               "p3d_rasterize_meshes_backward_ordered"),
        "scatter": (lambda: _C.scatter_face_grads(torch.rand(F, 3, 3), faces, V), "p3d_scatter_face_grads", "p3d_scatter_face_grads_ordered"),
        "points": (lambda: _C.rasterize_points_backward(pts, idx, g1, g1), "p3d_rasterize_points_backward", "p3d_rasterize_points_backward_ordered"),
        "fused points": (lambda: _C.rasterize_points_composite_backward(pts, feats, idx, g1, torch.rand(N, H, W, C), 1.0, "norm"),
                         "p3d_rasterize_points_composite_backward", "p3d_rasterize_points_composite_backward_ordered"),
        "interp": (lambda: _C.interp_face_attrs_backward(flat, torch.rand(S, 3), torch.rand(F, 3, D), torch.rand(S, D)),
                   "p3d_interp_face_attrs_backward", "p3d_interp_face_attrs_backward_ordered"),
        "interp, image-shaped": (lambda: _C.interp_face_attrs_backward(flat, torch.rand(S, 3), torch.rand(F, 3, D), torch.rand(S, D),
                                                                       image_shape=(N, H, W, K)),
                                 "p3d_interp_face_attrs_backward_nhwk", "p3d_interp_face_attrs_backward_ordered"),
    }
    for name in ("accum_alphacomposite_backward", "accum_weightedsumnorm_backward", "accum_weightedsum_backward"):
        calls[name] = (comp(name), "p3d_composite_backward", "p3d_composite_backward_ordered")
    return calls


def test_host_switch(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(_C, "_need_gpu", lambda t, name: None)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device: types.SimpleNamespace(cuda_stream=0))
    # _lib.call with the recorder behind the real marshallers: the CPU stand-ins still have to fit every entry's declaration
    monkeypatch.setattr(_lib, "_CALLS", {n: _lib.bind(getattr(rec, n), n, *d) for n, d in _lib.DECLARATIONS.items() if _lib.marshaller(n, *d)[2]})
    for name, (call, atomic, ordered) in _host_calls().items():
        for tag, ctx, want in (("flag off", _mode(False), atomic), ("warn only", _mode(True, warn_only=True), atomic),
                               ("strict", _mode(True), ordered)):
            rec.calls.clear()
            with ctx:
                call()
            assert rec.launched() == [want], (name, tag, rec.calls)
    # float64 interp keeps its refusal, and says which
    with _mode(True), pytest.raises(RuntimeError, match="float64"):
        _C.interp_face_attrs_backward(torch.zeros(4, dtype=torch.int64), torch.rand(4, 3).double(), torch.rand(2, 3, 2).double(), torch.rand(4, 2).double())


def test_hit_lists_are_sorted_stably():
    idx = torch.tensor([[3, -1, 0, 3], [0, 2, -1, 3]]).t()  # a strided view: the list follows the LOGICAL order
    hits = _C._sorted_hits(idx)
    flat = idx.reshape(-1)
    assert flat[hits].tolist() == sorted(v for v in flat.tolist() if v >= 0)
    for v in set(flat[hits].tolist()):
        mine = hits[flat[hits] == v].tolist()
        assert mine == sorted(mine) and mine == [i for i, x in enumerate(flat.tolist()) if x == v]
    assert _C._sorted_hits(torch.full((5,), -1)).numel() == 0
    faces = torch.tensor([[0, 2, -1], [2, 7, 0], [-4, 1, 2]])  # V = 4: -1 -> 3, -4 -> 0, 7 is outside
    corners = _C._sorted_corners(faces, 4)
    assert corners.tolist() == [0, 5, 6, 7, 1, 3, 8, 2]


def test_shaders_keep_their_refusal():
    from pytorch3d_amd import shading

    with _mode(True):
        with pytest.raises(RuntimeError, match="deterministic"):
            shading._PhongShade.backward(types.SimpleNamespace(), torch.zeros(1))
        with pytest.raises(RuntimeError, match="deterministic"):
            shading._SoftPhong.backward(types.SimpleNamespace(), torch.zeros(1))
