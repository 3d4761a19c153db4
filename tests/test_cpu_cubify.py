"""cubify without a GPU: the nested-loop restatement of tests/cubify_case.py pinned to the reference's recorded results
(tests/golden/cubify_ref.npz), the torch formulation against both, other dtypes and strided views, the contract's errors and empties,
three deliberately wrong variants refused by the same comparison, the C entries' argument checks, and the shim.  Every comparison is
torch.equal (cubify_case.misses): the contract is integers and exactly specified float32 arithmetic."""
import functools
import importlib
import json
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cubify_case as C  # noqa: E402

import pytorch3d_amd as A  # noqa: E402
from pytorch3d_amd import _C, _lib  # noqa: E402

M = importlib.import_module("pytorch3d_amd.cubify")  # (the package re-exports the FUNCTION cubify over the sub-module)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _formulation(voxels, thresh, feats, align, **kw):
    return C.lists_of(M.cubify_packed_torch(voxels, thresh, feats, align, **kw))


def _public(voxels, thresh, feats, align):
    m = A.cubify(voxels, thresh, feats=feats, align=align)
    return m.verts_list(), m.faces_list(), m.textures


def test_fixture_holds_every_case_and_what_the_contract_promises():
    fix = C.fixture()
    assert {k.split("/")[0] for k in fix} == set(C.cases()) and len(C.cases()) == 4 * 3 * 2 + 6
    assert os.path.getsize(C.FIXTURE) < 1 << 20
    assert (fix["solid3/nv"].tolist(), fix["solid3/nf"].tolist()) == ([56], [108])
    assert fix["checker/nf"].tolist() == [12 * 32] * 2  # every voxel of a checkerboard exposes all six sides
    assert int(fix["all_empty/ndim"]) == 1 and [tuple(v.shape) for v in C.expected("all_empty")[0]] == [(0,)] * 3
    assert [tuple(f.shape) for f in C.expected("some_empty")[1]][0::2] == [(0, 3)] * 3
    assert fix["feats_center/tex"].shape == (int(fix["feats_center/nf"].sum()), 3)
    one = torch.zeros((1, 3, 3, 3))
    one[0, 1, 1, 1] = 1
    verts, faces, _ = C.restate(one, 0.5)
    assert verts[0].shape == (8, 3) and faces[0].shape == (12, 3)


@pytest.mark.parametrize("name", C.cases())
def test_restatement_equals_the_reference(name):
    assert C.misses(C.restate(*C.inputs(name)), C.expected(name), name) == []


@pytest.mark.parametrize("name", C.cases())
def test_formulation_equals_the_reference_and_the_restatement(name):
    got = _formulation(*C.inputs(name))
    assert C.misses(got, C.expected(name), name) == []
    assert C.misses(got, C.restate(*C.inputs(name)), name) == []
    assert C.misses(_public(*C.inputs(name)), C.expected(name), name) == []  # CPU tensors: the public function takes the formulation
    assert not M.kernel_path(*C.inputs(name)[:1])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16])
def test_other_dtypes_round_the_threshold_to_theirs(dtype):
    for name in ("g2345_center_p7", "g2532_topleft_p3", "thresh07", "feats_center"):
        voxels, thresh, feats, align = C.inputs(name)
        voxels = voxels.to(dtype)
        feats = None if feats is None else feats.to(dtype)
        got = _formulation(voxels, thresh, feats, align)
        assert C.misses(got, C.restate(voxels, thresh, feats, align), name) == []
        assert got[0][0].dtype == torch.float32 and (feats is None or got[2][0].dtype == dtype)
    # float32(0.7) < 0.7, and `ge` rounds the threshold to the tensor's dtype: the same stored value is occupied as float32, not as float64
    at = torch.full((1, 2, 2, 2), 0.7, dtype=torch.float32)
    assert int(M.cubify_packed_torch(at, 0.7)[3].sum()) == 48 and int(M.cubify_packed_torch(at.double(), 0.7)[3].sum()) == 0


def test_strided_voxels_and_feats():
    gen = torch.Generator().manual_seed(5)
    base = torch.rand((2, 4, 3, 5), generator=gen)  # (N, H, D, W) in memory
    view = base.permute(0, 2, 1, 3)
    assert not view.is_contiguous()
    assert C.misses(_formulation(view, 0.5, None, "corner"), C.restate(view.contiguous(), 0.5, None, "corner")) == []
    wide = torch.rand((2, 3, 3, 4, 2), generator=gen)  # (N, C, D, H, W): the voxel head's channel 1
    feats = torch.rand((2, 3, 4, 2, 5), generator=gen).permute(0, 4, 1, 2, 3)  # (N, K=5, D, H, W), K innermost in memory
    got = _formulation(wide[:, 1], 0.4, feats, "center")
    assert C.misses(got, C.restate(wide[:, 1].contiguous(), 0.4, feats.contiguous(), "center")) == [] and got[2][0].shape[1:] == (1, 1, 5)


def test_errors_and_empties():
    v = torch.rand((2, 3, 3, 3))
    for fn in (A.cubify, lambda *a, **k: A.cubify_packed(*a, **k), lambda *a, **k: M.cubify_packed_torch(*a, **k)):
        with pytest.raises(ValueError, match=r"Align mode must be one of \(topleft, corner, center\)\."):
            fn(v, 0.5, align="middle")
        for axis, name in ((1, "D"), (2, "H"), (3, "W")):
            shape = [2, 3, 3, 3]
            shape[axis] = 1
            with pytest.raises(ValueError, match=name + " = 1"):
                fn(torch.rand(shape), 0.5)
    none = A.cubify(torch.zeros((0, 3, 3, 3)), 0.5)
    assert len(none) == 0 and none.verts_list() == [] and none.faces_list() == []
    packed = A.cubify_packed(torch.zeros((0, 3, 3, 3)), 0.5)
    assert packed[0].shape == (0,) and packed[2].shape == (0,)
    empty = A.cubify(torch.zeros((2, 2, 2, 2)), 0.5)
    assert [(t.shape, t.dtype) for t in empty.verts_list() + empty.faces_list()] == [((0,), torch.float32)] * 2 + [((0,), torch.int64)] * 2
    nan = A.cubify_packed(torch.full((1, 2, 2, 2), float("nan")), float("-inf"))
    assert nan[0].shape == (0,)  # NaN is never occupied


def test_feats_are_ignored_unless_align_is_center():
    voxels, thresh, feats, _ = C.inputs("feats_center")
    for align in ("topleft", "corner"):
        assert M.cubify_packed_torch(voxels, thresh, feats, align)[4] is None
        assert A.cubify(voxels, thresh, feats=feats, align=align).textures is None
        assert M.cubify_packed_torch(voxels, thresh, torch.rand(3), align)[4] is None  # not even looked at
    tex = A.cubify(voxels, thresh, feats=feats, align="center").textures
    assert [t.shape for t in tex] == [(int(n), 1, 1, 3) for n in C.fixture()["feats_center/nf"]]
    with pytest.raises(ValueError, match="feats must have shape"):
        A.cubify(voxels, thresh, feats=feats[:, :, :2], align="center")


@pytest.mark.parametrize("wrong", ["gt", "memory_order", "all_vertices"])
def test_wrong_variants_are_rejected_by_the_same_comparison(wrong):
    assert C.failures(_formulation) == []
    failed = C.failures(functools.partial(_formulation, _wrong=wrong))
    assert failed, wrong
    if wrong == "gt":  # only where a value equals the threshold
        assert {m.split()[0] for m in failed} == {"thresh07"}
    else:
        assert len({m.split()[0] for m in failed}) >= 20


def test_c_abi_argument_checks_and_lists():
    lib = _lib.load()
    header = open(_lib.EXTENSION_HEADER_PATH).read()
    for name in ("p3di_cubify_workspace_bytes", "p3di_cubify_count", "p3di_cubify_emit"):
        assert name + "(" in header and name in _lib.EXTENSION_SYMBOLS and name not in _lib.EXPORTED_SYMBOLS
    for const in ("CUBIFY_BLOCK", "CUBIFY_ITEMS", "CUBIFY_CARRY_BLOCK"):
        assert const in _lib.EXTENSION_CONSTANTS and getattr(_lib, const) == _lib.EXTENSION_CONSTANTS[const]
    assert _lib.CUBIFY_ITEMS % _lib.CUBIFY_BLOCK == 0 and _lib.CUBIFY_BLOCK % 64 == 0
    from pytorch3d_amd import build, shim

    assert "cubify.hip" in build.SOURCES and "cubify" not in shim.EXPORTS
    assert ("pytorch3d.ops.cubify", ("pytorch3d.ops",), shim._cubify) in shim._FUNCTION_PATCHES
    assert "cubify" in A.__doc__ and A.cubify is M.cubify and A.cubify_packed is M.cubify_packed

    f, i = torch.zeros(64), torch.zeros(64, dtype=torch.int64)
    p, q = f.data_ptr(), i.data_ptr()
    s4, s5 = (_lib.c_i64 * 4)(27, 9, 3, 1), (_lib.c_i64 * 5)(81, 27, 9, 3, 1)
    need = lib.p3di_cubify_workspace_bytes(2, 3, 3, 3)
    assert need >= 2 * 27 + 4 * 2 * 64 and lib.p3di_cubify_workspace_bytes(-1, 3, 3, 3) == 0
    assert lib.p3di_cubify_workspace_bytes(1, 2048, 2048, 2048) == 0  # beyond int32: refused, the Python layer takes the formulation
    assert not _C.cubify_fits(1, 2048, 2048, 2048) and not _C.cubify_fits(64, 152, 152, 152) and _C.cubify_fits(64, 24, 24, 24)
    # zero sizes: P3D_OK without a launch (runs without a GPU)
    assert lib.p3di_cubify_count(None, s4, 0, 3, 3, 3, 0.5, None, 0, None, None) == _lib.OK
    assert lib.p3di_cubify_emit(None, None, s5, 0, 2, 3, 3, 3, 0, 0, None, 0, None, None, None, None) == _lib.OK
    for N, D, H, W in ((-1, 3, 3, 3), (2, 0, 3, 3), (2, 3, -1, 3), (2, 3, 3, 0), (1, 2048, 2048, 2048)):
        assert lib.p3di_cubify_count(p, s4, N, D, H, W, 0.5, p, 1 << 20, q, None) == _lib.ERR_INVALID_ARG
        assert lib.p3di_cubify_emit(p, None, s5, 0, N, D, H, W, 8, 12, p, 1 << 20, p, q, None, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_cubify_count(None, s4, 2, 3, 3, 3, 0.5, p, need, q, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_cubify_count(p, s4, 2, 3, 3, 3, 0.5, p, need, None, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_cubify_count(p, None, 2, 3, 3, 3, 0.5, p, need, q, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_cubify_count(p, s4, 2, 3, 3, 3, 0.5, p, need - 1, q, None) == _lib.ERR_WORKSPACE
    assert lib.p3di_cubify_count(p, s4, 2, 3, 3, 3, 0.5, None, need, q, None) == _lib.ERR_WORKSPACE
    for verts, faces, coords in ((None, q, p), (p, None, p), (p, q, None)):
        assert lib.p3di_cubify_emit(coords, None, s5, 0, 2, 3, 3, 3, 8, 12, p, need, verts, faces, None, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_cubify_emit(p, p, s5, 3, 2, 3, 3, 3, 8, 12, p, need, p, q, None, None) == _lib.ERR_INVALID_ARG  # feats, no output
    assert lib.p3di_cubify_emit(p, p, None, 3, 2, 3, 3, 3, 8, 12, p, need, p, q, p, None) == _lib.ERR_INVALID_ARG
    for K, tv, tf in ((-1, 8, 12), (0, -1, 12), (0, 8, -1), (0, 2 * 64 + 1, 12), (0, 8, 12 * 54 + 1), (0, 0, 12)):
        assert lib.p3di_cubify_emit(p, None, s5, K, 2, 3, 3, 3, tv, tf, p, need, p, q, None, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_cubify_emit(p, None, s5, 0, 2, 3, 3, 3, 8, 12, p, need - 1, p, q, None, None) == _lib.ERR_WORKSPACE
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        _C.cubify_count(torch.zeros((1, 2, 2, 2)), 0.5)


def test_the_shim_replaces_and_restores_both_holders():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    if not os.path.isdir(os.path.join(stage, "pytorch3d", "ops")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_cubify_case.py"), "cpu"], capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    assert rec["plain_leaves_cubify_alone"] and rec["plain_misses"] == [] and rec["calls_before_patch"] == 0
    assert rec["patched"] and rec["device_misses"] == [] and rec["host_misses"] == [] and rec["float64_misses"] == []
    assert rec["device_calls"] == [0, rec["cases"]] and rec["host_and_float64_calls"] == [0, 3]  # CPU tensors: the formulation, counted as fallbacks
    assert rec["restored"]
