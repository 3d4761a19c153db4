"""Marching cubes without a GPU: the triangle table of csrc/marching_cubes_tables.h re-derived entry by entry from the record of the 256
sign configurations (tests/golden/marching_cubes_ref.npz, made by the reference's compiled CPU operator); the nested-loop restatement of
tests/marching_cubes_case.py pinned to every record and its device form tied to it; the library's host loop against every record; the
torch formulation against the device form; the return shapes, the backward's ValueError, the dtype refusal; deliberately wrong
variants refused by the same gate; the C entries' argument checks; the shim.  World coordinates, faces and counts are compared
exactly (NaN equal to NaN), local coordinates within 4 x the reference's own float32 rounding of the case (marching_cubes_case.misses)."""
import importlib
import json
import os
import re
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import marching_cubes_case as C  # noqa: E402

import pytorch3d_amd as A  # noqa: E402
from pytorch3d_amd import _C, _lib, build, shim  # noqa: E402

M = importlib.import_module("pytorch3d_amd.marching_cubes")  # (the package re-exports the FUNCTION over the sub-module)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("p3di_marching_cubes_workspace_bytes", "p3di_marching_cubes_count", "p3di_marching_cubes_emit", "p3di_marching_cubes_host")


def test_fixture_holds_every_case_and_what_the_contract_promises():
    fix = C.fixture()
    assert {k.split("/")[0] for k in fix} == set(C.cases()) | {"err"} and os.path.getsize(C.FIXTURE) < 1 << 20
    assert fix["cfg256/vol"].shape == (256, 2, 2, 2) and fix["cfg256/0/nf"].max() == 5 and fix["cfg256/0/nf"][[0, 255]].tolist() == [0, 0]
    assert fix["degen/0/nf"].tolist() == [0] * 4  # the reference dropped the later triangles with the first
    assert all(len(f) > 0 for f in C.restated("degen", False, "device")[1])  # which the device contract keeps
    world = fix["rand579/0/verts"]
    assert (((world != world.round()).sum(1)) >= 2).any()  # a constant coordinate that is not the integer
    assert float(fix["rand579/iso"]) == 0.1 and float(torch.tensor(0.1)) != 0.1
    nf = fix["mixed_empty/0/nf"].tolist()
    assert nf[0] > 0 and nf[1:4] == [0, 0, 0] and nf[4] > 0 and C.expected("mixed_empty", True)[0][2] == []
    assert all(int(fix[n + "/0/nf"].sum()) == 0 for n in ("thin_d", "thin_h", "thin_w"))
    assert C.inputs("isonone")[1] is None and fix["isonone/0/nf"].min() > 0
    assert all(not C.inputs(n)[0].is_contiguous() for n in C.STRIDED)
    assert sorted(n for n in C.cases() if C.has_drops(n)) == ["degen", "naninf", "snap"]
    assert 0 < float(fix["err/local/rand345"]) < 2e-7 and float(fix["err/local/cfg256"]) == 0.0


def test_the_table_header_entry_by_entry_and_the_crossed_edges():
    header = open(os.path.join(ROOT, "pytorch3d_amd", "csrc", "marching_cubes_tables.h")).read()
    counts = [int(x) for x in re.search(r"counts\[256\] = \{(.*?)\};", header, re.S).group(1).replace("\n", " ").split(",") if x.strip()]
    rows = [[int(e) for e in row.split(",")] for row in re.findall(r"\{([^{}]*)\}", re.search(r"entries\[256\]\[16\] = \{(.*?)\};", header, re.S).group(1))]
    record = C.table()
    assert len(counts) == 256 and len(rows) == 256 and len(record) == 256
    for config in range(256):
        want = list(record[config])
        assert rows[config] == want + [255] * (16 - len(want)), config  # every entry, and 255 behind the last
        assert counts[config] == len(want) // 3 <= 5, config
        assert set(want) == C.crossed_edges(config), config  # a configuration names exactly the edges whose ends differ
        assert all(not (e & 7) >> (e >> 3) & 1 for e in want)  # an edge starts at the corner whose axis bit is 0
    assert M.triangle_table() == tuple(record)
    assert sum(counts) == 820 and counts[0] == counts[255] == 0


@pytest.mark.parametrize("name", C.cases())
def test_restatement_equals_the_record_and_its_device_form_is_tied_to_it(name):
    for local in (False, True):
        assert C.misses(C.restated(name, local, "cpu"), C.expected(name, local), name, C.tolerance(name, local)) == []
    assert C.tie_misses(name) == []
    vol, iso = C.inputs(name)
    for v in vol:
        level = ((v.max() + v.min()) / 2).item() if iso is None else iso
        ids = C.restate_device_one(v.numpy(), level)[2]
        assert bool((ids[1:] > ids[:-1]).all())


def test_host_loop_equals_every_record():
    before = dict(M.CALLS)
    assert C.failures(lambda v, i, l: A.marching_cubes(v, i, l), "cpu") == []
    assert M.CALLS["host"] - before["host"] == 2 * len(C.cases()) and M.CALLS["fused"] == before["fused"]
    assert C.failures(lambda v, i, l: C.to_lists(*A.marching_cubes_packed(v, i, l)), "cpu", names=["rand345", "mixed_empty", "snap"]) == []


def test_formulation_equals_the_device_form_on_every_case():
    assert C.failures(lambda v, i, l: C.to_lists(*A.marching_cubes_torch(v, i, l)), "device") == []
    for name in ("rand579", "snap", "naninf"):  # and is tied to the record like the restatement
        assert C.tie_misses(name, C.to_lists(*A.marching_cubes_torch(*C.inputs(name), False))) == []
    vol, iso = C.inputs("rand345")
    ids = M._torch_packed(vol, M.isolevels(vol, iso), False)[1]
    want = C.restate_device_one(vol[0].numpy(), iso)[2]
    assert len(want) > 0 and torch.equal(ids[:len(want)], want)


def test_return_shapes_lists_and_empties():
    vol, iso = C.inputs("mixed_empty")
    verts, faces = A.marching_cubes(vol, iso)
    assert isinstance(verts, list) and isinstance(faces, list) and len(verts) == len(faces) == 5
    assert verts[1] == [] and faces[1] == [] and verts[3] == [] and verts[0].shape[1:] == (3,) and faces[0].dtype == torch.int64
    packed = A.marching_cubes_packed(vol, iso)
    assert packed[2].tolist() == [len(v) for v in verts] and packed[3].tolist() == [len(f) for f in faces]
    assert packed[0].shape == (sum(packed[2].tolist()), 3) and packed[1].shape == (sum(packed[3].tolist()), 3)
    assert A.marching_cubes(torch.zeros((0, 3, 3, 3)), 0.0) == ([], [])
    assert A.marching_cubes(torch.zeros((2, 1, 3, 3)), None) == ([[], []], [[], []])
    out = M.marching_cubes_op(vol[1], 0.0)
    assert [tuple(t.shape) for t in out] == [(0, 3), (0, 3), (0,)]
    verts0, faces0, ids0 = M.marching_cubes_op(vol[0], 0.0)
    want = C.expected("mixed_empty", False)
    assert torch.equal(verts0, want[0][0]) and torch.equal(faces0, want[1][0]) and torch.equal(ids0, torch.zeros(len(verts0), dtype=torch.int64))
    with pytest.raises(ValueError):
        A.marching_cubes(vol[0], 0.0)
    assert not M.kernel_path(vol) and not M.kernel_path(vol.double())


def test_backward_raises_as_the_reference_does():
    vol = C.inputs("rand345")[0].clone().requires_grad_(True)
    verts, faces = A.marching_cubes(vol, 0.0)
    assert verts[0].requires_grad and not faces[0].requires_grad
    with pytest.raises(ValueError, match="marching_cubes backward is not supported"):
        verts[0].sum().backward()
    packed = A.marching_cubes_packed(vol, 0.0)
    with pytest.raises(ValueError, match="marching_cubes backward is not supported"):
        packed[0].sum().backward()
    assert not A.marching_cubes(vol.detach(), 0.0)[0][0].requires_grad


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.int32])
def test_other_dtypes_are_refused(dtype):
    vol = C.inputs("rand345")[0].to(dtype)
    for fn in (A.marching_cubes, A.marching_cubes_packed, A.marching_cubes_torch):
        with pytest.raises(RuntimeError, match="expected scalar type Float"):
            fn(vol, 0.0)
    with pytest.raises(RuntimeError, match="expected scalar type Float"):
        M.marching_cubes_op(vol[0], 0.0)


WRONG = {  # variant -> (contract it misreads, cases that must refuse it)
    "integer_constant": ("cpu", ["rand579"]), "lerp": ("cpu", ["rand579"]), "le": ("cpu", ["snap", "degen"]),
    "no_snap": ("cpu", ["snap"]), "drop_alone": ("cpu", ["degen"]), "drop_degenerate": ("device", ["degen", "snap"]),
    "first_use": ("device", ["rand345"]), "zyx": ("device", ["rand345"]),
}


@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_wrong_variants_are_refused_by_the_same_gate(wrong):
    contract, names = WRONG[wrong]
    for name in names:
        vol, iso = C.inputs(name)
        want = C.expected(name, False) if contract == "cpu" else C.restated(name, False, "device")
        assert C.misses(C.restate(vol, iso, False, contract, wrong), want, name) != [], (wrong, name)
        assert C.misses(C.restate(vol, iso, False, contract), want, name) == []


def test_c_abi_argument_checks():
    header = open(_lib.EXTENSION_HEADER_PATH).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header) and name in _lib.EXTENSION_SYMBOLS and name not in _lib.EXPORTED_SYMBOLS
    for const in ("MARCHING_CUBES_BLOCK", "MARCHING_CUBES_ITEMS", "MARCHING_CUBES_CARRY_BLOCK"):
        assert const in _lib.EXTENSION_CONSTANTS and getattr(_lib, const) == _lib.EXTENSION_CONSTANTS[const] > 0
    assert "marching_cubes.hip" in build.SOURCES and shim.EXPORTS["marching_cubes"] == ("marching_cubes", "marching_cubes_op")
    assert ("pytorch3d.ops.marching_cubes", ("pytorch3d.ops",), shim._marching_cubes) in shim._FUNCTION_PATCHES
    assert _C.marching_cubes_fits(8, 128, 128, 128) and not _C.marching_cubes_fits(1, 1024, 1024, 1024) and not _C.marching_cubes_fits(2, 0, 3, 3)
    lib = _lib.load()
    need = lib.p3di_marching_cubes_workspace_bytes(2, 3, 3, 3)
    assert need >= 4 * 2 * 27 + 2 * 4 * 3 and lib.p3di_marching_cubes_workspace_bytes(-1, 3, 3, 3) == 0
    assert lib.p3di_marching_cubes_workspace_bytes(1, 1024, 1024, 1024) == 0  # beyond int32: refused, the Python layer takes the formulation
    import ctypes

    s4, s3 = (ctypes.c_int64 * 4)(27, 9, 3, 1), (ctypes.c_int64 * 3)(9, 3, 1)
    buf = torch.zeros(1 << 18, dtype=torch.int64)
    p = buf.data_ptr()
    assert lib.p3di_marching_cubes_count(None, s4, 0, 3, 3, 3, None, None, 0, None, None) == _lib.OK  # no launch: runs without a GPU
    assert lib.p3di_marching_cubes_emit(None, s4, 2, 3, 3, 3, None, 0, 0, 0, None, 0, None, None, None, None) == _lib.OK
    for N, D, H, W in ((-1, 3, 3, 3), (2, 0, 3, 3), (2, 3, 3, 0), (1, 1024, 1024, 1024)):
        assert lib.p3di_marching_cubes_count(p, s4, N, D, H, W, p, p, 1 << 21, p, None) == _lib.ERR_INVALID_ARG
        assert lib.p3di_marching_cubes_emit(p, s4, N, D, H, W, p, 0, 8, 12, p, 1 << 21, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_marching_cubes_count(None, s4, 2, 3, 3, 3, p, p, need, p, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_marching_cubes_count(p, s4, 2, 3, 3, 3, None, p, need, p, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_marching_cubes_count(p, s4, 2, 3, 3, 3, p, p, need, None, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_marching_cubes_count(p, None, 2, 3, 3, 3, p, p, need, p, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_marching_cubes_count(p, s4, 2, 3, 3, 3, p, p, need - 1, p, None) == _lib.ERR_WORKSPACE
    assert lib.p3di_marching_cubes_count(p, s4, 2, 3, 3, 3, p, None, need, p, None) == _lib.ERR_WORKSPACE
    for tv, tf in ((-1, 12), (8, -1), (3 * 2 * 27 + 1, 12), (8, 5 * 2 * 27 + 1), (0, 12)):
        assert lib.p3di_marching_cubes_emit(p, s4, 2, 3, 3, 3, p, 0, tv, tf, p, need, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_marching_cubes_emit(p, s4, 2, 3, 3, 3, p, 0, 8, 12, p, need, p, None, p, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_marching_cubes_emit(p, s4, 2, 1, 3, 3, p, 0, 8, 12, p, need, p, p, p, None) == _lib.ERR_INVALID_ARG  # no cube, yet faces
    assert lib.p3di_marching_cubes_emit(p, s4, 2, 3, 3, 3, p, 0, 8, 12, p, need - 1, p, p, p, None) == _lib.ERR_WORKSPACE
    # the host entry: a counting call without outputs, capacities respected
    vol, iso = C.inputs("rand345")
    counts = torch.zeros(2, dtype=torch.int64)
    rank = torch.full((3 * 60,), -1, dtype=torch.int64)
    s3 = (ctypes.c_int64 * 3)(*vol[0].stride())
    assert lib.p3di_marching_cubes_host(vol[0].data_ptr(), s3, 3, 4, 5, iso, rank.data_ptr(), None, 0, None, 0, counts.data_ptr()) == _lib.OK
    want = C.expected("rand345", False)
    assert counts.tolist() == [len(want[0][0]), len(want[1][0])]
    assert lib.p3di_marching_cubes_host(vol[0].data_ptr(), s3, 1, 4, 5, iso, None, None, 0, None, 0, counts.data_ptr()) == _lib.OK and counts.tolist() == [0, 0]
    assert lib.p3di_marching_cubes_host(vol[0].data_ptr(), s3, 3, 4, 5, iso, rank.data_ptr(), None, 4, None, 0, counts.data_ptr()) == _lib.ERR_INVALID_ARG
    assert lib.p3di_marching_cubes_host(vol[0].data_ptr(), s3, 0, 4, 5, iso, rank.data_ptr(), None, 0, None, 0, counts.data_ptr()) == _lib.ERR_INVALID_ARG
    assert lib.p3di_marching_cubes_host(None, s3, 3, 4, 5, iso, rank.data_ptr(), None, 0, None, 0, counts.data_ptr()) == _lib.ERR_INVALID_ARG
    assert lib.p3di_marching_cubes_host(vol[0].data_ptr(), s3, 3, 4, 5, iso, rank.data_ptr(), None, 0, None, 0, None) == _lib.ERR_INVALID_ARG
    with pytest.raises(RuntimeError, match="CPU tensor"):
        _C.marching_cubes_host(vol, iso)


def test_the_shim_serves_the_reference_function_and_rebinds_it():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    if not os.path.isdir(os.path.join(stage, "pytorch3d", "ops")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_marching_cubes_case.py"), "cpu"], capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    assert rec["plain_is_the_reference_function"] and rec["plain_misses"] == [] and rec["calls_before_patch"] == 0
    assert rec["patched"] and rec["patched_misses"] == [] and rec["patched_calls"] == [0, 2 * rec["cases"]]  # CPU tensors: counted as fallbacks
    assert rec["restored"] and rec["restored_misses"] == []
