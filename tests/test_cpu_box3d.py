"""box3d_overlap without a GPU: the library's host loop (p3d_iou_box3d_host, the geometry of csrc/box3d_geom.h that the kernels share)
against the reference's recorded results (tests/golden/box3d_ref.npz, made by tests/golden/make_golden_box3d.py from the reference's
own CPU operator and an independent float64 intersection), the validation, the shim module and the C ABI's declarations.

Tolerances: tests/box3d_case.py gate() -- 4 x the reference's own float32 error per family against the float64 figures and against
the reference's outputs, never below one float32 ulp of the case's largest value; the lattice cases with the unit-scale tolerance;
the reference's test data under its tests' assertClose defaults.  Every entry of every case is compared.
"""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import box3d_case as C

import pytorch3d_amd as p3d
from pytorch3d_amd import _C, _lib, iou_box3d as mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", C.all_cases())
def test_host_path_matches_the_reference(name):
    b1, b2 = C.inputs(name)
    vol, iou = p3d.box3d_overlap(b1, b2)
    assert not mod.kernel_path(b1, b2)
    assert C.gate(name, vol, iou, show=print) == []
    # (both argument orders: the rot, lattice and real cases hold the two boxes on both sides, so [0, 1] and [1, 0] are the two orders)
    if C.family(name) in ("random", "objectron"):  # the swapped call is the transpose up to the reference's own asymmetry
        vol_t, iou_t = p3d.box3d_overlap(b2, b1)
        assert vol_t.shape == (b2.shape[0], b1.shape[0]) and torch.equal(vol_t == 0, vol.t() == 0)


def test_a_pair_without_fragments_is_exactly_zero():
    z = C.fixture()
    for name in ("lattice_disjoint_same_floor", "random_24x24"):
        vol, iou = p3d.box3d_overlap(*C.inputs(name))
        apart = z[name + "/vol"] == 0
        assert apart.any() and torch.equal(vol == 0, apart) and torch.equal(iou == 0, apart)


def test_shape_dtype_and_device_errors():
    b = C.inputs("random_3x5")[0]
    with pytest.raises(ValueError, match=re.escape("Each box in the batch must be of shape (8, 3)")):
        p3d.box3d_overlap(b, torch.zeros(4, 10, 3))
    with pytest.raises(ValueError, match=re.escape("Each box in the batch must be of shape (8, 3)")):
        p3d.box3d_overlap(torch.zeros(4, 8, 2), b)
    with pytest.raises(ValueError, match="float32"):
        mod.iou_box3d_op(b.double(), b.double())
    with pytest.raises(ValueError, match="boxes1 is torch.float32 and boxes2 torch.float64"):
        mod.iou_box3d_op(b, b.double())
    with pytest.raises(ValueError, match=re.escape("(B, 8, 3)")):
        mod.iou_box3d_op(b[0], b)
    with pytest.raises(ValueError, match="boxes1 is on cpu and boxes2 on meta"):
        mod.iou_box3d_op(b, b.to("meta"))
    with pytest.raises(RuntimeError, match="GPU path only"):  # the device entry is not a fallback for CPU tensors
        _C.iou_box3d(b, b)


def test_input_checks_raise_with_the_reference_messages():
    sheared, flat = C.bad_boxes()
    good = C.inputs("random_3x5")[0]
    for a, b in ((sheared, good), (good, sheared)):
        with pytest.raises(ValueError, match="Plane vertices are not coplanar"):
            p3d.box3d_overlap(a, b)
    for a, b in ((flat, good), (good, flat)):
        with pytest.raises(ValueError, match="Planes have zero areas"):
            p3d.box3d_overlap(a, b)
    with pytest.raises(ValueError, match="Plane vertices are not coplanar"):  # the reference checks the planes of both boxes first
        p3d.box3d_overlap(flat, sheared)
    unit = C.inputs("lattice_itself")[0][:1]
    p3d.box3d_overlap(sheared, unit, eps=0.3)  # eps is the threshold of both checks, as in the reference
    with pytest.raises(ValueError, match="Planes have zero areas"):
        p3d.box3d_overlap(good, good, eps=10.0)


def test_backward_raises():
    b1, b2 = C.inputs("random_3x5")
    vol, iou = p3d.box3d_overlap(b1.requires_grad_(True), b2)
    assert vol.requires_grad
    with pytest.raises(ValueError, match="box3d_overlap backward is not supported"):
        (vol.sum() + iou.sum()).backward()


def test_empty_batches():
    b = C.inputs("random_3x5")[0]
    for n, m in ((0, 3), (3, 0), (0, 0)):
        vol, iou = p3d.box3d_overlap(b[:n], b[:m])
        assert vol.shape == (n, m) and iou.shape == (n, m) and vol.dtype == torch.float32


def test_a_non_contiguous_view_gives_the_bits_of_its_copy():
    b1, b2 = C.inputs("random_7x9")
    wide = torch.zeros(7, 8, 5)
    wide[:, :, 1:4] = b1
    view = wide[:, :, 1:4]
    every_other = torch.stack([b2, b2.flip(0)], 1).reshape(18, 8, 3)[::2]
    assert not view.is_contiguous() and not every_other.is_contiguous()
    got, want = p3d.box3d_overlap(view, every_other), p3d.box3d_overlap(b1, b2)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_the_gates_refuse_three_wrong_answers():
    z = C.fixture()
    # identical boxes with the coplanar faces counted twice: 2.0 for 1.0
    vol, iou = p3d.box3d_overlap(*C.inputs("lattice_itself"))
    assert C.gate("lattice_itself", vol, iou) == []
    assert C.gate("lattice_itself", vol * 2, iou) != []
    # the output transposed on a non-square case (the same values, laid out (M, N) and read as (N, M))
    vol, iou = p3d.box3d_overlap(*C.inputs("random_3x5"))
    assert C.gate("random_3x5", vol, iou) == []
    assert C.gate("random_3x5", vol.t().contiguous().view(3, 5), iou.t().contiguous().view(3, 5)) != []
    assert C.gate("random_3x5", vol.t(), iou.t()) != []
    # iou with the union taken as vol1 + vol2
    for name in ("random_7x9", "objectron", "lattice_half_shift"):
        vol, iou = p3d.box3d_overlap(*C.inputs(name))
        wrong = torch.where(iou > 0, vol / (vol / iou.clamp_min(1e-30) + vol), iou)  # vol / iou = vol1 + vol2 - vol
        assert C.gate(name, vol, iou) == [] and C.gate(name, vol, wrong) != []
    assert float(z["err/random"][0]) < 1e-5  # the gates are as tight as the module docstring says


def test_abi_declares_both_entries():
    header = open(os.path.join(ROOT, "include", "p3d_amd.h")).read()
    for name in ("p3d_iou_box3d", "p3d_iou_box3d_host", "p3d_iou_box3d_workspace_bytes"):
        assert re.search(r"\b%s\(" % name, header) and name in _lib.EXPORTED_SYMBOLS
    for macro, value in (("P3D_BOX3D_LDS_CAPACITY", _lib.BOX3D_LDS_CAPACITY), ("P3D_BOX3D_WAVES_PER_GROUP", _lib.BOX3D_WAVES_PER_GROUP),
                         ("P3D_BOX3D_MAX_GROUPS", _lib.BOX3D_MAX_GROUPS)):
        assert int(re.search(r"#define %s (\d+)" % macro, header).group(1)) == value
    lib = _lib.load()
    assert lib.p3d_iou_box3d_host(None, None, -1, 1, None, None) == -1 and lib.p3d_iou_box3d_host(None, None, 0, 5, None, None) == 0
    assert lib.p3d_iou_box3d(None, None, 2, 2, 11, None, None, None, 0, None) == -1  # a capacity below the 12 triangles of a box
    assert lib.p3d_iou_box3d(None, None, 0, 2, 64, None, None, None, 0, None) == 0   # nothing to do: no launch
    assert lib.p3d_iou_box3d_workspace_bytes(3, 5) > 15 * 4 and "iou_box3d" in _C.BOX3D_EXPORTS


def test_shim_module_serves_the_operator_in_both_flavours_on_the_cpu():
    from pytorch3d_amd import shim

    b1, b2 = C.inputs("random_3x5")
    want = _C.iou_box3d_host(b1, b2)
    for flavour in ("ctypes", "pybind"):  # (the compiled boundary is built with the library; a failure to load it fails here)
        served = shim.make_module(flavour).iou_box3d
        got = served(b1, b2)
        assert served is mod.iou_box3d_op and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_reference_function_through_the_shim_on_the_cpu():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    if not os.path.isdir(os.path.join(stage, "pytorch3d", "ops")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_box3d_case.py"), "cpu"], capture_output=True, text=True,
                         timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    print(json.dumps(rec))
    assert rec["unpatched_is_the_reference"] and rec["calls_before_patch"] == 0
    assert rec["plain_misses"] == [] and rec["plain_backward_raises"] and rec["plain_checks_raise"]
    assert rec["patched_everywhere"] and rec["patched_misses"] == [] and rec["patched_checks_raise"] and rec["restored"]
    # CPU tensors: the host loop, counted as fallbacks -- one call per case
    assert rec["fused_calls"] == 0 and rec["fallback_calls"] == len(C.all_cases())
