"""box3d_overlap on the GPU: csrc/box3d.hip against the reference's recorded results (tests/golden/box3d_ref.npz) and against the
library's host loop, with the gates of tests/box3d_case.py; the overflow path (lists in the workspace slab) by lowering the LDS
capacity, an ordinary argument of the C entry; the grid-stride loop; run-to-run and stream-to-stream bits; the shim."""
import json
import os
import subprocess
import sys

import pytest
import torch

import box3d_case as C

import pytorch3d_amd as p3d
from pytorch3d_amd import _C, _lib, iou_box3d as mod

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("name", C.all_cases())
def test_kernel_matches_the_reference_and_the_host_path(name):
    z = C.fixture()
    b1, b2 = C.inputs(name)
    assert mod.kernel_path(b1.to(DEV), b2.to(DEV))
    vol, iou = p3d.box3d_overlap(b1.to(DEV), b2.to(DEV))
    assert vol.device == DEV and C.gate(name, vol, iou, show=print) == []
    # against the host path, within the same bounds (bit-equality is reported, not relied on)
    hv, hi = _C.iou_box3d_host(b1, b2)
    print(name, "kernel == host loop, bit for bit:", _same((vol.cpu(), iou.cpu()), (hv, hi)))
    for what, got, want in (("vol", vol.cpu(), hv), ("iou", iou.cpu(), hi)):
        if C.family(name) in ("objectron", "real"):
            excess = ((got - want).abs() - (1e-8 + 1e-5 * want.abs())).max().item()
        else:
            excess = (got.double() - want.double()).abs().max().item() - C.tolerances(name, z)[what == "iou"]
        assert excess <= 0, (name, what, excess)


def test_same_bits_on_a_second_run_and_a_second_stream():
    b1, b2 = (t.to(DEV) for t in C.inputs("random_24x24"))
    first = _C.iou_box3d(b1, b2)
    second = _C.iou_box3d(b1, b2)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        third = _C.iou_box3d(b1, b2)
    side.synchronize()
    assert _same(first, second) and _same(first, third)


def test_a_lowered_capacity_sends_most_overlapping_pairs_to_the_slab_launch_with_the_same_bits():
    z = C.fixture()
    b1, b2 = (t.to(DEV) for t in C.inputs("random_24x24"))
    overlapping = int((z["random_24x24/vol"] > 0).sum())
    vol, iou, redone = _C.iou_box3d(b1, b2, return_overflow=True)
    low_vol, low_iou, low_redone = _C.iou_box3d(b1, b2, lds_capacity=16, return_overflow=True)
    print("pairs redone in the slab launch: %d at the default capacity, %d of %d overlapping at capacity 16"
          % (int(redone), int(low_redone), overlapping))
    assert int(redone) <= overlapping // 10            # the default capacity holds nearly every pair on chip
    assert overlapping // 2 < int(low_redone) <= b1.shape[0] * b2.shape[0]
    assert _same((vol, iou), (low_vol, low_iou))
    assert C.gate("random_24x24", low_vol, low_iou) == []
    with pytest.raises(RuntimeError, match="p3d error -1"):  # below the 12 triangles of a box, above the LDS buffers
        _C.iou_box3d(b1, b2, lds_capacity=11)
    with pytest.raises(RuntimeError, match="p3d error -1"):
        _C.iou_box3d(b1, b2, lds_capacity=_lib.BOX3D_LDS_CAPACITY + 1)


def test_more_pairs_than_one_grid_take_the_stride_loop():
    per_round = _lib.BOX3D_MAX_GROUPS * _lib.BOX3D_WAVES_PER_GROUP
    n, m = 129, 128
    assert per_round < n * m <= 2 * per_round  # the last rows of boxes1 are reached in the loop's second round only
    gen = torch.Generator().manual_seed(C.SEED)
    b1, b2 = C.random_boxes(n, gen).float(), C.random_boxes(m, gen).float()
    vol, iou = _C.iou_box3d(b1.to(DEV), b2.to(DEV))
    # 64 pairs against the host loop, half of them from the second round
    rows, cols = torch.tensor([0, 1, 64, 127, 128, 128, 128, 128]), torch.tensor([0, 5, 17, 31, 64, 90, 126, 127])
    assert (rows[4:] * m + cols[4:] >= per_round).all()
    hv, hi = _C.iou_box3d_host(b1[rows], b2[cols])
    z = C.fixture()
    tol_v = max(C.MARGIN * float(z["err/random"][0]), C.ulp32(hv.max()))
    tol_i = max(C.MARGIN * float(z["err/random"][1]), C.ulp32(hi.max()))
    assert (hv > 0).any() and (hv[4:] > 0).any()
    assert (vol.cpu()[rows][:, cols] - hv).abs().max().item() <= tol_v and (iou.cpu()[rows][:, cols] - hi).abs().max().item() <= tol_i
    # the same boxes in two halves, each within one round
    top, bottom = _C.iou_box3d(b1[:65].to(DEV), b2.to(DEV)), _C.iou_box3d(b1[65:].to(DEV), b2.to(DEV))
    assert torch.equal(torch.cat([top[0], bottom[0]]), vol) and torch.equal(torch.cat([top[1], bottom[1]]), iou)


def test_empty_batches_and_views_on_the_device():
    b1, b2 = (t.to(DEV) for t in C.inputs("random_7x9"))
    for n, m in ((0, 3), (3, 0)):
        vol, iou = p3d.box3d_overlap(b1[:n], b2[:m])
        assert vol.shape == (n, m) and iou.shape == (n, m) and vol.device == DEV
    wide = torch.zeros(7, 8, 5, device=DEV)
    wide[:, :, 1:4] = b1
    assert _same(p3d.box3d_overlap(wide[:, :, 1:4], b2), p3d.box3d_overlap(b1, b2))
    with pytest.raises(ValueError, match="boxes1 is on cuda:0 and boxes2 on cpu"):
        mod.iou_box3d_op(b1, b2.cpu())
    vol, _ = p3d.box3d_overlap(b1.clone().requires_grad_(True), b2)
    with pytest.raises(ValueError, match="box3d_overlap backward is not supported"):
        vol.sum().backward()


def test_reference_function_through_the_shim():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_box3d_case.py"), "cuda:0"], capture_output=True, text=True,
                         timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    print(json.dumps(rec))
    assert rec["unpatched_is_the_reference"] and rec["calls_before_patch"] == 0
    assert rec["plain_misses"] == [] and rec["plain_backward_raises"] and rec["plain_checks_raise"]
    assert rec["patched_everywhere"] and rec["patched_misses"] == [] and rec["patched_checks_raise"] and rec["restored"]
    # GPU tensors: the kernels, one call per case
    assert rec["fused_calls"] == len(C.all_cases()) and rec["fallback_calls"] == 0
