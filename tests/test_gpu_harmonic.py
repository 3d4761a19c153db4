"""csrc/harmonic.hip on the GPU: every case of tests/harmonic_case.py through the kernels and the gates of the case file (gate 1 with
the device's own sinf / expf error measured from the torch chain, never from the kernel), every needs_input_grad combination, the
exact parts (appended block, layouts, streams, zero rows, module == function), one launch beyond the group cap, the stratified
depths bit for bit against the reference's recording, and the unmodified reference through the shim (tests/shim_harmonic_case.py)."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import harmonic_case as C  # noqa: E402

import pytorch3d_amd as A  # noqa: E402
from pytorch3d_amd import _C, _lib  # noqa: E402

H = importlib.import_module("pytorch3d_amd.harmonic_embedding")
RS = importlib.import_module("pytorch3d_amd.raysampling")

pytestmark = pytest.mark.gpu
CASES = C.cases()
DEPTHS = C.depth_cases()
DEV = "cuda:0"


def fused(x, f, cov, append):
    assert H.kernel_path(x, f, cov, append)
    before = H.CALLS["fused"]
    out = A.harmonic_embedding(x, f, cov, append)
    assert H.CALLS["fused"] == before + 1
    return out


@pytest.fixture(scope="module")
def e_device():
    """The error of the device's own sin / exp under the argument-exact truth, from the reference's formula (the torch chain) on the
    device: what gate 1 allows on top of the CPU's E_sin / E_exp."""
    worst = {"sin": 0.0, "exp": 0.0}
    for case in CASES:
        x, cov, f, _ = C.inputs(case, DEV)
        with torch.no_grad():
            out = H.harmonic_embedding_torch(x, f, cov, case.append)
        which = "exp" if case.cov else "sin"
        worst[which] = max(worst[which], C.argument_error(case, out.double().cpu().numpy(), (x, cov, f, None)))
    print("E_device", worst, "E_sin", float(C.fixture()["E_sin"]), "E_exp", float(C.fixture()["E_exp"]))
    return worst


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_kernels_against_the_gates(case, e_device):
    assert C.failures([case], fused, device=DEV, e_device=e_device) == []


@pytest.mark.parametrize("need", [(True, False), (False, True), (False, False)], ids=["x", "cov", "none"])
def test_every_needs_input_grad_combination(need, e_device):
    for cid in ("cov-d3-n4", "cov-underflow", "hand-cov", "small-d3-n10-r5-a1"):
        case = C.case_by_id(cid)
        assert C.failures([case], fused, device=DEV, e_device=e_device, need=need) == []
        full, part = C.run(fused, case, device=DEV), C.run(fused, case, device=DEV, need=need)
        for q in ("grad_x", "grad_cov"):
            assert part[q] is None or np.array_equal(part[q], full[q]), (cid, q)  # the same sums whatever else is asked for


def test_exact_parts_layouts_and_zero_rows():
    for cid in ("transposed", "slice", "special"):
        case = C.case_by_id(cid)
        x, cov, f, g = C.inputs(case, DEV)
        out, same = fused(x, f, cov, case.append), fused(x.contiguous(), f, cov, case.append)
        assert (cid == "special") == x.is_contiguous()
        assert torch.equal(out.view(torch.int32), same.view(torch.int32)), cid
        assert torch.equal(out[..., 2 * case.dim * case.n:].view(torch.int32), x.contiguous().view(torch.int32)), cid  # NaN and -0.0 included
    f = torch.tensor([1.0, 2.0], device=DEV)
    for shape, cov in (((0, 3), False), ((4, 0, 3), False), ((0, 3), True)):
        x = torch.zeros(shape, device=DEV, requires_grad=True)
        out = fused(x, f, torch.zeros(shape, device=DEV) if cov else None, True)
        assert out.shape == shape[:-1] + (15,) and out.device == x.device
        out.sum().backward()
        assert x.grad.shape == shape
    one = fused(torch.tensor([0.5, -2.0, 3.0], device=DEV), f, None, False)  # no leading shape
    assert one.shape == (12,)


def test_backward_has_the_same_bits_on_every_run_and_stream():
    for cid in ("small-d3-n6-r65-a1", "cov-underflow", next(c.id for c in CASES if C.width(c) == 268 and c.lead == (31,))):
        case = C.case_by_id(cid)
        first, second = C.run(fused, case, device=DEV), C.run(fused, case, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            third = C.run(fused, case, device=DEV)
        side.synchronize()
        torch.use_deterministic_algorithms(True)
        try:
            fourth = C.run(fused, case, device=DEV)  # no second form under the flag: the same node
        finally:
            torch.use_deterministic_algorithms(False)
        for q in C.QUANTITIES:
            if first[q] is not None:
                assert all(np.array_equal(first[q], other[q], equal_nan=True) for other in (second, third, fourth)), (cid, q)


def test_module_equals_the_function():
    for cid in ("small-d3-n10-r5-a1", "small-lin-omegapi", "cov-d2-n6-noappend"):
        case = C.case_by_id(cid)
        module = A.HarmonicEmbedding(case.n, case.omega, case.logspace, case.append).to(DEV)
        x, cov, f, _ = C.inputs(case, DEV)
        before = H.CALLS["fused"]
        assert torch.equal(module(x, diag_cov=cov), fused(x, f, cov, case.append)) and H.CALLS["fused"] == before + 2
    assert module.double()(x.double()).dtype == torch.float64 and H.CALLS["fused"] == before + 2  # float64: the chain


def test_more_row_tiles_than_the_group_cap():
    """group cap x rows per tile + 1 rows at dim = 1, n = 1, no append (4 MB of output): the forward and the backward go round their
    grid-stride loops a second time, and the last row is alone in the last tile."""
    rows = _lib.HARMONIC_MAX_GROUPS * _lib.HARMONIC_FWD_ROWS + 1
    W = 2
    fwd_tiles, bwd_tiles = -(-rows // _lib.HARMONIC_FWD_ROWS), -(-rows // C.backward_tile_rows(W, _lib))
    assert fwd_tiles == _lib.HARMONIC_MAX_GROUPS + 1 and bwd_tiles > _lib.HARMONIC_MAX_GROUPS and rows * W * 4 < 8 * 2 ** 20
    g = torch.Generator().manual_seed(C.SEED + 5)
    x = (2 * torch.rand((rows, 1), generator=g) - 1).to(DEV).requires_grad_(True)
    f = torch.tensor([3.0], device=DEV)
    grad = torch.randn((rows, W), generator=g).to(DEV)
    out = fused(x, f, None, False)
    (gx,) = torch.autograd.grad(out, x, grad)
    xd = x.detach().double().requires_grad_(True)
    truth = H.harmonic_embedding_torch(xd, f.double(), None, False)
    (tgx,) = torch.autograd.grad(truth, xd, grad.double())
    out, truth = out.detach(), truth.detach()
    fix = C.fixture()
    small = C.case_by_id("rows257")
    assert float((out.double() - truth).abs().max()) <= C.GATE_FACTOR * C.e_ref(small, "out") * float(truth.abs().max())
    assert float((gx.double() - tgx).abs().max()) <= C.GATE_FACTOR * C.e_ref(small, "grad_x") * float(tgx.abs().max())
    # the argument-exact gate on the device: float32 argument, float64 sine
    a = (x.detach() * f)[:, None, :] + torch.tensor([0.0, float(C.HALF_PI32)], device=DEV)[:, None]
    chain = H.harmonic_embedding_torch(x.detach(), f, None, False)
    exact = a.double().sin().reshape(rows, W)
    e_dev = float((chain.double() - exact).abs().max())
    assert float((out.double() - exact).abs().max()) <= C.GATE_FACTOR * max(float(fix["E_sin"]), e_dev)
    # the second pass and the last row were reached: the rows of the second pass are not what an untouched buffer holds
    tail = fused(x.detach()[-1:], f, None, False)
    assert torch.equal(out[-1:], tail) and torch.equal(out[_lib.HARMONIC_MAX_GROUPS * _lib.HARMONIC_FWD_ROWS - 1:][:1],
                                                        fused(x.detach()[-2:-1], f, None, False))
    assert bool(gx[-1].abs() > 0) == bool(tgx[-1].abs() > 0)


@pytest.mark.parametrize("case", DEPTHS, ids=[c.id for c in DEPTHS])
def test_stratified_depths_bit_equal_to_the_reference_s_recording(case):
    fix = C.fixture()
    centers = C.depth_centers(case, DEV)
    u = torch.from_numpy(fix[C.key(case.id, "uniforms")]).to(DEV)
    want = torch.from_numpy(fix[C.key(case.id, "depths")])
    keep_c, keep_u, strides = centers.clone(), u.clone(), centers.stride()
    assert RS.kernel_path(centers, u)
    before = RS.CALLS["fused"]
    got = A.stratified_depths(centers, u)
    assert RS.CALLS["fused"] == before + 1 and got.shape == centers.shape and got.is_contiguous()
    assert torch.equal(got.cpu(), want)  # the kernel == the reference's own function on the CPU
    assert torch.equal(A.stratified_depths(centers.cpu(), u.cpu()), want)  # == this package's chain on the CPU
    assert torch.equal(RS.stratified_depths_torch(centers, u), got)  # == the chain on the GPU
    assert torch.equal(A.stratified_depths(centers.contiguous(), u), got)  # the expanded view against the contiguous tensor
    assert torch.equal(centers, keep_c) and torch.equal(u, keep_u) and centers.stride() == strides
    if case.form == "expand" and case.rows > 1:
        assert centers.stride(0) == 0 and centers.reshape(-1, case.n).data_ptr() == centers.data_ptr()
    if not case.edge:
        torch.manual_seed(C.depth_seed(case))
        drawn = A.stratified_depths(centers)
        torch.manual_seed(C.depth_seed(case))
        assert torch.equal(drawn, RS.stratified_depths_torch(centers))  # the same draw as the chain's rand_like


def test_stratified_depths_leading_shapes_and_strided_rows():
    line = torch.linspace(0.5, 4.0, 7, device=DEV)
    view = line[None, None].expand(2, 5, 7)  # what the ray samplers pass: (batch, rays, points), strides (0, 0, 1)
    u = torch.rand(2, 5, 7, device=DEV)
    assert torch.equal(A.stratified_depths(view, u), RS.stratified_depths_torch(view, u))
    rows = torch.sort(torch.rand(6, 14, device=DEV), dim=-1).values[:, ::2]  # a column stride of 2
    u = torch.rand(6, 7, device=DEV)
    assert rows.stride() == (14, 2) and torch.equal(A.stratified_depths(rows, u), RS.stratified_depths_torch(rows, u))
    assert torch.equal(A.stratified_depths(line, u[0]), RS.stratified_depths_torch(line, u[0]))  # no leading shape
    grad = line.clone().requires_grad_(True)
    before = RS.CALLS["chain"]
    A.stratified_depths(grad, u[0]).sum().backward()  # centres that require grad: the chain, differentiable
    assert RS.CALLS["chain"] == before + 1 and grad.grad is not None


def test_unmodified_reference_through_the_shim():
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shim_harmonic_case.py")
    res = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in out:
        pytest.skip(out["skipped"])
    print(json.dumps(out))
    assert out["not_patched_by_plain_install"] and out["patched"]
    for name in ("embedding_10", "embedding_4_no_append"):
        r = out[name]
        assert r["fused_calls"] == 1 and r["fallback_calls"] == 0, r
        assert r["out_difference"] <= r["out_gate"] and r["grad_difference"] <= r["grad_gate"] and r["grad_max"] > 0, r
    for name in ("ndc_multinomial", "monte_carlo"):
        r = out[name]
        assert r["same_bits"] and r["fused_calls"] == 1 and r["fallback_calls"] == 0 and r["jiggled"], r
    assert out["lengths_without_stratification_stride"] == 0
    assert out["cpu_embedding"] == {"fused": 0, "fallback": 1} and out["float64_embedding"] == {"fused": 0, "fallback": 1}
    assert out["cpu_depths"] == {"fused": 0, "fallback": 1} and out["float64_depths"] == {"fused": 0, "fallback": 1}
    assert out["restored"] and out["plain_install_after_restore_patches_neither"]
