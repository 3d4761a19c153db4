"""csrc/implicit.hip on the GPU: sample_pdf bit-equal to the reference's compiled operator and to the library's host loop, the
raymarch kernels through the gates of tests/implicit_case.py (4 E_ref per quantity, E_ref from the fixture), the same bits on every
run, stream and under the strict deterministic flag, and the unmodified reference classes through the shim (a subprocess)."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import implicit_case as C  # noqa: E402

import pytorch3d_amd as A  # noqa: E402
from pytorch3d_amd import _lib, implicit  # noqa: E402

pytestmark = pytest.mark.gpu
D = "cuda:0"
PDF_CASES, RAY_CASES = C.pdf_cases(), C.ray_cases()


def _kernel(bins, weights, u, eps):
    out = u.to(D)
    version = out._version
    assert implicit.sample_pdf_op(bins.to(D), weights.to(D), out, eps) is None
    assert out._version > version
    return out.cpu()


@pytest.mark.parametrize("case", PDF_CASES, ids=[c[0] for c in PDF_CASES])
def test_sample_pdf_kernel_equals_the_reference_operator_bit_for_bit(case):
    bins, weights, u, eps = C.pdf_inputs(case)
    if case[3] == C.LONG_BINS:  # the workspace form is what runs: from the library's constants
        assert (case[3] | 1) > _lib.SAMPLE_PDF_LDS_FLOATS and _lib.load().p3di_sample_pdf_workspace_bytes(case[2], case[3]) > 0
    assert C.same_bits(_kernel(bins, weights, u, eps).numpy(), C.fixture()["pdf/" + case[0]])


@pytest.mark.parametrize("B,n,S", [(100, 17, 33), (1000, 128, 64), (17, 4000, 7), (3, 8191, 3), (3, 9000, 4), (4097, 63, 16)])
def test_sample_pdf_kernel_equals_the_host_loop_on_other_shapes(B, n, S):
    g = torch.Generator().manual_seed(B * 31 + n)
    bins = torch.cumsum(torch.rand((B, n + 1), generator=g), 1)
    weights = torch.rand((B, n), generator=g) * (torch.rand((B, n), generator=g) < 0.7)
    u = torch.rand((B, S), generator=g)
    host = u.clone()
    implicit.sample_pdf_op(bins, weights, host, 1e-5)
    assert C.same_bits(_kernel(bins, weights, u, 1e-5).numpy(), host.numpy())


def test_public_sample_pdf_on_the_gpu():
    case = next(c for c in PDF_CASES if c[0] == "special-det")
    bins, weights, u, eps = C.pdf_inputs(case)
    got = A.sample_pdf(bins.to(D).reshape(2, 4, -1), weights.to(D).reshape(2, 4, -1), case[4], det=True, eps=eps)
    assert got.is_cuda and C.same_bits(got.reshape(8, -1).cpu().numpy(), C.fixture()["pdf/special-det"])
    views = A.sample_pdf(bins.to(D).t().contiguous().t(), weights.to(D).t().contiguous().t(), case[4], det=True, eps=eps)  # strided inputs
    assert C.same_bits(views.cpu().numpy(), C.fixture()["pdf/special-det"])


@pytest.mark.parametrize("case", RAY_CASES, ids=[c[0] for c in RAY_CASES])
def test_raymarch_kernels_pass_the_gates(case):
    d, f = C.ray_inputs(case)[:2]
    assert implicit.kernel_path(d.to(D), f.to(D), case[4])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = C.run_ray(A.ea_raymarch, case, device=D)
    assert bool(caught) == (case[5] == "over")  # the reference's bounds warning, and only there
    errors = C.ray_errors(case, got)
    for q, (err, gate) in errors.items():
        print("%-15s error %.3e gate %.3e" % (q, err, gate))
    assert all(err <= gate for err, gate in errors.values()), errors


def test_absorption_only_kernel():
    for case in RAY_CASES[::5]:
        d = C.ray_inputs(case)[0]
        d64 = d.double().requires_grad_(True)
        truth = implicit.absorption_only_raymarch_torch(d64)
        g = torch.randn(truth.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
        (truth_grad,) = torch.autograd.grad((truth * g).sum(), d64)
        dg = d.to(D).requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = A.absorption_only_raymarch(dg)
        (got_grad,) = torch.autograd.grad((got * g.float().to(D)).sum(), dg)
        assert got.shape == truth.shape and got_grad.shape == d.shape
        assert np.array_equal(truth.detach().numpy(), C.fixture()[C.key(case[0], "opacities")])
        assert (got.cpu().double() - truth).abs().max() <= C.GATE_FACTOR * C.e_ref("opacities") * truth.abs().max()
        assert (got_grad.cpu().double() - truth_grad).abs().max() <= C.GATE_FACTOR * C.e_ref("grad_densities") * truth_grad.abs().max()


def _raymarch_bits(case, stream=None):
    d, f, g_out, g_w, eps = C.ray_inputs(case)
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        d, f = d.to(D).requires_grad_(True), f.to(D).requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out, w = A.ea_raymarch(d, f, eps, case[4], return_weights=True)
        loss = (out * g_out.to(D)).sum() + (w * (g_w.to(D) if g_w is not None else 1.0)).sum()
        gd, gf = torch.autograd.grad(loss, (d, f))
        torch.cuda.synchronize()
    return [t.detach().cpu() for t in (out, w, gd, gf)]


def test_same_bits_on_every_run_stream_and_under_the_deterministic_flag():
    cases = [c for c in RAY_CASES if c[0].startswith("x-")] + RAY_CASES[:45:6]
    pdf = next(c for c in PDF_CASES if c[0] == "grid-B257-n63-S129-rand")
    bins, weights, u, eps = C.pdf_inputs(pdf)
    first = {c[0]: _raymarch_bits(c) for c in cases}
    first_pdf = _kernel(bins, weights, u, eps)
    side = torch.cuda.Stream()
    for c in cases:
        for again in (_raymarch_bits(c), _raymarch_bits(c, side)):
            assert all(torch.equal(a, b) for a, b in zip(first[c[0]], again)), c[0]
    with torch.cuda.stream(side):
        assert torch.equal(_kernel(bins, weights, u, eps), first_pdf)
    torch.use_deterministic_algorithms(True)
    try:
        for c in cases:
            assert all(torch.equal(a, b) for a, b in zip(first[c[0]], _raymarch_bits(c))), c[0]
        assert torch.equal(_kernel(bins, weights, u, eps), first_pdf)
    finally:
        torch.use_deterministic_algorithms(False)


def test_one_node_strided_inputs_and_a_gradient_into_the_weights_alone():
    case = next(c for c in RAY_CASES if c[0].startswith("x-2x3x4"))
    d, f, g_out, g_w, eps = C.ray_inputs(case)
    dg = d.to(D).requires_grad_(True)
    fg = f.to(D).transpose(-1, -2).contiguous().transpose(-1, -2).requires_grad_(True)  # a strided view of the same values
    out, w = A.ea_raymarch(dg, fg, eps, case[4], return_weights=True)
    assert out.grad_fn.next_functions[0][0] is w.grad_fn.next_functions[0][0]  # both are views of ONE node's outputs
    want = C.run_ray(A.ea_raymarch, case, device=D)
    assert np.array_equal(out.detach().cpu().double().numpy()[..., :3], want["features"])
    # the weights alone: grad_out is absent, not zeros
    gd, gf = torch.autograd.grad((w * g_w.to(D)).sum(), (dg, fg))
    d64, f64 = d.double().requires_grad_(True), f.double().requires_grad_(True)
    _, w64 = implicit.ea_raymarch_torch(d64, f64, eps, case[4], True)
    (gd64,) = torch.autograd.grad((w64 * g_w.double()).sum(), d64)
    assert (gd.cpu().double() - gd64).abs().max() <= C.GATE_FACTOR * C.e_ref("grad_densities") * gd64.abs().max()
    assert not gf.any()


@pytest.fixture(scope="module")
def shim_report():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_implicit_case.py")], capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    print(json.dumps(rec))
    return rec


def test_the_unmodified_reference_runs_through_the_shim(shim_report):
    r = shim_report
    assert r["install_alone"]["gpu_bit_equal"] and r["install_alone"]["cpu_bit_equal"] and r["install_alone"]["gpu_equals_cpu"]
    assert r["patched"]["ea"] and r["patched"]["ao"]
    n = r["renderer"]
    assert n["fused_calls"] > 0 and n["fallback_calls"] == 0 and n["finite"]
    for q in ("images", "grad_params"):
        assert n[q + "_difference"] <= n[q + "_gate"], (q, n)
    assert r["cpu_call"] == {"fused": 0, "fallback": 2}
    assert r["warning_kept"] and r["restored"]
