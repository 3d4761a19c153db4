"""csrc/volume_sample.hip on the GPU: every case of tests/volume_sampler_case.py against the fixture's float64 truth with the atomic
and the ordered backward, the ordered backward's bits across runs and streams, strided and shared-grid volumes, the launch forms
(ray gradients alone, volume gradients alone, more rounds than workgroups), the lattice cases bit for bit, and the unmodified
VolumeRenderer through the shim (tests/shim_volume_sampler_case.py, in a process of its own)."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import volume_sampler_case as C  # noqa: E402

import pytorch3d_amd as A  # noqa: E402
from pytorch3d_amd import _C, _lib, volume_sampler  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = C.cases()
DEV = "cuda:0"


@contextlib.contextmanager
def deterministic(on=True):
    before = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(before[0], warn_only=before[1])


def fused(dens, feats, o, d, l, **modes):
    assert volume_sampler.kernel_path(dens, feats, o, d, l, modes.get("sample_mode", "bilinear"), modes.get("padding_mode", "zeros"))
    return A.sample_volumes(dens, feats, o, d, l, **modes)


def chunks(case):
    """(rays per wave round, chunks per ray) of the backward for the case's P, from the header's constants."""
    G = 1
    while G < _lib.VOLUME_SAMPLE_CHUNK and G < case.P:
        G *= 2
    return _lib.VOLUME_SAMPLE_CHUNK // G, -(-case.P // G)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_kernels_against_the_fixture_atomic_and_ordered(case):
    before = dict(_C.VOLUME_SAMPLE_CALLS)
    assert C.failures([case], fused, device=DEV) == []
    assert _C.VOLUME_SAMPLE_CALLS["atomic"] == before["atomic"] + 1 and _C.VOLUME_SAMPLE_CALLS["ordered"] == before["ordered"]
    with deterministic():
        assert C.failures([case], fused, device=DEV) == []
    assert _C.VOLUME_SAMPLE_CALLS["ordered"] == before["ordered"] + 1 and _C.VOLUME_SAMPLE_CALLS["atomic"] == before["atomic"] + 1


def test_the_cases_reach_every_backward_layout():
    layouts = {chunks(c) for c in CASES}
    assert {(32, 1), (16, 1), (1, 2), (1, 3), (1, 5)} <= layouts and (4, 1) in layouts  # P = 1, 2, 63 / 64, 65, 130, and 5
    assert {chunks(c)[1] for c in CASES if c.P in (65, 130)} == {3, 5}  # the carry across chunks
    assert any(c.R * c.N > chunks(c)[0] * 4 for c in CASES if c.R == 257)  # more than one workgroup


def test_ordered_backward_has_the_same_bits_on_every_run_and_stream():
    for cid in ("collide", "rays-shared-N3", next(c.id for c in CASES if c.P == 130 and c.mode == "bilinear")):
        case = C.case_by_id(cid)
        with deterministic():
            first = C.run(fused, case, device=DEV)
            second = C.run(fused, case, device=DEV)
            side = torch.cuda.Stream(device=DEV)
            side.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(side):
                third = C.run(fused, case, device=DEV)
            side.synchronize()
        for q in C.QUANTITIES:
            if first[q] is not None:
                assert np.array_equal(first[q], second[q]) and np.array_equal(first[q], third[q]), (cid, q)


def test_ray_gradients_are_the_same_bits_in_both_modes_and_runs():
    case = next(c for c in CASES if c.kind == "rays" and c.P == 65 and c.mode == "bilinear" and c.padding == "border")
    assert chunks(case)[1] == 3
    a = C.run(fused, case, device=DEV)
    b = C.run(fused, case, device=DEV)
    with deterministic():
        c = C.run(fused, case, device=DEV)
    for q in ("grad_origins", "grad_directions", "grad_lengths", "rays_densities"):
        assert np.array_equal(a[q], b[q]) and np.array_equal(a[q], c[q]), q  # shuffle trees, no atomic: nothing to reorder


def _run_partial(case, need_volumes, need_rays):
    dens, feats, o, d, l, g_d, g_f = (None if t is None else t.to(DEV) for t in C.inputs(case))
    for t in (dens, feats):
        if t is not None:
            t.requires_grad_(need_volumes)
    for t in (o, d, l):
        t.requires_grad_(need_rays)
    rd, rf = fused(dens, feats, o, d, l, sample_mode=case.mode, padding_mode=case.padding, align_corners=case.align)
    ((rd * g_d).sum() + ((rf * g_f).sum() if feats is not None else 0.0)).backward()
    return {"grad_densities": dens.grad, "grad_features": None if feats is None else feats.grad, "grad_origins": o.grad,
            "grad_directions": d.grad, "grad_lengths": l.grad}


@pytest.mark.parametrize("cid", ["collide", "rays-shared-N3", "world", "rays-R257"])
def test_no_ray_gradient_form_and_ray_gradients_alone(cid):
    case, fix = C.case_by_id(cid), C.fixture()
    with deterministic():
        full = _run_partial(case, True, True)
        volumes_only = _run_partial(case, True, False)
    for q in ("grad_densities", "grad_features"):
        assert torch.equal(full[q], volumes_only[q]), q
    assert volumes_only["grad_origins"] is None
    atomic_volumes_only = _run_partial(case, True, False)  # the kernel compiled without any read of the volumes
    rays_only = _run_partial(case, False, True)
    assert rays_only["grad_densities"] is None
    for q, got in list(atomic_volumes_only.items())[:2] + list(rays_only.items())[2:]:
        truth = fix[C.key(case.id, q)]
        assert float(np.abs(got.double().cpu().numpy() - truth).max()) <= C.GATE_FACTOR * C.e_ref(q) * float(np.abs(truth).max()), q
    for q in ("grad_origins", "grad_directions", "grad_lengths"):
        assert torch.equal(rays_only[q], full[q]), q


def test_strided_and_expanded_volumes_are_read_in_place():
    case = C.case_by_id("rays-shared-N3")
    dens, feats, o, d, l, g_d, g_f = (t.to(DEV) for t in C.inputs(case))
    fix = C.fixture()
    # a channel slice of a larger tensor, and an expand along the batch: what the fitting tutorial passes
    big = torch.randn((1, 2 + case.Cd + case.Cf, *case.grid), device=DEV)
    big[:, 1:1 + case.Cd], big[:, 1 + case.Cd:1 + case.Cd + case.Cf] = dens, feats
    big.requires_grad_(True)
    dens_view = big[:, 1:1 + case.Cd].expand(case.N, -1, -1, -1, -1)
    feats_view = big[:, 1 + case.Cd:1 + case.Cd + case.Cf].expand(case.N, -1, -1, -1, -1)
    assert dens_view.stride(0) == 0 and not dens_view.is_contiguous() and dens_view.data_ptr() != big.data_ptr()
    for strict in (False, True):
        big.grad = None
        with deterministic(strict):
            rd, rf = fused(dens_view, feats_view, o, d, l, sample_mode=case.mode, padding_mode=case.padding, align_corners=case.align)
            ((rd * g_d).sum() + (rf * g_f).sum()).backward()
        got = {"rays_densities": rd, "rays_features": rf, "grad_densities": big.grad[:, 1:1 + case.Cd],
               "grad_features": big.grad[:, 1 + case.Cd:1 + case.Cd + case.Cf]}
        for q, t in got.items():
            truth = fix[C.key(case.id, q)]
            assert t.shape == truth.shape, q
            assert float(np.abs(t.detach().double().cpu().numpy() - truth).max()) <= C.GATE_FACTOR * C.e_ref(q) * float(np.abs(truth).max()), (q, strict)
        assert not big.grad[:, 0].any() and not big.grad[:, -1].any()  # the channels around the slice are untouched
    # a batch that is NOT shared, with permuted spatial strides (x is not the fastest axis)
    case = next(c for c in CASES if c.kind == "rays" and c.N == 2 and c.Cf is not None and c.mode == "bilinear")

    def fn(dens_, feats_, *rest, **modes):
        views = [t.permute(0, 1, 4, 3, 2).contiguous().permute(0, 1, 4, 3, 2) for t in (dens_, feats_)]
        assert all(v.stride(4) != 1 and v.shape == t.shape for v, t in zip(views, (dens_, feats_)))
        return fused(*views, *rest, **modes)

    assert C.failures([case], fn, device=DEV) == []
    with deterministic():
        assert C.failures([case], fn, device=DEV) == []


def test_nan_under_border_is_what_minus_inf_is():
    with deterministic():  # (the ordered backward: two runs of the atomics need not agree in the last bit)
        assert C.nan_equals_minus_inf_under_border(fused, device=DEV) == []


def test_lattice_cases_bit_equal_to_grid_sample_and_to_the_chain_on_the_gpu():
    fix = C.fixture()
    for case in (c for c in CASES if c.kind == "lattice"):
        dens, feats, o, d, l, _, _ = (t.to(DEV) for t in C.inputs(case))
        modes = dict(sample_mode=case.mode, padding_mode=case.padding, align_corners=case.align)
        with torch.no_grad():
            rd, rf = fused(dens, feats, o, d, l, **modes)
            cd, cf = volume_sampler.sample_volumes_torch(dens, feats, o, d, l, **modes)
        assert torch.equal(rd, cd) and torch.equal(rf, cf), case.id
        assert C.same_bits(rd.cpu().numpy(), fix[C.key(case.id, "f32_densities")]) and C.same_bits(rf.cpu().numpy(), fix[C.key(case.id, "f32_features")])
        got = C.run(fused, case, device=DEV)  # exact arithmetic: the gradients equal the float64 truth too
        for q in C.QUANTITIES:
            assert np.array_equal(got[q], fix[C.key(case.id, q)]), (case.id, q)


def test_points_form_without_lengths():
    case = C.case_by_id("edges-bil-zer-ac")
    dens, feats, o, d, l, _, _ = (t.to(DEV) for t in C.inputs(case))
    rd, rf = _C.volume_sample_forward(dens, feats, o, None, None, _lib.VOLUME_SAMPLE_CORNERS)
    rd2, rf2 = fused(dens, feats, o, d, l, align_corners=True)  # direction 0, length 1: the same points
    assert rd.shape == (1, case.R, 1, 1) and torch.equal(rd, rd2) and torch.equal(rf, rf2)
    grads = _C.volume_sample_backward(torch.ones_like(rd), torch.ones_like(rf), dens, feats, o, None, None, _lib.VOLUME_SAMPLE_CORNERS,
                                      (True, True), (True, True, True))
    o2 = o.clone().requires_grad_(True)
    dens2, feats2 = dens.clone().requires_grad_(True), feats.clone().requires_grad_(True)
    rd3, rf3 = fused(dens2, feats2, o2, d, l, align_corners=True)
    (rd3.sum() + rf3.sum()).backward()
    assert grads[3] is None and grads[4] is None and torch.equal(grads[2], o2.grad)
    assert torch.allclose(grads[0], dens2.grad, rtol=1e-5, atol=1e-6) and torch.allclose(grads[1], feats2.grad, rtol=1e-5, atol=1e-6)


def test_more_points_and_rounds_than_one_pass_of_the_launch():
    """One launch beyond the grid-stride loops' first pass, on a small grid: the forward walks points, the backward rounds of 8 rays.
    (16^3 voxels and not fewer: the float64 chain that makes the truth scatters with compare-and-swap loops, which crawl on a few
    dozen addresses.)"""
    N, R, P = 1, 540_000, 4
    lanes = _lib.VOLUME_SAMPLE_MAX_GROUPS * 256
    rays_per_round = _lib.VOLUME_SAMPLE_CHUNK // 4
    assert N * R * P > lanes and -(-N * R // rays_per_round) > _lib.VOLUME_SAMPLE_MAX_GROUPS * 4
    g = torch.Generator().manual_seed(C.SEED + 77)
    S = 16
    dens = torch.rand((1, 1, S, S, S), generator=g).to(DEV).requires_grad_(True)
    o = (1.6 * torch.rand((N, R, 3), generator=g) - 0.8).to(DEV).requires_grad_(True)
    d = (0.4 * torch.rand((N, R, 3), generator=g) - 0.2).to(DEV).requires_grad_(True)
    l = torch.rand((N, R, P), generator=g).to(DEV).requires_grad_(True)
    g_d = torch.randn((N, R, P, 1), generator=g).to(DEV)
    rd, rf = fused(dens, None, o, d, l)
    assert rf.shape == (N, R, P, 0)
    got = torch.autograd.grad((rd * g_d).sum(), (dens, o, d, l))
    leaves = [t.detach().double().requires_grad_(True) for t in (dens, o, d, l)]
    td, _ = volume_sampler.sample_volumes_torch(leaves[0], None, *leaves[1:])
    truth = torch.autograd.grad((td * g_d.double()).sum(), leaves)
    # points within CLEARANCE of a lattice plane floor differently in float32 and float64: their rays are left out of the ray gradients
    pts = leaves[1][:, :, None] + leaves[3][..., None] * leaves[2][:, :, None]
    idx = (pts + 1) / 2 * (S - 1)
    clear = ((idx - idx.round()).abs() >= C.CLEARANCE).all(-1)  # (N, R, P)
    ray_clear = clear.all(-1)
    assert float(ray_clear.float().mean()) > 0.99

    def within(a, b, q, mask=None):
        a, b = a.detach().double(), b.detach()
        if mask is not None:
            a, b = a[mask], b[mask]
        return float((a - b).abs().max()) <= C.GATE_FACTOR * C.e_ref(q) * float(b.abs().max())

    assert within(rd, td, "rays_densities")
    # 17 million float atomics into 4096 voxels: the rounding of a float32 sum grows with its number of terms, which E_ref, measured on
    # sums of a few terms, does not hold; a voxel's terms have random signs, so the gate scales by the square root of the mean number
    terms = 8 * N * R * P / S ** 3
    assert terms > 1000
    assert float((got[0].double() - truth[0]).abs().max()) <= C.GATE_FACTOR * C.e_ref("grad_densities") * float(truth[0].abs().max()) * terms ** 0.5
    assert within(got[1], truth[1], "grad_origins", ray_clear) and within(got[2], truth[2], "grad_directions", ray_clear)
    assert within(got[3], truth[3], "grad_lengths", clear)
    # the last point and the last ray were reached
    assert torch.equal(rd[0, -1], _C.volume_sample_forward(dens.detach(), None, o.detach()[:, -1:], d.detach()[:, -1:], l.detach()[:, -1:], 4)[0][0, 0])
    assert bool(got[1][0, -1].any()) or not bool(truth[1][0, -1].any())


def test_ordered_form_refuses_sizes_beyond_its_keys_and_the_node_falls_back():
    dens = torch.zeros((1, 1, 2, 2, 2), device=DEV)
    o = torch.zeros((1, 1, 3), device=DEV)
    assert not _C.volume_sample_fits(1, 2048, 2048, 2048, 1, 1, 1)
    with pytest.raises(RuntimeError):  # the entry itself
        _lib.call("p3di_volume_sample_keys", "keys", torch.device(DEV), 2048, 2048, 2048, 0, o, o, o, 1, 1, 1, 4, torch.zeros(8, dtype=torch.int32, device=DEV))
    real = _C.volume_sample_fits
    _C.volume_sample_fits = lambda *a: False
    try:
        case = C.case_by_id("rays-shared-N3")
        with deterministic(), pytest.raises(RuntimeError, match="deterministic"):
            C.run(fused, case, device=DEV)  # NotImplementedError inside the node: the chain's own backward, which torch refuses here
    finally:
        _C.volume_sample_fits = real


def test_unmodified_volume_renderer_through_the_shim():
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shim_volume_sampler_case.py")
    res = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in out:
        pytest.skip(out["skipped"])
    print(json.dumps(out))
    assert out["patched"] and out["not_patched_by_plain_install"]
    r = out["renderer"]
    assert r["fused_calls"] == 1 and r["fallback_calls"] == 0 and r["fused_calls_when_restored"] == 0 and r["finite"], r
    assert r["images_difference"] <= r["images_gate"] and r["grad_volumes_difference"] <= r["grad_volumes_gate"], r
    assert r["grad_volumes_max"] > 0 and r["grad_pose_difference"] <= r["grad_pose_gate"] and r["grad_pose_max"] > 0, r
    assert out["deterministic"]["fused_calls"] == 1 and out["deterministic"]["ordered_calls"] == 1 and out["deterministic"]["same_bits"], out["deterministic"]
    assert out["cpu_call"] == {"fused": 0, "fallback": 1} and out["reflection_call"] == {"fused": 0, "fallback": 1}
    assert out["restored"]
