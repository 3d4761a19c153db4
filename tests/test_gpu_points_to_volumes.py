"""points_to_volumes on the GPU (csrc/points_to_volumes.hip) against the reference's recorded results
(tests/golden/points_to_volumes_ref.npz): the atomic forward, the ordered forward of the strict deterministic flag, and the backward.

Lattice cases must equal the reference's bits in both forward forms; random cases must lie, like the reference's own result, within
(n + 2) 2^-24 sum |t_i| of the float64 restatement of the same n terms (tests/points_to_volumes_case.py).  The launches do not cap
their grids (one lane per sample, no grid-stride loop), so there is no second round of a loop; the second rounds that exist are
ordered_sum.h's -- pass2_kernel's second block (more than 256 waves of sorted samples) and a segment that runs over many waves --
and the cases here stop at 65 waves: tests/test_gpu_cloud_kernel_edges.py (section D, "long": 938 waves) reaches them.
"""
import contextlib
import importlib
import json
import os
import subprocess
import sys

import pytest
import torch

import points_to_volumes_case as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = C.all_cases()


def _dev():
    return torch.device("cuda:0")


def _mod():
    return importlib.import_module("pytorch3d_amd.points_to_volumes")


@contextlib.contextmanager
def _flag(on, warn_only=False):
    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(on, warn_only=warn_only)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])


def _calls():
    from pytorch3d_amd import _C

    return dict(_C.POINTS_TO_VOLUMES_CALLS)


@pytest.mark.parametrize("form", ["atomic", "ordered"])
@pytest.mark.parametrize("case", CASES, ids=C.case_id)
def test_kernels_match_the_reference(case, form):
    m = _mod()
    inp = C.inputs(case)
    before = _calls()
    with _flag(form == "ordered"):
        got = C.run_operators(case, inp, _dev(), m.points_to_volumes_forward_op, m.points_to_volumes_backward_op)
    after = _calls()
    assert after[form] == before[form] + 1 and sum(after.values()) == sum(before.values()) + 1  # the form that was asked for ran
    C.judge(case, inp, got)


def test_strided_volume_view_is_updated_in_place():
    m = _mod()
    case = ("lattice", "mixed_grids", "trilinear", False)
    inp = C.inputs(case)
    z = C.fixture()
    d = _dev()
    N = inp["points_3d"].shape[0]
    dims = inp["densities"].shape[2:]
    for form in ("atomic", "ordered"):
        big_d = torch.full((N, 2, dims[0] + 1, dims[1] + 2, dims[2] * 2), -7.0, device=d)
        big_f = torch.full((N, 3, dims[0] + 1, dims[1] + 2, dims[2] * 2), -7.0, device=d)
        view_d, view_f = big_d[:, 1:2, 1:, 1:-1, ::2], big_f[:, :, 1:, 1:-1, 1::2]
        assert not view_d.is_contiguous() and not view_f.is_contiguous()
        view_d.copy_(inp["densities"])
        view_f.copy_(inp["volume_features"])
        before_d, before_f = big_d.clone(), big_f.clone()
        with _flag(form == "ordered"):
            m.points_to_volumes_forward_op(inp["points_3d"].to(d), inp["features"].to(d), view_d, view_f, inp["grid_sizes"].to(d),
                                           inp["mask"].to(d), 1.0, False, True)
        assert torch.equal(view_d.cpu(), z[C.key(case, "densities")]) and torch.equal(view_f.cpu(), z[C.key(case, "features")]), form
        view_d.copy_(inp["densities"])
        view_f.copy_(inp["volume_features"])
        assert torch.equal(big_d, before_d) and torch.equal(big_f, before_f), form  # nothing outside the view was touched


def test_backward_reads_an_expanded_gradient_and_a_strided_buffer():
    """sum().backward() hands over gradients of stride 0; the gradient buffers of the operator may be strided."""
    m = _mod()
    case = ("lattice", "mixed_grids", "trilinear", True)
    inp = C.inputs(case)
    d = _dev()
    N, P, Cf = inp["features"].shape
    dims = tuple(inp["densities"].shape[2:])
    ones_d, ones_f = torch.ones((), device=d).expand(N, 1, *dims), torch.ones((), device=d).expand(N, Cf, *dims)
    gp_big, gf_big = torch.zeros(N, P, 6, device=d), torch.zeros(N, P, 2 * Cf, device=d)
    args = (inp["points_3d"].to(d), inp["features"].to(d), inp["grid_sizes"].to(d), inp["mask"].to(d), 1.0, True, True)
    m.points_to_volumes_backward_op(*args, ones_d, ones_f, gp_big[:, :, ::2], gf_big[:, :, 1::2])
    gp, gf = torch.zeros(N, P, 3), torch.zeros(N, P, Cf)
    m.points_to_volumes_backward_op(*(a.cpu() if torch.is_tensor(a) else a for a in args), ones_d.cpu(), ones_f.cpu(), gp, gf)
    assert torch.equal(gp_big[:, :, ::2].cpu(), gp) and torch.equal(gf_big[:, :, 1::2].cpu(), gf)  # lattice: exact
    assert not gp_big[:, :, 1::2].any() and not gf_big[:, :, ::2].any() and gp.any() and gf.any()


@pytest.mark.parametrize("mode", ["trilinear", "nearest"])
def test_public_functions_on_stand_in_structures(mode):
    import pytorch3d_amd as p3d

    case = ("lattice", "mixed_grids", mode, True)
    inp = C.inputs(case)
    z = C.fixture()
    clouds, vols = C.stand_ins(inp, True, _dev())
    out = p3d.add_pointclouds_to_volumes(clouds, vols, mode=mode, rescale_features=False)
    assert out.densities().is_cuda
    assert torch.equal(out.densities().cpu(), z[C.key(case, "densities")]) and torch.equal(out.features().cpu(), z[C.key(case, "features")])
    # the tensor function as one autograd node, rescaled, volume_features=None, a mask of stride 0
    d = _dev()
    pts, feats = inp["points_3d"].to(d).requires_grad_(True), inp["features"].to(d).requires_grad_(True)
    dens0 = inp["densities"].to(d).requires_grad_(True)
    feat, dens = p3d.add_points_features_to_volume_densities_features(pts, feats, dens0 * 1, None, mode=mode, min_weight=0.75)
    cpu_feat, cpu_dens = p3d.add_points_features_to_volume_densities_features(inp["points_3d"], inp["features"], inp["densities"].clone(),
                                                                              None, mode=mode, min_weight=0.75)
    # lattice sums are exact; the one division may round differently on the two devices: one unit in the last place each
    assert torch.equal(dens.detach().cpu(), cpu_dens) and torch.allclose(feat.detach().cpu(), cpu_feat, rtol=2.0 ** -22, atol=0)
    (feat.sum() + dens.sum()).backward()
    assert torch.isfinite(feats.grad).all() and feats.grad.abs().sum() > 0 and dens0.grad is not None
    assert (pts.grad is not None and pts.grad.abs().sum() > 0) if mode == "trilinear" else pts.grad is None


def test_strict_flag_gives_the_same_bits_on_every_run_and_stream():
    """The contended 2 x 2 x 2 case with continuous values: 300 x 8 samples on 8 voxels, every ordered segment spans several waves."""
    m = _mod()
    d = _dev()
    gen = torch.Generator().manual_seed(11)
    N, P, Cf = 1, 300, 5
    pts = (torch.rand(N, P, 3, generator=gen) * 2.2 - 1.1).to(d)
    feats = torch.randn(N, P, Cf, generator=gen).to(d)
    grid = torch.tensor([[2, 2, 2]], device=d)
    mask = torch.ones(N, P, device=d)
    dens0, feat0 = torch.rand(N, 1, 2, 2, 2, generator=gen).to(d), torch.randn(N, Cf, 2, 2, 2, generator=gen).to(d)

    def run():
        dens, feat = dens0.clone(), feat0.clone()
        m.points_to_volumes_forward_op(pts, feats, dens, feat, grid, mask, 0.5, True, True)
        return dens, feat

    before = _calls()
    with _flag(True):
        a = run()
        b = run()
        side = torch.cuda.Stream(device=d)
        side.wait_stream(torch.cuda.current_stream(d))
        with torch.cuda.stream(side):
            c = run()
        torch.cuda.current_stream(d).wait_stream(side)
    after = _calls()
    assert after["ordered"] == before["ordered"] + 3 and after["atomic"] == before["atomic"]
    assert all(torch.equal(a[i], b[i]) and torch.equal(a[i], c[i]) for i in range(2))
    with _flag(True, warn_only=True):
        w = run()
    assert _calls()["atomic"] == after["atomic"] + 1 and _calls()["ordered"] == after["ordered"]  # warn-only keeps the atomics
    assert torch.isfinite(w[0]).all() and torch.isfinite(w[1]).all()


def test_strict_flag_refuses_a_key_beyond_int32():
    """N * D * H * W beyond an int32: the ordered form raises instead of silently taking the atomics.  The volumes are views of
    stride 0 -- nothing of that size is allocated, and nothing is launched."""
    m = _mod()
    d = _dev()
    N, side = 2, 1100  # 2 * 1100^3 > 2^31
    dens = torch.zeros((), device=d).expand(N, 1, side, side, side)
    feat = torch.zeros((), device=d).expand(N, 1, side, side, side)
    grid = torch.tensor([[1, 1, 1]] * N, device=d)
    args = (torch.zeros(N, 4, 3, device=d), torch.zeros(N, 4, 1, device=d), dens, feat, grid, torch.ones(N, 4, device=d), 1.0, True, True)
    before = _calls()
    with _flag(True):
        with pytest.raises(RuntimeError, match="int32"):
            m.points_to_volumes_forward_op(*args)
    assert _calls() == before


def test_shim_operators_on_gpu():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_points_to_volumes_case.py"), "cuda"], capture_output=True,
                         text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    print(json.dumps(rec))
    assert rec["operators_exist"] == {"ctypes": True, "pybind": True} and rec["operators_match_fixture"]
