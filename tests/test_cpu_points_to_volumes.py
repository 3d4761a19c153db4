"""points_to_volumes on the CPU: the package's torch formulation of the compiled operator's contract against the reference's
recorded results (tests/golden/points_to_volumes_ref.npz), the autograd node, the public functions and the shim.

Lattice cases must equal the reference's bits; random cases must lie, like the reference's own result, within
(n + 2) 2^-24 sum |t_i| of the float64 restatement of the same n terms (tests/points_to_volumes_case.py)."""
import importlib
import json
import os
import subprocess
import sys

import pytest
import torch

import points_to_volumes_case as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = C.all_cases()


def _mod():
    return importlib.import_module("pytorch3d_amd.points_to_volumes")


@pytest.mark.parametrize("case", CASES, ids=C.case_id)
def test_formulation_matches_the_reference(case):
    m = _mod()
    inp = C.inputs(case)
    got = C.run_operators(case, inp, "cpu", m.points_to_volumes_forward_op, m.points_to_volumes_backward_op)
    C.judge(case, inp, got)


def test_compiled_contract_is_not_the_python_twin():
    """The two quirks, on the formulation: half away from zero (grid 5, aligned, locations 0.5, 1.5, 2.5 -> voxels 1, 2, 3) and the
    extrapolation below 0 (p = -0.9, grid 4, unaligned: location -0.3 -> +1.3 on voxel 0, -0.3 on voxel 1)."""
    import pytorch3d_amd as p3d

    pts = torch.tensor([[[-0.75, -1.0, -1.0], [-0.25, -1.0, -1.0], [0.25, -1.0, -1.0]]])
    dens = torch.zeros(1, 1, 5, 5, 5)
    _, d = p3d.add_points_features_to_volume_densities_features(pts, torch.ones(1, 3, 1), dens, None, mode="nearest", rescale_features=False)
    assert d[0, 0, 0, 0].tolist() == [0.0, 1.0, 1.0, 1.0, 0.0]
    dens = torch.zeros(1, 1, 1, 1, 4)
    pts = torch.tensor([[[-0.9, 0.0, 0.0]]])
    _, d = p3d.add_points_features_to_volume_densities_features(pts, torch.ones(1, 1, 1), dens, None, align_corners=False,
                                                                rescale_features=False)
    want = torch.tensor([1.0 - (-0.3), -0.3, 0.0, 0.0])
    assert torch.allclose(d[0, 0, 0, 0], want, atol=1e-6) and d[0, 0, 0, 0, 0] > 1.0 and d[0, 0, 0, 0, 1] < 0.0
    # exactly -0.5 rounds to -1 and is dropped (nearest, unaligned: p = -1)
    dens = torch.zeros(1, 1, 1, 1, 4)
    pts = torch.tensor([[[-1.0, 0.0, 0.0]]])
    _, d = p3d.add_points_features_to_volume_densities_features(pts, torch.ones(1, 1, 1), dens, None, mode="nearest", align_corners=False,
                                                                rescale_features=False)
    assert not d.any()


def test_bad_coordinates_are_skipped():
    import pytorch3d_amd as p3d

    pts = torch.tensor([[[float("nan"), 0, 0], [float("inf"), 0, 0], [3e38, 0, 0], [0.0, 0.0, 0.0]]])
    for mode in ("trilinear", "nearest"):
        dens = torch.zeros(1, 1, 3, 3, 3)
        f, d = p3d.add_points_features_to_volume_densities_features(pts, torch.ones(1, 4, 2), dens, None, mode=mode, rescale_features=False)
        assert torch.isfinite(d).all() and float(d.sum()) == 1.0 and float(d[0, 0, 1, 1, 1]) == 1.0 and float(f.sum()) == 2.0


def test_argument_errors():
    import pytorch3d_amd as p3d

    fn = p3d.add_points_features_to_volume_densities_features
    pts, feats, dens = torch.zeros(2, 5, 3), torch.zeros(2, 5, 4), torch.zeros(2, 1, 3, 3, 3)
    with pytest.raises(ValueError, match="No such interpolation mode"):
        fn(pts, feats, dens, None, mode="cubic")
    with pytest.raises(ValueError, match="one-dimensional densities"):
        fn(pts, feats, torch.zeros(2, 2, 3, 3, 3), None)
    with pytest.raises(ValueError, match="points_3d must be 3D"):
        fn(torch.zeros(2, 5, 2), feats, dens, None)
    with pytest.raises(ValueError, match="Bad points_features shape"):
        fn(pts, torch.zeros(2, 6, 4), dens, None)
    with pytest.raises(ValueError, match="Bad volume_densities shape"):
        fn(pts, feats, torch.zeros(3, 1, 3, 3, 3), None)
    with pytest.raises(ValueError, match="Bad volume_features shape"):
        fn(pts, feats, dens, torch.zeros(2, 5, 3, 3, 3))
    with pytest.raises(ValueError, match="Bad grid_sizes.shape"):
        fn(pts, feats, dens, None, grid_sizes=torch.ones(2, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="Bad mask shape"):
        fn(pts, feats, dens, None, mask=torch.ones(2, 4))
    with pytest.raises(ValueError, match="points_3d must be float32"):
        fn(pts.double(), feats, dens, None)
    with pytest.raises(ValueError, match="points_features must be float32"):
        fn(pts, feats.double(), dens, None)
    with pytest.raises(ValueError, match="volume_densities must be float32"):
        fn(pts, feats, dens.double(), None)
    with pytest.raises(ValueError, match="mask must be float32"):
        fn(pts, feats, dens, None, mask=torch.ones(2, 5, dtype=torch.bool))
    with pytest.raises(ValueError, match="grid_sizes must be int64"):
        fn(pts, feats, dens, None, grid_sizes=torch.ones(2, 3, dtype=torch.int32))

    class Clouds:
        def __len__(self):
            return 3

        def features_padded(self):
            return None

        def points_padded(self):
            return torch.zeros(3, 4, 3)

    class Vols:
        def __init__(self, n):
            self.n = n

        def __len__(self):
            return self.n

    with pytest.raises(ValueError, match="same batch size"):
        p3d.add_pointclouds_to_volumes(Clouds(), Vols(2))
    with pytest.raises(ValueError, match="'features' defined"):
        p3d.add_pointclouds_to_volumes(Clouds(), Vols(3))


@pytest.mark.parametrize("case", [c for c in CASES if c[1] in ("mixed_grids", "ragged")], ids=C.case_id)
def test_autograd_node_gives_the_four_gradients(case):
    """One node, the volumes marked dirty: gradients for the points (trilinear), the features and BOTH initial volumes (the upstream
    gradients themselves)."""
    import pytorch3d_amd as p3d

    inp = C.inputs(case)
    mode, align = case[2], case[3]
    pts, feats = inp["points_3d"].clone().requires_grad_(True), inp["features"].clone().requires_grad_(True)
    dens0, feat0 = inp["densities"].clone().requires_grad_(True), inp["volume_features"].clone().requires_grad_(True)
    dens_in, feat_in = dens0 * 1, feat0 * 1  # (a leaf that requires grad cannot be modified in place)
    feat, dens = p3d.add_points_features_to_volume_densities_features(pts, feats, dens_in, feat_in, mode=mode, mask=inp["mask"],
                                                                      grid_sizes=inp["grid_sizes"], rescale_features=False,
                                                                      align_corners=align)
    assert dens is dens_in and feat is feat_in  # modified in place and returned
    assert inp["point_weight"] == 1.0  # (the public function adds with weight 1: the fixture of these cases was recorded so)
    torch.autograd.backward((dens, feat), (inp["grad_densities"], inp["grad_features"]))
    got = {"densities": dens.detach(), "features": feat.detach(), "grad_points_features": feats.grad}
    if mode == "trilinear":
        got["grad_points_3d"] = pts.grad
    else:
        assert pts.grad is None
    C.judge(case, inp, got)
    assert torch.equal(dens0.grad, inp["grad_densities"]) and torch.equal(feat0.grad, inp["grad_features"])


@pytest.mark.parametrize("mode", ["trilinear", "nearest"])
def test_rescale_features(mode):
    import pytorch3d_amd as p3d

    case = ("lattice", "mixed_grids", mode, True)
    inp = C.inputs(case)
    z = C.fixture()
    args = dict(mode=mode, mask=inp["mask"], grid_sizes=inp["grid_sizes"], align_corners=True)
    feat, dens = p3d.add_points_features_to_volume_densities_features(inp["points_3d"], inp["features"], inp["densities"].clone(),
                                                                      inp["volume_features"].clone(), min_weight=0.75, **args)
    want_d, want_f = z[C.key(case, "densities")], z[C.key(case, "features")]
    assert torch.equal(dens, want_d)
    assert torch.equal(feat, want_f / want_d.clamp(0.75 if mode == "trilinear" else 1.0))
    assert not torch.equal(feat, want_f)


def test_volume_features_none_and_default_grid():
    import pytorch3d_amd as p3d

    case = ("lattice", "contended", "trilinear", True)
    inp = C.inputs(case)
    dens = torch.zeros_like(inp["densities"])
    feat, dens_out = p3d.add_points_features_to_volume_densities_features(inp["points_3d"], inp["features"], dens, None, mask=inp["mask"],
                                                                          rescale_features=False)
    z = C.fixture()
    # the fixture started from non-zero volumes; lattice sums are exact, so the initial content subtracts out exactly.  The public
    # function adds with weight 1 and the case was recorded with 0.5: exact factor 2
    assert dens_out is dens and feat.shape == inp["volume_features"].shape
    assert torch.equal(dens_out, (z[C.key(case, "densities")] - inp["densities"]) * 2)
    assert torch.equal(feat, (z[C.key(case, "features")] - inp["volume_features"]) * 2)


def test_stride0_mask_and_strided_volume_view():
    m = _mod()
    case = ("lattice", "mixed_grids", "trilinear", False)
    inp = C.inputs(case)
    z = C.fixture()
    N, P, _ = inp["points_3d"].shape
    ones = inp["points_3d"].new_ones(1).expand(N, P)
    assert ones.stride() == (0, 0)
    plain = dict(inp, mask=torch.ones(N, P))
    a = C.run_operators(case, dict(inp, mask=None), "cpu", m.points_to_volumes_forward_op, m.points_to_volumes_backward_op)
    b = C.run_operators(case, plain, "cpu", m.points_to_volumes_forward_op, m.points_to_volumes_backward_op)
    assert all(torch.equal(a[k], b[k]) for k in a)
    # a view into a larger, padded buffer is updated in place; what lies outside the view is left alone
    dims = inp["densities"].shape[2:]
    big_d = torch.full((N, 2, dims[0] + 1, dims[1] + 2, dims[2] * 2), -7.0)
    big_f = torch.full((N, 3, dims[0] + 1, dims[1] + 2, dims[2] * 2), -7.0)
    view_d, view_f = big_d[:, 1:2, 1:, 1:-1, ::2], big_f[:, :, 1:, 1:-1, 1::2]
    view_d.copy_(inp["densities"])
    view_f.copy_(inp["volume_features"])
    before_d, before_f = big_d.clone(), big_f.clone()
    m.points_to_volumes_forward_op(inp["points_3d"], inp["features"], view_d, view_f, inp["grid_sizes"], inp["mask"], 1.0, False, True)
    assert torch.equal(view_d, z[C.key(case, "densities")]) and torch.equal(view_f, z[C.key(case, "features")])
    view_d.copy_(inp["densities"])
    view_f.copy_(inp["volume_features"])
    assert torch.equal(big_d, before_d) and torch.equal(big_f, before_f)


def test_public_function_on_stand_in_structures():
    import pytorch3d_amd as p3d

    case = ("lattice", "mixed_grids", "nearest", True)
    inp = C.inputs(case)
    z = C.fixture()
    clouds, vols = C.stand_ins(inp, align_corners=True)
    out = p3d.add_pointclouds_to_volumes(clouds, vols, mode="nearest", rescale_features=False)
    assert torch.equal(out.densities(), z[C.key(case, "densities")]) and torch.equal(out.features(), z[C.key(case, "features")])


def test_reference_functions_through_the_shim_on_cpu():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    if not os.path.isdir(os.path.join(stage, "pytorch3d", "ops")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_points_to_volumes_case.py"), "cpu"], capture_output=True,
                         text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    print(json.dumps(rec))
    assert rec["operators_exist"] == {"ctypes": True, "pybind": True} and rec["operators_match_fixture"]
    assert rec["unpatched_is_the_reference"] and rec["plain_reference_matches_fixture"] and rec["calls_before_patch"] == 0
    assert rec["patched_everywhere"] and rec["patched_matches_fixture"] and rec["python_twin_still_the_reference"] and rec["restored"]
    assert all(v == 0 for v in rec["fused_calls"].values()) and all(v >= 1 for v in rec["fallback_calls"].values())
