"""sample_farthest_points / ball_query / masked_gather without a GPU: the package's torch formulation against the reference's recorded
results (tests/golden/fps_ball_ref.npz, made by tests/golden/make_golden_fps_ball.py from the reference's own naive code), the
validation, the shim module and the C ABI's declarations.

Tolerances.  The fixture's random cases keep a relative gap of >= 1e-5 -- more than 8 x the (D + 2) 2^-24 rounding of one float32
distance -- between the two largest minimum distances of every sampling step and between every pair's distance and radius^2, so idx
must match bit for bit and dists within 2e-6 relative.  The lattice cases are exact in float32.  Gradients: a row of grad_p1 sums at
most K terms and a row of grad_p2 at most P1 K, float32 against float64: 1e-5 relative to the largest entry.
"""
import importlib
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import fps_ball_case as C

import pytorch3d_amd as p3d
from pytorch3d_amd import _C, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (importlib: the package re-exports the functions of these names over the sub-modules)
fps_mod = importlib.import_module("pytorch3d_amd.sample_farthest_points")
ball_mod = importlib.import_module("pytorch3d_amd.ball_query")


def _ball_cases():
    out = [(name, K) for name, *_r, Ks, _radius in C.BALL_RANDOM for K in Ks]
    return out + [("lattice", C.BALL_LATTICE_K)]


def _ball_case(name):
    if name == "lattice":
        return None, None, C.BALL_LATTICE_RADIUS
    _, _, _, _, _, l1, l2, _, radius = next(c for c in C.BALL_RANDOM if c[0] == name)
    return C.lengths_tensor(l1), C.lengths_tensor(l2), radius


@pytest.mark.parametrize("name", [c[0] for c in C.FPS_RANDOM] + list(C.FPS_LATTICE))
def test_fps_formulation_matches_the_reference(name):
    z = C.fixture()
    points = z["fps/%s/points" % name]
    if name in C.FPS_LATTICE:
        lengths, K = None, C.FPS_LATTICE_K[name]
    else:
        _, _, _, _, lengths, K = next(c for c in C.FPS_RANDOM if c[0] == name)
    assert not fps_mod.kernel_path(points)
    sel, idx = p3d.sample_farthest_points(points, C.lengths_tensor(lengths), C.k_arg(K))
    want = z["fps/%s/idx" % name]
    assert idx.dtype == torch.int64 and sel.dtype == torch.float32
    assert torch.equal(idx, want)
    assert torch.equal(sel, z["fps/%s/sel" % name]) and torch.equal(sel, p3d.masked_gather(points, idx))
    assert not sel[idx < 0].any()  # padding: exactly -1 / 0


def test_fps_lattice_cases_tie_and_repeat_index_zero():
    z = C.fixture()
    assert z["fps/same/idx"].tolist() == [[0] * 6]
    doubled = z["fps/grid_doubled/idx"][0]
    assert doubled[:36].tolist() == sorted(set(doubled[:36].tolist()), key=doubled[:36].tolist().index)  # 36 distinct places first
    assert (doubled[:36] % 2 == 0).all()  # of two coinciding points the lower index
    assert not doubled[36:].any()  # then every minimum is 0: index 0 again and again
    # the grid: the replay in float64 (exact) finds the maximum more than once at 23 of the 29 steps, and the first one is recorded
    pts, idx = z["fps/grid/points"][0].double(), z["fps/grid/idx"][0]
    m = torch.full((pts.shape[0],), float("inf"), dtype=torch.float64)
    tied = 0
    for s in range(1, idx.shape[0]):
        m = torch.minimum(m, ((pts[idx[s - 1]] - pts) ** 2).sum(1))
        tied += int((m == m.max()).sum()) >= 2
        assert int(torch.nonzero(m == m.max())[0]) == int(idx[s])
    assert tied == 23


@pytest.mark.parametrize("name,K", _ball_cases())
def test_ball_formulation_matches_the_reference(name, K):
    z = C.fixture()
    l1, l2, radius = _ball_case(name)
    p1, p2 = z["ball/%s/p1" % name], z["ball/%s/p2" % name]
    assert not ball_mod.kernel_path(p1, p2, K)
    got = p3d.ball_query(p1, p2, l1, l2, K=K, radius=radius)
    want_i, want_d = z["ball/%s/idx/%d" % (name, K)], z["ball/%s/dists/%d" % (name, K)]
    assert got.idx.dtype == torch.int64 and got.dists.dtype == torch.float32
    assert torch.equal(got.idx, want_i)
    assert float(((got.dists - want_d).abs() - 2e-6 * want_d.abs()).max()) <= 0.0
    pad = want_i < 0
    assert (got.idx[pad] == -1).all() and not got.dists[pad].any() and not got.knn[pad].any()
    assert torch.equal(got.knn, p3d.masked_gather(p2, got.idx))
    assert p3d.ball_query(p1, p2, l1, l2, K=K, radius=radius, return_nn=False).knn is None
    flagged = p3d.ball_query(p1, p2, l1, l2, K=K, radius=radius, skip_points_outside_cube=True)
    assert torch.equal(flagged.idx, got.idx) and torch.equal(flagged.dists, got.dists)


def test_lattice_points_at_distance_exactly_radius_are_no_hits():
    z = C.fixture()
    p1, p2 = z["ball/lattice/p1"], z["ball/lattice/p2"]
    d = ((p1[0, :, None] - p2[0, None]) ** 2).sum(2)
    r2 = C.BALL_LATTICE_RADIUS ** 2
    assert int((d == r2).sum()) > 0
    idx = z["ball/lattice/idx/%d" % C.BALL_LATTICE_K][0]
    assert [int(v) for v in (idx >= 0).sum(1)] == [int(v) for v in (d < r2).sum(1)]


def test_cube_flag_with_points_on_the_faces_of_the_cube():
    # float32 points whose offsets from the query are exactly +-r in one coordinate (on a face), just inside and just outside
    r = 0.25
    q = torch.tensor([[[0.5, 0.5, 0.5]]])
    eps = 2.0 ** -20
    offs = torch.tensor([[r, 0, 0], [-r, 0, 0], [0, r, 0], [0, 0, -r], [r - eps, 0, 0], [r + eps, 0, 0], [r, r, r], [0.1, 0.1, 0.1],
                         [r - eps, eps, 0], [float("nan"), 0, 0]])
    p2 = q + offs[None]
    plain = p3d.ball_query(q, p2, K=8, radius=r)
    flagged = p3d.ball_query(q, p2, K=8, radius=r, skip_points_outside_cube=True)
    assert torch.equal(plain.idx, flagged.idx) and torch.equal(plain.dists, flagged.dists)
    assert plain.idx[0, 0].tolist() == [4, 7, 8, -1, -1, -1, -1, -1]  # on a face: distance exactly r, no hit; a NaN: no hit


def test_argument_errors_carry_the_references_messages():
    pts = torch.rand(2, 10, 3)
    with pytest.raises(ValueError, match="points and lengths must have same batch dimension."):
        p3d.sample_farthest_points(pts, torch.tensor([10]))
    with pytest.raises(ValueError, match="A value in lengths was too large."):
        p3d.sample_farthest_points(pts, torch.tensor([10, 11]))
    with pytest.raises(ValueError, match="K and points must have the same batch dimension"):
        p3d.sample_farthest_points(pts, K=[3])
    with pytest.raises(ValueError, match="pts1 and pts2 must have the same batch dimension."):
        p3d.ball_query(pts, torch.rand(3, 10, 3))
    with pytest.raises(ValueError, match="pts1 and pts2 must have the same point dimension."):
        p3d.ball_query(pts, torch.rand(2, 10, 2))
    with pytest.raises(ValueError, match="points and idx must have the same batch dimension"):
        p3d.masked_gather(pts, torch.zeros(3, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="idx format is not supported"):
        p3d.masked_gather(pts, torch.zeros(2, dtype=torch.int64))


def test_k_as_int_list_and_tensor():
    pts = C.fixture()["fps/ragged3/points"]
    lengths = torch.tensor([200, 77, 1])
    by_int = p3d.sample_farthest_points(pts, lengths, 12)[1]
    assert by_int.shape == (3, 12) and (by_int[2, 1:] == -1).all() and int(by_int[2, 0]) == 0
    by_list = p3d.sample_farthest_points(pts, lengths, [12, 5, 0])[1]
    by_tensor = p3d.sample_farthest_points(pts, lengths, torch.tensor([12, 5, 0], dtype=torch.int32))[1]
    assert torch.equal(by_list, by_tensor) and by_list.shape == (3, 12)
    assert torch.equal(by_list[0], by_int[0]) and torch.equal(by_list[1, :5], by_int[1, :5])
    assert (by_list[1, 5:] == -1).all() and (by_list[2] == -1).all()  # K[n] = 0: a row of -1
    assert p3d.sample_farthest_points(pts, lengths, 0)[1].shape == (3, 0)
    empty = p3d.sample_farthest_points(pts, torch.tensor([0, 3, 200]), 4)
    assert (empty[1][0] == -1).all() and not empty[0][0].any() and (empty[1][1] >= 0).sum() == 3


def test_start_idxs_against_random_start_point():
    pts = C.fixture()["fps/ragged3/points"]
    lengths = torch.tensor([200, 77, 1])
    torch.manual_seed(7)
    drawn = p3d.sample_farthest_points(pts, lengths, 9, random_start_point=True)[1]
    torch.manual_seed(7)
    start = (lengths * torch.rand(lengths.size())).to(torch.int64)  # the reference's draw for ragged clouds
    assert torch.equal(drawn[:, 0], start) and start[2] == 0
    assert torch.equal(p3d.sample_farthest_points(pts, lengths, 9, start_idxs=start)[1], drawn)
    torch.manual_seed(8)
    full = p3d.sample_farthest_points(pts, None, 9, random_start_point=True)[1]
    torch.manual_seed(8)
    start = torch.randint(high=200, size=(3,))  # the reference's draw for full clouds
    assert torch.equal(full[:, 0], start)
    assert torch.equal(p3d.sample_farthest_points(pts, None, 9, start_idxs=start)[1], full)
    assert not torch.equal(full, p3d.sample_farthest_points(pts, None, 9)[1])
    # out of range: clamped into the cloud
    clamped = p3d.sample_farthest_points(pts, lengths, 3, start_idxs=torch.tensor([-4, 500, 9]))[1]
    assert clamped[:, 0].tolist() == [0, 76, 0]


def test_float64_and_other_dimensions_take_the_formulation():
    gen = torch.Generator().manual_seed(3)
    pts = torch.rand(2, 60, 5, generator=gen, dtype=torch.float64)
    sel, idx = p3d.sample_farthest_points(pts, None, 10)
    assert sel.dtype == torch.float64 and C.fps_smallest_gap(pts, None, 10, idx) > 0  # (asserts the float64 arg-max at every step)
    res = p3d.ball_query(pts[:, :20], pts, K=7, radius=0.6)
    assert res.dists.dtype == torch.float64
    d = ((pts[:, :20, None] - pts[:, None]) ** 2).sum(3)
    for n in range(2):
        for i in range(20):
            want = torch.nonzero(d[n, i] < 0.6 * 0.6)[:7, 0].tolist()
            assert res.idx[n, i, :len(want)].tolist() == want and (res.idx[n, i, len(want):] == -1).all()


@pytest.mark.parametrize("name,K", [("ragged3", 5), ("ragged3", 64), ("full2", 8)])
def test_ball_gradients_match_float64_autograd(name, K):
    z = C.fixture()
    l1, l2, radius = _ball_case(name)
    p1 = z["ball/%s/p1" % name].clone().requires_grad_(True)
    p2 = z["ball/%s/p2" % name].clone().requires_grad_(True)
    got = p3d.ball_query(p1, p2, l1, l2, K=K, radius=radius)
    g = torch.randn(got.dists.shape, generator=torch.Generator().manual_seed(11))
    h = torch.randn(got.knn.shape, generator=torch.Generator().manual_seed(12))
    gp1, gp2 = torch.autograd.grad((got.dists * g).sum() + (got.knn * h).sum(), (p1, p2))
    q1, q2 = p1.detach().double().requires_grad_(True), p2.detach().double().requires_grad_(True)
    truth = (C.ball_dists64(q1, q2, got.idx) * g.double()).sum() + (fps_mod.masked_gather(q2, got.idx) * h.double()).sum()
    t1, t2 = torch.autograd.grad(truth, (q1, q2))
    for a, t in ((gp1, t1), (gp2, t2)):
        assert float((a.double() - t).abs().max()) <= 1e-5 * max(1.0, float(t.abs().max()))
    if l1 is not None:
        rows = torch.arange(p1.shape[1])[None, :] >= l1[:, None]
        assert not gp1[rows].any()  # rows past lengths1 get nothing
        cols = torch.arange(p2.shape[1])[None, :] >= l2[:, None]
        assert not gp2[cols].any()


def test_abi_declares_and_exports_the_new_entries():
    header = open(os.path.join(ROOT, "include", "p3d_amd.h")).read()
    for name in ("p3d_sample_farthest_points_workspace_bytes", "p3d_sample_farthest_points", "p3d_ball_query"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\b(int|size_t) %s\(" % name, header), name
    assert re.search(r"#define P3D_FPS_REGISTER_POINTS %d\b" % _lib.FPS_REGISTER_POINTS, header)
    assert "fps_ball.hip" in importlib.import_module("pytorch3d_amd.build").SOURCES
    assert not any(n.endswith("_ordered") for n in ("p3d_sample_farthest_points", "p3d_ball_query"))
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.p3d_sample_farthest_points_workspace_bytes(3, _lib.FPS_REGISTER_POINTS) == 0
        assert lib.p3d_sample_farthest_points_workspace_bytes(3, _lib.FPS_REGISTER_POINTS + 1) == 3 * (_lib.FPS_REGISTER_POINTS + 1) * 4
        # the argument checks need no device: unsupported D, bad sizes and null pointers, empty problems
        fps, ball = lib.p3d_sample_farthest_points, lib.p3d_ball_query
        assert fps(None, None, None, None, 1, 8, 5, 4, None, None, 0, None) == -6
        assert fps(None, None, None, None, 1, -1, 3, 4, None, None, 0, None) == -1
        assert fps(None, None, None, None, 1, 8, 3, 4, None, None, 0, None) == -1
        assert fps(None, None, None, None, 0, 8, 3, 4, None, None, 0, None) == 0
        assert fps(None, None, None, None, 2, 0, 3, 4, None, None, 0, None) == 0
        assert ball(None, None, None, None, 1, 8, 8, 4, 5, 0.2, None, None, None) == -6
        assert ball(None, None, None, None, 1, 8, 8, 3, 0, 0.2, None, None, None) == -1
        assert ball(None, None, None, None, 1, 8, 8, 3, 5, 0.2, None, None, None) == -1
        assert ball(None, None, None, None, 0, 8, 8, 3, 5, 0.2, None, None, None) == 0
        assert ball(None, None, None, None, 2, 0, 8, 2, 5, 0.2, None, None, None) == 0


def test_shim_module_binds_both_operators_and_the_wrappers_refuse_cpu_tensors():
    import pytorch3d_amd.shim as shim

    assert _C.POINT_CLOUD_EXPORTS == ("sample_farthest_points", "ball_query")
    assert not set(_C.POINT_CLOUD_EXPORTS) & set(_C.HOT_PATH_EXPORTS) and len(_C.HOT_PATH_EXPORTS) == 20
    mod = shim.make_module()
    assert mod.sample_farthest_points is fps_mod.sample_farthest_points_op and mod.ball_query is ball_mod.ball_query_op
    pts = torch.rand(2, 9, 3)
    with pytest.raises(RuntimeError, match="must be a CUDA/HIP tensor"):
        _C.sample_farthest_points(pts, None, None, None, 3)
    with pytest.raises(RuntimeError, match="must be a CUDA/HIP tensor"):
        _C.ball_query(pts, pts, None, None, 3, 0.2, False)
    # the module's operators take the reference's positional arguments and serve CPU tensors by the formulation
    lengths, K, start = torch.tensor([9, 4]), torch.tensor([3, 6]), torch.tensor([0, 2])
    idx = mod.sample_farthest_points(pts, lengths, K, start)  # max_K read from K
    assert idx.shape == (2, 6) and idx[:, 0].tolist() == [0, 2] and (idx[0, 3:] == -1).all() and (idx[1, 4:] == -1).all()
    assert torch.equal(idx, mod.sample_farthest_points(pts, lengths, K, start, 6))
    bi, bd = mod.ball_query(pts, pts, lengths, lengths, 4, 0.5, True)
    want = p3d.ball_query(pts, pts, lengths, lengths, K=4, radius=0.5)
    assert torch.equal(bi, want.idx) and torch.equal(bd, want.dists)


def test_shim_on_the_cpu():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    if not os.path.isdir(os.path.join(stage, "pytorch3d", "ops")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_fps_ball_case.py"), "cpu"], capture_output=True, text=True,
                         timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    print(json.dumps(rec))
    assert rec["unpatched_is_the_reference"] and rec["calls_before_patch"] == 0
    assert rec["plain_golden_equal"] and rec["plain_golden_dists_error"] <= 0.0 and rec["plain_backward_meets_the_stub"]
    assert rec["patched_everywhere"] and rec["patched_golden_equal"] and rec["patched_golden_dists_error"] <= 0.0
    assert rec["set_abstraction_equal"] and rec["set_abstraction_grad_finite"] and rec["restored"]
    # CPU tensors: the package's torch formulation, counted as fallbacks
    assert all(v == 0 for v in rec["fused_calls"].values()) and all(v >= 1 for v in rec["fallback_calls"].values())
