"""iterative_closest_point / corresponding_points_alignment on the GPU (csrc/points_alignment.hip) through the gates of
tests/points_alignment_case.py against the reference's recorded float64 run (tests/golden/points_alignment_ref.npz): every
tolerance is MARGIN x the reference's own float32 figure recorded there, per family.  The search is held to knn_points(K=1) bit for
bit: around the tile size, on ragged clouds with decoys in the padding, for every forced split with uneven slices and duplicates in
different slices.  Then the loop (iteration counts, the neighbours of every iteration, the history, max_iterations, thresholds, the
warnings), reproducibility across runs and streams, the dispatch, and the unmodified reference through the shim."""
import importlib
import json
import os
import subprocess
import sys
import warnings

import pytest
import torch

import points_alignment_case as C
from pytorch3d_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PA = importlib.import_module("pytorch3d_amd.points_alignment")
TILE = _lib.KNN_TILE
SPLITS = (0, 1, 2, 4, 8)
assert max(SPLITS) == _lib.ICP_MAX_SPLIT


def _dev():
    return torch.device("cuda:0")


def _knn_idx(X, Y, l1=None, l2=None):
    from pytorch3d_amd import knn_points

    return knn_points(X, Y, lengths1=l1, lengths2=l2, K=1).idx[:, :, 0]


def _fused(fn, *args, **kwargs):
    before = dict(PA.CALLS)
    out = fn(*args, **kwargs)
    assert PA.CALLS["fused"] == before["fused"] + 1 and PA.CALLS["chain"] == before["chain"], "the kernels did not run"
    return out


# ---- the search ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P2", (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 76))
@pytest.mark.parametrize("P1", (63, 64, 65))
def test_match_is_knn_points_around_the_wave_and_the_tile(P1, P2):
    from pytorch3d_amd import _C

    assert (P1 - 64) in (-1, 0, 1) and (P2 == 1 or abs(P2 - TILE) <= 1 or P2 > 2 * TILE)  # one / two workgroups; one, two, three tiles
    gen = torch.Generator().manual_seed(100 * P1 + P2)
    X, Y = torch.randn(2, P1, 3, generator=gen).to(_dev()), torch.randn(2, P2, 3, generator=gen).to(_dev())
    want = _knn_idx(X, Y)
    for split in SPLITS:  # a slice is ceil(P2 / split) points: uneven for every P2 here but 512, empty for most waves at P2 = 1
        assert torch.equal(_C.icp_match(X, Y, split=split), want), split


def test_match_ragged_clouds_with_decoys_in_the_padding():
    from pytorch3d_amd import _C

    gen = torch.Generator().manual_seed(7)
    P1, P2 = 150, 2 * TILE + 40
    X, Y = torch.randn(3, P1, 3, generator=gen), torch.randn(3, P2, 3, generator=gen)
    l1, l2 = torch.tensor([150, 64, 1]), torch.tensor([P2, TILE + 3, 0])
    for n in range(3):  # behind the end of Y: copies of X's own points, which would win every search
        k = P2 - int(l2[n])
        Y[n, int(l2[n]):] = X[n, torch.arange(k) % P1]
    X, Y, l1, l2 = (t.to(_dev()) for t in (X, Y, l1, l2))
    want = _knn_idx(X, Y, l1, l2)
    assert bool((want[1, 64:] == 0).all()) and bool((want[2] == 0).all())  # rows past lengths1, and an empty cloud of Y
    for split in SPLITS:
        got = _C.icp_match(X, Y, l1, l2, split=split)
        assert torch.equal(got, want), split
        assert bool((got < l2.clamp(min=1)[:, None]).all())


def test_match_duplicates_in_different_slices_go_to_the_smaller_index():
    from pytorch3d_amd import _C

    gen = torch.Generator().manual_seed(11)
    P2 = 2 * TILE + 76  # split 8: slices of 138, split 4: 275, split 2: 550
    X, Y = torch.randn(1, 130, 3, generator=gen), torch.randn(1, P2, 3, generator=gen) + 5.0
    spots = [5, 140, 300, 700, 1000, P2 - 1]  # one copy per slice of split 8 and more
    Y[0, spots] = X[0, 17]  # six exact copies of one query: distance 0 in slices of every split
    Y[0, [900, 450]] = X[0, 40]  # and a pair that no wave of split 4 or 8 sees both of
    X, Y = X.to(_dev()), Y.to(_dev())
    want = _knn_idx(X, Y)
    assert int(want[0, 17]) == 5 and int(want[0, 40]) == 450
    for split in SPLITS:
        assert torch.equal(_C.icp_match(X, Y, split=split), want), split


def test_match_under_a_transform_is_knn_points_of_the_returned_Xt():
    from pytorch3d_amd import _C

    case = ("icp_scale", "130x70", 0)
    d = C.icp_inputs(case)
    X, Y = C.to(d, _dev())
    sol = _fused(C.run_icp, PA.iterative_closest_point, case, device=_dev())
    for split in SPLITS:
        got = _C.icp_match(X, Y, None, None, *sol.RTs, split=split)
        assert torch.equal(got, _knn_idx(sol.Xt, Y)), split


# ---- moments and solve: corresponding_points_alignment ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.ALIGN_CASES, ids=C.case_id)
def test_alignment_cases_pass_the_reference_gates(case):
    C.check_inputs("align", case)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        out = _fused(C.run_align, PA.corresponding_points_alignment, case, device=_dev())
    assert isinstance(out, PA.SimilarityTransform) and out.R.shape == (3, 3, 3) and out.T.shape == (3, 3) and out.s.shape == (3,)
    C.check("align", case, C.align_values(out), "kernel")
    det = torch.linalg.det(out.R.double().cpu())
    want = -1.0 if case[:2] == ("reflect", "allow") else 1.0
    assert float((det - want).abs().max()) <= 1e-5, det  # det < 0 data: fixed unless reflections are allowed
    low_rank = [w for w in seen if "Excessively low rank" in str(w.message)]
    assert len(low_rank) == (1 if case[1] in ("exact", "zero") else 0)  # sigma = 0 exactly: the reference warns there too
    if case[1] == "zero":  # a cloud without weight: the identity, as the reference's decomposition of a zero matrix gives
        assert torch.equal(out.R[1].cpu(), torch.eye(3)) and not bool(out.T[1].any()) and float(out.s[1]) == 0.0


def test_alignment_of_fewer_than_four_points_warns_and_keeps_its_shapes():
    gen = torch.Generator().manual_seed(3)
    X, Y = torch.randn(2, 3, 3, generator=gen).to(_dev()), torch.randn(2, 3, 3, generator=gen).to(_dev())
    with pytest.warns(UserWarning, match="The size of one of the point clouds is <= dim\\+1"):
        out = _fused(PA.corresponding_points_alignment, X, Y)
    assert out.R.shape == (2, 3, 3) and out.T.shape == (2, 3) and out.s.shape == (2,) and bool(torch.isfinite(out.R).all())
    with pytest.warns(UserWarning, match="The size of one of the point clouds is <= dim\\+1"):
        sol = _fused(PA.iterative_closest_point, X, Y, max_iterations=2)
    assert sol.Xt.shape == (2, 3, 3) and len(sol.t_history) <= 2 and sol.rmse.shape == (2,)


# ---- the loop ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.ICP_CASES, ids=C.case_id)
def test_icp_cases_pass_the_reference_gates(case):
    from pytorch3d_amd import _C

    C.check_inputs("icp", case)
    z = C.fixture()
    d = C.icp_inputs(case)
    sol = _fused(C.run_icp, PA.iterative_closest_point, case, device=_dev())
    its = int(z[C.key("icp", case, "iterations")])
    print("iterations", len(sol.t_history), "recorded", its, "per cloud", z[C.key("icp", case, "first")].tolist())
    assert isinstance(sol, PA.ICPSolution) and isinstance(sol.converged, bool)
    assert len(sol.t_history) == its and sol.converged == bool(z[C.key("icp", case, "converged")])
    assert sol.converged != (case[1] in C.UNCONVERGED)
    C.check("icp", case, C.icp_values(sol), "kernel")
    # the neighbours of every iteration are the float64 run's: the search under the transform the iteration started from
    X, Y = C.to(d, _dev())
    Xp, Yp = C._padded(X), C._padded(Y)
    l1 = None if d["lengths1"] is None else d["lengths1"].to(_dev())
    l2 = None if d["lengths2"] is None else d["lengths2"].to(_dev())
    start = None if d["init"] is None else tuple(t.to(_dev()) for t in d["init"])
    recorded = z[C.key("icp", case, "idx")].long()
    for k in range(its):
        t = start if k == 0 else sol.t_history[k - 1]
        got = _C.icp_match(Xp, Yp, l1, l2, *(t if t is not None else ()))
        assert torch.equal(got.cpu(), recorded[k]), k
    # the history: views of one buffer, its last entry the result; the Xt is the input under it
    assert all(torch.equal(a, b) for a, b in zip(sol.t_history[-1], sol.RTs))
    assert sol.t_history[0].R.untyped_storage().data_ptr() == sol.t_history[-1].R.untyped_storage().data_ptr()
    if isinstance(X, C.Clouds):
        assert isinstance(sol.Xt, C.Clouds) and torch.equal(sol.Xt.num_points_per_cloud(), X.num_points_per_cloud())
    # every split: the same bits
    for split in (1, 8):
        PA.SPLIT = split
        try:
            again = C.run_icp(PA.iterative_closest_point, case, device=_dev())
        finally:
            PA.SPLIT = 0
        assert len(again.t_history) == its and torch.equal(C._padded(again.Xt), C._padded(sol.Xt)) and torch.equal(again.rmse, sol.rmse)
        assert all(torch.equal(a, b) for s, t in zip(again.t_history, sol.t_history) for a, b in zip(s, t))


def test_history_holds_what_shorter_runs_return_and_zero_iterations_the_start():
    case = ("icp_rigid", "maxiter", 0)
    d = C.icp_inputs(case)
    X, Y = C.to(d, _dev())
    full = _fused(PA.iterative_closest_point, X, Y, max_iterations=3)
    assert len(full.t_history) == 3 and not full.converged
    for m in (1, 2):
        part = PA.iterative_closest_point(X, Y, max_iterations=m)
        assert len(part.t_history) == m and not part.converged
        assert all(torch.equal(a, b) for a, b in zip(part.RTs, full.t_history[m - 1]))
    none = PA.iterative_closest_point(X, Y, max_iterations=0)
    assert none.converged is False and none.rmse is None and none.t_history == [] and torch.equal(none.Xt, X)
    assert torch.equal(none.RTs.R.cpu(), torch.eye(3).expand(3, 3, 3)) and not bool(none.RTs.T.any()) and bool((none.RTs.s == 1).all())
    init = tuple(t.to(_dev()) for t in C.icp_inputs(("icp_rigid", "init", 0))["init"])
    none = PA.iterative_closest_point(X, Y, init_transform=init, max_iterations=0)
    assert all(torch.equal(a, b) for a, b in zip(none.RTs, init)) and torch.equal(none.Xt, PA.apply_similarity_transform(X, *init))
    with pytest.raises(ValueError, match="The initial transformation init_transform has to be"):
        PA.iterative_closest_point(X, Y, init_transform=(init[0], init[1][:, :2], init[2]))
    one = _fused(PA.iterative_closest_point, X, Y, relative_rmse_thr=1.0)  # the first relative decrease is 1: converged at once
    assert one.converged and len(one.t_history) == 1
    assert all(torch.equal(a, b) for a, b in zip(one.RTs, full.t_history[0]))


def test_low_rank_warning_is_raised_once_per_call():
    d = C.align_inputs(("planar", "exact", 0))  # z = 0 in both clouds: sigma3 = 0 in every iteration
    X, Y = d["X"].to(_dev()), d["Y"].to(_dev())
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        sol = _fused(PA.iterative_closest_point, X, Y, max_iterations=4)
    assert len(sol.t_history) >= 2
    assert len([w for w in seen if "Excessively low rank" in str(w.message)]) == 1
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        _fused(C.run_icp, PA.iterative_closest_point, ("icp_rigid", "thr1", 0), device=_dev())
    assert not [w for w in seen if "corresponding_points_alignment" in str(w.message)]


def test_two_runs_and_a_side_stream_give_the_same_bits():
    case = ("icp_ragged", "hetero", 0)

    def run():
        sol = C.run_icp(PA.iterative_closest_point, case, device=_dev())
        align = C.run_align(PA.corresponding_points_alignment, ("weights", "rand", 0), device=_dev())
        return [C._padded(sol.Xt), sol.rmse, *sol.RTs, *align] + [t for h in sol.t_history for t in h]

    first, second = run(), run()
    side = torch.cuda.Stream(_dev())
    side.wait_stream(torch.cuda.current_stream(_dev()))
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    assert len(first) == len(second) == len(third)
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_dispatch_takes_the_chain_where_the_kernels_do_not_apply():
    d = C.icp_inputs(("icp_scale", "130x70", 0))
    X, Y = d["X"].to(_dev()), d["Y"].to(_dev())
    assert PA.kernel_path(X, Y) and PA.kernel_path(X, X, torch.ones(3, 130, device=_dev()))
    assert not PA.kernel_path(X.double(), Y.double()) and not PA.kernel_path(X.cpu(), Y.cpu()) and not PA.kernel_path(X[..., :2], Y[..., :2])
    assert not PA.kernel_path(X.clone().requires_grad_(True), Y) and not PA.kernel_path(X, X, [torch.ones(130, device=_dev())] * 3)
    fused = PA.iterative_closest_point(X, Y, estimate_scale=True)
    before = dict(PA.CALLS)
    chain = PA.iterative_closest_point(X.double(), Y.double(), estimate_scale=True)
    leaf = X.clone().requires_grad_(True)
    grad = PA.corresponding_points_alignment(leaf, X * 1.5 + 0.25, estimate_scale=True)
    assert PA.CALLS["chain"] == before["chain"] + 2 and PA.CALLS["fused"] == before["fused"]
    assert len(chain.t_history) == len(fused.t_history) and chain.converged == fused.converged
    assert float((chain.RTs.R.float() - fused.RTs.R).abs().max()) <= 1e-5 and float((chain.Xt.float() - fused.Xt).abs().max()) <= 1e-5
    (grad.R.sum() + grad.T.sum() + grad.s.sum()).backward()  # autograd through the restated chain
    assert bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().sum()) > 0
    with pytest.raises(ValueError, match="number of batches and data dimensions"):
        PA.iterative_closest_point(X, Y[:2])
    with pytest.raises(ValueError, match="weights should have the same first two dimensions as X"):
        PA.corresponding_points_alignment(X, X, weights=torch.ones(3, 7, device=_dev()))


def test_reference_functions_through_the_shim():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_points_alignment_case.py"), "cuda:0"], capture_output=True,
                         text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    print(json.dumps(rec))
    assert rec["unpatched_is_the_reference"] and rec["calls_before_patch"] == 0 and rec["patched_everywhere"]
    assert rec["icp_equal"] and rec["icp_types"] and rec["align_equal"] and rec["pointclouds_updated"]
    assert rec["fused_calls"] == {"iterative_closest_point": 2, "corresponding_points_alignment": 1}
    assert rec["fallback_calls"] == {"iterative_closest_point": 0, "corresponding_points_alignment": 0}
    assert rec["float64_counted_as_fallback"] == 1 and rec["restored"]
