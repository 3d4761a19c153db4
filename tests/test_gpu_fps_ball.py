"""sample_farthest_points / ball_query on the GPU (csrc/fps_ball.hip) against the reference's recorded results
(tests/golden/fps_ball_ref.npz) and against the package's float32 torch formulation run on the CPU.

The formulation performs the kernels' float32 operations in the kernels' order (per coordinate a subtraction, a multiplication and
an addition, nothing fused), so on every generated shape the indices must be EQUAL outright -- no entry is left out -- and the
distances bit-equal.  Gradients of the ball query (the nearest neighbours' backward kernels) are gated the way chamfer's are: within
4 x the error of the float32 formulation against float64 autograd.
"""
import contextlib
import importlib
import json
import os
import subprocess
import sys

import pytest
import torch

import fps_ball_case as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    return torch.device("cuda:0")


def _to(t):
    return None if t is None else (C.lengths_tensor(t) if isinstance(t, list) else t).to(_dev())


def _mods():
    # (importlib: the package re-exports the functions of these names over the sub-modules)
    return importlib.import_module("pytorch3d_amd.sample_farthest_points"), importlib.import_module("pytorch3d_amd.ball_query")


@contextlib.contextmanager
def _flag(on):
    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])


def _cloud(N, P, D, seed):
    return torch.rand(N, P, D, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _fps_both(points, lengths, K, start=None):
    """(kernel idx, kernel selected points) after asserting both equal to the float32 formulation on the CPU."""
    import pytorch3d_amd as p3d

    fps_mod, _ = _mods()
    assert fps_mod.kernel_path(points.to(_dev()))
    Kd = K if isinstance(K, int) else _to(C.k_arg(K))
    sel, idx = p3d.sample_farthest_points(points.to(_dev()), _to(lengths), Kd, start_idxs=_to(start))
    want_sel, want = p3d.sample_farthest_points(points, C.lengths_tensor(lengths) if isinstance(lengths, list) else lengths, C.k_arg(K),
                                                start_idxs=start)
    assert idx.dtype == torch.int64 and torch.equal(idx.cpu(), want)
    assert torch.equal(sel.cpu(), want_sel)
    return idx, sel


# ---- farthest point sampling ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in C.FPS_RANDOM] + list(C.FPS_LATTICE))
def test_fps_matches_the_reference(name):
    z = C.fixture()
    points = z["fps/%s/points" % name]
    if name in C.FPS_LATTICE:
        lengths, K = None, C.FPS_LATTICE_K[name]
    else:
        _, _, _, _, lengths, K = next(c for c in C.FPS_RANDOM if c[0] == name)
    idx, sel = _fps_both(points, lengths, K)
    assert torch.equal(idx.cpu(), z["fps/%s/idx" % name]) and torch.equal(sel.cpu(), z["fps/%s/sel" % name])


# one point below, at and above every rung of the ladder: 64 .. 1024 lanes with one point each, then 2 .. 16 points per lane of 1024;
# 1 and 63 / 64 / 65: a single wave, then the first reduction across waves; 16 385: the workspace form
RUNGS = [1] + [p + e for p in (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384) for e in (-1, 0, 1)]


@pytest.mark.parametrize("D", [3, 2])
@pytest.mark.parametrize("P", RUNGS)
def test_fps_at_every_rung_of_the_ladder(P, D):
    from pytorch3d_amd import _lib

    assert _lib.FPS_REGISTER_POINTS == 16384
    points = _cloud(2, P, D, 100 + P)
    _fps_both(points, [P, max(1, (2 * P) // 3)], 8, start=torch.tensor([P - 1, 0]))


def test_fps_workspace_form_with_ragged_clouds():
    P = 16384 + 700
    points = _cloud(3, P, 3, 5)
    _fps_both(points, [P, 16385, 3], [8, 6, 5])


def test_fps_ragged_lengths_k_tensor_and_start_indices_in_one_launch():
    points = _cloud(5, 300, 3, 9)
    points[3, 150:] = float("nan")  # padding is never read as a point
    idx, sel = _fps_both(points, [0, 1, 300, 150, 7], [4, 3, 20, 0, 12], start=torch.tensor([0, 0, 17, 3, 6]))
    idx = idx.cpu()
    assert (idx[0] == -1).all() and idx[1].tolist() == [0] + [-1] * 19 and (idx[3] == -1).all()  # length 0, length 1, K[n] = 0
    assert idx[2, 0] == 17 and (idx[2] >= 0).all() and idx[4, 0] == 6
    assert sorted(idx[4, :7].tolist()) == list(range(7)) and (idx[4, 7:] == -1).all()  # K above the length: every point once
    assert not sel.cpu()[idx < 0].any()


def test_fps_without_lengths_and_with_an_int_k_needs_no_host_sync():
    import pytorch3d_amd as p3d

    points = _cloud(2, 500, 3, 3).to(_dev())
    p3d.sample_farthest_points(points, None, 4)  # (the library is loaded, the workspace pool warm)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        sel, idx = p3d.sample_farthest_points(points, None, 16)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert idx.shape == (2, 16) and sel.shape == (2, 16, 3)


def test_fps_same_bits_on_a_second_run_and_a_second_stream():
    import pytorch3d_amd as p3d

    torch.cuda.synchronize()
    for P in (1500, 16384 + 64):
        points = _cloud(2, P, 3, P).to(_dev())
        first = p3d.sample_farthest_points(points, None, 24)[1]
        again = p3d.sample_farthest_points(points, None, 24)[1]
        stream = torch.cuda.Stream(device=_dev())
        stream.wait_stream(torch.cuda.current_stream(_dev()))
        with torch.cuda.stream(stream):
            other = p3d.sample_farthest_points(points, None, 24)[1]
        stream.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(first, again) and torch.equal(first, other), P


def test_fps_with_non_finite_coordinates_stays_inside_the_cloud():
    import pytorch3d_amd as p3d

    points = _cloud(2, 700, 3, 2)
    points[0, 5] = float("nan")
    points[0, 300, 1] = float("inf")
    points[1, ::7] = float("nan")
    idx = p3d.sample_farthest_points(points.to(_dev()), _to([700, 650]), 40)[1].cpu()
    assert (idx[0] >= 0).all() and (idx[0] < 700).all() and (idx[1] >= 0).all() and (idx[1] < 650).all()


# ---- ball query ---------------------------------------------------------------------------------------------------------------------
def _ball_edge_case(which, D):
    """Clouds in the unit cube with the first three queries of every cloud far away (no hits), p2's padding filled with copies of the
    queries (distance 0) and p1's padding with NaN: decoys that must never appear."""
    gen = torch.Generator().manual_seed(40 + D)
    if which == "tiles":  # lengths2 around the tile of 512 and the full 1030 in one launch
        P1, P2, l1, l2 = 70, 1030, [70, 64, 33, 0], [1030, 512, 513, 511]
    else:  # K above the length
        P1, P2, l1, l2 = 40, 48, [40, 33, 2], [40, 17, 5]
    N = len(l1)
    p1, p2 = torch.rand(N, P1, D, generator=gen), torch.rand(N, P2, D, generator=gen)
    p1[:, :3] += 5.0
    for n in range(N):
        pad = P2 - l2[n]
        if pad:
            p2[n, l2[n]:] = p1[n, torch.arange(pad) % max(l1[n], 1)]
        p1[n, l1[n]:] = float("nan")
    return p1, p2, l1, l2


@pytest.mark.parametrize("D", [3, 2])
@pytest.mark.parametrize("which,K", [("tiles", 1), ("tiles", 5), ("tiles", 64), ("tiles", 500), ("short", 64), ("short", 5)])
def test_ball_query_equals_the_formulation(which, K, D):
    import pytorch3d_amd as p3d

    _, ball_mod = _mods()
    p1, p2, l1, l2 = _ball_edge_case(which, D)
    radius = 0.2 if D == 3 else 0.1
    assert ball_mod.kernel_path(p1.to(_dev()), p2.to(_dev()), K)
    got = p3d.ball_query(p1.to(_dev()), p2.to(_dev()), _to(l1), _to(l2), K=K, radius=radius, skip_points_outside_cube=bool(K % 2))
    want = p3d.ball_query(p1, p2, C.lengths_tensor(l1), C.lengths_tensor(l2), K=K, radius=radius)
    assert got.idx.dtype == torch.int64 and torch.equal(got.idx.cpu(), want.idx)
    assert torch.equal(got.dists.cpu(), want.dists) and torch.equal(got.knn.cpu(), want.knn)
    idx = got.idx.cpu()
    hits = (idx >= 0).sum(2)
    for n in range(len(l1)):
        assert int(idx[n].max()) < max(l2[n], 1) and (idx[n, l1[n]:] == -1).all()  # no decoy, no padding row
        assert not hits[n, :min(3, l1[n])].any()  # the far queries
    if which == "tiles" and K <= 5:
        assert (hits[0, 64:] == K).all()  # a wave whose live rows all fill up: it leaves the scan early
    if which == "tiles" and K >= 64:
        assert 0 < int(hits[0, 3:].min()) and int(hits[0, 3:].max()) < K  # rows with some hits and room left


@pytest.mark.parametrize("name,K", [(name, K) for name, *_r, Ks, _radius in C.BALL_RANDOM for K in Ks] + [("lattice", C.BALL_LATTICE_K)])
def test_ball_query_matches_the_reference(name, K):
    import pytorch3d_amd as p3d

    z = C.fixture()
    if name == "lattice":
        l1, l2, radius = None, None, C.BALL_LATTICE_RADIUS
    else:
        _, _, _, _, _, l1, l2, _, radius = next(c for c in C.BALL_RANDOM if c[0] == name)
    got = p3d.ball_query(z["ball/%s/p1" % name].to(_dev()), z["ball/%s/p2" % name].to(_dev()), _to(l1), _to(l2), K=K, radius=radius)
    want_i, want_d = z["ball/%s/idx/%d" % (name, K)], z["ball/%s/dists/%d" % (name, K)]
    assert torch.equal(got.idx.cpu(), want_i)  # the lattice case: points at distance exactly 2 are no hits
    assert float(((got.dists.cpu() - want_d).abs() - 2e-6 * want_d.abs()).max()) <= 0.0
    assert not got.dists.cpu()[want_i < 0].any()


@pytest.fixture(scope="module")
def ball_grad_cases():
    """Per (case, D): upstream gradients, the float64 autograd truth, and the float32 formulation's own error against it (CPU)."""
    import pytorch3d_amd as p3d

    fps_mod, _ = _mods()
    out = {}
    for which, K in (("tiles", 5), ("short", 64)):
        for D in (3, 2):
            p1, p2, l1, l2 = _ball_edge_case(which, D)
            radius = 0.2 if D == 3 else 0.1
            a, b = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
            cpu = p3d.ball_query(a, b, C.lengths_tensor(l1), C.lengths_tensor(l2), K=K, radius=radius)
            g = torch.randn(cpu.dists.shape, generator=torch.Generator().manual_seed(17))
            f32 = torch.autograd.grad((cpu.dists * g).sum(), (a, b))
            # (the NaN padding rows of p1 take no part; as zeros they keep 0 * NaN out of float64 autograd)
            q1, q2 = torch.nan_to_num(p1).double().requires_grad_(True), p2.double().requires_grad_(True)
            truth = torch.autograd.grad((C.ball_dists64(q1, q2, cpu.idx) * g.double()).sum(), (q1, q2))
            out[(which, K, D)] = (cpu.idx, g, truth, [float((f.double() - t).abs().max()) for f, t in zip(f32, truth)])
    return out


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("D", [3, 2])
@pytest.mark.parametrize("which,K", [("tiles", 5), ("short", 64)])
def test_ball_query_gradients_within_the_gate(ball_grad_cases, which, K, D, ordered):
    import pytorch3d_amd as p3d

    idx, g, truth, e32 = ball_grad_cases[(which, K, D)]
    p1, p2, l1, l2 = _ball_edge_case(which, D)
    radius = 0.2 if D == 3 else 0.1

    def run():
        a, b = p1.to(_dev()).requires_grad_(True), p2.to(_dev()).requires_grad_(True)
        with _flag(ordered):
            got = p3d.ball_query(a, b, _to(l1), _to(l2), K=K, radius=radius, return_nn=False)
            assert type(got.dists.grad_fn).__name__ == "_BallQueryBackward"  # one autograd node
            grads = torch.autograd.grad((got.dists * g.to(_dev())).sum(), (a, b))
        assert torch.equal(got.idx.cpu(), idx)
        return grads

    grads = run()
    for which_g, got_g, t, e in zip(("grad_p1", "grad_p2"), grads, truth, e32):
        err = float((got_g.cpu().double() - t).abs().max())
        print(which, K, D, "ordered" if ordered else "atomic", which_g, "error %.3g" % err, "float32 formulation %.3g" % e)
        assert err <= 4 * e, which_g
    gp1, gp2 = grads[0].cpu(), grads[1].cpu()
    for n in range(len(l1)):  # padding: exactly zero, NaN rows and decoys included
        assert not gp1[n, l1[n]:].any() and not gp2[n, l2[n]:].any()
    if ordered:
        again = run()
        assert torch.equal(grads[1], again[1]) and torch.equal(grads[0], again[0])


# ---- drop-in ------------------------------------------------------------------------------------------------------------------------
def test_reference_functions_through_the_shim():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_fps_ball_case.py"), "cuda:0"], capture_output=True, text=True,
                         timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    print(json.dumps(rec))
    assert rec["unpatched_is_the_reference"] and rec["calls_before_patch"] == 0
    # plain install(): the unmodified reference functions on the kernels; the ball query's backward meets the stub
    assert rec["plain_golden_equal"] and rec["plain_golden_dists_error"] <= 0.0 and rec["plain_backward_meets_the_stub"]
    # patch_python: the golden again, a set-abstraction step equal to the formulation, and the fused path counted
    assert rec["patched_everywhere"] and rec["patched_golden_equal"] and rec["patched_golden_dists_error"] <= 0.0
    assert rec["set_abstraction_equal"] and rec["set_abstraction_grad_finite"] and rec["restored"]
    assert all(v >= 1 for v in rec["fused_calls"].values()) and all(v == 0 for v in rec["fallback_calls"].values())
