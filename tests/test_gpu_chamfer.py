"""csrc/knn.hip on the MI355X: knn_points (K = 1 and the register queues), chamfer_distance as one autograd node, their backwards
(gather, atomic scatter, ordered scatter) and the two patches of pytorch3d_amd.shim.

Yardsticks: tests/golden/chamfer_ref.npz -- the reference's own naive neighbours and its chamfer_distance, recorded on the CPU on
queries that keep a relative gap >= 1e-5 between consecutive distances, so idx must match BIT FOR BIT and dists within 2e-6 relative
-- and tests/chamfer_case.py: a float64 brute force in (dist, j) order for the exact ties, float64 restatements on given indices for
the gradients.  Gates, the measure of tests/test_gpu_mesh_normals.py / test_gpu_mesh_losses.py: a gradient within FOUR times the
largest error the float32 torch formulation makes on the CPU against the same truth; a summed loss within four times that
formulation's error plus D(n) 2^-24 S, D(n) = 6 + ceil(ceil(n / 64) / 256) + 8 the depth of the kernels' sum tree and S the float64
sum of the absolute terms; the star's grad_p2 (300 hits on one point) within in-degree x 2^-23 x the largest term.
"""
import contextlib
import json
import os
import subprocess
import sys
import warnings

import pytest
import torch

import _util as U
import chamfer_case as C

pytestmark = pytest.mark.gpu

ROOT = U.ROOT
FUSED_CASES = [c[0] for c in C.CHAMFER_CASES
               if not c[2] and c[5].get("point_reduction", "mean") in ("mean", "sum") and c[0] != "weights_zero"]


def _dev():
    return torch.device("cuda:0")


@contextlib.contextmanager
def _flag(on):
    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])


def _case(name):
    z = C.fixture()
    _, N, P1, P2, D, l1, l2, Ks, norms = next(c for c in C.KNN_CASES if c[0] == name)
    return z[C.knn_key(name, "p1")], z[C.knn_key(name, "p2")], l1, l2


def _to(t):
    return None if t is None else (C.lengths_tensor(t) if isinstance(t, list) else t).to(_dev())


def _knn_params():
    return [(name, K, norm) for name, *_r, Ks, norms in C.KNN_CASES for K in Ks for norm in norms]


@pytest.mark.parametrize("name,K,norm", _knn_params())
def test_forward_matches_the_reference_neighbours(name, K, norm):
    import pytorch3d_amd as p3d
    from pytorch3d_amd import knn as knn_mod

    z = C.fixture()
    p1, p2, l1, l2 = _case(name)
    a, b = p1.to(_dev()), p2.to(_dev())
    assert knn_mod.kernel_path(a, b, K) == (name not in ("d5", "k33"))
    got = p3d.knn_points(a, b, _to(l1), _to(l2), norm=norm, K=K)
    want_idx, want_d = z[C.knn_key(name, "idx", K, norm)], z[C.knn_key(name, "dists", K, norm)]
    assert torch.equal(got.idx.cpu(), want_idx)
    assert float(((got.dists.cpu() - want_d).abs() - 2e-6 * want_d.abs()).max()) <= 0.0


@pytest.mark.parametrize("name,K", [("pad", 8), ("pad", 1), ("empty", 3), ("wg_edge", 1)])
def test_the_kernel_writes_every_entry_and_padding_is_exactly_zero(name, K):
    from pytorch3d_amd import _C

    p1, p2, l1, l2 = _case(name)
    N, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    idx = torch.full((N, P1, K), -7, dtype=torch.int64, device=_dev())
    dists = torch.full((N, P1, K), float("nan"), device=_dev())
    got_idx, got_d = _C.knn_points_idx(p1.to(_dev()), p2.to(_dev()), _to(l1), _to(l2), 2, K, -1, _out=(idx, dists))
    assert got_idx is idx and got_d is dists
    assert not torch.isnan(dists).any() and (idx >= 0).all()
    valid = C.valid_mask(l1, l2, N, P1, P2, K)
    assert not idx.cpu()[~valid].any() and not dists.cpu()[~valid].any()
    want_idx, want_d = C.fixture()[C.knn_key(name, "idx", K, 2)], C.fixture()[C.knn_key(name, "dists", K, 2)]
    assert torch.equal(idx.cpu(), want_idx)
    # the gradients of the padding: rows past lengths1 of grad_p1, points past lengths2 of grad_p2
    g = torch.randn(N, P1, K, generator=torch.Generator().manual_seed(3)).to(_dev())
    for ordered in (False, True):
        with _flag(ordered):
            gp1, gp2 = _C.knn_points_backward(p1.to(_dev()), p2.to(_dev()), _to(l1), _to(l2), idx, 2, g)
        assert not gp1.cpu()[~valid.any(2)].any()
        l2t = torch.full((N,), P2) if l2 is None else torch.tensor(l2)
        l1t = torch.full((N,), P1) if l1 is None else torch.tensor(l1)
        outside = (torch.arange(P2)[None, :] >= l2t[:, None]) | (l1t[:, None] == 0)
        assert not gp2.cpu()[outside].any()
        assert torch.isfinite(gp1).all() and torch.isfinite(gp2).all()


@pytest.mark.parametrize("norm", [2, 1])
def test_exact_ties_go_to_the_smaller_index(norm):
    import pytorch3d_amd as p3d

    p1, p2 = C.tie_clouds()
    for K in (1, 2, 6, 32):
        want_idx, want_d = C.brute64(p1, p2, None, None, K, norm)
        got = p3d.knn_points(p1.to(_dev()), p2.to(_dev()), norm=norm, K=K)
        assert torch.equal(got.idx.cpu(), want_idx), K
        assert torch.equal(got.dists.cpu().double(), want_d), K


@pytest.fixture(scope="module")
def knn_grad_cases():
    """Per case: the upstream gradient, the float64 truth on the fixture's indices and the float32 CPU formulation's error against
    it -- computed once, never modified."""
    import pytorch3d_amd as p3d

    z = C.fixture()
    out = {}
    for name, K, norm in (("pad", 8, 2), ("pad", 3, 1), ("wg_edge", 1, 2), ("d2", 3, 2), ("d2", 3, 1), ("k32", 32, 2), ("tile_2p3", 3, 2),
                          ("empty", 3, 2)):
        p1, p2, l1, l2 = _case(name)
        idx = z[C.knn_key(name, "idx", K, norm)]
        g = torch.randn(idx.shape, generator=torch.Generator().manual_seed(17))
        truth = C.knn_grad_truth(p1, p2, l1, l2, idx, norm, g)
        a, b = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
        cpu = p3d.knn_points(a, b, C.lengths_tensor(l1), C.lengths_tensor(l2), norm=norm, K=K)
        assert torch.equal(cpu.idx, idx)
        f32 = torch.autograd.grad((cpu.dists * g).sum(), (a, b))
        out[(name, K, norm)] = (g, truth, [float((f.double() - t).abs().max()) for f, t in zip(f32, truth)])
    return out


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("name,K,norm", [("pad", 8, 2), ("pad", 3, 1), ("wg_edge", 1, 2), ("d2", 3, 2), ("d2", 3, 1), ("k32", 32, 2),
                                         ("tile_2p3", 3, 2), ("empty", 3, 2)])
def test_knn_gradients_within_the_gate(knn_grad_cases, name, K, norm, ordered):
    import pytorch3d_amd as p3d

    g, truth, e32 = knn_grad_cases[(name, K, norm)]
    p1, p2, l1, l2 = _case(name)
    a, b = p1.to(_dev()).requires_grad_(True), p2.to(_dev()).requires_grad_(True)
    with _flag(ordered):
        got = p3d.knn_points(a, b, _to(l1), _to(l2), norm=norm, K=K)
        assert type(got.dists.grad_fn).__name__ == "_KnnPointsBackward"  # one autograd node
        grads = torch.autograd.grad((got.dists * g.to(_dev())).sum(), (a, b))
    for which, got_g, t, e in zip(("grad_p1", "grad_p2"), grads, truth, e32):
        err = float((got_g.cpu().double() - t).abs().max())
        print(name, K, norm, "ordered" if ordered else "atomic", which, "error %.3g" % err, "float32 formulation %.3g" % e)
        assert err <= 4 * e, which


def test_return_nn_is_knn_gather_of_the_indices():
    import pytorch3d_amd as p3d

    p1, p2, l1, l2 = _case("pad")
    b = p2.to(_dev())
    got = p3d.knn_points(p1.to(_dev()), b, _to(l1), _to(l2), K=8, return_nn=True)
    assert got.knn.shape == (3, 70, 8, 3)
    assert torch.equal(got.knn, p3d.knn_gather(b, got.idx, _to(l2)))
    assert torch.equal(got.knn[0, 5, 2], b[0, got.idx[0, 5, 2]])
    assert not got.knn[2, :, 5:].any()


def _star_grad_p2(ordered, stream=None):
    import pytorch3d_amd as p3d

    p1, p2 = C.star_clouds()
    ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    with ctx, _flag(ordered):
        a, b = p1.to(_dev()), p2.to(_dev()).requires_grad_(True)
        got = p3d.knn_points(a, b, K=1)
        g = torch.cos(torch.arange(300, dtype=torch.float32)).reshape(1, 300, 1).to(_dev())
        (grad,) = torch.autograd.grad((got.dists * g).sum(), (b,))
    if stream is not None:
        stream.synchronize()
    return grad


def _pad_grad_p2(ordered, stream=None):
    import pytorch3d_amd as p3d

    p1, p2, l1, l2 = _case("pad")
    ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    with ctx, _flag(ordered):
        a, b = p1.to(_dev()), p2.to(_dev()).requires_grad_(True)
        got = p3d.knn_points(a, b, _to(l1), _to(l2), K=8)
        g = torch.randn(got.dists.shape, generator=torch.Generator().manual_seed(17)).to(_dev())
        (grad,) = torch.autograd.grad((got.dists * g).sum(), (b,))
    if stream is not None:
        stream.synchronize()
    return grad


@pytest.mark.parametrize("ordered", [False, True])
def test_star_scatter_within_its_bound(ordered):
    p1, p2 = C.star_clouds()
    g = torch.cos(torch.arange(300, dtype=torch.float64))
    terms = -2.0 * g[:, None] * (p1[0].double() - p2[0].double())  # what each of the 300 hits adds to the one point
    truth = terms.sum(0)
    bound = 300 * 2.0 ** -23 * float(terms.abs().max())
    got = _star_grad_p2(ordered).cpu().double()[0, 0]
    err = float((got - truth).abs().max())
    print("star", "ordered" if ordered else "atomic", "error %.3g" % err, "bound %.3g" % bound)
    assert err <= bound


def test_ordered_backward_gives_the_same_bits_on_two_runs_and_two_streams():
    torch.cuda.synchronize()
    for fn in (_star_grad_p2, _pad_grad_p2):
        first = fn(True)
        torch.cuda.synchronize()
        again = fn(True)
        other = fn(True, torch.cuda.Stream(device=_dev()))
        torch.cuda.synchronize()
        assert torch.equal(first, again) and torch.equal(first, other), fn.__name__
    # with the flag off the call neither raises nor warns
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _star_grad_p2(False)
        _pad_grad_p2(False)
    torch.cuda.synchronize()


# ---- chamfer_distance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in C.CHAMFER_CASES])
def test_chamfer_matches_the_reference(name):
    """Every case of the fixture on the GPU (tensors and Pointclouds-shaped objects); tolerances as in tests/test_cpu_chamfer.py."""
    import pytorch3d_amd as p3d

    z = C.fixture()
    x, y, args, kw = C.chamfer_inputs(name, device=_dev())
    result = p3d.chamfer_distance(*args, **kw)
    outs = C.flatten(result)
    assert (result[1] is not None) == bool(z[C.cham_key(name, "has_normals")])
    if name in FUSED_CASES:
        assert type(outs[0].grad_fn).__name__ == "_ChamferFusedBackward"  # one autograd node
    for i, t in enumerate(outs):
        want = z[C.cham_key(name, "out%d" % i)]
        assert t.shape == want.shape
        assert float((t.detach().cpu() - want).abs().max()) <= 1e-4 * max(1e-3, float(want.abs().max())), i
    gx, gy = torch.autograd.grad(C.scalarise(result), (x, y), allow_unused=True)
    for got, key in ((gx, "grad_x"), (gy, "grad_y")):
        want = z[C.cham_key(name, key)]
        got = torch.zeros_like(want) if got is None else got.cpu()
        assert float((got - want).abs().max()) <= 1e-4 * max(1e-3, float(want.abs().max())), key


@pytest.fixture(scope="module")
def chamfer_truths():
    """Per fused case: float64 loss and gradients on the neighbours of a float64 brute force, S, n, and the float32 CPU
    formulation's errors against them -- computed once, never modified."""
    import pytorch3d_amd as p3d

    out = {}
    for name in FUSED_CASES:
        _, clouds, _, weights, _, kwargs = next(c for c in C.CHAMFER_CASES if c[0] == name)
        N, P1, P2, D, l1, l2 = C.CHAMFER_CLOUDS[clouds]
        x, y, args, kw = C.chamfer_inputs(name)
        norm = kwargs.get("norm", 2)
        idx_x = C.brute64(x.detach(), y.detach(), l1, l2, 1, norm)[0][..., 0]
        idx_y = C.brute64(y.detach(), x.detach(), l2, l1, 1, norm)[0][..., 0]
        xd, yd = x.detach().double().requires_grad_(True), y.detach().double().requires_grad_(True)
        w = None if weights is None else torch.tensor(weights, dtype=torch.float64)
        restate = dict(weights=w, point_reduction=kwargs.get("point_reduction", "mean"), batch_reduction=kwargs.get("batch_reduction", "mean"),
                       norm=norm, single_directional=kwargs.get("single_directional", False))
        loss = C.chamfer_restated(xd, yd, l1, l2, idx_x, idx_y, **restate)
        gx, gy = torch.autograd.grad(C.scalarise((loss, None)), (xd, yd), allow_unused=True)
        gy = torch.zeros_like(yd) if gy is None else gy
        per = C.chamfer_restated(xd.detach(), yd.detach(), l1, l2, idx_x, idx_y, **dict(restate, batch_reduction=None))
        scale = 1.0
        if restate["batch_reduction"] == "mean":
            scale = 1.0 / (float(w.sum()) if w is not None else N)
        S = float(per.abs().sum()) * scale if restate["batch_reduction"] is not None else float(per.abs().max())
        f32 = p3d.chamfer_distance(*args, **kw)
        fx, fy = torch.autograd.grad(C.scalarise(f32), (x, y), allow_unused=True)
        fy = torch.zeros_like(y) if fy is None else fy
        out[name] = dict(loss=loss.detach(), gx=gx, gy=gy, S=S, n=max(P1, P2),
                         e_loss=float((f32[0].detach().double() - loss.detach()).abs().max()),
                         e_gx=float((fx.double() - gx).abs().max()), e_gy=float((fy.double() - gy).abs().max()))
    return out


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("name", FUSED_CASES)
def test_fused_chamfer_loss_and_gradients_within_the_gates(chamfer_truths, name, ordered):
    import pytorch3d_amd as p3d

    t = chamfer_truths[name]
    x, y, args, kw = C.chamfer_inputs(name, device=_dev())
    with _flag(ordered):
        result = p3d.chamfer_distance(*args, **kw)
        assert result[1] is None and type(result[0].grad_fn).__name__ == "_ChamferFusedBackward"
        gx, gy = torch.autograd.grad(C.scalarise(result), (x, y), allow_unused=True)
    gy = torch.zeros_like(y) if gy is None else gy
    err = float((result[0].detach().cpu().double() - t["loss"]).abs().max())
    gate = 4 * t["e_loss"] + C.tree_depth(t["n"]) * 2.0 ** -24 * t["S"]
    e_gx, e_gy = float((gx.cpu().double() - t["gx"]).abs().max()), float((gy.cpu().double() - t["gy"]).abs().max())
    print(name, "ordered" if ordered else "atomic", "loss error %.3g gate %.3g" % (err, gate),
          "grad_x %.3g (float32 formulation %.3g)" % (e_gx, t["e_gx"]), "grad_y %.3g (%.3g)" % (e_gy, t["e_gy"]))
    assert err <= gate
    assert e_gx <= 4 * t["e_gx"]
    assert e_gy <= 4 * t["e_gy"]


def test_fused_chamfer_is_the_same_on_two_runs_under_the_flag_and_never_waits_for_the_device():
    import pytorch3d_amd as p3d

    def run():
        x, y, args, kw = C.chamfer_inputs("red_mean_mean", device=_dev())
        loss, _ = p3d.chamfer_distance(*args, **kw)
        return (loss.detach(),) + torch.autograd.grad(loss, (x, y))

    with _flag(True):
        first, again = run(), run()
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    # without weights nothing reads a value back, lengths given or not.  The forwards and the backwards are watched in two separate
    # regions (torch's sync debug mode is process-wide; the backward runs on the autograd engine's thread), each on work that has run
    # once before, so that no first-use initialisation falls into a watched region.
    x, y, args, kw = C.chamfer_inputs("red_mean_mean", device=_dev())
    x2, y2, args2, kw2 = C.chamfer_inputs("full2d", device=_dev())
    g = torch.ones((), device=_dev())

    def watched(fn):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            return fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
            torch.cuda.synchronize()

    def forwards():
        return (p3d.chamfer_distance(*args, **kw)[0], p3d.chamfer_distance(*args2, **kw2)[0],
                p3d.knn_points(x2.detach(), y2.detach(), K=3, return_nn=True))

    def backwards(losses):
        # autograd.grad, not .backward(): the gradients come back from the node itself; the first assignment of a leaf's .grad by the
        # engine is torch's own work and not what is watched here
        return torch.autograd.grad(losses[0], (x, y), g) + torch.autograd.grad(losses[1], (x2, y2), g)

    backwards(forwards())  # once, unwatched
    losses = watched(forwards)
    grads = watched(lambda: backwards(losses))
    assert all(torch.isfinite(t).all() and float(t.abs().max()) > 0 for t in grads) and losses[2].knn.shape == (2, 65, 3, 2)


# ---- the shim ------------------------------------------------------------------------------------------------------------------------
def test_shim_patches_knn_points_and_chamfer_distance():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    if not os.path.isdir(os.path.join(stage, "pytorch3d", "loss")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_chamfer_case.py")], capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    print(json.dumps(rec))
    assert rec["patched_everywhere"]
    assert rec["knn_idx_equal"] and rec["knn_dists_error"] <= 0.0
    for name, case in rec["chamfer"].items():
        assert case["error"] <= case["tolerance"], name
        assert case["grad_error"] <= case["grad_tolerance"], name
    assert rec["fused_calls"] == {"knn_points": 1, "chamfer_distance": 3} and rec["fallbacks_in_fused_part"] == 0
    assert rec["d5_fallback_calls"] == {"knn_points": 1, "chamfer_distance": 1} and rec["d5_fused_calls"] == 0
    assert rec["d5_matches"]
    assert rec["restored"] and rec["reference_raises_again"]
