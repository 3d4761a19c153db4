"""csrc/chamfer_normals.hip on the MI355X: chamfer_distance with normals as one autograd node.

Inputs: seeded clouds of N = 3, P1 = 130 (three query blocks, the last partial), P2 = 1100 (three LDS tiles that split unevenly over
8 slices), ragged -- an empty x cloud, an x cloud of one point, a y cloud of 5 points (fewer than 8 slices) -- with unit normals and
planted rows: a zero normal, one of norm 1e-7 (below the cosine's eps) on either side, an exactly opposite and an exactly orthogonal
pair.  Every live query keeps a relative gap >= 1e-5 between its two nearest in both directions and norms (asserted), so the
neighbours are the same in float32 and float64.
Truth: this package's general form (knn_points' torch formulation + torch arithmetic) on the CPU in float64; yardstick: the same
form in float32.  Gates, the rule of tests/test_gpu_chamfer.py: per-point terms and gradients within 4 x the float32 form's largest
error (one ulp of the largest magnitude where that error is exactly 0); a summed loss within 4 x that error + D(n) 2^-24 S, S the
float64 sum of the absolute terms -- every term is >= 0 and every divisor > 0, so S is the float64 loss itself.
"""
import itertools

import numpy as np
import pytest
import torch

import chamfer_case as C

pytestmark = pytest.mark.gpu

SEED = 3
N, P1, P2 = 3, 130, 1100
LX, LY = [130, 0, 1], [1100, 600, 5]
WEIGHTS = [0.5, 2.0, 1.25]
NODE = "_ChamferNormalsFusedBackward"
_CACHE = {}


def _dev():
    return torch.device("cuda:0")


def _inputs():
    """(x, y, xn, yn) float32 on the CPU, computed once and never modified."""
    if "in" not in _CACHE:
        gen = torch.Generator().manual_seed(SEED)
        x, y = torch.rand(N, P1, 3, generator=gen), torch.rand(N, P2, 3, generator=gen)
        xn = torch.nn.functional.normalize(torch.randn(N, P1, 3, generator=gen), dim=2)
        yn = torch.nn.functional.normalize(torch.randn(N, P2, 3, generator=gen), dim=2)
        # The planted zero and tiny normals have gradients 10^6 times the others', so their rows set the gates.  A float32 sum of
        # k > 2 such terms depends on the order, and the order of the float atomics is nobody's: these rows are placed where at most
        # two terms meet -- x's rows 0 and 1 lie outside the cube, where no point of y has them as its nearest, and the planted
        # rows of y are the neighbour of one row of x each.
        x[0, 0] += 2.0
        x[0, 1] += torch.tensor([2.0, 2.5, 3.0])
        for a, b, la, lb in ((x, y, LX, LY), (y, x, LY, LX)):
            for norm in (1, 2):
                assert C.smallest_gap(a, b, la, lb, 1, norm) >= C.MIN_GAP
        near = C.brute64(x, y, LX, LY, 1, 2)[0][0, :, 0]  # cloud 0: the neighbours of x's rows
        back = C.brute64(y, x, LY, LX, 1, 2)[0][0, :, 0]
        assert len(set(near[2:6].tolist())) == 4 and not set(near[:2].tolist()) & set(near[2:6].tolist())
        assert int((back < 2).sum()) == 0 and all(int((near == near[k]).sum()) == 1 for k in (4, 5))
        xn[0, 0] = 0.0
        xn[0, 1] *= 1e-7
        xn[0, 2] = -yn[0, near[2]]
        xn[0, 3], yn[0, near[3]] = torch.tensor([1.0, 0.0, 0.0]), torch.tensor([0.0, 1.0, 0.0])
        yn[0, near[4]] *= 1e-7
        yn[0, near[5]] = 0.0
        _CACHE["in"] = (x, y, xn, yn)
    return _CACHE["in"]


def _call(device, dtype, **kw):
    """chamfer_distance on fresh leaves: (result, the four leaves)."""
    import pytorch3d_amd as p3d

    leaves = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in _inputs()]
    if kw.pop("weights", False):
        kw["weights"] = torch.tensor(WEIGHTS, dtype=dtype, device=device)
    lx, ly = C.lengths_tensor(LX).to(device), C.lengths_tensor(LY).to(device)
    result = p3d.chamfer_distance(leaves[0], leaves[1], x_lengths=lx, y_lengths=ly, x_normals=leaves[2], y_normals=leaves[3], **kw)
    return result, leaves


def _gate(e32, truth):
    return 4 * (e32 if e32 > 0 else float(np.spacing(np.float32(truth.abs().max()))))


@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("split", [1, 2, 4, 8])
def test_neighbours_are_knn_points_bits_for_every_split(split, norm):
    from pytorch3d_amd import _C, knn_points

    x, y, xn, yn = (t.to(_dev()) for t in _inputs())
    # the second input: far point 3 of cloud 0 again as the LAST point (the last slice), with an orthogonal normal; five queries
    # next to it that carry the normal of j = 3
    x2, y2, xn2, yn2 = x.clone(), y.clone(), xn.clone(), yn.clone()
    y2[0, P2 - 1] = y2[0, 3]
    x2[0, 10:15] = y2[0, 3] + 1e-4 * torch.arange(1, 6, device=_dev())[:, None]
    yn2[0, 3], yn2[0, P2 - 1] = torch.tensor([0.0, 0.0, 1.0]), torch.tensor([1.0, 0.0, 0.0])
    xn2[0, 10:15] = yn2[0, 3]
    lx, ly = C.lengths_tensor(LX).to(_dev()), C.lengths_tensor(LY).to(_dev())
    for a, b, an, bn in ((x, y, xn, yn), (x2, y2, xn2, yn2)):
        idx_x, idx_y, (dist_x, normal_x, dist_y, _) = _C.chamfer_normals_forward(a, b, an, bn, lx, ly, norm=norm, point_reduction=None,
                                                                                 split=split)
        for idx, dist, want in ((idx_x, dist_x, knn_points(a, b, lx, ly, norm=norm)), (idx_y, dist_y, knn_points(b, a, ly, lx, norm=norm))):
            assert torch.equal(idx, want.idx[..., 0]) and torch.equal(dist, want.dists[..., 0])
    assert bool((idx_x[0, 10:15] == 3).all()) and float(normal_x[0, 10:15].abs().max()) <= 1e-6  # j = P2 - 1 would give 1
    with pytest.raises(RuntimeError, match="p3d error"):
        _C.chamfer_normals_forward(x, y, xn, yn, lx, ly, point_reduction=None, split=3)


@pytest.mark.parametrize("point_reduction,abs_cosine,single,weights", list(itertools.product(["mean", "sum", None], [True, False], [False, True], [False, True])))
def test_values_and_gradients_within_the_gates(point_reduction, abs_cosine, single, weights):
    kw = dict(point_reduction=point_reduction, batch_reduction=None if point_reduction is None else "mean", abs_cosine=abs_cosine,
              single_directional=single, weights=weights)
    runs = {}
    for who, device, dtype in (("truth", "cpu", torch.float64), ("f32", "cpu", torch.float32), ("gpu", _dev(), torch.float32)):
        result, leaves = _call(device, dtype, **kw)
        grads = torch.autograd.grad(C.scalarise(result), leaves)
        runs[who] = ([t.detach().cpu().double() for t in C.flatten(result)], [g.cpu().double() for g in grads], result)
    for t in C.flatten(runs["gpu"][2]):
        assert type(t.grad_fn).__name__ == NODE  # loss and loss_normals hang on the one node
    bad = []
    for k, (t, f, g) in enumerate(zip(*(runs[w][0] for w in ("truth", "f32", "gpu")))):
        gate = _gate(float((f - t).abs().max()), t)
        if point_reduction is not None:
            gate += C.tree_depth(max(P1, P2)) * 2.0 ** -24 * float(t.abs().sum())
        err = float((g - t).abs().max())
        print("output", k, "error %.3g gate %.3g" % (err, gate))
        bad += [("output", k, err, gate)] * (not err <= gate)
    for name, t, f, g in zip(("x", "y", "x_normals", "y_normals"), *(runs[w][1] for w in ("truth", "f32", "gpu"))):
        gate, err = _gate(float((f - t).abs().max()), t), float((g - t).abs().max())
        print("grad", name, "error %.3g gate %.3g" % (err, gate))
        bad += [("grad", name, err, gate)] * (not err <= gate)
    assert not bad, bad


def test_the_other_cases_take_what_they_took():
    import pytorch3d_amd as p3d

    x, y, xn, yn = (t.to(_dev()).requires_grad_(True) for t in _inputs())

    def names(result):
        return {type(t.grad_fn).__name__ for t in C.flatten(result)}

    assert NODE not in names(p3d.chamfer_distance(x, y, point_reduction="max"))
    assert NODE not in names(p3d.chamfer_distance(x[..., :2], y[..., :2], x_normals=xn[..., :2], y_normals=yn[..., :2]))
    one = p3d.chamfer_distance(x, y, x_normals=xn)
    assert one[1] is None and NODE not in names(one)
    assert NODE not in names(p3d.chamfer_distance(x.double(), y.double(), x_normals=xn.double(), y_normals=yn.double()))
    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(True)
    try:
        strict = p3d.chamfer_distance(x, y, x_normals=xn, y_normals=yn)
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])
    assert NODE not in names(strict) and names(p3d.chamfer_distance(x, y, x_normals=xn, y_normals=yn)) == {NODE}


def test_forward_and_backward_never_wait_for_the_device():
    import pytorch3d_amd as p3d

    g = torch.ones((), device=_dev())
    x, y, xn, yn = (t.to(_dev()).requires_grad_(True) for t in _inputs())
    lx, ly = C.lengths_tensor(LX).to(_dev()), C.lengths_tensor(LY).to(_dev())

    def run():
        loss, loss_normals = p3d.chamfer_distance(x, y, x_lengths=lx, y_lengths=ly, x_normals=xn, y_normals=yn)
        return torch.autograd.grad(loss + loss_normals, (x, y, xn, yn), g)

    run()  # first-use initialisation stays outside the watched region
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
