"""csrc/knn_features.hip on the MI355X: knn_points at 4 <= D <= 256 (matrix-instruction screen, exact rescore) and its backward.

The forward must be the float32 torch formulation (knn.torch_knn_forward on CPU copies) BIT FOR BIT, and within two derived gates of
the float64 distances g = ((a[:, :, None] - b[:, None]) ** 2).sum(-1), u = 2^-24:
  |dists - g[idx]| <= (D + 3) u g[idx]            (three roundings per term, D - 1 adds, all terms >= 0)
  |g[idx[k]] - k-th smallest g| <= 2 (D + 4) u (k-th smallest g)   (an order decided by float32 distances swaps only pairs that close)
grad_p1 is torch_knn_backward's bit for bit; an entry of grad_p2 (float atomics, any order) lies within (m + 3) u S of float64, m the
hits on that point and S the float64 sum of their absolute terms.
Shapes: 31 / 33 / 129 queries around a wave's 32 and a workgroup's 128; 31 / 33 / 65 targets around a tile's 32; D = 4, 5 (padded to
even), 9 (past the screen's chunk of 8 coordinates), 33, 179 (the first D that runs two waves per workgroup) and 256.
"""
import contextlib

import pytest
import torch

from pytorch3d_amd import _C, knn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U24 = 2.0 ** -24
# P1, P2, D, K, kind, ragged
CASES = [
    (31, 31, 4, 1, "normal", False), (33, 33, 5, 3, "normal", True), (129, 65, 33, 32, "normal", True),
    (33, 65, 256, 3, "normal", False), (129, 33, 9, 32, "normal", False), (33, 65, 179, 20, "normal", True),
    (129, 65, 64, 20, "offset", False), (31, 33, 256, 32, "offset", True), (33, 31, 5, 1, "offset", False),
    (33, 65, 179, 3, "offset", False), (129, 65, 4, 32, "lattice", False), (33, 33, 5, 3, "lattice", True),
    (31, 65, 9, 1, "lattice", False), (129, 31, 33, 3, "lattice", True), (33, 33, 33, 32, "self", False),
    (129, 129, 4, 3, "self", True), (65, 65, 256, 1, "self", False), (33, 33, 5, 32, "huge", False),
    (129, 65, 33, 3, "huge", False), (31, 31, 256, 1, "huge", False),
]
BACKWARD = [CASES[i] for i in (1, 2, 3, 5, 11, 15)]


def _inputs(P1, P2, D, K, kind, ragged):
    """(p1, p2, lengths1, lengths2) on the CPU, float32 / int64; ragged: a full cloud, lengths1 = 0, lengths2 = 0, lengths2 = 2."""
    gen = torch.Generator().manual_seed(1000 * P1 + 10 * D + K)
    N = 4 if ragged else 2
    if kind == "lattice":
        p1, p2 = (torch.randint(0, 3, (N, P, D), generator=gen).float() for P in (P1, P2))
    else:
        scale, centre = (0.01, 100.0) if kind == "offset" else (1.0, 0.0)
        p1, p2 = (torch.randn(N, P, D, generator=gen) * scale + centre for P in (P1, P2))
    if kind == "self":
        p2 = p1
    if kind == "huge":
        p2[:, 7] = 2.0 ** 64
    if not ragged:
        return p1, p2, None, None
    return p1, p2, torch.tensor([P1, 0, P1 - 3, 7]), torch.tensor([P2 - 2, P2, 0, 2])


def _gpu(*tensors):
    return [None if t is None else t.to(DEV) for t in tensors]


def _valid(p1, p2, l1, l2, K):
    N, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    return knn._valid(l1, l2, N, P1, P2, K, p1.device)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_forward_is_the_float32_formulation_and_within_the_float64_gates(case):
    P1, P2, D, K, kind, _ = case
    p1, p2, l1, l2 = _inputs(*case)
    g1, g2, gl1, gl2 = _gpu(p1, p2, l1, l2)
    if kind == "self":
        g2 = g1
    assert knn.feature_kernel_path(g1, g2, K, 2) and not knn.kernel_path(g1, g2, K)
    out = knn.knn_points(g1, g2, gl1, gl2, K=K)
    idx, dists = out.idx.cpu(), out.dists.cpu()
    want_idx, want_dists = knn.torch_knn_forward(p1, p2, l1, l2, 2, K)
    assert torch.equal(idx, want_idx)
    assert torch.equal(dists, want_dists)
    # float64
    g = ((p1.double()[:, :, None] - p2.double()[:, None]) ** 2).sum(-1)
    g = g.masked_fill(torch.arange(P2)[None, None] >= knn._full(l2, p1.shape[0], P2, "cpu")[:, None, None], float("inf"))
    valid = _valid(p1, p2, l1, l2, K)
    picked = torch.gather(g, 2, idx)
    order = torch.sort(g, dim=2, stable=True)
    take = min(K, P2)
    kth = torch.zeros_like(picked)
    kth[:, :, :take] = order.values[:, :, :take]
    assert bool((((dists.double() - picked).abs() <= (D + 3) * U24 * picked) | ~valid).all())
    assert bool((((picked - kth).abs() <= 2 * (D + 4) * U24 * kth) | ~valid).all())
    if kind == "lattice":
        assert torch.equal(idx[:, :, :take][valid[:, :, :take]], order.indices[:, :, :take][valid[:, :, :take]])


def test_every_entry_is_written_and_padding_is_zero():
    case = (33, 65, 5, 3, "normal", True)
    p1, p2, l1, l2 = _inputs(*case)
    g1, g2, gl1, gl2 = _gpu(p1, p2, l1, l2)
    idx = torch.full((4, 33, 3), -7, dtype=torch.int64, device=DEV)
    dists = torch.full((4, 33, 3), float("nan"), device=DEV)
    _C.knn_features_idx(g1, g2, gl1, gl2, 3, _out=(idx, dists))
    want_idx, want_dists = knn.torch_knn_forward(p1, p2, l1, l2, 2, 3)
    assert torch.equal(idx.cpu(), want_idx) and torch.equal(dists.cpu(), want_dists)
    valid = _valid(p1, p2, l1, l2, 3)
    assert bool((idx.cpu()[~valid] == 0).all()) and bool((dists.cpu()[~valid] == 0).all()) and bool((~valid).any())


@contextlib.contextmanager
def _deterministic():
    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])


def _grad_p2_gate(p1, p2, l1, l2, idx, grad_dists, got):
    """|got - float64| <= (m + 3) u S per entry of grad_p2, all three from scatter_adds over the float64 terms."""
    N, P1, D = p1.shape
    K = idx.shape[2]
    valid = _valid(p1, p2, l1, l2, K)
    j = idx.reshape(N, P1 * K, 1).expand(-1, -1, D)
    diff = p1.double()[:, :, None, :] - torch.gather(p2.double(), 1, j).reshape(N, P1, K, D)
    t = ((2.0 * grad_dists.double())[..., None] * diff).masked_fill(~valid[..., None], 0.0).reshape(N, P1 * K, D)
    want = torch.zeros_like(p2, dtype=torch.float64).scatter_add_(1, j, -t)
    S = torch.zeros_like(want).scatter_add_(1, j, t.abs())
    m = torch.zeros_like(want).scatter_add_(1, j, valid.double().reshape(N, P1 * K, 1).expand(-1, -1, D))
    assert bool(((got.double() - want).abs() <= (m + 3) * U24 * S).all())


@pytest.mark.parametrize("case", BACKWARD, ids=lambda c: "-".join(map(str, c)))
def test_backward_gather_is_the_formulation_and_scatter_within_its_gate(case):
    P1, P2, D, K, kind, _ = case
    p1, p2, l1, l2 = _inputs(*case)
    idx, _dists = knn.torch_knn_forward(p1, p2, l1, l2, 2, K)
    grad_dists = torch.randn(idx.shape, generator=torch.Generator().manual_seed(D))
    want_p1, _ = knn.torch_knn_backward(p1, p2, l1, l2, idx, 2, grad_dists)
    g1, g2, gl1, gl2, gidx, gg = _gpu(p1, p2, l1, l2, idx, grad_dists)
    got_p1, got_p2 = _C.knn_features_backward(g1, g2, gl1, gl2, gidx, gg)
    assert torch.equal(got_p1.cpu(), want_p1)
    _grad_p2_gate(p1, p2, l1, l2, idx, grad_dists, got_p2.cpu())


@pytest.mark.parametrize("strict", [False, True])
def test_autograd_node_and_the_deterministic_flag(strict):
    case = (129, 65, 33, 3, "normal", True)
    p1, p2, l1, l2 = _inputs(*case)
    g1, g2, gl1, gl2 = _gpu(p1, p2, l1, l2)
    g1.requires_grad_(True), g2.requires_grad_(True)
    with (_deterministic() if strict else contextlib.nullcontext()):
        out = knn.knn_points(g1, g2, gl1, gl2, K=3)
        out.dists.sum().backward()
        if strict:  # the forward is still the kernel, the backward the formulation's on the same tensors
            again = knn.torch_knn_backward(g1.detach(), g2.detach(), gl1, gl2, out.idx, 2, torch.ones_like(out.dists))
            assert torch.equal(g1.grad, again[0]) and torch.equal(g2.grad, again[1])
    idx, dists = knn.torch_knn_forward(p1, p2, l1, l2, 2, 3)
    assert torch.equal(out.idx.cpu(), idx) and torch.equal(out.dists.detach().cpu(), dists)
    assert torch.equal(g1.grad.cpu(), knn.torch_knn_backward(p1, p2, l1, l2, idx, 2, torch.ones_like(dists))[0])
    _grad_p2_gate(p1, p2, l1, l2, idx, torch.ones_like(dists), g2.grad.cpu())


def test_routing():
    a3, a5 = torch.zeros(1, 8, 3, device=DEV), torch.zeros(1, 8, 5, device=DEV)
    assert knn.kernel_path(a3, a3, 4) and not knn.feature_kernel_path(a3, a3, 4, 2)
    assert knn.feature_kernel_path(a5, a5, 32, 2) and not knn.kernel_path(a5, a5, 32)
    for p, K, norm in ((a5, 4, 1), (a5, 33, 2), (a5.double(), 4, 2), (a5.cpu(), 4, 2)):
        assert not knn.kernel_path(p, p, K) and not knn.feature_kernel_path(p, p, K, norm)
