"""csrc/knn_tree.hip on the MI355X: the tree search must return what the scan of all pairs returns, bit for bit.

Every case calls _C.knn_tree_idx and asserts
  torch.equal of idx and of dists with knn.torch_knn_forward in float32 on the same tensors (the contract's own formulation), and
  |dists - k-th smallest float64 distance| <= 4 x the worst such error of the float32 formulation on the same case, and
  zeros outside the valid rows and slots.
The shapes come from the header's two constants, LEAF (64) and FAN (8).  Cases: a ragged batch of LEAF * FAN^2 + a bit points (three
levels, a partial last leaf and a partial last inner node, a P1 that is no multiple of 64); a 12^3 lattice against itself (every
distance tied: only the strict rule and the (dist, j) queue give the formulation's indices); queries far outside and astride the box;
flat, linear, single-point, one-point, shorter-than-K and empty clouds; one far outlier; eight tight clusters with 1 % of the points
in a box 1000 times larger, the distribution that sinks a uniform grid; a NaN query and an infinite target, a whole wave of NaN
queries, and a whole wave of +inf queries with a +inf target (every lane's bound to a box is NaN there: the children's order must
stay total), these three against the all-pairs kernel.  Then the public route with knn.TREE_MIN_P2 = 256.
"""
import pytest
import torch

from pytorch3d_amd import _C, _lib, knn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LEAF, FAN = _lib.KNN_TREE_LEAF, _lib.KNN_TREE_FANOUT
P_RAGGED = LEAF * FAN * 9 + LEAF * 6 + 8  # 5000: 79 leaves (the last one of 8 points), 10 nodes above them (the last one of 7), 2, 1
CASES = {"ragged": (1, 8, 32), "ties": (1, 7, 27), "outside": (8,), "plane": (8,), "line": (8,), "point": (8,), "single": (8,),
         "short": (8,), "empty": (8,), "outlier": (8,), "clusters": (1, 8), "nonfinite": (8,), "nanwave": (8,), "infwave": (8,)}
NONFINITE = ("nonfinite", "nanwave", "infwave")


def _cloud(name):
    """(p1, p2, lengths1, lengths2) of a case on the GPU, seeded."""
    gen = torch.Generator().manual_seed(len(name) * 131 + ord(name[0]))
    rand = lambda *shape: torch.rand(*shape, generator=gen)  # noqa: E731
    l1 = l2 = None
    p1, p2 = rand(2, 300, 3), rand(2, 700, 3)
    if name == "ragged":
        p2 = rand(2, P_RAGGED, 3)
        l1, l2 = torch.tensor([300, 257]), torch.tensor([P_RAGGED, P_RAGGED - 5 * LEAF - 7])
    elif name == "ties":
        p1 = p2 = torch.cartesian_prod(*[torch.arange(12.0)] * 3)[None]
    elif name == "outside":  # the cloud shifted by 10 box sizes along x, then queries astride the box's faces
        p1 = torch.cat([p2[:, :200] + torch.tensor([10.0, 0.0, 0.0]), rand(2, 300, 3) * 2.0 - 0.5], 1)
    elif name == "plane":
        p2[:, :, 2] = 0.5
    elif name == "line":
        p2[:, :, 1:] = 0.25
    elif name == "point":
        p2 = p2[:, :1].repeat(1, 700, 1)
    elif name == "single":
        p2 = p2[:, :1]
    elif name == "short":
        p2 = p2[:, :5]
    elif name == "empty":
        l1, l2 = torch.tensor([40, 0]), torch.tensor([0, 50])
    elif name == "outlier":
        p2[:, 13] = 1.0e4
    elif name == "clusters":
        def mixed(P):
            x = rand(1, 8, 3)[:, torch.randint(0, 8, (P,), generator=gen)] + 0.01 * torch.randn(1, P, 3, generator=gen)
            return torch.where(rand(1, P, 1) < 0.01, 1000.0 * (rand(1, P, 3) - 0.5), x)
        p1, p2 = mixed(2000), mixed(20000)
    elif name == "nonfinite":
        p1[0, 17, 1] = float("nan")
        p2[1, 400, 0] = float("inf")
    elif name == "nanwave":  # 100 queries of NaN alone share key 0: the first wave of each cloud holds nothing else
        p1[:, 100:200] = float("nan")
    elif name == "infwave":  # 108 queries at +inf share the largest key: slots 192 .. 299, a whole wave of them, and a target at +inf
        p1[:, 100:208] = float("inf")
        p2[:, 400] = float("inf")
    return [None if t is None else t.to(DEV) for t in (p1, p2, l1, l2)]


@pytest.mark.parametrize("name,K", [(name, K) for name, Ks in CASES.items() for K in Ks])
def test_tree_search_is_the_formulation_bit_for_bit(name, K):
    p1, p2, l1, l2 = _cloud(name)
    N, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    idx, dists = _C.knn_tree_idx(p1, p2, l1, l2, K)
    if name in NONFINITE:  # the formulation sorts NaN and +inf distances into the slots; the kernels never select them
        want_idx, want_dists = _C.knn_points_idx(p1, p2, l1, l2, 2, K)
        assert torch.equal(idx, want_idx) and torch.equal(dists.view(torch.int32), want_dists.view(torch.int32))
        return
    want_idx, want_dists = knn.torch_knn_forward(p1, p2, l1, l2, 2, K)
    assert torch.equal(idx, want_idx)
    assert torch.equal(dists, want_dists)
    # float64: the k-th smallest distance of a brute force
    d64 = knn._pair_dists(p1.double(), p2.double(), 2)
    d64 = d64.masked_fill(torch.arange(P2, device=DEV)[None, None] >= knn._full(l2, N, P2, DEV)[:, None, None], float("inf"))
    take = min(K, P2)
    kth = torch.zeros((N, P1, K), dtype=torch.float64, device=DEV)
    kth[:, :, :take] = torch.topk(d64, take, dim=2, largest=False, sorted=True).values
    valid = knn._valid(l1, l2, N, P1, P2, K, DEV)
    own = (want_dists.double() - kth).abs()[valid]
    got = (dists.double() - kth).abs()[valid]
    print(f"{name} K={K}: formulation's worst error {own.max().item() if own.numel() else 0.0:.3e}, "
          f"tree's {got.max().item() if got.numel() else 0.0:.3e}")
    assert bool((got <= 4.0 * (own.max() if own.numel() else 0.0)).all())
    assert bool((idx[~valid] == 0).all()) and bool((dists[~valid] == 0).all())


@pytest.mark.parametrize("strict", [False, True])
def test_public_route_and_the_backward_of_the_points_route(monkeypatch, strict):
    p1, p2, l1, l2 = _cloud("ragged")
    P2 = p2.shape[1]
    calls = []
    monkeypatch.setattr(_C, "knn_tree_idx", lambda *a, _f=_C.knn_tree_idx, **k: calls.append(1) or _f(*a, **k))

    def run(threshold):
        monkeypatch.setattr(knn, "TREE_MIN_P2", threshold)
        a, b = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
        out = knn.knn_points(a, b, l1, l2, K=8)
        out.dists.sum().backward()
        return out.idx, out.dists.detach(), a.grad, b.grad

    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(strict)
    try:
        brute = run(None)
        assert not calls
        tree = run(256)
        assert len(calls) == 1
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])
    assert all(torch.equal(g, b) for g, b in zip(tree[:3], brute[:3]))  # idx, dists, grad_p1 (a gather): bit for bit
    if strict:
        assert torch.equal(tree[3], brute[3])  # the ordered sum
    else:  # float atomics in any order: m hits on a point, terms |t| <= 2 sqrt(3); a sum errs by <= m u m |t|, two differ by twice that
        hits = torch.zeros(2 * P2, device=DEV).index_add_(
            0, (tree[0] + torch.arange(2, device=DEV)[:, None, None] * P2).flatten(), torch.ones(2 * 300 * 8, device=DEV))
        assert bool(((tree[3] - brute[3]).abs() <= (2.0 * hits.reshape(2, P2, 1) ** 2 * 2.0 ** -24 * 2 * 3 ** 0.5)).all())
    # the tree goes ahead of the grid; everything else keeps its route
    monkeypatch.setattr(knn, "GRID_MIN_P2", 256)
    assert knn.TREE_MIN_P2 == 256 and knn.tree_kernel_path(p1, p2, 8, 2)
    knn.knn_points(p1, p2, l1, l2, K=8)
    assert len(calls) == 2
    monkeypatch.setattr(knn, "GRID_MIN_P2", None)
    for a, b, norm in ((p1[..., :2], p2[..., :2], 2), (p1, p2, 1), (p1, p2[:, :255], 2), (p1[:, :255], p2, 2)):
        assert not knn.tree_kernel_path(a, b, 8, norm) and knn.kernel_path(a, b, 8)
        knn.knn_points(a.contiguous(), b.contiguous(), K=8, norm=norm)
    assert len(calls) == 2
