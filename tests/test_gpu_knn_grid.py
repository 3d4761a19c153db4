"""csrc/knn_grid.hip on the MI355X: the grid search must return what the scan of all pairs returns, bit for bit.

Every case calls _C.knn_grid_idx with a small occupancy, so that small clouds have many cells and several rings, and asserts
  torch.equal of idx and of dists with knn.torch_knn_forward in float32 on the same tensors (the contract's own formulation), and
  |dists - k-th smallest float64 distance| <= 4 x the worst such error of the float32 formulation on the same case.
Cases: a ragged batch (several rings, a P1 that is no multiple of 64); a 7 x 7 x 7 lattice against itself (every distance tied: only
the (dist, j) queue and the strict stopping rule give the formulation's indices; run twice, the ticket order changes); queries far
outside and astride the box; flat, linear, single-point, one-point, shorter-than-K and empty clouds; points on the box's maximum faces
and on cell boundaries (multiples of 1 / 8 in a grid of side 1 / 8); one far outlier (one cell longer than the LDS tile);
1 x 5000 x 20 000 at the default occupancy (14^3 cells: many workgroups, one scan round); 1 x 1000 x 20 000 at occupancy 2 (22^3 =
10 648 cells: two scan rounds of 8192, the carry between them).  Then the public route with knn.GRID_MIN_P2 = 256.
"""
import pytest
import torch

from pytorch3d_amd import _C, knn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# name: K values, occupancy
CASES = {"ragged": ((1, 8, 32), 3), "ties": ((1, 7, 27), 2), "outside": ((8,), 3), "plane": ((8,), 2), "line": ((8,), 2),
         "point": ((8,), 2), "single": ((1, 8), 2), "short": ((8,), 2), "empty": ((8,), 2), "faces": ((1, 8), 2), "outlier": ((8,), 4),
         "large": ((8,), 0), "rounds": ((8,), 2)}


def _cloud(name):
    """(p1, p2, lengths1, lengths2) of a case on the GPU, seeded."""
    gen = torch.Generator().manual_seed(len(name) * 131 + ord(name[0]))
    rand = lambda *shape: torch.rand(*shape, generator=gen)  # noqa: E731
    l1 = l2 = None
    p1, p2 = rand(2, 300, 3), rand(2, 700, 3)
    if name == "ragged":
        l1, l2 = torch.tensor([300, 257]), torch.tensor([700, 333])
    elif name == "ties":
        p1 = p2 = torch.cartesian_prod(*[torch.arange(7.0)] * 3)[None]
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
    elif name == "faces":
        # P2 = 1024 at occupancy 2: 512 cells wanted in the box [0, 1]^3, side cbrt(1 / 512) = 1 / 8, inv_h = 8.0f (the float
        # rounding absorbs an ulp of the double cbrt) and dims ceil(1 / h) = 8 a side: (x - 0) * 8 is an exact integer at every
        # coordinate here, so floor() sits on a cell boundary for every point and the bound's B - t is 0 for queries on a face
        p1, p2 = (torch.randint(0, 9, (2, P, 3), generator=gen) / 8.0 for P in (300, 1024))
        p2[:, 0], p2[:, 1] = 0.0, 1.0  # both faces of the box on every axis
    elif name == "outlier":
        p2[:, 13] = 1.0e4
    elif name == "large":
        p1, p2 = rand(1, 5000, 3), rand(1, 20000, 3)
    elif name == "rounds":  # 10 000 cells wanted: side 0.0464, 22^3 = 10 648 cells <= the cap of 20 000
        p1, p2 = rand(1, 1000, 3), rand(1, 20000, 3)
    return [None if t is None else t.to(DEV) for t in (p1, p2, l1, l2)]


@pytest.mark.parametrize("name,K", [(name, K) for name, (Ks, _) in CASES.items() for K in Ks])
def test_grid_search_is_the_formulation_bit_for_bit(name, K):
    p1, p2, l1, l2 = _cloud(name)
    N, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    idx, dists = _C.knn_grid_idx(p1, p2, l1, l2, K, CASES[name][1])
    want_idx, want_dists = knn.torch_knn_forward(p1, p2, l1, l2, 2, K)
    assert torch.equal(idx, want_idx)
    assert torch.equal(dists, want_dists)
    if name == "ties":  # the order inside a cell differs from run to run; the result may not
        again = _C.knn_grid_idx(p1, p2, l1, l2, K, CASES[name][1])
        assert torch.equal(again[0], idx) and torch.equal(again[1], dists)
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
          f"grid's {got.max().item() if got.numel() else 0.0:.3e}")
    assert bool((got <= 4.0 * (own.max() if own.numel() else 0.0)).all())
    assert bool((idx[~valid] == 0).all()) and bool((dists[~valid] == 0).all())


@pytest.mark.parametrize("strict", [False, True])
def test_public_route_and_the_backward_of_the_points_route(monkeypatch, strict):
    p1, p2, l1, l2 = _cloud("ragged")
    calls = []
    monkeypatch.setattr(_C, "knn_grid_idx", lambda *a, _f=_C.knn_grid_idx, **k: calls.append(1) or _f(*a, **k))

    def run(threshold):
        monkeypatch.setattr(knn, "GRID_MIN_P2", threshold)
        a, b = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
        out = knn.knn_points(a, b, l1, l2, K=8)
        out.dists.sum().backward()
        return out.idx, out.dists.detach(), a.grad, b.grad

    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(strict)
    try:
        brute = run(None)
        assert not calls
        grid = run(256)
        assert len(calls) == 1
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])
    assert all(torch.equal(g, b) for g, b in zip(grid[:3], brute[:3]))  # idx, dists, grad_p1 (a gather): bit for bit
    if strict:
        assert torch.equal(grid[3], brute[3])  # the ordered sum
    else:  # float atomics in any order: m hits on a point, terms |t| <= 2 sqrt(3); a sum errs by <= m u m |t|, two differ by twice that
        hits = torch.zeros(p2.shape[:2], device=DEV).flatten().index_add_(
            0, (grid[0] + torch.arange(2, device=DEV)[:, None, None] * 700).flatten(), torch.ones(2 * 300 * 8, device=DEV))
        assert bool(((grid[3] - brute[3]).abs() <= (2.0 * hits.reshape(2, 700, 1) ** 2 * 2.0 ** -24 * 2 * 3 ** 0.5)).all())
    # everything else keeps its route
    assert knn.GRID_MIN_P2 == 256 and knn.grid_kernel_path(p1, p2, 8, 2)
    for a, b, norm in ((p1[..., :2], p2[..., :2], 2), (p1, p2, 1), (p1, p2[:, :255], 2)):
        assert not knn.grid_kernel_path(a, b, 8, norm) and knn.kernel_path(a, b, 8)
        knn.knn_points(a.contiguous(), b.contiguous(), K=8, norm=norm)
    assert len(calls) == 1
