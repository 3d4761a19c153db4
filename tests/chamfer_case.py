"""The cases of the nearest-neighbour / chamfer tests, shared by tests/golden/make_golden_chamfer.py (which records the reference's
results into tests/golden/chamfer_ref.npz), tests/test_cpu_chamfer.py, tests/test_gpu_chamfer.py and tests/shim_chamfer_case.py.

The fixture holds the inputs too, so nothing depends on a random generator staying the same.  Independent of the package: a float64
brute force in (dist, j) order, a float64 restatement of the distances / the chamfer loss on GIVEN indices (differentiated by
autograd) and the gates built from them.
"""
import math
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "chamfer_ref.npz")

TILE = 512  # p2 points the kernel stages per step (include/p3d_amd.h: P3D_KNN_TILE)
MIN_GAP = 1e-5  # relative gap between consecutive distances the generator asserts on every recorded query

# name, N, P1, P2, D, lengths1, lengths2, Ks, norms
KNN_CASES = [
    ("pad", 3, 70, 130, 3, [70, 1, 33], [130, 64, 5], (1, 3, 8), (2, 1)),   # padding at K > 5, a wave edge at 64 / 65
    ("wg_edge", 2, 257, 300, 3, [257, 100], [300, 299], (1,), (2, 1)),      # more than 256 queries per cloud
    ("d2", 2, 65, 40, 2, None, None, (3,), (2, 1)),
    ("k32", 1, 40, 50, 3, None, None, (32,), (2,)),                         # the largest queue
    ("d5", 1, 40, 50, 5, None, None, (32,), (2,)),                          # torch formulation: D
    ("k33", 1, 40, 50, 3, None, None, (33,), (2,)),                         # torch formulation: K
    ("tile_m1", 1, 20, TILE - 1, 3, None, None, (1, 3), (2,)),
    ("tile", 1, 20, TILE, 3, None, None, (1, 3), (2,)),
    ("tile_p1", 1, 20, TILE + 1, 3, None, None, (1, 3), (2, 1)),
    ("tile_2p3", 1, 20, 2 * TILE + 3, 3, None, None, (1, 3), (2,)),
    ("empty", 2, 10, 7, 3, [0, 10], [7, 0], (1, 3), (2, 1)),                # a cloud with lengths1 = 0, one with lengths2 = 0
]

# the clouds of the chamfer cases: name -> (N, P1, P2, D, lengths1, lengths2)
CHAMFER_CLOUDS = {
    "base": (3, 70, 130, 3, [70, 1, 33], [130, 64, 5]),
    "full2d": (2, 65, 40, 2, None, None),
    "hetero": (3, 33, 50, 3, [20, 0, 33], [50, 17, 5]),  # handed over as Pointclouds-shaped objects; cloud 1 of x is empty
}
_W = [0.5, 2.0, 1.25]
_PAIRS = [(p, b) for p in ("mean", "sum", "max", None) for b in ("mean", "sum", None) if not (p is None and b is not None)]
# name, clouds, normals, weights, as objects, keyword arguments of chamfer_distance
CHAMFER_CASES = (
    [("red_%s_%s" % (p, b), "base", False, None, False, dict(point_reduction=p, batch_reduction=b)) for p, b in _PAIRS]
    + [("weights_mean", "base", False, _W, False, {}),
       ("weights_sum_none", "base", False, _W, False, dict(point_reduction="sum", batch_reduction=None)),
       ("weights_zero", "base", False, [0.0, 0.0, 0.0], False, {}),
       ("normals_abs", "base", True, None, False, {}),
       ("normals_signed", "base", True, None, False, dict(abs_cosine=False)),
       ("normals_none_none", "base", True, _W, False, dict(point_reduction=None, batch_reduction=None)),
       ("single", "base", False, None, False, dict(single_directional=True)),
       ("single_normals", "base", True, None, False, dict(single_directional=True, point_reduction="sum")),
       ("l1_mean", "base", False, None, False, dict(norm=1)),
       ("l1_sum_weights", "base", False, _W, False, dict(norm=1, point_reduction="sum", batch_reduction="sum")),
       ("full2d", "full2d", False, None, False, {}),
       ("full2d_l1", "full2d", False, None, False, dict(norm=1, batch_reduction=None)),
       ("hetero", "hetero", False, None, True, {}),
       ("hetero_normals", "hetero", True, None, True, dict(batch_reduction="sum"))])


def knn_key(name, what, K=None, norm=None):
    return "knn/%s/%s" % (name, what) if K is None else "knn/%s/K%d_n%d/%s" % (name, K, norm, what)


def cham_key(name, what):
    return "cham/%s/%s" % (name, what)


_LOADED = {}


def fixture():
    if "z" not in _LOADED:
        with np.load(FIXTURE) as z:
            _LOADED["z"] = {k: torch.from_numpy(z[k]) for k in z.files}
    return _LOADED["z"]


def lengths_tensor(lengths):
    return None if lengths is None else torch.tensor(lengths, dtype=torch.int64)


class Clouds:
    """Anything with points_padded / num_points_per_cloud / normals_padded: what chamfer_distance takes besides tensors."""

    def __init__(self, points, lengths, normals=None):
        self._points, self._lengths, self._normals = points, lengths, normals

    def points_padded(self):
        return self._points

    def num_points_per_cloud(self):
        return self._lengths

    def normals_padded(self):
        return self._normals


def chamfer_inputs(name, device="cpu", dtype=torch.float32, requires_grad=True):
    return chamfer_inputs_from(fixture(), name, device, dtype, requires_grad)


def chamfer_inputs_from(z, name, device="cpu", dtype=torch.float32, requires_grad=True):
    """(x, y, (first, second), kwargs) of a chamfer case: chamfer_distance(first, second, **kwargs); x / y are the leaves behind
    first / second (the tensors themselves, or the tensors inside the Clouds objects).  z: the fixture (or the generator's inputs)."""
    _, clouds, normals, weights, as_objects, kwargs = next(c for c in CHAMFER_CASES if c[0] == name)
    N, P1, P2, D, l1, l2 = CHAMFER_CLOUDS[clouds]
    x = z["clouds/%s/x" % clouds].to(device=device, dtype=dtype).requires_grad_(requires_grad)
    y = z["clouds/%s/y" % clouds].to(device=device, dtype=dtype).requires_grad_(requires_grad)
    xn = z["clouds/%s/xn" % clouds].to(device=device, dtype=dtype) if normals else None
    yn = z["clouds/%s/yn" % clouds].to(device=device, dtype=dtype) if normals else None
    l1 = None if l1 is None else lengths_tensor(l1).to(device)
    l2 = None if l2 is None else lengths_tensor(l2).to(device)
    kw = dict(kwargs)
    if weights is not None:
        kw["weights"] = torch.tensor(weights, dtype=dtype, device=device)
    if as_objects:
        return x, y, (Clouds(x, l1, xn), Clouds(y, l2, yn)), kw
    kw.update(x_lengths=l1, y_lengths=l2, x_normals=xn, y_normals=yn)
    return x, y, (x, y), kw


def flatten(result):
    """The tensors of chamfer_distance's (loss, loss_normals) in a fixed order: tuples opened, None dropped."""
    out = []
    for part in result:
        if part is None:
            continue
        out.extend(part if isinstance(part, (tuple, list)) else [part])
    return out


def scalarise(result):
    """One scalar that weighs every output entry differently (cos of its position), for the gradients."""
    total = 0.0
    for i, t in enumerate(flatten(result)):
        w = torch.cos(torch.arange(t.numel(), dtype=torch.float64) + i).to(device=t.device, dtype=t.dtype).reshape(t.shape)
        total = total + (t * w).sum()
    return total


# ---- float64 brute force and restatements ------------------------------------------------------------------------------------------
def pair_dists64(p1, p2, norm):
    d = p1.double()[:, None, :] - p2.double()[None, :, :]
    return (d * d).sum(2) if norm == 2 else d.abs().sum(2)


def brute64(p1, p2, lengths1, lengths2, K, norm):
    """(idx, dists float64) by the contract: ascending (dist, j), zeros in the padding.  p1, p2 CPU tensors of any float type (the
    distances are those of the float32 VALUES, taken in float64)."""
    N, P1, _ = p1.shape
    P2 = p2.shape[1]
    idx = torch.zeros((N, P1, K), dtype=torch.int64)
    dists = torch.zeros((N, P1, K), dtype=torch.float64)
    for n in range(N):
        n1 = P1 if lengths1 is None else int(lengths1[n])
        n2 = P2 if lengths2 is None else int(lengths2[n])
        k = min(K, n2)
        if n1 == 0 or k == 0:
            continue
        d = pair_dists64(p1[n, :n1], p2[n, :n2], norm)
        sd, sj = torch.sort(d, dim=1, stable=True)
        idx[n, :n1, :k], dists[n, :n1, :k] = sj[:, :k], sd[:, :k]
    return idx, dists


def smallest_gap(p1, p2, lengths1, lengths2, K, norm):
    """The smallest relative gap between consecutive distances among each query's first min(K, len2) + 1 neighbours (float64)."""
    N, P1, _ = p1.shape
    P2 = p2.shape[1]
    worst = math.inf
    for n in range(N):
        n1 = P1 if lengths1 is None else int(lengths1[n])
        n2 = P2 if lengths2 is None else int(lengths2[n])
        k = min(min(K, n2) + 1, n2)
        if n1 == 0 or k < 2:
            continue
        sd = torch.sort(pair_dists64(p1[n, :n1], p2[n, :n2], norm), dim=1).values[:, :k]
        worst = min(worst, float(((sd[:, 1:] - sd[:, :-1]) / sd[:, 1:]).min()))
    return worst


def valid_mask(lengths1, lengths2, N, P1, P2, K):
    l1 = torch.full((N,), P1) if lengths1 is None else torch.as_tensor(lengths1).cpu()
    l2 = torch.full((N,), P2) if lengths2 is None else torch.as_tensor(lengths2).cpu()
    return (torch.arange(P1)[None, :, None] < l1[:, None, None]) & (torch.arange(K)[None, None, :] < l2[:, None, None])


def dists_on_indices(p1, p2, idx, valid, norm):
    """(N, P1, K) distances to the points idx names, 0 where not valid; differentiable, in the dtype of p1."""
    N, P1, K = idx.shape
    D = p1.shape[2]
    near = torch.gather(p2, 1, idx.reshape(N, P1 * K, 1).expand(-1, -1, D)).reshape(N, P1, K, D)
    diff = p1[:, :, None, :] - near
    d = (diff * diff).sum(3) if norm == 2 else diff.abs().sum(3)
    return d * valid.to(d.dtype)


def knn_grad_truth(p1, p2, lengths1, lengths2, idx, norm, grad_dists):
    """float64 (grad_p1, grad_p2) of sum(dists * grad_dists) on the given indices."""
    a, b = p1.detach().double().cpu().requires_grad_(True), p2.detach().double().cpu().requires_grad_(True)
    N, P1, K = idx.shape
    valid = valid_mask(lengths1, lengths2, N, P1, p2.shape[1], K)
    d = dists_on_indices(a, b, idx.cpu(), valid, norm)
    return torch.autograd.grad((d * grad_dists.double().cpu()).sum(), (a, b))


def chamfer_restated(x, y, lx, ly, idx_x, idx_y, weights=None, point_reduction="mean", batch_reduction="mean", norm=2,
                     single_directional=False):
    """chamfer_distance without normals on GIVEN nearest-neighbour indices (idx_x (N, P1), idx_y (N, P2)), in the dtype of x:
    point_reduction "sum" / "mean" only.  Also returns S, the sum of the absolute terms of the whole loss (for the sum tree's bound)."""
    N = x.shape[0]

    def direction(a, b, la, lb, idx):
        P = a.shape[1]
        valid = valid_mask(la, lb, N, P, b.shape[1], 1)
        d = dists_on_indices(a, b, idx[..., None], valid, norm)[..., 0]
        if weights is not None:
            d = d * weights.to(d.dtype)[:, None]
        s = d.sum(1)
        if point_reduction == "mean":
            s = s / (torch.full((N,), float(max(P, 1)), dtype=d.dtype) if la is None else torch.as_tensor(la).clamp(min=1).to(d.dtype))
        return s

    per = direction(x, y, lx, ly, idx_x)
    if not single_directional:
        per = per + direction(y, x, ly, lx, idx_y)
    if batch_reduction is None:
        return per
    out = per.sum()
    if batch_reduction == "mean":
        out = out / (weights.sum().to(out.dtype) if weights is not None else max(N, 1))
    return out


def tree_depth(n):
    """Additions a term passes through in the per-cloud sum of n terms (include/p3d_amd.h)."""
    return 6 + math.ceil(math.ceil(n / 64) / 256) + 8


# ---- exact ties and the star ---------------------------------------------------------------------------------------------------------
def tie_clouds():
    """p2: 24 lattice points, every one twice (j and j + 24 are the same point); p1: the midpoints of lattice neighbours -- equidistant
    from two DIFFERENT p2 points, exactly, in float32 -- and some of the lattice points themselves (distance 0 to a duplicated pair)."""
    base = torch.tensor([[i, j, k] for i in range(4) for j in range(3) for k in range(2)], dtype=torch.float32) * 0.5
    p2 = torch.cat([base, base], 0)[None]
    mids = (base[:-1] + base[1:]) / 2  # exact: halves of small integers
    p1 = torch.cat([mids, base[::3]], 0)[None]
    return p1.contiguous(), p2.contiguous()


def star_clouds():
    """P2 = 1, P1 = 300: every query hits the one point (the worst case of the scatter)."""
    gen = torch.Generator().manual_seed(5)
    return torch.randn(1, 300, 3, generator=gen), torch.randn(1, 1, 3, generator=gen)
