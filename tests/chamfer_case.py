"""The cases of the nearest-neighbour / chamfer tests, shared by tests/golden/make_golden_chamfer.py (which records the reference's
results into tests/golden/chamfer_ref.npz), tests/test_cpu_chamfer.py, tests/test_gpu_chamfer.py and tests/shim_chamfer_case.py.

The fixture holds the inputs too, so nothing depends on a random generator staying the same.  Independent of the package: a float64
brute force in (dist, j) order, a float64 restatement of the distances / the chamfer loss on GIVEN indices (differentiated by
autograd) and the gates built from them.  At the end: the generated shapes of tests/test_cpu_loss_kernel_edges.py and
tests/test_gpu_loss_kernel_edges.py (seeded generators, no fixture).
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


# ---- generated shapes: every queue rung, ragged clouds over tile and wave edges, the second round of the sums and loops --------------
# (tests/test_cpu_loss_kernel_edges.py, tests/test_gpu_loss_kernel_edges.py)
EDGE_SEED = 31
# name -> (N, P1, P2, lengths1, lengths2)
EDGE_SHAPES = {
    "rungs": (4, 130, 2 * TILE + 6, [130, 64, 65, 1], [2 * TILE + 6, TILE, TILE + 1, TILE - 1]),  # clouds that scan 3, 1, 2 and 1 tiles
    "short": (3, 70, 40, [70, 1, 33], [40, 17, 5]),                                                  # K > lengths2 on the rungs 8, 16, 32
}
EDGE_KS = (1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32)  # both ends and the inside of every queue capacity 1, 2, 4, 8, 16, 32
EDGE_BACKWARD = [("rungs", K) for K in (2, 5, 9, 16, 17, 32)] + [("short", K) for K in (8, 16)]
EDGE_DN = ((3, 2), (2, 1))  # (D, norm) of the backward cases
MAX_LEFT_OUT = 0.05  # of a case's live queries may fall outside the admission (point_mesh_case.MAX_DROPPED)
STREAM_CAP = 256 * 16 * 256  # items one pass of a grid-stride loop covers (csrc/p3d_common.h: stream_blocks, 4 096 blocks of 256 threads)
BIG_P1 = STREAM_CAP + 300

_EDGE = {}


def edge_clouds(shape, D):
    """(p1, p2, lengths1, lengths2) of a generated shape: uniform in the unit cube, drawn p1 then p2 per (shape, D), D = 3 first, from
    ONE generator.  p2 beyond lengths2[n] holds copies of that cloud's own live p1 points -- decoys at distance 0: a scan that reads
    past the length finds them nearer than anything -- and p1 beyond lengths1[n] holds NaN."""
    if not _EDGE:
        gen = torch.Generator().manual_seed(EDGE_SEED)
        for name, (N, P1, P2, l1, l2) in EDGE_SHAPES.items():
            for d in (3, 2):
                p1, p2 = torch.rand(N, P1, d, generator=gen), torch.rand(N, P2, d, generator=gen)
                for n in range(N):
                    if l2[n] < P2:
                        p2[n, l2[n]:] = p1[n, torch.arange(P2 - l2[n]) % l1[n]]
                    p1[n, l1[n]:] = float("nan")
                _EDGE[(name, d)] = (p1.contiguous(), p2.contiguous(), l1, l2)
    return _EDGE[(shape, D)]


def live_rows(lengths1, N, P1):
    l1 = torch.full((N,), P1) if lengths1 is None else torch.as_tensor(lengths1).cpu()
    return torch.arange(P1)[None, :] < l1[:, None]


def admitted_queries(sorted_dists, lengths1, lengths2, K):
    """(N, P1) bool from the ascending float64 distances (N, P1, >= min(K + 1, P2)) of every query, +inf past lengths2: the live
    queries whose consecutive distances among the first min(K, len2) + 1 neighbours all differ by at least MIN_GAP relative (the rule
    smallest_gap states for a whole case, here per query)."""
    N, P1, M = sorted_dists.shape
    l2 = torch.full((N,), M, device=sorted_dists.device) if lengths2 is None else torch.as_tensor(lengths2).to(sorted_dists.device)
    k = torch.minimum(torch.clamp(l2, max=K) + 1, l2).clamp(max=M)  # neighbours looked at, per cloud
    sd = sorted_dists[:, :, :min(K + 1, M)]
    gap = (sd[:, :, 1:] - sd[:, :, :-1]) / sd[:, :, 1:]
    looked_at = torch.arange(gap.shape[2], device=sd.device)[None, None, :] < (k - 1)[:, None, None]
    ok = (gap >= MIN_GAP) | ~looked_at
    return ok.all(2) & live_rows(lengths1, N, P1).to(sd.device)


def sorted_dists64(p1, p2, lengths1, lengths2, norm, keep):
    """(idx, dists) of the first `keep` neighbours of every query in ascending (dist, j), float64, as ONE vectorised pass on the
    device of p1 (the brute force for shapes where brute64's loop over the clouds on the CPU would do, restated for the large ones):
    +inf / an arbitrary index past lengths2, whatever the row holds past lengths1."""
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    a, b = p1.double(), p2.double()
    total = None
    for c in range(D):  # (N, P1, P2) without the (N, P1, P2, D) intermediate
        d = a[:, :, c, None] - b[:, None, :, c]
        d = d * d if norm == 2 else d.abs()
        total = d if total is None else total + d
    if lengths2 is not None:
        l2 = torch.as_tensor(lengths2).to(p1.device)
        total = total.masked_fill(torch.arange(P2, device=p1.device)[None, None, :] >= l2[:, None, None], float("inf"))
    sd, sj = torch.sort(total, dim=2, stable=True)
    return sj[:, :, :keep], sd[:, :, :keep]


def brute64_device(p1, p2, lengths1, lengths2, K, norm):
    """brute64 from sorted_dists64: (idx, dists float64, admitted (N, P1)) on the device of p1, zeros in the padding."""
    N, P1, _ = p1.shape
    P2 = p2.shape[1]
    sj, sd = sorted_dists64(p1, p2, lengths1, lengths2, norm, min(K + 1, P2))
    ok = admitted_queries(sd, lengths1, lengths2, K)
    valid = valid_mask(lengths1, lengths2, N, P1, P2, K).to(p1.device)
    idx = torch.zeros((N, P1, K), dtype=torch.int64, device=p1.device)
    dists = torch.zeros((N, P1, K), dtype=torch.float64, device=p1.device)
    k = min(K, P2)
    idx[:, :, :k], dists[:, :, :k] = sj[:, :, :k], sd[:, :, :k]
    return idx.masked_fill(~valid, 0), dists.masked_fill(~valid, 0.0), ok


_EDGE_TRUTH = {}


def edge_truth(shape, D, norm, K):
    """(idx, dists float64, admitted (N, P1), live (N, P1)) of a generated knn case by brute64 -- computed once, never modified."""
    key = (shape, D, norm, K)
    if key not in _EDGE_TRUTH:
        p1, p2, l1, l2 = edge_clouds(shape, D)
        N, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
        idx, dists = brute64(p1, p2, l1, l2, K, norm)
        sd = torch.full((N, P1, min(K + 1, P2)), float("inf"), dtype=torch.float64)
        for n in range(N):
            m = min(K + 1, l2[n])
            sd[n, :l1[n], :m] = torch.sort(pair_dists64(p1[n, :l1[n]], p2[n, :l2[n]], norm), dim=1).values[:, :m]
        _EDGE_TRUTH[key] = (idx, dists, admitted_queries(sd, l1, l2, K), live_rows(l1, N, P1))
    return _EDGE_TRUTH[key]


def check_knn_forward(who, got_idx, got_dists, want_idx, want_dists, ok, live, valid):
    """The contract of the fixture test on a generated case: idx bit-equal on admitted queries, dists within 2e-6 relative on every
    valid slot, padding rows and slots exactly 0 in both, at most MAX_LEFT_OUT of the live queries outside the admission."""
    got_idx, got_dists = got_idx.to(want_idx.device), got_dists.to(want_idx.device).double()
    left_out = 1.0 - float(ok.sum()) / max(int(live.sum()), 1)
    wrong = int((got_idx != want_idx)[ok].sum())
    rel = ((got_dists - want_dists).abs() / want_dists.abs().clamp_min(1e-300))[valid]
    err = float(rel.max()) if rel.numel() else 0.0
    print("%s: %d of %d live queries admitted (left out %.2f %%, cap %.0f %%), %d wrong indices among them, dists %.3g relative (gate 2e-6)"
          % (who, int(ok.sum()), int(live.sum()), 100 * left_out, 100 * MAX_LEFT_OUT, wrong, err))
    assert left_out <= MAX_LEFT_OUT, "too many queries outside the admission"
    assert wrong == 0, "idx differs on admitted queries"
    assert float(((got_dists - want_dists).abs() - 2e-6 * want_dists.abs())[valid].max()) <= 0.0 if rel.numel() else True
    assert not bool(got_idx[~valid].any()) and not bool(got_dists[~valid].any()), "padding rows and slots are exactly 0"
    assert bool((got_idx >= 0).all()) and not bool(torch.isnan(got_dists).any())


def edge_backward_truth(p1, p2, lengths1, lengths2, idx, norm, grad_dists):
    """knn_grad_truth with the NaN of p1's padding rows taken out first (0 x NaN is NaN under autograd), and the float32 torch
    formulation's errors against it on the CPU with the SAME indices: (truth (grad_p1, grad_p2), [e_p1, e_p2])."""
    from pytorch3d_amd import knn as knn_mod

    a, b, idx, g = p1.cpu(), p2.cpu(), idx.cpu(), grad_dists.cpu()
    truth = knn_grad_truth(torch.nan_to_num(a, nan=0.0), b, lengths1, lengths2, idx, norm, g)
    f32 = knn_mod.torch_knn_backward(a, b, lengths_tensor(lengths1), lengths_tensor(lengths2), idx, norm, g)
    return truth, [float((f.double() - t).abs().max()) for f, t in zip(f32, truth)]


def check_knn_backward(who, grads, truth, e32, lengths1, lengths2):
    """Each gradient within 4 x the float32 formulation's error; the padding rows of grad_p1 and the padding points of grad_p2
    exactly 0."""
    bad = []
    for which, got, t, e in zip(("grad_p1", "grad_p2"), grads, truth, e32):
        err = float((got.cpu().double() - t).abs().max())
        print(who, which, "error %.3g" % err, "float32 formulation %.3g (gate 4 x)" % e)
        if not err <= 4 * e:
            bad.append((which, err, 4 * e))
    assert not bad, bad
    N, P1, P2 = grads[0].shape[0], grads[0].shape[1], grads[1].shape[1]
    assert not bool(grads[0].cpu()[~live_rows(lengths1, N, P1)].any()), "the gradient of a padding row is not exactly 0"
    assert not bool(grads[1].cpu()[~live_rows(lengths2, N, P2)].any()), "the gradient of a padding point is not exactly 0"


# ---- runs in the scatter ----------------------------------------------------------------------------------------------------------------
RUN_BLOCKS = (40, 1, 27, 1, 1, 50, 3, 1, 33, 1, 42)  # consecutive queries around one target: 200 in all, the target changes per block


def star_clouds_d2():
    """The star in the plane: 300 queries, one target -- ten waves of 32 hits, each one run."""
    gen = torch.Generator().manual_seed(6)
    return torch.randn(1, 300, 2, generator=gen), torch.randn(1, 1, 2, generator=gen)


def few_targets_clouds(D):
    """P1 = 200 against P2 = 3: the queries come in blocks of RUN_BLOCKS around one target each, so with K = 1 the hits in their
    order are runs of 40, 1, 27, 1, 1, 50, ... -- longer than a wave's 32 (D = 2) or 21 (D = 3) hits, across its boundary, with runs of
    one in between; with K = 2 a hit's neighbour in the order is the same query's OTHER target: runs of one and two."""
    gen = torch.Generator().manual_seed(8)
    targets = torch.tensor([[0.1, 0.2, 0.3], [0.9, 0.3, 0.6], [0.4, 0.9, 0.1]])[:, :D]
    owner = torch.cat([torch.full((n,), b % 3, dtype=torch.int64) for b, n in enumerate(RUN_BLOCKS)])
    p1 = targets[owner] + 0.1 * (torch.rand(owner.shape[0], D, generator=gen) - 0.5)
    return p1[None].contiguous(), targets[None].contiguous(), owner


def run_lengths(idx_flat):
    """The lengths of the runs of equal consecutive entries."""
    change = torch.nonzero(idx_flat[1:] != idx_flat[:-1]).squeeze(1) + 1
    edges = torch.cat([torch.zeros(1, dtype=torch.int64), change, torch.tensor([idx_flat.numel()])])
    return (edges[1:] - edges[:-1]).tolist()


def scatter_truth(p1, p2, idx, g):
    """(truth (P2, D) float64, bound): the float64 sum of what each hit adds to its target (norm 2: -2 g (x - y)) and the star's bound,
    the largest in-degree x 2^-23 x the largest term.  One cloud; idx, g (P1, K)."""
    x, y = p1[0].double(), p2[0].double()
    terms = -2.0 * g.double()[..., None] * (x[:, None, :] - y[idx])  # (P1, K, D)
    truth = torch.zeros_like(y).index_add(0, idx.reshape(-1), terms.reshape(-1, x.shape[1]))
    degree = int(torch.bincount(idx.reshape(-1), minlength=y.shape[0]).max())
    return truth, degree * 2.0 ** -23 * float(terms.abs().max()), terms


# ---- the second round of the chamfer sum ---------------------------------------------------------------------------------------------
SUM_SHAPE = (2, 16500, 40, [16500, 16385], [40, 3])  # 16 385 queries: 257 wave partials per cloud; the reverse direction scans 33 tiles
SUM_WEIGHTS = [0.5, 2.0]
SUM_CASES = [dict(point_reduction=p, batch_reduction=b, weights=w) for p in ("mean", "sum") for w in (None, SUM_WEIGHTS) for b in ("mean", None)]


def sum_case_name(D, kw):
    return "d%d_%s_%s_%s" % (D, kw["point_reduction"], kw["batch_reduction"], "weights" if kw["weights"] else "plain")


def sum_clouds(D):
    """(x, y) of SUM_SHAPE, uniform in the unit cube; the padding of each holds copies of the OTHER's live points of that cloud."""
    N, P1, P2, lx, ly = SUM_SHAPE
    gen = torch.Generator().manual_seed(EDGE_SEED + D)
    x, y = torch.rand(N, P1, D, generator=gen), torch.rand(N, P2, D, generator=gen)
    for n in range(N):
        if ly[n] < P2:
            y[n, ly[n]:] = x[n, torch.arange(P2 - ly[n]) % lx[n]]
        if lx[n] < P1:
            x[n, lx[n]:] = y[n, torch.arange(P1 - lx[n]) % ly[n]]
    return x.contiguous(), y.contiguous()


def sum_inputs(D, kw, device="cpu"):
    """(x, y leaves, keyword arguments) for chamfer_distance(x, y, **kwargs) on a device."""
    N, P1, P2, lx, ly = SUM_SHAPE
    x, y = sum_clouds(D)
    x, y = x.to(device).requires_grad_(True), y.to(device).requires_grad_(True)
    out = dict(x_lengths=lengths_tensor(lx).to(device), y_lengths=lengths_tensor(ly).to(device), point_reduction=kw["point_reduction"],
               batch_reduction=kw["batch_reduction"])
    if kw["weights"] is not None:
        out["weights"] = torch.tensor(kw["weights"], dtype=torch.float32, device=device)
    return x, y, out


_SUM_IDX, _SUM_TRUTH = {}, {}


def sum_truth(D, kw):
    name = sum_case_name(D, kw)
    if name not in _SUM_TRUTH:
        _SUM_TRUTH[name] = _sum_truth(D, kw)
    return _SUM_TRUTH[name]


def _sum_truth(D, kw):
    """As test_gpu_chamfer.chamfer_truths for one case of SUM_CASES: float64 loss and gradients on the float64 neighbours, S, n, the
    float32 CPU formulation's errors against them, and the per-cloud float64 terms of the x -> y direction (N, P1) with their
    weights and divisors (for the deliberately wrong sum of the CPU leg), and that formulation's own results under "f32".  Computed
    once per case, never modified."""
    import pytorch3d_amd as p3d

    N, P1, P2, lx, ly = SUM_SHAPE
    x, y, ckw = sum_inputs(D, kw)
    if D not in _SUM_IDX:
        _SUM_IDX[D] = (brute64(x.detach(), y.detach(), lx, ly, 1, 2)[0][..., 0], brute64(y.detach(), x.detach(), ly, lx, 1, 2)[0][..., 0])
    idx_x, idx_y = _SUM_IDX[D]
    xd, yd = x.detach().double().requires_grad_(True), y.detach().double().requires_grad_(True)
    w = None if kw["weights"] is None else torch.tensor(kw["weights"], dtype=torch.float64)
    restate = dict(weights=w, point_reduction=kw["point_reduction"], batch_reduction=kw["batch_reduction"])
    loss = chamfer_restated(xd, yd, lx, ly, idx_x, idx_y, **restate)
    gx, gy = torch.autograd.grad(scalarise((loss, None)), (xd, yd))
    per = chamfer_restated(xd.detach(), yd.detach(), lx, ly, idx_x, idx_y, **dict(restate, batch_reduction=None))
    scale = 1.0
    if kw["batch_reduction"] == "mean":
        scale = 1.0 / (float(w.sum()) if w is not None else N)
    S = float(per.abs().sum()) * scale if kw["batch_reduction"] is not None else float(per.abs().max())
    f32 = p3d.chamfer_distance(x, y, **ckw)
    fx, fy = torch.autograd.grad(scalarise(f32), (x, y))
    terms_x = dists_on_indices(xd.detach(), yd.detach(), idx_x[..., None], valid_mask(lx, ly, N, P1, P2, 1), 2)[..., 0]
    return dict(loss=loss.detach(), gx=gx, gy=gy, S=S, n=max(P1, P2), scale=scale, per=per, terms_x=terms_x,
                f32=(f32[0].detach(), fx, fy),
                e_loss=float((f32[0].detach().double() - loss.detach()).abs().max()),
                e_gx=float((fx.double() - gx).abs().max()), e_gy=float((fy.double() - gy).abs().max()))


def check_sum_case(who, t, loss, gx, gy):
    """The gates of test_fused_chamfer_loss_and_gradients_within_the_gates; returns whether all three hold (and prints them)."""
    err = float((loss.detach().cpu().double() - t["loss"]).abs().max())
    gate = 4 * t["e_loss"] + tree_depth(t["n"]) * 2.0 ** -24 * t["S"]
    e_gx, e_gy = float((gx.cpu().double() - t["gx"]).abs().max()), float((gy.cpu().double() - t["gy"]).abs().max())
    print(who, "loss error %.3g gate %.3g = 4 x %.3g + %d x 2^-24 x %.3g" % (err, gate, t["e_loss"], tree_depth(t["n"]), t["S"]),
          "grad_x %.3g (float32 formulation %.3g)" % (e_gx, t["e_gx"]), "grad_y %.3g (%.3g)" % (e_gy, t["e_gy"]))
    return err <= gate, e_gx <= 4 * t["e_gx"], e_gy <= 4 * t["e_gy"]


# ---- the second pass of the grid-stride loops ------------------------------------------------------------------------------------------
def big_clouds(D):
    """N = 1, P1 = STREAM_CAP + 300 queries against 8 targets: the gather (one lane per query) and the scatter (one lane per hit and
    coordinate) both go round their loops a second time."""
    gen = torch.Generator().manual_seed(EDGE_SEED + 10 + D)
    return torch.rand(1, BIG_P1, D, generator=gen), torch.rand(1, 8, D, generator=gen)
