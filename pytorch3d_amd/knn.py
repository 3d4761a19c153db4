"""K nearest neighbours between padded point clouds on the HIP kernels of csrc/knn.hip.

    knn_points(p1, p2, lengths1=None, lengths2=None, norm=2, K=1, version=-1, return_nn=False, return_sorted=True)
    knn_gather(x, idx, lengths=None)                                                   pytorch3d/ops/knn.py

Same names, defaults, checks and return values as the reference: a namedtuple (dists, idx, knn) with dists (N, P1, K) -- squared L2
or L1 --, idx (N, P1, K) int64 and knn (N, P1, K, D) or None.  For each query the min(K, lengths2[n]) nearest points of its cloud,
ascending by (dist, j): a tie goes to the smaller index.  Rows past lengths1[n] and slots past lengths2[n] hold 0 in both.  `version`
is accepted and ignored; the result is always sorted.  One autograd node; `lengths=None` never waits for the device.

float32 GPU tensors with D in {2, 3} and K <= 32 take the kernels (include/p3d_amd.h).  Everything else -- CPU tensors, float64,
other D, larger K -- takes the torch formulation below: the same contract, the (P1, P2) distances computed in bounded chunks,
differentiated by an explicit backward with the kernels' formulas.  The backward's scatter into grad_p2 uses float atomics, or,
under torch.use_deterministic_algorithms(True), the ordered sum of csrc/ordered_sum.h (the same bits on every run and stream).
"""
from collections import namedtuple

import torch

from . import _C, _lib

_KNN = namedtuple("KNN", "dists idx knn")

CHUNK_ELEMENTS = 1 << 22  # the torch formulation keeps at most this many distances (N x rows x P2) alive at a time


def kernel_path(p1, p2, K):
    """Whether knn_points(p1, p2, K=K) runs csrc/knn.hip (else: the torch formulation)."""
    return (torch.is_tensor(p1) and torch.is_tensor(p2) and p1.is_cuda and p2.is_cuda and p1.device == p2.device
            and p1.dtype == torch.float32 and p2.dtype == torch.float32 and p1.dim() == 3 and p2.dim() == 3
            and p1.shape[2] in (2, 3) and 1 <= K <= _lib.KNN_MAX_K)


def _lengths_arg(lengths, N, device, name):
    """None stays None (the kernels read it as `full`); a tensor becomes int64, contiguous, on the device."""
    if lengths is None:
        return None
    if lengths.dim() != 1 or lengths.shape[0] != N:
        raise ValueError(f"{name} must have shape (N,)")
    return lengths.to(device=device, dtype=torch.int64).contiguous()


def _full(lengths, N, P, device):
    return torch.full((N,), P, dtype=torch.int64, device=device) if lengths is None else lengths.clamp(0, P)


def _valid(lengths1, lengths2, N, P1, P2, K, device):
    """(N, P1, K) bool: the entries that hold a neighbour."""
    rows = torch.arange(P1, device=device)[None, :] < _full(lengths1, N, P1, device)[:, None]
    slots = torch.arange(K, device=device)[None, :] < _full(lengths2, N, P2, device)[:, None]
    return rows[:, :, None] & slots[:, None, :]


# ---- the torch formulation -------------------------------------------------------------------------------------------------------
def _pair_dists(a, b, norm):
    """a (N, R, D), b (N, P2, D) -> (N, R, P2): per coordinate the difference, squared or absolute, accumulated in coordinate order."""
    total = None
    for c in range(a.shape[2]):
        d = a[:, :, c, None] - b[:, None, :, c]
        d = d * d if norm == 2 else d.abs()
        total = d if total is None else total + d
    return total


def torch_knn_forward(p1, p2, lengths1, lengths2, norm, K):
    """(idx, dists) by the contract of the module docstring, any device, dtype, D and K."""
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    dev = p1.device
    idx = torch.zeros((N, P1, K), dtype=torch.int64, device=dev)
    dists = torch.zeros((N, P1, K), dtype=p1.dtype, device=dev)
    take = min(K, P2)
    if N == 0 or P1 == 0 or take == 0 or D == 0:
        return idx, dists
    outside = torch.arange(P2, device=dev)[None, None, :] >= _full(lengths2, N, P2, dev)[:, None, None]
    rows = max(1, CHUNK_ELEMENTS // max(1, N * P2))
    for r0 in range(0, P1, rows):
        d = _pair_dists(p1[:, r0:r0 + rows], p2, norm).masked_fill(outside, float("inf"))
        # a stable sort keeps equal distances in ascending j: the (dist, j) order
        sd, sj = torch.sort(d, dim=2, stable=True)
        dists[:, r0:r0 + rows, :take] = sd[:, :, :take]
        idx[:, r0:r0 + rows, :take] = sj[:, :, :take]
    valid = _valid(lengths1, lengths2, N, P1, P2, K, dev)
    return idx.masked_fill(~valid, 0), dists.masked_fill(~valid, 0.0)


def torch_knn_backward(p1, p2, lengths1, lengths2, idx, norm, grad_dists):
    """(grad_p1, grad_p2) by the formulas of include/p3d_amd.h (knn_cpu.cpp:101-126)."""
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    K = idx.shape[2]
    grad_p1, grad_p2 = torch.zeros_like(p1), torch.zeros_like(p2)
    if N == 0 or P1 == 0 or P2 == 0 or K == 0 or D == 0:
        return grad_p1, grad_p2
    valid = _valid(lengths1, lengths2, N, P1, P2, K, p1.device) & (idx >= 0) & (idx < P2)
    j = idx.clamp(0, P2 - 1).reshape(N, P1 * K, 1).expand(-1, -1, D)
    diff = p1[:, :, None, :] - torch.gather(p2, 1, j).reshape(N, P1, K, D)
    g = grad_dists.to(p1.dtype)[..., None]
    if norm == 2:
        t = (2.0 * g) * diff
    else:
        t = torch.where(diff > 0, g, -g)
    t = t.masked_fill(~valid[..., None], 0.0)
    for k in range(K):  # k ascending, as the gather kernel adds
        grad_p1 += t[:, :, k]
    grad_p2.scatter_add_(1, j, (-t).reshape(N, P1 * K, D))
    return grad_p1, grad_p2


# ---- the kernels -------------------------------------------------------------------------------------------------------------------
def _sorted_hits(idx, lengths1, lengths2, P2):
    """The hits of idx (N, P1, K) sorted stably by their p2 point n * P2 + j: sorted_samples of the ordered backward."""
    N, P1, K = idx.shape
    valid = _valid(lengths1, lengths2, N, P1, P2, K, idx.device) & (idx >= 0) & (idx < P2)
    key = torch.where(valid, idx + torch.arange(N, device=idx.device)[:, None, None] * P2, torch.full_like(idx, -1))
    return _C._sorted_hits(key)


def backward_kernels(p1, p2, lengths1, lengths2, idx, K, norm, grad_dists, cloud_scale, grad_p1, grad_p2, accumulate_p2=False):
    """p3d_knn_points_backward[_ordered] on torch's current stream: grad_p1 / grad_p2 are written where given (None: skipped);
    accumulate_p2 adds the hits to what grad_p2 holds.  idx (N, P1, K) or, for K = 1, (N, P1)."""
    lib, dev = _lib.load(), p1.device
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    flags = _lib.KNN_ACCUMULATE_P2 if accumulate_p2 else 0
    ordered = grad_p2 is not None and _C._ordered()
    _lib.call("p3d_knn_points_backward", "knn_points backward", dev, p1, p2, lengths1, lengths2, idx, grad_dists, cloud_scale, N, P1, P2, D, K,
              norm, flags, grad_p1, None if ordered else grad_p2)
    if ordered:
        hits = _sorted_hits(idx.reshape(N, P1, K), lengths1, lengths2, P2)
        nbytes = lib.p3d_knn_points_ordered_backward_workspace_bytes(hits.numel())
        ws = _C._workspace(nbytes, dev)
        _lib.call("p3d_knn_points_ordered_backward", "knn_points backward (ordered)", dev, p1, p2, lengths1, lengths2, idx, grad_dists,
                  cloud_scale, hits, hits.numel(), N, P1, P2, D, K, norm, flags, grad_p2, ws, nbytes)


class _KnnPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p1, p2, lengths1, lengths2, K, norm, fused):
        if fused:
            idx, dists = _C.knn_points_idx(p1, p2, lengths1, lengths2, norm, K, -1)
        else:
            idx, dists = torch_knn_forward(p1, p2, lengths1, lengths2, norm, K)
        ctx.save_for_backward(p1, p2, idx)
        ctx.lengths = (lengths1, lengths2)
        ctx.norm, ctx.fused = norm, fused
        ctx.mark_non_differentiable(idx)
        return dists, idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_dists, _grad_idx):
        p1, p2, idx = ctx.saved_tensors
        lengths1, lengths2 = ctx.lengths
        if ctx.fused:
            grad_p1, grad_p2 = _C.knn_points_backward(p1, p2, lengths1, lengths2, idx, ctx.norm, grad_dists,
                                                      _needs=ctx.needs_input_grad[:2])
        else:
            grad_p1, grad_p2 = torch_knn_backward(p1, p2, lengths1, lengths2, idx, ctx.norm, grad_dists)
        return grad_p1, grad_p2, None, None, None, None, None


def knn_points(p1, p2, lengths1=None, lengths2=None, norm: int = 2, K: int = 1, version: int = -1, return_nn: bool = False,
               return_sorted: bool = True):
    """See the module docstring.  p1 (N, P1, D), p2 (N, P2, D); lengths1 / lengths2 (N,) integers or None."""
    if p1.shape[0] != p2.shape[0]:
        raise ValueError("pts1 and pts2 must have the same batch dimension.")
    if p1.shape[2] != p2.shape[2]:
        raise ValueError("pts1 and pts2 must have the same point dimension.")
    if not ((norm == 1) or (norm == 2)):
        raise ValueError("Support for 1 or 2 norm.")
    K = int(K)
    if K < 1:
        raise ValueError("K must be at least 1.")
    p1, p2 = p1.contiguous(), p2.contiguous()
    N = p1.shape[0]
    lengths1 = _lengths_arg(lengths1, N, p1.device, "lengths1")
    lengths2 = _lengths_arg(lengths2, N, p1.device, "lengths2")
    fused = kernel_path(p1, p2, K)
    if not fused and p1.dtype != p2.dtype:
        p2 = p2.to(p1.dtype)
    dists, idx = _KnnPoints.apply(p1, p2, lengths1, lengths2, K, int(norm), fused)
    nn = knn_gather(p2, idx, lengths2) if return_nn else None
    return _KNN(dists=dists, idx=idx, knn=nn)


def knn_gather(x, idx, lengths=None):
    """x (N, M, U), idx (N, L, K) from knn_points -> (N, L, K, U) with out[n, l, k] = x[n, idx[n, l, k]], 0 in the slots
    k >= lengths[n].  No host sync: the mask is applied whether or not a cloud is short."""
    N, M, U = x.shape
    _N, L, K = idx.shape
    if N != _N:
        raise ValueError("x and idx must have same batch dimension.")
    out = torch.gather(x, 1, idx.reshape(N, L * K, 1).expand(-1, -1, U)).reshape(N, L, K, U)
    if lengths is not None:
        empty = torch.arange(K, device=x.device)[None, :] >= lengths.to(x.device)[:, None]
        out = out.masked_fill(empty[:, None, :, None], 0.0)
    return out
