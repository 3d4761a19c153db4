"""Ball query between padded point clouds on the HIP kernel of csrc/fps_ball.hip.

    ball_query(p1, p2, lengths1=None, lengths2=None, K=500, radius=0.2, return_nn=True, skip_points_outside_cube=False)
                                                                                                      pytorch3d/ops/ball_query.py

Same name, defaults, checks and return value as the reference: the namedtuple of knn_points (dists, idx, knn) with dists (N, P1, K)
squared distances, idx (N, P1, K) int64 and knn (N, P1, K, D) or None.  For each query the FIRST K points of its cloud, ascending in
index, whose squared distance is < radius^2 -- strictly, radius^2 formed in the clouds' dtype -- in the order found, not sorted by
distance.  The slots behind a row's hits and the rows past lengths1[n] hold -1 in idx and 0 in dists and knn.  One autograd node;
its backward is the nearest neighbours' (pytorch3d_amd.knn.backward_kernels, norm 2: float atomics or, under
torch.use_deterministic_algorithms(True), the ordered sum), which skips the -1 entries.  `lengths=None` never waits for the device.

`skip_points_outside_cube` is accepted and ignored: it cannot change a result.  A point outside the cube has |diff| > r in some
coordinate; rounding is monotone, so fl(diff^2) >= fl(r^2) = radius2, and adding non-negative terms never rounds below the larger
operand: the point fails `dist2 < radius2` anyway.  A NaN coordinate fails the cube test and the distance test alike.

float32 GPU tensors with D in {2, 3} take the kernel (include/p3d_amd.h).  Everything else -- CPU tensors, float64, other D --
takes the torch formulation below: the same contract with the distances of pytorch3d_amd.knn (per coordinate a subtraction, a
multiplication and an addition, never `.sum`), in float32 bit for bit what the kernel computes.
"""
import torch

from . import _C
from .knn import _KNN, CHUNK_ELEMENTS, _full, _lengths_arg, _pair_dists, torch_knn_backward
from .sample_farthest_points import masked_gather


def kernel_path(p1, p2, K=1):
    """Whether ball_query(p1, p2, K=K) runs csrc/fps_ball.hip (else: the torch formulation)."""
    return (torch.is_tensor(p1) and torch.is_tensor(p2) and p1.is_cuda and p2.is_cuda and p1.device == p2.device
            and p1.dtype == torch.float32 and p2.dtype == torch.float32 and p1.dim() == 3 and p2.dim() == 3
            and p1.shape[2] in (2, 3) and K >= 1)


def radius_squared(radius, dtype):
    """radius * radius rounded as the clouds' dtype rounds it (float32: the reference's `float radius`), as a Python float."""
    r = torch.tensor(float(radius), dtype=dtype)
    return float(r * r)


# ---- the torch formulation -------------------------------------------------------------------------------------------------------
def torch_ball_query_forward(p1, p2, lengths1, lengths2, K, radius):
    """(idx, dists) by the contract of the module docstring, any device, float dtype, D and K."""
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    dev = p1.device
    idx = torch.full((N, P1, K), -1, dtype=torch.int64, device=dev)
    dists = torch.zeros((N, P1, K), dtype=p1.dtype, device=dev)
    if N == 0 or P1 == 0 or P2 == 0 or K == 0 or D == 0:
        return idx, dists
    r2 = radius_squared(radius, p1.dtype)
    inside2 = torch.arange(P2, device=dev)[None, None, :] < _full(lengths2, N, P2, dev)[:, None, None]
    inside1 = torch.arange(P1, device=dev)[None, :] < _full(lengths1, N, P1, dev)[:, None]
    j = torch.arange(P2, device=dev)[None, None, :]
    rows = max(1, CHUNK_ELEMENTS // max(1, N * P2))
    for r0 in range(0, P1, rows):
        d = _pair_dists(p1[:, r0:r0 + rows], p2, 2)
        hit = (d < r2) & inside2 & inside1[:, r0:r0 + rows, None]
        slot = torch.cumsum(hit, dim=2) - 1  # the slot a hit takes: ascending j
        slot = torch.where(hit & (slot < K), slot, torch.full_like(slot, K))  # everything else lands in a column that is cut off
        R = d.shape[1]
        buf_i = torch.full((N, R, K + 1), -1, dtype=torch.int64, device=dev)
        buf_d = torch.zeros((N, R, K + 1), dtype=p1.dtype, device=dev)
        buf_i.scatter_(2, slot, j.expand(N, R, P2))
        buf_d.scatter_(2, slot, d)
        idx[:, r0:r0 + rows] = buf_i[:, :, :K]
        dists[:, r0:r0 + rows] = buf_d[:, :, :K]
    return idx, dists


def ball_query_op(p1, p2, lengths1, lengths2, K, radius, skip_points_outside_cube=False):
    """`pytorch3d._C.ball_query` of the shim module: the kernel where it applies, the torch formulation elsewhere.  (idx, dists)."""
    K = int(K)
    if kernel_path(p1, p2, K) and all(t is None or t.is_cuda for t in (lengths1, lengths2)):
        return _C.ball_query(p1, p2, lengths1, lengths2, K, radius, skip_points_outside_cube)
    p1, p2 = p1.contiguous(), p2.contiguous()
    if p2.dtype != p1.dtype:
        p2 = p2.to(p1.dtype)
    return torch_ball_query_forward(p1, p2, lengths1, lengths2, max(K, 0), radius)


class _BallQuery(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p1, p2, lengths1, lengths2, K, radius, fused):
        if fused:
            idx, dists = _C.ball_query(p1, p2, lengths1, lengths2, K, radius)
        else:
            idx, dists = torch_ball_query_forward(p1, p2, lengths1, lengths2, K, radius)
        ctx.save_for_backward(p1, p2, idx)
        ctx.lengths = (lengths1, lengths2)
        ctx.fused = fused
        ctx.mark_non_differentiable(idx)
        return dists, idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_dists, _grad_idx):
        p1, p2, idx = ctx.saved_tensors
        lengths1, lengths2 = ctx.lengths
        if ctx.fused:
            grad_p1, grad_p2 = _C.knn_points_backward(p1, p2, lengths1, lengths2, idx, 2, grad_dists, _needs=ctx.needs_input_grad[:2])
        else:
            grad_p1, grad_p2 = torch_knn_backward(p1, p2, lengths1, lengths2, idx, 2, grad_dists)
        return grad_p1, grad_p2, None, None, None, None, None


def ball_query(p1, p2, lengths1=None, lengths2=None, K: int = 500, radius: float = 0.2, return_nn: bool = True,
               skip_points_outside_cube: bool = False):
    """See the module docstring.  p1 (N, P1, D), p2 (N, P2, D); lengths1 / lengths2 (N,) integers or None."""
    if p1.shape[0] != p2.shape[0]:
        raise ValueError("pts1 and pts2 must have the same batch dimension.")
    if p1.shape[2] != p2.shape[2]:
        raise ValueError("pts1 and pts2 must have the same point dimension.")
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
    dists, idx = _BallQuery.apply(p1, p2, lengths1, lengths2, K, float(radius), fused)
    nn = masked_gather(p2, idx) if return_nn else None
    return _KNN(dists=dists, idx=idx, knn=nn)
