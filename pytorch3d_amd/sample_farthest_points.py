"""Farthest point sampling of padded point clouds on the HIP kernels of csrc/fps_ball.hip.

    sample_farthest_points(points, lengths=None, K=50, random_start_point=False, *, start_idxs=None)
    masked_gather(points, idx)                                                       pytorch3d/ops/sample_farthest_points.py, utils.py

Same names, defaults, checks and return values as the reference: (selected_points (N, max_K, D), idx (N, max_K) int64).  Row n of idx
holds min(K[n], lengths[n]) indices: the start index, then again and again the point with the LARGEST minimum squared distance to
the points chosen so far -- equal minima go to the LOWEST index, so a cloud of coinciding points repeats index 0 -- and -1 behind
them; selected_points holds zeros there.  A cloud without points, or with K[n] = 0, is a row of -1 (the reference writes index 0
into its first entry).  The randomness is an input: `start_idxs=` (N,) gives every cloud's first index; without it
`random_start_point` draws them exactly as the reference does.  An int K costs no host sync; a tensor K is read once for max(K).

float32 GPU tensors with D in {2, 3} take the kernels (include/p3d_amd.h): one workgroup per cloud, a cloud of up to 16 384 points
in the workgroup's registers.  Everything else -- CPU tensors, float64, other D -- takes the torch formulation below: the same
contract with the same float operations in the same order (per coordinate a subtraction, a multiplication and an addition, never
`.sum`), so that in float32 it agrees with the kernels bit for bit.  Other dtypes are computed in float32, as the reference does.
The indices carry no gradient; selected_points is torch's gather of `points`.
"""
import torch

from . import _C


def masked_gather(points, idx):
    """points (N, P, D), idx (N, K) or (N, L, K) with -1 for padding -> (N, K, D) / (N, L, K, D): points[n, idx[n, ...]], zeros where
    idx is -1 (pytorch3d/ops/utils.py)."""
    if len(idx) != len(points):
        raise ValueError("points and idx must have the same batch dimension")
    if idx.ndim not in (2, 3):
        raise ValueError("idx format is not supported %s" % repr(idx.shape))
    N, P, D = points.shape
    pad = idx.eq(-1)
    if P == 0:
        return points.new_zeros(tuple(idx.shape) + (D,))
    flat = idx.masked_fill(pad, 0).reshape(N, -1, 1).expand(-1, -1, D)
    out = torch.gather(points, 1, flat).reshape(tuple(idx.shape) + (D,))
    return out.masked_fill(pad[..., None], 0.0)


def kernel_path(points):
    """Whether sample_farthest_points(points, ...) runs csrc/fps_ball.hip (else: the torch formulation)."""
    return torch.is_tensor(points) and points.is_cuda and points.dtype == torch.float32 and points.dim() == 3 and points.shape[2] in (2, 3)


# ---- the torch formulation -------------------------------------------------------------------------------------------------------
def torch_sample_farthest_points(points, lengths, K, start_idxs, max_K):
    """idx (N, max_K) int64 by the contract of the module docstring, any device, float dtype and D.  lengths, K, start_idxs: (N,)
    integer tensors or None (full clouds, max_K samples, start at 0)."""
    N, P, D = points.shape
    dev = points.device
    idx = torch.full((N, max_K), -1, dtype=torch.int64, device=dev)
    if N == 0 or P == 0 or max_K == 0:
        return idx
    length = torch.full((N,), P, dtype=torch.int64, device=dev) if lengths is None else lengths.to(dev, torch.int64).clamp(0, P)
    count = torch.full((N,), max_K, dtype=torch.int64, device=dev) if K is None else K.to(dev, torch.int64).clamp(0, max_K)
    count = torch.minimum(count, length)
    start = torch.zeros((N,), dtype=torch.int64, device=dev) if start_idxs is None else start_idxs.to(dev, torch.int64)
    sel = torch.minimum(start.clamp(min=0), (length - 1).clamp(min=0))
    ar = torch.arange(P, device=dev)
    held = ar[None, :] < length[:, None]
    # the running minimum: +inf for a held point, -1 for padding -- below every distance, and no distance (a NaN neither) is < -1
    m = torch.where(held, torch.full((N, P), float("inf"), dtype=points.dtype, device=dev), points.new_full((N, P), -1.0))
    idx[:, 0] = torch.where(count > 0, sel, torch.full_like(sel, -1))
    for s in range(1, max_K):
        last = torch.gather(points, 1, sel[:, None, None].expand(-1, 1, D))  # (N, 1, D)
        d = None
        for c in range(D):
            diff = last[:, :, c] - points[:, :, c]
            sq = diff * diff
            d = sq if d is None else d + sq
        m = torch.where(d < m, d, m)
        top = m.max(dim=1, keepdim=True).values
        sel = torch.where(m == top, ar[None, :], torch.full_like(ar, P)[None, :]).min(dim=1).values  # the first of the largest
        idx[:, s] = torch.where(s < count, sel, torch.full_like(sel, -1))
    return idx


def sample_farthest_points_op(points, lengths, K, start_idxs, max_K_known=-1):
    """`pytorch3d._C.sample_farthest_points` of the shim module: the kernels where they apply, the torch formulation elsewhere."""
    if kernel_path(points) and all(t is None or t.is_cuda for t in (lengths, K, start_idxs)):
        return _C.sample_farthest_points(points, lengths, K, start_idxs, max_K_known)
    max_K = int(max_K_known)
    if max_K < 0:
        max_K = int(K.max()) if K.numel() else 0
    return torch_sample_farthest_points(points, lengths, K, start_idxs, max(max_K, 0))


def sample_farthest_points(points, lengths=None, K=50, random_start_point: bool = False, *, start_idxs=None):
    """See the module docstring.  points (N, P, D); lengths (N,) integers or None; K an int, a list or an (N,) tensor."""
    N, P, D = points.shape
    dev = points.device
    constant_length = lengths is None
    if lengths is not None:
        if lengths.shape != (N,):
            raise ValueError("points and lengths must have same batch dimension.")
        if not lengths.is_cuda and lengths.numel() and lengths.max() > P:  # (a device tensor is clamped instead: no host sync)
            raise ValueError("A value in lengths was too large.")
        lengths = lengths.to(device=dev, dtype=torch.int64)
    if isinstance(K, int):
        max_K, K = K, None
    else:
        if isinstance(K, list):
            K = torch.tensor(K, dtype=torch.int64)
        if K.shape[0] != N:
            raise ValueError("K and points must have the same batch dimension")
        max_K = int(K.max()) if K.numel() else 0  # the one host sync of a tensor K
        K = K.to(device=dev, dtype=torch.int64)
    max_K = max(int(max_K), 0)
    if points.dtype not in (torch.float32, torch.float64):
        points = points.to(torch.float32)
    if start_idxs is not None:
        if start_idxs.shape != (N,):
            raise ValueError("points and start_idxs must have same batch dimension.")
        start_idxs = start_idxs.to(device=dev, dtype=torch.int64)
    elif random_start_point:  # drawn as pytorch3d/ops/sample_farthest_points.py:88-94 draws them
        if constant_length:
            start_idxs = torch.randint(high=P, size=(N,), device=dev)
        else:
            start_idxs = (lengths * torch.rand(lengths.size(), device=dev)).to(torch.int64)
    with torch.no_grad():
        if kernel_path(points):
            idx = _C.sample_farthest_points(points.contiguous(), lengths, K, start_idxs, max_K)
        else:
            idx = torch_sample_farthest_points(points, lengths, K, start_idxs, max_K)
    return masked_gather(points, idx), idx
