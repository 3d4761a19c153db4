"""iterative_closest_point and corresponding_points_alignment on csrc/points_alignment.hip.

    SimilarityTransform(R, T, s), ICPSolution(converged, rmse, Xt, RTs, t_history)                 the reference's named tuples
    iterative_closest_point(X, Y, init_transform=None, max_iterations=100, relative_rmse_thr=1e-6,
                            estimate_scale=False, allow_reflection=False, verbose=False)
    corresponding_points_alignment(X, Y, weights=None, estimate_scale=False, allow_reflection=False, eps=1e-9)
    apply_similarity_transform(X, R, T, s)                                                         s X R + T
    iterative_closest_point_torch(...), corresponding_points_alignment_torch(...)                  the reference's chain restated
    kernel_path(X, Y, weights=None, init_transform=None)                                           whether the kernels run

Names, defaults, checks, error texts and return values are those of pytorch3d/ops/points_alignment.py.  X and Y are padded tensors
(b, P, d) or anything with points_padded(), num_points_per_cloud() and, for the Xt of an ICPSolution, update_padded().

The reference's mask rule is kept as written: inside iterative_closest_point the weights of X are its length mask only when some
cloud is padded AND some num_points_X differs from num_points_Y; otherwise they are ones, padded rows included (a padded row is then
paired with Y[n, 0], as the reference's knn_points leaves it).  A weight enters the covariance squared, as in the reference.

The kernels take float32 GPU tensors with d == 3, no input requiring grad and sizes within int32 (`kernel_path`): one ICP iteration
is six launches and ONE 4-byte host read (the convergence flag), the 3 x 3 decomposition runs in float64 on the device, and the
transforms of all iterations are written into one history buffer that `t_history` holds views of.  Every per-cloud sum is the fixed
tree of csrc/fixed_sum.h: the same bits on every run, stream and process.  Everything else -- CPU tensors, float64, other d, an input
that requires grad, list weights -- takes the torch formulation: the reference's chain over this package's knn_points,
differentiated by autograd.  There is no backward kernel.

Deviations from the reference, kernel path only: the "low rank" warning is issued once after the loop (from a device flag) instead
of in every iteration, and the `num_points < d + 1` warning once before it; the singular values the flag looks at are those of the
float64 decomposition.  verbose=True reads the rmse of every iteration.
"""
import warnings
from typing import List, NamedTuple, Union

import torch

from . import _C
from .knn import knn_points

CALLS = {"fused": 0, "chain": 0}  # what ran (the shim's PATCH_CALLS and the tests read it)

AMBIGUOUS_ROT_SINGULAR_THR = 1e-15
SPLIT = 0  # waves per workgroup of the search: 0 lets the launch decide; tests force 1, 2, 4, 8


class SimilarityTransform(NamedTuple):
    R: torch.Tensor
    T: torch.Tensor
    s: torch.Tensor


class ICPSolution(NamedTuple):
    converged: bool
    rmse: Union[torch.Tensor, None]
    Xt: torch.Tensor
    RTs: SimilarityTransform
    t_history: List[SimilarityTransform]


_FEW_POINTS = ("The size of one of the point clouds is <= dim+1. "
               + "corresponding_points_alignment cannot return a unique rotation.")
_LOW_RANK = ("Excessively low rank of "
             + "cross-correlation between aligned point clouds. "
             + "corresponding_points_alignment cannot return a unique rotation.")
_INIT_TRANSFORM = ("The initial transformation init_transform has to be "
                   "a named tuple SimilarityTransform with elements (R, T, s). "
                   "R are dim x dim orthonormal matrices of shape "
                   "(minibatch, dim, dim), T is a batch of dim-dimensional "
                   "translations of shape (minibatch, dim) and s is a batch "
                   "of scalars of shape (minibatch,).")


def is_pointclouds(pcl):
    return hasattr(pcl, "points_padded") and hasattr(pcl, "num_points_per_cloud")


def _convert(pcl):
    """ops/utils.py convert_pointclouds_to_tensor: (padded points, num_points (b,) int64)."""
    if is_pointclouds(pcl):
        return pcl.points_padded(), pcl.num_points_per_cloud()
    if torch.is_tensor(pcl):
        return pcl, pcl.shape[1] * torch.ones(pcl.shape[0], device=pcl.device, dtype=torch.int64)
    raise ValueError("The inputs X, Y should be either Pointclouds objects or tensors.")


def wmean(x, weight=None, dim=-2, keepdim=True, eps=1e-9):
    """ops/utils.py wmean: mean(x, dim), or sum(x w, dim) / max(sum(w, dim), eps)."""
    if weight is None:
        return x.mean(dim=dim, keepdim=keepdim)
    if any(xd != wd and xd != 1 and wd != 1 for xd, wd in zip(x.shape[-2::-1], weight.shape[::-1])):
        raise ValueError("wmean: weights are not compatible with the tensor")
    return (x * weight[..., None]).sum(dim=dim, keepdim=keepdim) / weight[..., None].sum(dim=dim, keepdim=keepdim).clamp(eps)


def apply_similarity_transform(X, R, T, s):
    """s[:, None, None] * bmm(X, R) + T[:, None, :] for X (b, P, d), R (b, d, d), T (b, d), s (b,)."""
    return s[:, None, None] * torch.bmm(X, R) + T[:, None, :]


def _list_to_padded(weights):
    n = max((int(w.shape[0]) for w in weights), default=0)
    out = weights[0].new_zeros((len(weights), n)) if weights else torch.zeros((0, 0))
    for k, w in enumerate(weights):
        out[k, :w.shape[0]] = w
    return out


def _check_alignment(Xt, num_points, Yt, num_points_Y, weights, full=False):
    """The reference's checks of corresponding_points_alignment -> weights as a padded tensor or None.  full: both inputs are tensors,
    whose counts are their shapes (nothing is read from the device)."""
    if (Xt.shape != Yt.shape) or (not full and (num_points != num_points_Y).any()):
        raise ValueError(
            "Point sets X and Y have to have the same \
            number of batches, points and dimensions."
        )
    if weights is not None:
        if isinstance(weights, list):
            if any(np != w.shape[0] for np, w in zip(num_points, weights)):
                raise ValueError("number of weights should equal to the " + "number of points in the point cloud.")
            weights = _list_to_padded(weights)
        if Xt.shape[:2] != weights.shape:
            raise ValueError("weights should have the same first two dimensions as X.")
    return weights


def _differentiable(*tensors):
    return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors)


def _is_hip_f32(t, dev=None):
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and (dev is None or t.device == dev)


def kernel_path(X, Y, weights=None, init_transform=None):
    """Whether iterative_closest_point(X, Y, init_transform) / corresponding_points_alignment(X, Y, weights) run
    csrc/points_alignment.hip (else: the torch formulation)."""
    try:
        Xt, _ = _convert(X)
        Yt, _ = _convert(Y)
    except ValueError:
        return False
    if not (_is_hip_f32(Xt) and _is_hip_f32(Yt, Xt.device) and Xt.dim() == 3 and Yt.dim() == 3 and Xt.shape[2] == 3
            and Yt.shape[2] == 3 and Xt.shape[0] == Yt.shape[0] and _C.points_alignment_fits(Xt.shape[0], Xt.shape[1], Yt.shape[1])):
        return False
    extra = [weights] if weights is not None else []
    if init_transform is not None:
        try:
            extra += list(init_transform)
        except TypeError:
            return False
    if not all(_is_hip_f32(t, Xt.device) for t in extra):  # (list weights: the formulation)
        return False
    return not _differentiable(Xt, Yt, *extra)


# ---- the torch formulation: the reference's chain, restated -------------------------------------------------------------------------
def corresponding_points_alignment_torch(X, Y, weights=None, estimate_scale=False, allow_reflection=False, eps=1e-9):
    """pytorch3d/ops/points_alignment.py corresponding_points_alignment, line for line, on any device and dtype."""
    Xt, num_points = _convert(X)
    Yt, num_points_Y = _convert(Y)
    weights = _check_alignment(Xt, num_points, Yt, num_points_Y, weights)
    b, n, dim = Xt.shape
    if (num_points < Xt.shape[1]).any() or (num_points < Yt.shape[1]).any():
        mask = (torch.arange(n, dtype=torch.int64, device=Xt.device)[None] < num_points[:, None]).type_as(Xt)
        weights = mask if weights is None else mask * weights.type_as(Xt)
    Xmu = wmean(Xt, weight=weights, eps=eps)
    Ymu = wmean(Yt, weight=weights, eps=eps)
    Xc = Xt - Xmu
    Yc = Yt - Ymu
    total_weight = torch.clamp(num_points, 1)
    if weights is not None:
        Xc = Xc * weights[:, :, None]
        Yc = Yc * weights[:, :, None]
        total_weight = torch.clamp(weights.sum(1), eps)
    if (num_points < (dim + 1)).any():
        warnings.warn(_FEW_POINTS)
    XYcov = torch.bmm(Xc.transpose(2, 1), Yc)
    XYcov = XYcov / total_weight[:, None, None]
    U, S, Vh = torch.linalg.svd(XYcov)  # (torch.svd of the reference: the same decomposition, V = Vh^T)
    V = Vh.transpose(2, 1)
    if (S.abs() <= AMBIGUOUS_ROT_SINGULAR_THR).any() and not (num_points < (dim + 1)).any():
        warnings.warn(_LOW_RANK)
    E = torch.eye(dim, dtype=XYcov.dtype, device=XYcov.device)[None].repeat(b, 1, 1)
    if not allow_reflection:
        R_test = torch.bmm(U, V.transpose(2, 1))
        E[:, -1, -1] = torch.det(R_test)
    R = torch.bmm(torch.bmm(U, E), V.transpose(2, 1))
    if estimate_scale:
        trace_ES = (torch.diagonal(E, dim1=1, dim2=2) * S).sum(1)
        Xcov = (Xc * Xc).sum((1, 2)) / total_weight
        s = trace_ES / torch.clamp(Xcov, eps)
        T = Ymu[:, 0, :] - s[:, None] * torch.bmm(Xmu, R)[:, 0, :]
    else:
        T = Ymu[:, 0, :] - torch.bmm(Xmu, R)[:, 0, :]
        s = T.new_ones(b)
    return SimilarityTransform(R, T, s)


def _icp_inputs(X, Y, init_transform):
    """The reference's prologue: (Xt, num_points_X, Yt, num_points_Y, heterogeneous, init (R, T, s) or None)."""
    Xt, num_points_X = _convert(X)
    Yt, num_points_Y = _convert(Y)
    b, size_X, dim = Xt.shape
    if (Xt.shape[2] != Yt.shape[2]) or (Xt.shape[0] != Yt.shape[0]):
        raise ValueError("Point sets X and Y have to have the same " + "number of batches and data dimensions.")
    if is_pointclouds(X) or is_pointclouds(Y):  # (tensors are full: no read of the device)
        heterogeneous = bool(((num_points_Y < Yt.shape[1]).any() or (num_points_X < Xt.shape[1]).any())
                             and (num_points_Y != num_points_X).any())
    else:
        heterogeneous = False
    init = None
    if init_transform is not None:
        try:
            R, T, s = init_transform
            assert (R.shape == torch.Size((b, dim, dim)) and T.shape == torch.Size((b, dim)) and s.shape == torch.Size((b,)))
        except Exception:
            raise ValueError(_INIT_TRANSFORM) from None
        init = (R, T, s)
    return Xt, num_points_X, Yt, num_points_Y, heterogeneous, init


def iterative_closest_point_torch(X, Y, init_transform=None, max_iterations=100, relative_rmse_thr=1e-6, estimate_scale=False,
                                  allow_reflection=False, verbose=False, _record=None):
    """pytorch3d/ops/points_alignment.py iterative_closest_point, line for line, over this package's knn_points.  _record (not part
    of the reference's signature): a list that receives the neighbour indices (b, P1) of every iteration."""
    Xt, num_points_X, Yt, num_points_Y, heterogeneous, init = _icp_inputs(X, Y, init_transform)
    b, size_X, dim = Xt.shape
    if heterogeneous:
        mask_X = (torch.arange(size_X, dtype=torch.int64, device=Xt.device)[None] < num_points_X[:, None]).type_as(Xt)
    else:
        mask_X = Xt.new_ones(b, size_X)
    Xt_init = Xt.clone()
    if init is not None:
        R, T, s = init
        Xt = apply_similarity_transform(Xt, R, T, s)
    else:
        R = torch.eye(dim, device=Xt.device, dtype=Xt.dtype)[None].repeat(b, 1, 1)
        T = Xt.new_zeros((b, dim))
        s = Xt.new_ones(b)
    prev_rmse = None
    rmse = None
    iteration = -1
    converged = False
    t_history = []
    for iteration in range(max_iterations):
        nn = knn_points(Xt, Yt, lengths1=num_points_X, lengths2=num_points_Y, K=1, return_nn=True)
        if _record is not None:
            _record.append(nn.idx[:, :, 0])
        Xt_nn_points = nn.knn[:, :, 0, :]
        R, T, s = corresponding_points_alignment_torch(Xt_init, Xt_nn_points, weights=mask_X, estimate_scale=estimate_scale,
                                                       allow_reflection=allow_reflection)
        Xt = apply_similarity_transform(Xt_init, R, T, s)
        t_history.append(SimilarityTransform(R, T, s))
        Xt_sq_diff = torch.square(Xt - Xt_nn_points).sum(2)
        rmse = wmean(Xt_sq_diff[:, :, None], mask_X).sqrt()[:, 0, 0]
        if prev_rmse is None:
            relative_rmse = rmse.new_ones(b)
        else:
            relative_rmse = (prev_rmse - rmse) / prev_rmse
        if verbose:
            print(f"ICP iteration {iteration}: mean/max rmse = " + f"{rmse.mean():1.2e}/{rmse.max():1.2e} "
                  + f"; mean relative rmse = {relative_rmse.mean():1.2e}")
        if (relative_rmse <= relative_rmse_thr).all():
            converged = True
            break
        prev_rmse = rmse
    if verbose:
        if converged:
            print(f"ICP has converged in {iteration + 1} iterations.")
        else:
            print(f"ICP has not converged in {max_iterations} iterations.")
    if is_pointclouds(X):
        Xt = X.update_padded(Xt)
    return ICPSolution(converged, rmse, Xt, SimilarityTransform(R, T, s), t_history)


# ---- the kernels -------------------------------------------------------------------------------------------------------------------
def _alignment_fused(Xt, num_points, Yt, weights, estimate_scale, allow_reflection, eps, padded):
    CALLS["fused"] += 1
    b, n, dim = Xt.shape
    few = n < dim + 1 or (padded is not False and bool((num_points < (dim + 1)).any()))
    if few:
        warnings.warn(_FEW_POINTS)
    mask_len = num_points if padded is not False else None  # (a mask of ones where no cloud is padded: the same weights)
    R, T, s, status = _C.points_alignment(Xt.detach(), Yt.detach(), mask_len, None if weights is None else weights.detach(),
                                          estimate_scale, allow_reflection, eps)
    if not few and int(status[1]):
        warnings.warn(_LOW_RANK)
    return SimilarityTransform(R, T, s)


def corresponding_points_alignment(X, Y, weights=None, estimate_scale=False, allow_reflection=False, eps=1e-9):
    """pytorch3d.ops.corresponding_points_alignment: the similarity transform (R, T, s) with s X R + T = Y in the least squares sense
    (Umeyama).  See the module docstring."""
    if not kernel_path(X, Y, weights):
        CALLS["chain"] += 1
        return corresponding_points_alignment_torch(X, Y, weights, estimate_scale, allow_reflection, eps)
    Xt, num_points = _convert(X)
    Yt, num_points_Y = _convert(Y)
    padded = None if (is_pointclouds(X) or is_pointclouds(Y)) else False  # tensors are full: nothing is read from the device
    weights = _check_alignment(Xt, num_points, Yt, num_points_Y, weights, full=padded is False)
    return _alignment_fused(Xt, num_points, Yt, weights, estimate_scale, allow_reflection, eps, padded)


def _icp_fused(X, Xt, num_points_X, Yt, num_points_Y, heterogeneous, init, max_iterations, relative_rmse_thr, estimate_scale,
               allow_reflection, verbose):
    CALLS["fused"] += 1
    b, size_X, dim = Xt.shape
    dev = Xt.device
    Xt_init = Xt.detach().contiguous()
    Yt = Yt.detach().contiguous()
    clouds = is_pointclouds(X), num_points_Y is not None
    lengths1 = num_points_X.to(device=dev, dtype=torch.int64).contiguous() if clouds[0] else None
    lengths2 = num_points_Y.to(device=dev, dtype=torch.int64).contiguous() if clouds[1] else None
    mask_len = lengths1 if heterogeneous else None
    M = int(max_iterations)
    # the transforms and the rmse of every iteration: one buffer, t_history holds views of it
    hist_R = torch.empty((M, b, 3, 3), dtype=torch.float32, device=dev)
    hist_T = torch.empty((M, b, 3), dtype=torch.float32, device=dev)
    hist_s = torch.empty((M, b), dtype=torch.float32, device=dev)
    hist_rmse = torch.empty((M, b), dtype=torch.float32, device=dev)
    idx = torch.empty((b, size_X), dtype=torch.int64, device=dev)
    out = torch.empty((b, size_X, 3), dtype=torch.float32, device=dev)
    status = torch.zeros((2,), dtype=torch.int32, device=dev)
    ws = _C.icp_workspace(b, size_X, dev)
    current = None if init is None else tuple(t.detach().to(torch.float32).contiguous() for t in init)
    if size_X < dim + 1:
        warnings.warn(_FEW_POINTS)
    converged = False
    it = -1
    for it in range(M):
        _C.icp_iteration(ws, Xt_init, Yt, lengths1, lengths2, mask_len, current, hist_rmse[it - 1] if it else None, SPLIT, estimate_scale,
                         allow_reflection, relative_rmse_thr, hist_R[it], hist_T[it], hist_s[it], idx, out, hist_rmse[it], status)
        current = (hist_R[it], hist_T[it], hist_s[it])
        if verbose:
            rmse = hist_rmse[it]
            relative = torch.ones_like(rmse) if it == 0 else (hist_rmse[it - 1] - rmse) / hist_rmse[it - 1]
            print(f"ICP iteration {it}: mean/max rmse = " + f"{rmse.mean():1.2e}/{rmse.max():1.2e} "
                  + f"; mean relative rmse = {relative.mean():1.2e}")
        if int(status[0]):  # the iteration's one host read: 4 bytes
            converged = True
            break
    if verbose:
        print(f"ICP has converged in {it + 1} iterations." if converged else f"ICP has not converged in {max_iterations} iterations.")
    if size_X >= dim + 1 and int(status[1]):
        warnings.warn(_LOW_RANK)
    t_history = [SimilarityTransform(hist_R[k], hist_T[k], hist_s[k]) for k in range(it + 1)]
    Xt_out = X.update_padded(out) if is_pointclouds(X) else out
    return ICPSolution(converged, hist_rmse[it], Xt_out, t_history[-1], t_history)


def iterative_closest_point(X, Y, init_transform=None, max_iterations=100, relative_rmse_thr=1e-6, estimate_scale=False,
                            allow_reflection=False, verbose=False):
    """pytorch3d.ops.iterative_closest_point: see the module docstring."""
    if not kernel_path(X, Y, None, init_transform) or int(max_iterations) <= 0:
        # (max_iterations = 0 runs nothing: the formulation's prologue answers it as the reference does)
        CALLS["chain"] += 1
        return iterative_closest_point_torch(X, Y, init_transform, max_iterations, relative_rmse_thr, estimate_scale, allow_reflection,
                                             verbose)
    Xt, num_points_X, Yt, num_points_Y, heterogeneous, init = _icp_inputs(X, Y, init_transform)
    return _icp_fused(X, Xt, num_points_X, Yt, num_points_Y if is_pointclouds(Y) else None, heterogeneous, init, max_iterations,
                      relative_rmse_thr, estimate_scale, allow_reflection, verbose)
