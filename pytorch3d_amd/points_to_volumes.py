"""Point clouds added to voxel grids on the HIP kernels of csrc/points_to_volumes.hip.

    add_pointclouds_to_volumes(pointclouds, initial_volumes, mode="trilinear", min_weight=1e-4, rescale_features=True)
    add_points_features_to_volume_densities_features(points_3d, points_features, volume_densities, volume_features,
                                                     mode="trilinear", min_weight=1e-4, mask=None, grid_sizes=None,
                                                     rescale_features=True, align_corners=True)
                                                                                            pytorch3d/ops/points_to_volumes.py

Same names, defaults and return values as the reference.  The contract is the reference's COMPILED operator
(csrc/points_to_volumes/points_to_volumes_cpu.cpp, .cu), which differs from the Python twin behind its `_python=True`:

* a location on an axis is (p + 1) * 0.5 * (grid - (align_corners ? 1 : 0)) - (align_corners ? 0 : 0.5), the sum in float32 and the
  rest in float64 (the twin ignores align_corners and stays in float32);
* nearest: the float64 location rounded half AWAY from zero (lround; the twin rounds half to even);
* trilinear: the location rounded once to float32 and split by modf, which truncates TOWARD ZERO (the twin takes the floor).  A
  location in (-1, 0) therefore extrapolates: with remainder r < 0 voxel 0 receives 1 - r > 1 and voxel 1 receives r < 0.  Kept,
  because a drop-in returns what the compiled operator returns.
* a corner outside [0, grid) on any axis is skipped, a point with mask == 0 is skipped, and so is a point whose location is not
  finite or does not fit an int64 (undefined behaviour in the reference).

The volumes are modified IN PLACE through their strides (a strided view works) and contributions are added to what they hold.  One
autograd node marks both dirty; its backward is a gather per point.  float32 tensors on one GPU take the kernels: float atomics, or
under torch.use_deterministic_algorithms(True) the ordered sum (no float atomics, the same bits on every run; warn_only=True keeps
the atomics).  CPU tensors take the torch formulation below of the same contract.  Other dtypes raise, as in the reference.
"""
import torch

from . import _C

TOO_LARGE = 9.0e18  # below 2^63: a location under it converts to int64


def kernel_path(*tensors):
    """Whether these tensors run csrc/points_to_volumes.hip (else: the torch formulation)."""
    return all(torch.is_tensor(t) and t.is_cuda and t.device == tensors[0].device for t in tensors)


# ---- the torch formulation ------------------------------------------------------------------------------------------------------
_CORNERS = tuple((j >> 2, (j >> 1) & 1, j & 1) for j in range(8))  # (ux, uy, uz) in the reference's order


def _locations(points_3d, grid_sizes, align_corners):
    """(N, P, 3) float64 locations in x, y, z order and the (N, 3) grid in that order."""
    grid_xyz = grid_sizes[:, [2, 1, 0]]
    scale = (grid_xyz - (1 if align_corners else 0)).to(torch.float64)
    loc = (points_3d + 1).to(torch.float64) * 0.5 * scale[:, None, :] - (0.0 if align_corners else 0.5)
    return loc, grid_xyz


def torch_corners(points_3d, grid_sizes, mask, dims, align_corners, splat):
    """The samples of the contract: voxel (N, P, K, 3) int64 in x, y, z order (clamped to 0 where invalid), valid (N, P, K) bool and
    the axis weights (N, P, K, 3) float32, K = 8 corners in the reference's order or 1.  dims = (D, H, W) of the tensors."""
    loc, grid_xyz = _locations(points_3d, grid_sizes, align_corners)
    live = mask != 0
    if splat:
        lf = loc.to(torch.float32)
        finite = (lf.abs() < TOO_LARGE).all(dim=2)
        lf = torch.where(finite[..., None], lf, torch.zeros_like(lf))
        base = torch.trunc(lf)
        rem = lf - base
        up = torch.tensor(_CORNERS, dtype=torch.float32, device=points_3d.device)  # (8, 3)
        voxel = (base[:, :, None, :] + up).to(torch.int64)
        weights = torch.where(up.bool(), rem[:, :, None, :], (1 - rem)[:, :, None, :])
    else:
        finite = (loc.abs() < TOO_LARGE).all(dim=2)
        loc = torch.where(finite[..., None], loc, torch.zeros_like(loc))
        base = torch.trunc(loc)
        away = ((loc - base).abs() >= 0.5).to(loc.dtype) * torch.where(loc < 0, -1.0, 1.0)
        voxel = (base + away).to(torch.int64)[:, :, None, :]
        weights = torch.ones(voxel.shape, dtype=torch.float32, device=points_3d.device)
    bound = torch.minimum(grid_xyz, torch.tensor([dims[2], dims[1], dims[0]], dtype=grid_xyz.dtype, device=grid_xyz.device))
    valid = ((voxel >= 0) & (voxel < bound[:, None, None, :])).all(dim=3) & (live & finite)[:, :, None]
    voxel = torch.where(valid[..., None], voxel, torch.zeros_like(voxel))
    return voxel, valid, weights


def torch_points_to_volumes_forward(points_3d, points_features, volume_densities, volume_features, grid_sizes, mask, point_weight,
                                    align_corners, splat):
    """The forward of the contract on any device: index_put_(accumulate=True) on the (strided) volumes, in place."""
    N, P, C = points_features.shape
    voxel, valid, w = torch_corners(points_3d, grid_sizes, mask, volume_densities.shape[2:], align_corners, splat)
    weight = w[..., 0] * w[..., 1] * w[..., 2]  # float32, from the left
    n, p, k = torch.nonzero(valid, as_tuple=True)  # point-major, corners in order
    x, y, z = voxel[n, p, k].unbind(1)
    wv = weight[n, p, k]
    pw = float(point_weight)
    volume_densities[:, 0].index_put_((n, z, y, x), wv * pw, accumulate=True)
    if C > 0:
        volume_features.permute(0, 2, 3, 4, 1).index_put_((n, z, y, x), points_features[n, p] * wv[:, None] * pw, accumulate=True)


def torch_points_to_volumes_backward(points_3d, points_features, grid_sizes, mask, point_weight, align_corners, splat,
                                     grad_volume_densities, grad_volume_features, grad_points_3d, grad_points_features):
    """The backward of the contract on any device: adds to grad_points_features and, with splat, to grad_points_3d, in place."""
    N, P, C = grad_points_features.shape
    voxel, valid, w = torch_corners(points_3d, grid_sizes, mask, grad_volume_densities.shape[2:], align_corners, splat)
    K = voxel.shape[2]
    pw = float(point_weight)
    n = torch.arange(N, device=voxel.device)[:, None, None].expand(N, P, K)
    x, y, z = voxel.unbind(3)
    gvf = grad_volume_features.permute(0, 2, 3, 4, 1)[n, z, y, x]  # (N, P, K, C)
    weight = w[..., 0] * w[..., 1] * w[..., 2]
    gf = grad_points_features.clone()
    zero = torch.zeros((), dtype=gf.dtype, device=gf.device)
    for j in range(K):  # corners in order, as the reference accumulates
        gf = gf + torch.where(valid[:, :, j, None], gvf[:, :, j] * weight[:, :, j, None] * pw, zero)
    grad_points_features.copy_(gf)
    if not splat:
        return
    src = grad_volume_densities[:, 0][n, z, y, x].to(torch.float64)  # (N, P, K)
    for c in range(C):  # channels ascending: each product in float32, the sum in float64
        src = src + (points_features[:, :, None, c] * gvf[..., c]).to(torch.float64)
    scale = (grid_sizes[:, [2, 1, 0]] - (1 if align_corners else 0)).to(torch.float64)  # (N, 3)
    gp = grad_points_3d.clone()
    zero64 = torch.zeros((), dtype=torch.float64, device=gp.device)
    wd = w.to(torch.float64)
    for j, u in enumerate(_CORNERS):
        for a in range(3):
            o1, o2 = [b for b in range(3) if b != a]
            term = src[:, :, j] * (1.0 if u[a] else -1.0) * wd[:, :, j, o1] * wd[:, :, j, o2] * 0.5 * scale[:, None, a] * pw
            gp[:, :, a] = (gp[:, :, a].to(torch.float64) + torch.where(valid[:, :, j], term, zero64)).to(torch.float32)
    grad_points_3d.copy_(gp)


# ---- the operators of the shim module ----------------------------------------------------------------------------------------------
def _check_float32(**tensors):
    for name, t in tensors.items():
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32")


def _one_device(**tensors):
    devices = {t.device for t in tensors.values()}
    if len(devices) != 1:
        raise RuntimeError("Expected all tensors to be on the same device, got " + ", ".join(f"{k}: {t.device}" for k, t in tensors.items()))


def points_to_volumes_forward_op(points_3d, points_features, volume_densities, volume_features, grid_sizes, mask, point_weight,
                                 align_corners, splat):
    """`pytorch3d._C.points_to_volumes_forward` of the shim module: the reference's signature, positional, in place, no return."""
    _check_float32(points_3d=points_3d, points_features=points_features, volume_densities=volume_densities,
                   volume_features=volume_features, mask=mask)
    if grid_sizes.dtype != torch.int64:
        raise ValueError("grid_sizes must be int64")
    every = (points_3d, points_features, volume_densities, volume_features, grid_sizes, mask)
    _one_device(points_3d=points_3d, points_features=points_features, volume_densities=volume_densities,
                volume_features=volume_features, grid_sizes=grid_sizes, mask=mask)
    if kernel_path(*every):
        _C.points_to_volumes_forward(*every, point_weight, align_corners, splat)
    else:
        with torch.no_grad():
            torch_points_to_volumes_forward(*every, point_weight, align_corners, splat)
    for t in (volume_densities, volume_features):  # the writes went past autograd's version counter
        torch.autograd.graph.increment_version(t)


def points_to_volumes_backward_op(points_3d, points_features, grid_sizes, mask, point_weight, align_corners, splat, grad_volume_densities,
                                  grad_volume_features, grad_points_3d, grad_points_features):
    """`pytorch3d._C.points_to_volumes_backward` of the shim module: adds into grad_points_3d (with splat) and grad_points_features."""
    _check_float32(points_3d=points_3d, mask=mask, grad_volume_densities=grad_volume_densities,
                   grad_volume_features=grad_volume_features, grad_points_features=grad_points_features)
    if grid_sizes.dtype != torch.int64:
        raise ValueError("grid_sizes must be int64")
    every = (points_3d, points_features, grid_sizes, mask)
    grads = (grad_volume_densities, grad_volume_features, grad_points_3d, grad_points_features)
    _one_device(points_3d=points_3d, grid_sizes=grid_sizes, mask=mask, grad_volume_densities=grad_volume_densities,
                grad_volume_features=grad_volume_features, grad_points_features=grad_points_features)
    if kernel_path(points_3d, grid_sizes, mask, grad_volume_densities, grad_volume_features, grad_points_features):
        _C.points_to_volumes_backward(*every, point_weight, align_corners, splat, *grads)
    else:
        with torch.no_grad():
            torch_points_to_volumes_backward(*every, point_weight, align_corners, splat, *grads)


# ---- the autograd node ----------------------------------------------------------------------------------------------------------------
class _PointsToVolumes(torch.autograd.Function):
    """Differentiable in points_features and both volumes; with splat in points_3d too.  The volumes are the outputs, modified in
    place; their gradients are the incoming gradients themselves (the forward adds something that does not depend on them)."""

    @staticmethod
    def forward(ctx, points_3d, points_features, volume_densities, volume_features, grid_sizes, point_weight, mask, align_corners, splat):
        ctx.mark_dirty(volume_densities, volume_features)
        if points_3d.dim() != 3 or points_3d.shape[2] != 3:
            raise ValueError("points_3d must be 3D")
        N, P, _ = points_3d.shape
        if points_features.dim() != 3 or points_features.shape[:2] != (N, P):
            raise ValueError("Bad points_features shape")
        C = points_features.shape[2]
        if volume_densities.dim() != 5 or volume_densities.shape[:2] != (N, 1):
            raise ValueError("Bad volume_densities shape")
        if volume_features.shape != (N, C) + tuple(volume_densities.shape[2:]):
            raise ValueError("Bad volume_features shape")
        if grid_sizes.shape != (N, 3):
            raise ValueError("Bad grid_sizes.shape")
        if mask.shape != (N, P):
            raise ValueError("Bad mask shape")
        points_to_volumes_forward_op(points_3d, points_features, volume_densities, volume_features, grid_sizes, mask, point_weight,
                                     align_corners, splat)
        ctx.save_for_backward(points_3d, points_features if splat else None, grid_sizes, mask)
        ctx.settings = (point_weight, align_corners, splat)
        return volume_densities, volume_features

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_volume_densities, grad_volume_features):
        points_3d, points_features, grid_sizes, mask = ctx.saved_tensors
        point_weight, align_corners, splat = ctx.settings
        N, P, _ = points_3d.shape
        C = grad_volume_features.shape[1]
        grad_points_3d = torch.zeros_like(points_3d, memory_format=torch.contiguous_format) if splat else None
        grad_points_features = points_3d.new_zeros(N, P, C)
        points_to_volumes_backward_op(points_3d, points_features, grid_sizes, mask, point_weight, align_corners, splat,
                                      grad_volume_densities, grad_volume_features, grad_points_3d, grad_points_features)
        return grad_points_3d, grad_points_features, grad_volume_densities, grad_volume_features, None, None, None, None, None


# ---- the public functions -------------------------------------------------------------------------------------------------------------
def add_points_features_to_volume_densities_features(points_3d, points_features, volume_densities, volume_features, mode="trilinear",
                                                     min_weight=1e-4, mask=None, grid_sizes=None, rescale_features=True,
                                                     align_corners=True):
    """See the module docstring.  points_3d (N, P, 3) in the volume's local coordinates, points_features (N, P, C), volume_densities
    (N, 1, D, H, W) and volume_features (N, C, D, H, W) or None (zeros), both modified in place; mask (N, P) or None; grid_sizes (N, 3)
    int64 (depth, height, width) or None (the whole tensor for every cloud).  Returns (volume_features, volume_densities): the
    features divided by densities.clamp(min_weight) -- clamp(1.0) for nearest -- when rescale_features, the densities as summed."""
    if volume_densities.shape[1] != 1:
        raise ValueError("Only one-dimensional densities are allowed.")
    if mode == "trilinear":
        splat = True
    elif mode == "nearest":
        splat = False
    else:
        raise ValueError('No such interpolation mode "%s"' % mode)
    N, P, C = points_features.shape
    if grid_sizes is None:
        grid_sizes = torch.tensor(list(volume_densities.shape[2:]), dtype=torch.int64, device=volume_densities.device).expand(N, 3)
    if volume_features is None:
        volume_features = volume_densities.new_zeros(N, C, *volume_densities.shape[2:])
    if mask is None:
        mask = points_3d.new_ones(1).expand(points_3d.shape[:2])
    volume_densities, volume_features = _PointsToVolumes.apply(points_3d, points_features, volume_densities, volume_features, grid_sizes,
                                                               1.0, mask, align_corners, splat)
    if rescale_features:  # each feature divided by the total weight of its votes
        volume_features = volume_features / volume_densities.clamp(min_weight if splat else 1.0)
    return volume_features, volume_densities


def add_pointclouds_to_volumes(pointclouds, initial_volumes, mode="trilinear", min_weight=1e-4, rescale_features=True):
    """A batch of `Pointclouds` (with features) added to a batch of `Volumes`; returns the updated copy that
    `initial_volumes.update_padded` makes.  Duck-typed: points_padded, features_padded, num_points_per_cloud of the clouds;
    world_to_local_coords, features, densities, get_grid_sizes, get_align_corners, update_padded of the volumes."""
    if len(initial_volumes) != len(pointclouds):
        raise ValueError("'initial_volumes' and 'pointclouds' have to have the same batch size.")
    feats = pointclouds.features_padded()
    points = pointclouds.points_padded()
    if feats is None:
        raise ValueError("'pointclouds' have to have their 'features' defined.")
    counts = pointclouds.num_points_per_cloud().to(feats.device)
    mask = (torch.arange(points.shape[1], device=feats.device)[None, :] < counts[:, None]).to(feats.dtype)  # no wait for the device
    local = initial_volumes.world_to_local_coords(points)
    features_new, densities_new = add_points_features_to_volume_densities_features(
        points_3d=local, points_features=feats, volume_features=initial_volumes.features(), volume_densities=initial_volumes.densities(),
        min_weight=min_weight, grid_sizes=initial_volumes.get_grid_sizes(), mask=mask, mode=mode, rescale_features=rescale_features,
        align_corners=initial_volumes.get_align_corners())
    return initial_volumes.update_padded(new_densities=densities_new, new_features=features_new)
