"""VolumeSampler: voxel grids sampled at the points of rays, on csrc/volume_sample.hip, forward and backward.

    sample_volumes(densities, features, rays_origins_local, rays_directions_local, rays_lengths, *,
                   sample_mode="bilinear", padding_mode="zeros", align_corners=True) -> (rays_densities, rays_features)
    volume_sampler_forward(volumes, ray_bundle, sample_mode="bilinear", padding_mode="zeros") -> (rays_densities, rays_features)

`volume_sampler_forward` is the whole of the reference's VolumeSampler.forward (pytorch3d/renderer/implicit/renderer.py) with its
checks and messages.  Step 1 -- the rays into the volumes' local coordinates -- is the reference's own calls on the `Volumes` object:
small (N, R, 3) torch operations that stay differentiable, so gradients to the volumes' translation and voxel size keep flowing
through autograd.  Steps 2 and 3 are `sample_volumes`.

`sample_volumes` takes densities (N, Cd, D, H, W), features (N, Cf, D, H, W) or None, local origins and directions (N, ..., 3) and
lengths (N, ..., P), and returns (N, ..., P, Cd) and (N, ..., P, Cf) -- (..., P, 0) for features=None, as the reference's split gives.
The reference materialises the (N, ..., P, 3) ray points, runs F.grid_sample once per grid over the same points, permutes and copies
both results, and its backward runs grid_sampler_3d_backward twice (float atomics; it raises under
torch.use_deterministic_algorithms(True)).  Here float32 GPU tensors in the modes bilinear / nearest and the paddings zeros / border
are ONE autograd node: the point o + l d (one multiply, one add, no FMA) lives in registers, corners and weights are computed once per
point for all Cd + Cf channels, and the volumes are read in place through their strides -- a channel slice, or ONE grid shared by the N
ray batches: volumes whose first dimension is 1 against rays of batch N, or an `expand` along the batch (the fitting tutorial's
`densities[None].expand(batch, ...)`).  The volume gradients are float atomics, or under torch.use_deterministic_algorithms(True)
(not warn-only) a stable sort by voxel and the segmented sum of csrc/ordered_sum.h, the same bits on every run and stream; the
gradients to origins, directions and lengths are shuffle trees along the ray without atomics in both modes.

Contract: csrc/implicit_abi.h (ATen's grid_sampler_3d restated in float32; x indexes W, y indexes H, z indexes D).  Under zeros
padding a coordinate that is not finite, or whose source index does not fit an int32, gives a ZERO sample and zero gradients; under
border the clamp applies with NaN -> 0.  Everything else -- CPU tensors, float64, reflection, bicubic -- takes `sample_volumes_torch`,
the reference's chain restated, differentiated by autograd.
"""
import torch
import torch.nn.functional as F

from . import _C, _lib

CALLS = {"fused": 0, "chain": 0}  # what ran (the shim's PATCH_CALLS and the tests read it)


def sample_volumes_torch(densities, features, rays_origins_local, rays_directions_local, rays_lengths, *, sample_mode="bilinear",
                         padding_mode="zeros", align_corners=True):
    """Steps 2 and 3 of the reference's VolumeSampler.forward (renderer.py:360-415), any dtype, device and mode F.grid_sample takes."""
    points = rays_origins_local[..., None, :] + rays_lengths[..., :, None] * rays_directions_local[..., None, :]
    N = points.shape[0]
    flat = points.view(N, -1, 1, 1, 3)
    if densities.shape[0] == 1 and N > 1:
        densities = densities.expand(N, *densities.shape[1:])
        features = None if features is None else features.expand(N, *features.shape[1:])
    rays_densities = F.grid_sample(densities, flat, mode=sample_mode, padding_mode=padding_mode, align_corners=align_corners)
    rays_densities = rays_densities.permute(0, 2, 3, 4, 1).view(*points.shape[:-1], densities.shape[1])
    if features is None:
        _, rays_features = rays_densities.split([densities.shape[1], 0], dim=-1)
    else:
        rays_features = F.grid_sample(features, flat, mode=sample_mode, padding_mode=padding_mode, align_corners=align_corners)
        rays_features = rays_features.permute(0, 2, 3, 4, 1).view(*points.shape[:-1], features.shape[1])
    return rays_densities, rays_features


def kernel_path(densities, features, rays_origins_local, rays_directions_local, rays_lengths, sample_mode="bilinear", padding_mode="zeros"):
    """Whether sample_volumes(...) of these inputs runs csrc/volume_sample.hip's kernels (else: the reference's chain restated)."""
    o, d, l = rays_origins_local, rays_directions_local, rays_lengths
    tensors = [densities, o, d, l] + ([] if features is None else [features])
    if not all(torch.is_tensor(t) for t in tensors) or sample_mode not in ("bilinear", "nearest") or padding_mode not in ("zeros", "border"):
        return False
    if not all(t.is_cuda and t.dtype == torch.float32 and t.device == densities.device for t in tensors):
        return False
    if o.dim() < 2 or d.shape != o.shape or l.dim() != o.dim() or l.shape[:-1] != o.shape[:-1] or o.shape[-1] != 3:
        return False
    if densities.dim() != 5 or densities.shape[0] not in (1, o.shape[0]) or densities.shape[1] < 1 or min(densities.shape[2:]) < 1:
        return False
    if features is not None and (features.dim() != 5 or features.shape[0] != densities.shape[0] or features.shape[2:] != densities.shape[2:]):
        return False
    return max(densities.shape[2:]) <= _C.MAX_INT  # the kernels' voxel indices are int32 per axis


def _flags(sample_mode, padding_mode, align_corners):
    return ((_lib.VOLUME_SAMPLE_NEAREST if sample_mode == "nearest" else 0) | (_lib.VOLUME_SAMPLE_BORDER if padding_mode == "border" else 0)
            | (_lib.VOLUME_SAMPLE_CORNERS if align_corners else 0))


class _SampleVolumes(torch.autograd.Function):
    """(rays_densities (N, R, P, Cd), rays_features (N, R, P, Cf)) of volumes (N or 1, C, D, H, W) and rays (N, R, 3), (N, R, 3), (N, R, P)."""

    @staticmethod
    def forward(ctx, densities, features, origins, directions, lengths, modes):
        ctx.set_materialize_grads(False)
        ctx.modes = modes
        saved = [t if t is None else t.detach() for t in (densities, features, origins, directions, lengths)]
        ctx.save_for_backward(*saved)
        return _C.volume_sample_forward(*saved, _flags(*modes))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_d, grad_f):
        densities, features, origins, directions, lengths = ctx.saved_tensors
        need = ctx.needs_input_grad
        if grad_d is None and grad_f is None:
            return (None,) * 6
        try:
            grads = _C.volume_sample_backward(grad_d, grad_f, densities, features, origins, directions, lengths, _flags(*ctx.modes),
                                              (need[0], need[1] and features is not None), need[2:5])
        except NotImplementedError:  # the ordered form cannot key sizes this large: the chain's own backward
            with torch.enable_grad():
                leaves = [None if t is None else t.detach().requires_grad_(True) for t in (densities, features, origins, directions, lengths)]
                outs = sample_volumes_torch(*leaves, sample_mode=ctx.modes[0], padding_mode=ctx.modes[1], align_corners=ctx.modes[2])
                pairs = [(o, g) for o, g in zip(outs, (grad_d, grad_f)) if g is not None and o.requires_grad]
                wanted = [t for t, n in zip(leaves, need[:5]) if n and t is not None]
                got = iter(torch.autograd.grad([o for o, _ in pairs], wanted, [g for _, g in pairs], allow_unused=True))
            grads = [next(got) if n and t is not None else None for t, n in zip(leaves, need[:5])]
        return (*[g if n else None for g, n in zip(grads, need[:5])], None)


def sample_volumes(densities, features, rays_origins_local, rays_directions_local, rays_lengths, *, sample_mode: str = "bilinear",
                   padding_mode: str = "zeros", align_corners: bool = True):
    """See the module docstring."""
    o, d, l = rays_origins_local, rays_directions_local, rays_lengths
    if not kernel_path(densities, features, o, d, l, sample_mode, padding_mode):
        CALLS["chain"] += 1
        return sample_volumes_torch(densities, features, o, d, l, sample_mode=sample_mode, padding_mode=padding_mode, align_corners=align_corners)
    CALLS["fused"] += 1
    N, lead, P = o.shape[0], tuple(o.shape[:-1]), l.shape[-1]
    if N > 1 and densities.shape[0] == N and densities.stride(0) == 0 and (features is None or features.stride(0) == 0):
        # an expand along the batch: one grid, and one gradient of its size (autograd hands it on through the slice and the expand)
        densities, features = densities[:1], None if features is None else features[:1]
    out_d, out_f = _SampleVolumes.apply(densities, features, o.reshape(N, -1, 3), d.reshape(N, -1, 3), l.reshape(N, -1, P),
                                        (sample_mode, padding_mode, bool(align_corners)))
    return out_d.view(lead + (P, out_d.shape[-1])), out_f.view(lead + (P, out_f.shape[-1]))


def _validate_ray_bundle_variables(rays_origins, rays_directions, rays_lengths):
    """The reference's check (renderer/implicit/utils.py), message for message."""
    ndim = rays_origins.ndim
    if any(r.ndim != ndim for r in (rays_directions, rays_lengths)):
        raise ValueError("rays_origins, rays_directions and rays_lengths" + " have to have the same number of dimensions.")
    if ndim <= 2:
        raise ValueError("rays_origins, rays_directions and rays_lengths" + " have to have at least 3 dimensions.")
    spatial_size = rays_origins.shape[:-1]
    if any(spatial_size != r.shape[:-1] for r in (rays_directions, rays_lengths)):
        raise ValueError("The shapes of rays_origins, rays_directions and rays_lengths" + " may differ only in the last dimension.")
    if any(r.shape[-1] != 3 for r in (rays_origins, rays_directions)):
        raise ValueError("The size of the last dimension of rays_origins/rays_directions" + "has to be 3.")


def local_rays(volumes, rays_origins_world, rays_directions_world, batch):
    """Step 1 of VolumeSampler.forward by the reference's own calls on `volumes`: the origins through world_to_local_coords, the
    directions through the same matrix WITHOUT its translation row (VolumeSampler._get_ray_directions_transform)."""
    origins = volumes.world_to_local_coords(rays_origins_world)
    world2local = volumes.get_world_to_local_coords_transform().get_matrix()
    matrix = torch.eye(4, device=world2local.device, dtype=world2local.dtype)[None].repeat(world2local.shape[0], 1, 1)
    matrix[:, :3, :3] = world2local[:, :3, :3]
    directions = type(volumes.get_world_to_local_coords_transform())(matrix=matrix).transform_points(
        rays_directions_world.view(batch, -1, 3)).view(rays_directions_world.shape)
    return origins, directions


def volume_sampler_forward(volumes, ray_bundle, sample_mode: str = "bilinear", padding_mode: str = "zeros"):
    """See the module docstring."""
    origins_world, directions_world, lengths = ray_bundle.origins, ray_bundle.directions, ray_bundle.lengths
    _validate_ray_bundle_variables(origins_world, directions_world, lengths)
    if volumes.densities().shape[0] != origins_world.shape[0]:
        raise ValueError("Input volumes have to have the same batch size as rays.")
    origins, directions = local_rays(volumes, origins_world, directions_world, lengths.shape[0])
    return sample_volumes(volumes.densities(), volumes.features(), origins, directions, lengths, sample_mode=sample_mode,
                          padding_mode=padding_mode, align_corners=volumes.get_align_corners())
