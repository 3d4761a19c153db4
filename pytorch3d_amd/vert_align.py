"""vert_align: image features pooled at vertex positions ("perceptual feature pooling", Pixel2Mesh; "vert align", Mesh R-CNN) on
csrc/vert_align.hip, forward and backward.

    vert_align(feats, verts, return_packed=False, interp_mode="bilinear", padding_mode="zeros", align_corners=True)

Same name, defaults, checks, messages and return values as pytorch3d/ops/vert_align.py.  feats (N, C, H, W) or a list of such maps
(any C, H, W each); verts (N, V, 3) or an object with verts_padded() / points_padded(); (x, y) = (-1, -1) is the top-left and (+1, +1)
the bottom-right of a map.  Returns (N, V, sum C), or with return_packed (N * V, sum C) -- (sum V, sum C) when the object has
verts_padded_to_packed_idx().

The reference runs F.grid_sample per map, squeeze / transpose, a cat copy and a gather copy; its backward ends in
grid_sampler_2d_backward, which scatters with float atomics and has no deterministic GPU form.  Here one launch per map writes that
map's column block of the single output straight from the packed index (padding rows are never sampled), the maps are read through
their strides (NCHW, channels_last and sliced views without a copy), grad_verts is a gather, and grad_feats is float atomics -- or a
stable sort by pixel and the segmented sum of csrc/ordered_sum.h, the same bits on every run and stream: always under
torch.use_deterministic_algorithms(True), and by default for a map of 32 channels or more whose channels are not adjacent in memory
(NCHW), where the atomics of one wave land in 64 different lines and measured slower than the torch chain.

Contract (ATen's grid_sampler_2d restated in float32; checked against F.grid_sample on the CPU by the tests).  Source coordinate of c
on an axis of S pixels: ((c + 1) / 2) * (S - 1) with align_corners, ((c + 1) * S - 1) / 2 without.  border: min(max(i, 0), S - 1).
bilinear: x0 = floor(ix), y0 = floor(iy); weights nw (x0+1-ix)(y0+1-iy), ne (ix-x0)(y0+1-iy), sw (x0+1-ix)(iy-y0), se (ix-x0)(iy-y0);
the in-range corners summed in the order nw, ne, sw, se.  nearest: round half to even.  Gradients: weight x grad per corner to the map;
to verts x and y through the corner differences times (S - 1) / 2 or S / 2, 0 on an axis that border padding clipped (a coordinate at
or beyond an end), 0 for nearest; z always 0.
NON-FINITE COORDINATES are outside what the reference pins (its CPU build gives a NaN row for NaN / +-inf and a zero row for 1e30 under
zeros).  Here, under zeros a coordinate that is not finite, or whose source coordinate does not fit an int32, gives a ZERO row and
zero gradients; under border the clamp applies with NaN -> 0 (the reference's CPU answer).

The fused path takes float32 GPU tensors, interp_mode bilinear / nearest and padding_mode zeros / border.  reflection, other dtypes
and CPU tensors take the reference's chain restated here (`vert_align_torch`).
"""
import torch
import torch.nn.functional as F

from . import _C, _lib

CALLS = {"fused": 0, "chain": 0}  # what ran (the shim's PATCH_CALLS and the tests read it)


def _grid_of(verts):
    if torch.is_tensor(verts):
        if verts.dim() != 3:
            raise ValueError("verts tensor should be 3 dimensional")
        return verts
    if hasattr(verts, "verts_padded"):
        return verts.verts_padded()
    if hasattr(verts, "points_padded"):
        return verts.points_padded()
    raise ValueError("verts must be a tensor or have a " + "`points_padded' or`verts_padded` attribute.")


def _check_feats(feats, grid):
    feats = [feats] if torch.is_tensor(feats) else list(feats)
    for feat in feats:
        if feat.dim() != 4:
            raise ValueError("feats must have shape (N, C, H, W)")
        if grid.shape[0] != feat.shape[0]:
            raise ValueError("inconsistent batch dimension")
    return feats


def _chain(feats, grid, packed_idx, return_packed, interp_mode, padding_mode, align_corners):
    """pytorch3d/ops/vert_align.py:73-107 on a list of maps, the (N, V, >= 2) grid and the padded-to-packed index (or None)."""
    grid = grid[:, None, :, :2]  # (N, 1, V, 2)
    sampled = []
    for feat in feats:
        s = F.grid_sample(feat, grid, mode=interp_mode, padding_mode=padding_mode, align_corners=align_corners)  # (N, C, 1, V)
        sampled.append(s.squeeze(dim=2).transpose(1, 2))  # (N, V, C)
    out = torch.cat(sampled, dim=2)  # (N, V, sum(C))
    if return_packed:
        out = out.view(-1, out.shape[-1])
        if packed_idx is not None:
            out = out.gather(0, packed_idx.view(-1, 1).expand(-1, out.shape[-1]))
    return out


def vert_align_torch(feats, verts, return_packed=False, interp_mode="bilinear", padding_mode="zeros", align_corners=True):
    """The reference's chain (any dtype, device and mode F.grid_sample takes)."""
    grid = _grid_of(verts)
    feats = _check_feats(feats, grid)
    idx = verts.verts_padded_to_packed_idx() if return_packed and hasattr(verts, "verts_padded_to_packed_idx") else None
    return _chain(feats, grid, idx, return_packed, interp_mode, padding_mode, align_corners)


def kernel_path(feats, verts, interp_mode="bilinear", padding_mode="zeros"):
    """Whether vert_align(feats, verts, ...) runs csrc/vert_align.hip's kernels (else: the reference's chain)."""
    try:
        grid = _grid_of(verts)
        feats = _check_feats(feats, grid)
    except (ValueError, AttributeError, TypeError):
        return False
    tensors = [grid] + feats
    return (interp_mode in ("bilinear", "nearest") and padding_mode in ("zeros", "border") and len(feats) > 0 and grid.shape[2] >= 2
            and all(t.is_cuda and t.dtype == torch.float32 and t.device == grid.device for t in tensors)
            and all(f.shape[2] * f.shape[3] > 0 and (f.numel() == 0 or min(f.stride()) >= 0) for f in feats))


def _flags(interp_mode, padding_mode, align_corners):
    return ((_lib.VERT_ALIGN_NEAREST if interp_mode == "nearest" else 0) | (_lib.VERT_ALIGN_BORDER if padding_mode == "border" else 0)
            | (_lib.VERT_ALIGN_CORNERS if align_corners else 0))


class _VertAlign(torch.autograd.Function):
    """(rows, sum C) from the grid (N, V, >= 2), the padded-to-packed index (or None) and the maps."""

    @staticmethod
    def forward(ctx, grid, packed_idx, modes, *feats):
        ctx.modes = modes
        ctx.save_for_backward(grid, packed_idx, *feats)
        return _C.vert_align_forward([f.detach() for f in feats], grid.detach(), packed_idx, _flags(*modes))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        grid, packed_idx, *feats = ctx.saved_tensors
        need_verts, need_feats = ctx.needs_input_grad[0], list(ctx.needs_input_grad[3:])
        try:
            grads, gv = _C.vert_align_backward(grad_out, feats, grid, packed_idx, _flags(*ctx.modes), need_feats, need_verts)
        except NotImplementedError:  # the ordered form cannot key the pixels of a map this large: the chain's own backward
            with torch.enable_grad():
                leaves = [t.detach().requires_grad_(True) for t in [grid] + feats]
                out = _chain(leaves[1:], leaves[0], packed_idx, True, *ctx.modes)
                wanted = [t for t, need in zip(leaves, [need_verts] + need_feats) if need]
                got = iter(torch.autograd.grad(out, wanted, grad_out, allow_unused=True))
            res = [next(got) if need else None for need in [need_verts] + need_feats]
            return (res[0], None, None, *res[1:])
        if gv is not None and grid.shape[2] != 3:
            wide = gv.new_zeros(grid.shape)
            wide[:, :, :2] = gv[:, :, :2]
            gv = wide
        return (gv, None, None, *grads)


def vert_align(feats, verts, return_packed: bool = False, interp_mode: str = "bilinear", padding_mode: str = "zeros",
               align_corners: bool = True) -> torch.Tensor:
    """See the module docstring."""
    grid = _grid_of(verts)
    feats = _check_feats(feats, grid)
    idx = verts.verts_padded_to_packed_idx() if return_packed and hasattr(verts, "verts_padded_to_packed_idx") else None
    if not kernel_path(feats, grid, interp_mode, padding_mode) or (idx is not None and idx.device != grid.device):
        CALLS["chain"] += 1
        return _chain(feats, grid, idx, return_packed, interp_mode, padding_mode, align_corners)
    CALLS["fused"] += 1
    out = _VertAlign.apply(grid, idx, (interp_mode, padding_mode, bool(align_corners)), *feats)
    return out if return_packed else out.view(grid.shape[0], grid.shape[1], out.shape[1])
