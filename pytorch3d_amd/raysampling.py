"""Stratified ray depths: the per-point step of the reference's three ray samplers, on csrc/harmonic.hip.

    stratified_depths(bin_centers, uniforms=None) -> depths of bin_centers' shape
    stratified_depths_torch(bin_centers, uniforms=None)    the reference's chain restated

The reference's `_jiggle_within_stratas` (pytorch3d/renderer/implicit/raysampling.py) takes the bin centres (..., n) -- in the ray
samplers a stride-0 `expand` of one linspace, which costs no memory -- and materialises mids, upper, lower, the uniforms, a difference,
a product and the result: seven tensors of the full size for one that is needed.  Here float32 GPU centres are read in place through
their strides and the result is written once:

    lower = c[0] for k = 0, else 0.5 (c[k] + c[k-1]);   upper = c[n-1] for k = n - 1, else 0.5 (c[k+1] + c[k]);
    depths = lower + (upper - lower) u

in IEEE float32 without FMA: given the same u, the kernel, this chain on the CPU and this chain on the GPU write the same bits.  Without
`uniforms` the draw is torch.rand(bin_centers.shape, dtype, device) -- what the reference's torch.rand_like(lower) draws, so a seeded
run gives the same depths with and without the kernel.  `uniforms` is only read.  There is no backward: centres that require grad, CPU
tensors, other dtypes and sizes beyond 32-bit indices take the chain.  The rest of the ray samplers (the xy grid, the unprojection through
the cameras, origins and directions) is per ray, not per point, carries the camera gradients and stays the reference's torch.
"""
import torch

from . import _C

CALLS = {"fused": 0, "chain": 0}


def stratified_depths_torch(bin_centers, uniforms=None):
    """The reference's _jiggle_within_stratas (raysampling.py:715-720), with the draw as an optional argument."""
    mids = 0.5 * (bin_centers[..., 1:] + bin_centers[..., :-1])
    upper = torch.cat((mids, bin_centers[..., -1:]), dim=-1)
    lower = torch.cat((bin_centers[..., :1], mids), dim=-1)
    if uniforms is None:
        uniforms = torch.rand_like(lower)
    return lower + (upper - lower) * uniforms


def kernel_path(bin_centers, uniforms=None):
    """Whether stratified_depths(...) of these inputs runs the kernel (else: the chain)."""
    c, u = bin_centers, uniforms
    if not torch.is_tensor(c) or not c.is_cuda or c.dtype != torch.float32 or c.requires_grad or c.dim() < 1:
        return False
    if u is not None and not (torch.is_tensor(u) and u.device == c.device and u.dtype == c.dtype and u.shape == c.shape and not u.requires_grad):
        return False
    return c.shape[-1] >= 1 and c.numel() <= _C.MAX_INT


def stratified_depths(bin_centers, uniforms=None):
    """See the module docstring."""
    if not kernel_path(bin_centers, uniforms):
        CALLS["chain"] += 1
        return stratified_depths_torch(bin_centers, uniforms)
    CALLS["fused"] += 1
    n = bin_centers.shape[-1]
    if uniforms is None:
        uniforms = torch.rand(bin_centers.shape, dtype=bin_centers.dtype, device=bin_centers.device)
    # a view wherever the leading dimensions merge -- an expand of one row does, with row stride 0; anything else is copied by reshape
    out = _C.stratified_depths(bin_centers.reshape(-1, n), uniforms.reshape(-1, n))
    return out.view(bin_centers.shape)
