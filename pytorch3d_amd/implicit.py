"""The two per-ray operators every implicit renderer of the reference ends in, on csrc/implicit.hip.

    sample_pdf(bins, weights, n_samples, det=False, eps=1e-5, uniforms=None) -> samples (..., n_samples)
                                                                                  pytorch3d/renderer/implicit/sample_pdf.py
    ea_raymarch(rays_densities (..., P, 1), rays_features (..., P, C), eps=1e-10, surface_thickness=1, return_weights=False)
        -> features_opacities (..., C + 1) [, weights (..., P)]                   EmissionAbsorptionRaymarcher.forward
    absorption_only_raymarch(rays_densities (..., P, 1)) -> opacities (..., 1)    AbsorptionOnlyRaymarcher.forward

sample_pdf has the reference function's checks, messages and defaults and follows the contract of its compiled CPU operator
(csrc/implicit_abi.h: p3di_sample_pdf): float32 GPU tensors take the kernel, float32 CPU tensors the library's host loop on the same
per-sample function, and the two write the same bits.  `uniforms` (..., n_samples) makes the randomness an input, as in
sample_points_from_meshes; it is not modified.  `sample_pdf_op` is the in-place operator `pytorch3d._C.sample_pdf`.

The raymarchers compute, with x_k = float32(1 + eps) - d_k and s = surface_thickness,
    a_k = 1 for k < s, else prod_{j <= k - s} x_j;   w_k = d_k a_k;   features = sum_k w_k f_k;   opacity = 1 - prod_k (1 - d_k)
and write (features, opacity) into one tensor.  float32 on the GPU with s >= 1, P >= 1, C >= 1 and any leading shape (none included)
is ONE autograd node over the forward and backward kernels: the backward divides nothing, so a density of exactly 1 (a saturated
1 - exp(-x)) has its exact gradient, and there is no atomic -- the same bits on every run and stream.  return_weights=True also returns
w, what a coarse pass hands to sample_pdf; it is differentiable.  Everything else (CPU, float64, s < 1) takes the torch formulation
of the reference's chain below, differentiated by autograd.  Like the reference's modules, both functions warn about densities outside
[0, 1] (one host sync).
"""
import warnings

import numpy as np
import torch

from . import _C


# ---- sample_pdf -------------------------------------------------------------------------------------------------------------------
def sample_pdf_op(bins, weights, outputs, eps):
    """`pytorch3d._C.sample_pdf` of the shim module: in place over outputs (B, S), whose entries are the uniforms on entry; bins
    (B, n_bins + 1), weights (B, n_bins); float32 on one device.  Returns None."""
    if not (torch.is_tensor(bins) and torch.is_tensor(weights) and torch.is_tensor(outputs)):
        raise TypeError("sample_pdf: bins, weights and outputs must be tensors")
    with torch.no_grad():
        if bins.is_cuda:
            _C.sample_pdf(bins, weights, outputs, eps)
        else:
            _C.sample_pdf_host(bins, weights, outputs, eps)


def sample_pdf(bins, weights, n_samples: int, det: bool = False, eps: float = 1e-5, uniforms=None):
    """See the module docstring."""
    if torch.is_grad_enabled() and (bins.requires_grad or weights.requires_grad):
        raise NotImplementedError("sample_pdf differentiability.")
    if weights.min() <= -eps:
        raise ValueError("Negative weights provided.")
    batch_shape = bins.shape[:-1]
    n_bins = weights.shape[-1]
    if n_bins + 1 != bins.shape[-1] or weights.shape[:-1] != batch_shape:
        shapes = f"{bins.shape}{weights.shape}"
        raise ValueError("Inconsistent shapes of bins and weights: " + shapes)
    output_shape = batch_shape + (n_samples,)
    if uniforms is not None:
        if det:
            raise ValueError("sample_pdf: det=True draws nothing; pass det or uniforms, not both")
        if tuple(uniforms.shape) != tuple(output_shape) or uniforms.dtype != torch.float32 or uniforms.device != bins.device:
            raise ValueError(f"uniforms must be float32 of shape {tuple(output_shape)} on {bins.device}")
        output = uniforms.detach().clone(memory_format=torch.contiguous_format)
    elif det:
        u = torch.linspace(0.0, 1.0, n_samples, device=bins.device, dtype=torch.float32)
        output = u.expand(output_shape).contiguous()
    else:
        output = torch.rand(output_shape, dtype=torch.float32, device=bins.device)
    sample_pdf_op(bins.reshape(-1, n_bins + 1), weights.reshape(-1, n_bins), output.reshape(-1, n_samples), eps)
    return output


# ---- raymarching ------------------------------------------------------------------------------------------------------------------
def _check_raymarcher_inputs(rays_densities, rays_features, features_can_be_none):
    """The reference's _check_raymarcher_inputs (z_can_be_none=True, density_1d=True), message for message."""
    if not torch.is_tensor(rays_densities):
        raise ValueError("rays_densities has to be an instance of torch.Tensor.")
    if not features_can_be_none and not torch.is_tensor(rays_features):
        raise ValueError("rays_features has to be an instance of torch.Tensor.")
    if rays_densities.ndim < 1:
        raise ValueError("rays_densities have to have at least one dimension.")
    if rays_densities.shape[-1] != 1:
        raise ValueError("The size of the last dimension of rays_densities has to be one." + f" Got shape {rays_densities.shape}.")
    if not features_can_be_none and rays_features.shape[:-1] != rays_densities.shape[:-1]:
        raise ValueError("The first to previous to last dimensions of rays_features"
                         " have to be the same as all dimensions of rays_densities.")


def _check_density_bounds(rays_densities, bounds=(0.0, 1.0)):
    """The reference's warning, with one host sync instead of two."""
    with torch.no_grad():
        if rays_densities.numel() and bool((rays_densities.max() > bounds[1]) | (rays_densities.min() < bounds[0])):
            warnings.warn("One or more elements of rays_densities are outside of valid" + f"range {str(bounds)}")


def kernel_path(rays_densities, rays_features=None, surface_thickness=1):
    """Whether the raymarch of these inputs runs csrc/implicit.hip's kernels (else: the torch formulation below)."""
    d, f = rays_densities, rays_features
    ok = torch.is_tensor(d) and d.is_cuda and d.dtype == torch.float32 and d.dim() >= 2 and d.shape[-1] == 1 and d.shape[-2] >= 1
    if ok and f is not None:
        ok = torch.is_tensor(f) and f.dtype == torch.float32 and f.device == d.device and f.dim() == d.dim() and \
            f.shape[:-1] == d.shape[:-1] and f.shape[-1] >= 1
    return bool(ok and isinstance(surface_thickness, int) and surface_thickness >= 1)


def shifted_cumprod(x, shift=1):
    """The reference's _shifted_cumprod: cumprod along the last dimension behind `shift` ones, `shift` trailing elements dropped."""
    x_cumprod = torch.cumprod(x, dim=-1)
    return torch.cat([torch.ones_like(x_cumprod[..., :shift]), x_cumprod[..., :-shift]], dim=-1)


def ea_raymarch_torch(rays_densities, rays_features, eps=1e-10, surface_thickness=1, return_weights=False):
    """The reference's chain (raymarching.py: EmissionAbsorptionRaymarcher.forward), any float dtype and device."""
    d = rays_densities[..., 0]
    weights = d * shifted_cumprod((1.0 + eps) - d, shift=surface_thickness)
    features = (weights[..., None] * rays_features).sum(dim=-2)
    opacities = 1.0 - torch.prod(1.0 - d, dim=-1, keepdim=True)
    out = torch.cat((features, opacities), dim=-1)
    return (out, weights) if return_weights else out


def absorption_only_raymarch_torch(rays_densities):
    return 1.0 - torch.prod(1 - rays_densities[..., 0], dim=-1, keepdim=True)


class _EARaymarch(torch.autograd.Function):
    """(out (N, C + 1), weights (N, P) or None) of densities (N, P) and features (N, P, C) or None (absorption only)."""

    @staticmethod
    def forward(ctx, densities, features, shift, one_plus_eps, return_weights):
        ctx.set_materialize_grads(False)
        ctx.shift, ctx.one_plus_eps = shift, one_plus_eps
        densities = densities.detach().contiguous()
        features = None if features is None else features.detach().contiguous()
        ctx.save_for_backward(densities, features)
        out, weights = _C.ea_raymarch_forward(densities, features, shift, one_plus_eps, return_weights)
        return out, weights

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, grad_weights):
        densities, features = ctx.saved_tensors
        if grad_out is None:
            grad_out = densities.new_zeros((densities.shape[0], (0 if features is None else features.shape[2]) + 1))
        gd, gf = _C.ea_raymarch_backward(densities, features, grad_out, grad_weights, ctx.shift, ctx.one_plus_eps)
        return (gd if ctx.needs_input_grad[0] else None), (gf if features is not None and ctx.needs_input_grad[1] else None), None, None, None


def _one_plus_eps(eps):
    return float(np.float32(1.0 + float(eps)))  # what `(1.0 + eps) - tensor` subtracts from in float32


def ea_raymarch_unchecked(rays_densities, rays_features, eps=1e-10, surface_thickness=1, return_weights=False):
    """ea_raymarch behind somebody else's input checks (the shim's patched module calls the reference's own)."""
    if not kernel_path(rays_densities, rays_features, surface_thickness):
        return ea_raymarch_torch(rays_densities, rays_features, eps, surface_thickness, return_weights)
    lead, P, C = tuple(rays_densities.shape[:-2]), rays_densities.shape[-2], rays_features.shape[-1]
    out, weights = _EARaymarch.apply(rays_densities.reshape(-1, P), rays_features.reshape(-1, P, C), int(surface_thickness),
                                     _one_plus_eps(eps), bool(return_weights))
    out = out.reshape(lead + (C + 1,))
    return (out, weights.reshape(lead + (P,))) if return_weights else out


def ea_raymarch(rays_densities, rays_features, eps: float = 1e-10, surface_thickness: int = 1, return_weights: bool = False):
    """See the module docstring."""
    _check_raymarcher_inputs(rays_densities, rays_features, features_can_be_none=False)
    _check_density_bounds(rays_densities)
    return ea_raymarch_unchecked(rays_densities, rays_features, eps, surface_thickness, return_weights)


def absorption_only_raymarch_unchecked(rays_densities):
    if not kernel_path(rays_densities):
        return absorption_only_raymarch_torch(rays_densities)
    lead, P = tuple(rays_densities.shape[:-2]), rays_densities.shape[-2]
    out, _ = _EARaymarch.apply(rays_densities.reshape(-1, P), None, 1, 1.0, False)
    return out.reshape(lead + (1,))


def absorption_only_raymarch(rays_densities):
    """See the module docstring."""
    _check_raymarcher_inputs(rays_densities, None, features_can_be_none=True)
    _check_density_bounds(rays_densities[..., 0])
    return absorption_only_raymarch_unchecked(rays_densities)
