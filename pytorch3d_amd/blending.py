"""Host-side mirror of pytorch3d/renderer/blending.py:43-244 over the C ABI.

`hard_rgb_blend` (blending.py:54-88) is one kernel each way (p3d_hard_rgb_blend_forward / _backward).

`sigmoid_alpha_blend` goes through `pytorch3d_amd._C.sigmoid_alpha_blend[_backward]` exactly like the
reference's wrapper (blending.py:95-140).  `softmax_rgb_blend`, ~20 elementwise torch ops plus their autograd
graph in the reference (blending.py:147-244), is ONE kernel forward and ONE backward here
(include/p3d_amd.h: p3d_softmax_rgb_blend_forward / _backward); same arguments, defaults and return value.

`hard_depth_blend` / `soft_depth_blend` are the bodies of HardDepthShader.forward / SoftDepthShader.forward
(renderer/mesh/shader.py:377-445) after their camera lookup, one kernel each way as well.
"""
from typing import NamedTuple, Sequence, Union

import torch

from . import _C, _lib


class BlendParams(NamedTuple):
    """blending.py:20-40."""

    sigma: float = 1e-4
    gamma: float = 1e-4
    background_color: Union[torch.Tensor, Sequence[float]] = (1.0, 1.0, 1.0)


class _SigmoidAlphaBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dists, pix_to_face, sigma):
        alphas = _C.sigmoid_alpha_blend(dists, pix_to_face, sigma)
        ctx.save_for_backward(dists, pix_to_face, alphas)
        ctx.sigma = sigma
        return alphas

    @staticmethod
    def backward(ctx, grad_alphas):
        dists, pix_to_face, alphas = ctx.saved_tensors
        grad_dists = _C.sigmoid_alpha_blend_backward(grad_alphas, alphas, dists, pix_to_face, ctx.sigma)
        return grad_dists, None, None


def sigmoid_alpha_blend(colors, fragments, blend_params: BlendParams) -> torch.Tensor:
    """blending.py:118-144: RGB of the closest face, alpha from the 2D distance probability map."""
    N, H, W, K = fragments.pix_to_face.shape
    pixel_colors = torch.ones((N, H, W, 4), dtype=colors.dtype, device=colors.device)
    pixel_colors[..., :3] = colors[..., 0, :]
    pixel_colors[..., 3] = _SigmoidAlphaBlend.apply(fragments.dists, fragments.pix_to_face, blend_params.sigma)
    return pixel_colors


def _background(blend_params, device, who="softmax_rgb_blend"):
    bg = blend_params.background_color
    if isinstance(bg, torch.Tensor):
        if bg.requires_grad:
            # the reference keeps the background in the autograd graph (blending.py:183-186); the fused kernel takes it
            # as three constants -- refuse rather than return a silently missing gradient
            raise NotImplementedError(who + ": a background_color that requires grad is not supported by the "
                                      "fused kernel (it is passed as constants); detach it or blend with torch ops")
        bg = [float(x) for x in bg.detach().reshape(-1).tolist()]
    bg = [float(x) for x in bg]
    if len(bg) != 3:
        raise ValueError("background_color must have 3 elements")
    return tuple(bg)


def _plane(v, N, device):
    """znear / zfar: float, or a per-batch-element tensor (blending.py:205-210).  -> (scalar, device tensor or None)"""
    if torch.is_tensor(v):
        if v.requires_grad:
            raise NotImplementedError("softmax_rgb_blend: znear / zfar tensors that require grad are not supported by the "
                                      "fused kernel; detach them")
        t = v.detach().to(device=device, dtype=torch.float32).reshape(-1)
        if t.numel() == 1:
            t = t.expand(N)
        if t.numel() != N:
            raise ValueError("znear / zfar tensors must have one entry per batch element")
        return 0.0, t.contiguous()
    return float(v), None


class _SoftmaxRGBBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, colors, dists, zbuf, pix_to_face, sigma, gamma, bg, znear, zfar):
        N, H, W, K = pix_to_face.shape
        dev = colors.device
        c = _C._aligned(colors)
        d, z, p2f = _C._aligned(dists), _C._aligned(zbuf), _C._aligned(pix_to_face)
        zn, zn_t = _plane(znear, N, dev)
        zf, zf_t = _plane(zfar, N, dev)
        out = torch.empty((N, H, W, 4), dtype=torch.float32, device=dev)
        if out.numel():
            _lib.call("p3d_softmax_rgb_blend_forward", "softmax_rgb_blend", dev, c, p2f, d, z, float(sigma), float(gamma), bg, zn, zf, zn_t,
                      zf_t, N, H * W, K, out)
        ctx.save_for_backward(c, d, z, p2f, zn_t if zn_t is not None else torch.empty(0, device=dev),
                              zf_t if zf_t is not None else torch.empty(0, device=dev))
        ctx.params = (float(sigma), float(gamma), bg, zn, zf, zn_t is not None, zf_t is not None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        c, d, z, p2f, zn_t, zf_t = ctx.saved_tensors
        sigma, gamma, bg, zn, zf, has_zn, has_zf = ctx.params
        N, H, W, K = p2f.shape
        dev = c.device
        g = _C._aligned(grad_out)
        gc = torch.empty((N, H, W, K, 3), dtype=torch.float32, device=dev)
        gd = torch.empty((N, H, W, K), dtype=torch.float32, device=dev)
        gz = torch.empty((N, H, W, K), dtype=torch.float32, device=dev)
        if gd.numel():
            _lib.call("p3d_softmax_rgb_blend_backward", "softmax_rgb_blend_backward", dev, g, c, p2f, d, z, sigma, gamma, bg, zn, zf,
                      zn_t if has_zn else None, zf_t if has_zf else None, N, H * W, K, gc, gd, gz)
        return gc, gd, gz, None, None, None, None, None, None


def softmax_rgb_blend(colors, fragments, blend_params: BlendParams, znear: Union[float, torch.Tensor] = 1.0,
                      zfar: Union[float, torch.Tensor] = 100) -> torch.Tensor:
    """blending.py:147-244.  colors (N,H,W,K,3), fragments.{pix_to_face, dists, zbuf} (N,H,W,K) -> RGBA (N,H,W,4)."""
    _C._check_fragments("softmax_rgb_blend", fragments.pix_to_face, colors=colors, dists=fragments.dists, zbuf=fragments.zbuf)
    bg = _background(blend_params, colors.device)
    return _SoftmaxRGBBlend.apply(colors, fragments.dists, fragments.zbuf, fragments.pix_to_face, blend_params.sigma,
                                  blend_params.gamma, bg, znear, zfar)


class _HardRGBBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, colors, pix_to_face, bg):
        N, H, W, K = pix_to_face.shape
        dev = colors.device
        c, p2f = _C._aligned(colors), _C._aligned(pix_to_face)
        out = torch.empty((N, H, W, 4), dtype=torch.float32, device=dev)
        if out.numel():
            _lib.call("p3d_hard_rgb_blend_forward", "hard_rgb_blend", dev, c, p2f, bg, N * H * W, K, out)
        ctx.save_for_backward(p2f)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (p2f,) = ctx.saved_tensors
        N, H, W, K = p2f.shape
        dev = p2f.device
        g = _C._aligned(grad_out)
        gc = torch.empty((N, H, W, K, 3), dtype=torch.float32, device=dev)
        if gc.numel():
            _lib.call("p3d_hard_rgb_blend_backward", "hard_rgb_blend_backward", dev, g, p2f, N * H * W, K, gc)
        return gc, None, None


def hard_rgb_blend(colors, fragments, blend_params: BlendParams) -> torch.Tensor:
    """blending.py:54-88: RGB of the closest face (slot 0), the background colour where no face covers the pixel;
    alpha 1 / 0.  colors (N,H,W,K,3) -> RGBA (N,H,W,4)."""
    _C._check_fragments("hard_rgb_blend", fragments.pix_to_face, colors=colors)
    if colors.shape != tuple(fragments.pix_to_face.shape) + (3,) or fragments.pix_to_face.shape[3] < 1:
        raise ValueError("colors must have shape (N, H, W, K, 3) with K >= 1 matching pix_to_face")
    return _HardRGBBlend.apply(colors, fragments.pix_to_face, _background(blend_params, colors.device, "hard_rgb_blend"))


def _depth_zfar(zfar, who):
    """The depth shaders' far plane: a Python number or a one-element tensor that does not require grad (the reference's
    own forwards raise a shape error for anything longer; a gradient to zfar is not computed).  A device tensor is read
    back once per call."""
    if torch.is_tensor(zfar):
        if zfar.numel() != 1 or zfar.requires_grad:
            raise ValueError(who + ": zfar must be a number or a one-element tensor that does not require grad")
        return float(zfar.detach().reshape(()).item())
    if isinstance(zfar, bool) or not isinstance(zfar, (int, float)):
        raise ValueError(who + ": zfar must be a number or a one-element tensor that does not require grad")
    return float(zfar)


def _check_depth_fragments(who, fragments, with_dists):
    floats = {"zbuf": fragments.zbuf}
    if with_dists:
        floats["dists"] = fragments.dists
    _C._check_fragments(who, fragments.pix_to_face, **floats)
    shape = tuple(fragments.pix_to_face.shape)
    if len(shape) != 4 or shape[3] < 1:
        raise ValueError(who + ": pix_to_face must have shape (N, H, W, K) with K >= 1")
    if shape[3] > _C.kMaxPointsPerPixel:
        raise ValueError(f"{who}: K must be at most {_C.kMaxPointsPerPixel}")
    for name, t in floats.items():
        if tuple(t.shape) != shape:
            raise ValueError(f"{who}: {name} must have the shape of pix_to_face {shape}; got {tuple(t.shape)}")


class _SoftDepthBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dists, zbuf, pix_to_face, sigma, zfar):
        N, H, W, K = pix_to_face.shape
        dev = zbuf.device
        d, z, p2f = _C._aligned(dists), _C._aligned(zbuf), _C._aligned(pix_to_face)
        out = torch.empty((N, H, W, 1), dtype=torch.float32, device=dev)
        if out.numel():
            _lib.call("p3d_soft_depth_blend_forward", "soft_depth_blend", dev, d, z, p2f, sigma, zfar, N * H * W, K, out)
        ctx.save_for_backward(d, z, p2f)
        ctx.params = (sigma, zfar)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, grad_depth):
        if grad_depth is None:
            return None, None, None, None, None
        d, z, p2f = ctx.saved_tensors
        sigma, zfar = ctx.params
        N, H, W, K = p2f.shape
        dev = z.device
        g = grad_depth.contiguous()
        gd = torch.empty((N, H, W, K), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        gz = torch.empty((N, H, W, K), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        if p2f.numel() and (gd is not None or gz is not None):
            _lib.call("p3d_soft_depth_blend_backward", "soft_depth_blend_backward", dev, g, d, z, p2f, sigma, zfar, N * H * W, K, gd, gz)
        return gd, gz, None, None, None


def soft_depth_blend(fragments, blend_params: BlendParams, zfar: Union[float, torch.Tensor] = 100.0) -> torch.Tensor:
    """SoftDepthShader.forward (shader.py:419-445) after its camera lookup: the depths of a pixel's K slots weighted by the
    clamped running sum of their sigmoid(-dists / sigma) probabilities, zfar taking what is left of 1.  One kernel each way
    (p3d_soft_depth_blend_forward / _backward).  fragments.{pix_to_face, zbuf, dists} (N,H,W,K) -> depth (N,H,W,1)."""
    if fragments.dists is None:
        raise ValueError("SoftDepthShader requires Fragments.dists to be present.")
    _check_depth_fragments("soft_depth_blend", fragments, True)
    sigma = float(blend_params.sigma)
    if not sigma > 0.0:
        raise ValueError("soft_depth_blend: blend_params.sigma must be positive")
    return _SoftDepthBlend.apply(fragments.dists, fragments.zbuf, fragments.pix_to_face, sigma, _depth_zfar(zfar, "soft_depth_blend"))


class _HardDepthBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, zbuf, pix_to_face, zfar):
        N, H, W, K = pix_to_face.shape
        dev = zbuf.device
        z, p2f = _C._aligned(zbuf), _C._aligned(pix_to_face)
        out = torch.empty((N, H, W, 1), dtype=torch.float32, device=dev)
        if out.numel():
            _lib.call("p3d_hard_depth_blend_forward", "hard_depth_blend", dev, z, p2f, zfar, N * H * W, K, out)
        ctx.save_for_backward(p2f)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, grad_depth):
        if grad_depth is None or not ctx.needs_input_grad[0]:
            return None, None, None
        (p2f,) = ctx.saved_tensors
        N, H, W, K = p2f.shape
        dev = p2f.device
        g = grad_depth.contiguous()
        gz = torch.empty((N, H, W, K), dtype=torch.float32, device=dev)
        if gz.numel():
            _lib.call("p3d_hard_depth_blend_backward", "hard_depth_blend_backward", dev, g, p2f, N * H * W, K, gz)
        return gz, None, None


def hard_depth_blend(fragments, zfar: Union[float, torch.Tensor] = 100.0) -> torch.Tensor:
    """HardDepthShader.forward (shader.py:392-400) after its camera lookup: zbuf[..., 0] where slot 0 holds a face, zfar
    elsewhere.  One kernel each way (p3d_hard_depth_blend_forward / _backward).  -> depth (N,H,W,1)."""
    _check_depth_fragments("hard_depth_blend", fragments, False)
    return _HardDepthBlend.apply(fragments.zbuf, fragments.pix_to_face, _depth_zfar(zfar, "hard_depth_blend"))
