"""SplatterPhongShader's blend (pytorch3d/renderer/splatter_blend.py, Cole et al., "Differentiable Surface Rendering via
Non-differentiable Sampling") over the C ABI: one kernel forward, two backward (csrc/splatter.hip).

    splatter_blend(colors, pixel_coords_screen, background_mask, blend_params) -> RGBA (N,H,W,4)

is everything SplatterBlender.forward does after `cameras.transform_points_screen`: masking, the 9-direction occlusion
layers, splat weights, the three-buffer accumulation, normalisation and compositing.  The reference materialises several
(N,H,W,K,9,5) tensors for it (24 GB each at 64 x 512^2 x K = 8); here nothing of size 9 x K per pixel reaches memory.
Gradients flow to the colours and the screen x, y (z selects layers only and gets zero), without atomics: two backward
runs are bit-identical.  `SplatterBlender` keeps the reference's constructor and forward and calls the camera object
for the screen transform, so every camera class works.  `phong_shading_with_pixels` mirrors the reference's
`_phong_shading_with_pixels` (renderer/mesh/shading.py:60-97) with the fused Phong and interpolation kernels.
"""
from typing import Tuple

import torch

from . import _C, _lib
from .blending import _background
from .interp_face_attrs import interpolate_face_attributes
from .rasterize_meshes import gather_face_verts
from .shading import phong_shading


class _SplatterBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, colors, coords, mask, sigma, bg):
        N, H, W, K, _ = colors.shape
        dev = colors.device
        c, x, m = colors.contiguous(), coords.contiguous(), mask.contiguous()
        out = torch.empty((N, H, W, 4), dtype=torch.float32, device=dev)
        if out.numel():
            _lib.call("p3d_splatter_blend_forward", "splatter_blend", dev, c, x, m, sigma, bg, N, H, W, K, out)
        ctx.save_for_backward(c, x, m)
        ctx.meta = (sigma, bg)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        c, x, m = ctx.saved_tensors
        sigma, bg = ctx.meta
        N, H, W, K, _ = c.shape
        dev = c.device
        g = grad_out.contiguous()
        lib = _lib.load()
        gc = torch.empty_like(c)
        gx = torch.empty_like(x)
        if gc.numel():
            nbytes = lib.p3d_splatter_blend_backward_workspace_bytes(N, H, W)
            ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
            _lib.call("p3d_splatter_blend_backward", "splatter_blend_backward", dev, g, c, x, m, sigma, bg, N, H, W, K, gc, gx, ws, nbytes)
        return gc, gx, None, None, None


def splatter_blend(colors, pixel_coords_screen, background_mask, blend_params) -> torch.Tensor:
    """colors (N,H,W,K,3), pixel_coords_screen (N,H,W,K,3) (screen xyz, `with_xyflip=False`), background_mask (N,H,W,K)
    bool (`pix_to_face < 0`) -> RGBA (N,H,W,4).  Uses blend_params.sigma and .background_color.  Strided inputs are made
    contiguous here."""
    for name, t in (("colors", colors), ("pixel_coords_screen", pixel_coords_screen), ("background_mask", background_mask)):
        _C._need_gpu(t, name)
    for name, t in (("colors", colors), ("pixel_coords_screen", pixel_coords_screen)):
        if t.dtype != torch.float32:
            raise RuntimeError(f"splatter_blend: {name} must be float32, got {t.dtype}")
        if t.dim() != 5 or t.shape[-1] != 3:
            raise ValueError(f"splatter_blend: {name} must have shape (N, H, W, K, 3); got {tuple(t.shape)}")
    if pixel_coords_screen.shape != colors.shape:
        raise ValueError("splatter_blend: colors and pixel_coords_screen must have the same shape")
    if background_mask.dtype != torch.bool or tuple(background_mask.shape) != tuple(colors.shape[:4]):
        raise ValueError("splatter_blend: background_mask must be a bool tensor of shape (N, H, W, K)")
    if len({colors.device, pixel_coords_screen.device, background_mask.device}) != 1:
        raise RuntimeError("splatter_blend: all tensors must be on the same GPU")
    sigma = float(blend_params.sigma)
    if sigma <= 0.0:
        raise ValueError("Only positive standard deviations make sense.")  # splatter_blend.py:_get_splat_kernel_normalization
    if colors.shape[3] < 1:
        raise ValueError("splatter_blend: K must be at least 1")
    bg = _background(blend_params, colors.device, "splatter_blend")
    return _SplatterBlend.apply(colors, pixel_coords_screen, background_mask, sigma, bg)


class SplatterBlender(torch.nn.Module):
    """splatter_blend.py's SplatterBlender: same constructor and forward.  The shape given to the constructor is kept for
    reference; the kernel takes the shape of every call (no precomputed index tensors)."""

    def __init__(self, input_shape: Tuple[int, int, int, int], device):
        super().__init__()
        self.input_shape = tuple(input_shape)

    def to(self, device):
        return self

    def forward(self, colors, pixel_coords_cameras, cameras, background_mask, blend_params) -> torch.Tensor:
        N, H, W, K, _ = colors.shape
        pixel_coords_screen = cameras.transform_points_screen(
            pixel_coords_cameras.reshape([N, -1, 3]), image_size=(H, W), with_xyflip=False).reshape(pixel_coords_cameras.shape)
        return splatter_blend(colors, pixel_coords_screen, background_mask, blend_params)


def phong_shading_with_pixels(meshes, fragments, lights, cameras, materials, texels) -> Tuple[torch.Tensor, torch.Tensor]:
    """shading.py:60-97 -> (colors (N,H,W,K,3), pixel coordinates in the camera frame (N,H,W,K,3)): the fused Phong kernel
    and the interpolation kernel over the faces' vertex positions."""
    colors = phong_shading(meshes, fragments, lights, cameras, materials, texels)
    faces_verts = gather_face_verts(meshes.verts_packed(), meshes.faces_packed())
    pixel_coords = interpolate_face_attributes(fragments.pix_to_face, fragments.bary_coords, faces_verts)
    return colors, pixel_coords
