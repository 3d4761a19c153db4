#!/usr/bin/env python
"""Cameras that are being optimised, through the UNMODIFIED reference classes on the GPU with
pytorch3d_amd.shim.install(patch_python=True), in a process of its own (the shim replaces sys.modules entries):

  mesh_fov_T              MeshRenderer(MeshRasterizer, SoftSilhouetteShader), FoVPerspectiveCameras whose T requires grad
                          (near-plane clipping by default: the speculative un-clipped path)
  mesh_fov_T_zclip        the same with shim.SPECULATE_NO_CLIPPING off: the z-clip path
  mesh_perspective_focal  PerspectiveCameras whose focal_length requires grad
  points_T                PointsRenderer(PointsRasterizer, AlphaCompositor), 2 000 points, T requires grad

Each step runs with the patches (shim.PATCH_CALLS says which branch ran) and again after shim.uninstall_python_patches():
the reference's own Python and torch autograd over the same `_C`.  The parameter gradients of the two are compared with
the tolerance of the world-transform tests (rtol 5e-3, atol 5e-4 * the largest reference entry).
Prints one JSON line; tests/test_gpu_camera_grad.py asserts on it."""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    ref_root = next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage)
                     if c and os.path.isdir(os.path.join(c, "pytorch3d", "renderer"))), None)
    if ref_root is None:
        print(json.dumps({"skipped": "the reference's Python package is not on this machine"}))
        return
    import torch

    import _util as U
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    shim.install(ref_root, patch_python=True)
    from pytorch3d.renderer import (AlphaCompositor, BlendParams, FoVPerspectiveCameras, MeshRasterizer, MeshRenderer,
                                    PerspectiveCameras, PointsRasterizationSettings, PointsRasterizer, PointsRenderer,
                                    RasterizationSettings, SoftSilhouetteShader, look_at_view_transform)
    from pytorch3d.structures import Meshes, Pointclouds

    d = torch.device("cuda:0")
    sigma, K = 1e-4, 4
    v0, f0 = U.ico_sphere(2)
    v1, f1 = U.torus(0.35, 0.9, 10, 14)
    R, T0 = look_at_view_transform(dist=2.7, elev=10.0, azim=20.0)
    R, T0 = R.to(d), T0.to(d)
    gen = torch.Generator().manual_seed(231)
    grad_mesh = torch.randn(2, 48, 48, 4, generator=gen).to(d)
    grad_points = torch.randn(1, 48, 48, 3, generator=gen).to(d)
    points = (torch.randn(2000, 3, generator=gen) * 0.45).to(d)
    colours = torch.rand(2000, 3, generator=gen).to(d)

    def mesh_step(make_cameras):
        def step():
            param, cameras = make_cameras()
            meshes = Meshes(verts=[v0.to(d), (v1 * 0.9).to(d)], faces=[f0.to(d), f1.to(d)])
            settings = RasterizationSettings(image_size=48, blur_radius=math.log(1.0 / 1e-4 - 1.0) * sigma, faces_per_pixel=K)
            renderer = MeshRenderer(MeshRasterizer(cameras=cameras, raster_settings=settings),
                                    SoftSilhouetteShader(blend_params=BlendParams(sigma=sigma)))
            (renderer(meshes) * grad_mesh).sum().backward()
            return param.grad.detach().clone()
        return step

    def fov_T():
        T = T0.clone().requires_grad_(True)
        return T, FoVPerspectiveCameras(R=R, T=T, znear=1.0, zfar=100.0, device=d)

    def perspective_focal():
        focal = torch.tensor([[2.0, 2.2]], device=d, requires_grad=True)
        return focal, PerspectiveCameras(focal_length=focal, R=R, T=T0, device=d)

    def points_step():
        T = T0.clone().requires_grad_(True)
        cameras = FoVPerspectiveCameras(R=R, T=T, znear=1.0, zfar=100.0, device=d)
        settings = PointsRasterizationSettings(image_size=48, radius=0.05, points_per_pixel=K)
        renderer = PointsRenderer(rasterizer=PointsRasterizer(cameras=cameras, raster_settings=settings), compositor=AlphaCompositor())
        (renderer(Pointclouds(points=[points], features=[colours])) * grad_points).sum().backward()
        return T.grad.detach().clone()

    cases = {"mesh_fov_T": (mesh_step(fov_T), True), "mesh_fov_T_zclip": (mesh_step(fov_T), False),
             "mesh_perspective_focal": (mesh_step(perspective_focal), True), "points_T": (points_step, True)}
    out, patched = {}, {}
    for name, (step, speculate) in cases.items():
        shim.SPECULATE_NO_CLIPPING = speculate
        shim.PATCH_CALLS.clear()
        patched[name] = step()
        torch.cuda.synchronize()
        out[name] = {"calls": {k: list(v) for k, v in shim.PATCH_CALLS.items()}}
    shim.SPECULATE_NO_CLIPPING = True
    shim.uninstall_python_patches()
    for name, (step, _) in cases.items():
        got, want = patched[name], step()
        scale = float(want.abs().max())
        close = torch.isclose(got, want, rtol=5e-3, atol=5e-4 * scale)
        out[name].update({"grad": got.flatten().tolist(), "reference_grad": want.flatten().tolist(),
                          "grad_finite": bool(torch.isfinite(got).all()), "grad_max": float(got.abs().max()),
                          "max_abs_diff": float((got - want).abs().max()), "beyond_tolerance": int((~close).sum())})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
