#!/usr/bin/env python
"""Two small meshes rendered by the UNMODIFIED reference's MeshRenderer(MeshRasterizer, SoftDepthShader) and
MeshRenderer(MeshRasterizer, HardDepthShader) on the GPU through pytorch3d_amd.shim.install(patch_python=True), forward and
backward to the vertices, in a process of its own (the shim replaces sys.modules entries).  The image is compared with
tests/depth_restatement.py applied to the very fragments the rasterizer returned in this process (captured by a forward hook).
Prints one JSON line; tests/test_gpu_depth_blend.py asserts on it."""
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
    import depth_restatement as dr
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    shim.install(ref_root, patch_python=True)
    from pytorch3d.renderer import (BlendParams, FoVPerspectiveCameras, MeshRasterizer, MeshRenderer, RasterizationSettings,
                                    look_at_view_transform)
    from pytorch3d.renderer.mesh.shader import HardDepthShader, SoftDepthShader  # (not re-exported by pytorch3d.renderer)
    from pytorch3d.structures import Meshes

    d = torch.device("cuda:0")
    sigma, K, zfar = 1e-4, 4, 100.0
    v0, f0 = U.ico_sphere(2)
    v1, f1 = U.torus(0.35, 0.9, 10, 14)
    R, T = look_at_view_transform(dist=2.7, elev=10.0, azim=20.0)
    cameras = FoVPerspectiveCameras(R=R, T=T, znear=1.0, zfar=zfar, device=d)  # one camera for both meshes: zfar is a (1,) tensor
    settings = RasterizationSettings(image_size=48, blur_radius=math.log(1.0 / 1e-4 - 1.0) * sigma, faces_per_pixel=K)
    gen = torch.Generator().manual_seed(11)
    grad_image = torch.randn(2, 48, 48, 1, generator=gen).to(d)
    out = {}
    for cls in (SoftDepthShader, HardDepthShader):
        verts_l = [v0.to(d).requires_grad_(True), (v1 * 0.9).to(d).requires_grad_(True)]
        meshes = Meshes(verts=verts_l, faces=[f0.to(d), f1.to(d)])
        renderer = MeshRenderer(MeshRasterizer(cameras=cameras, raster_settings=settings),
                                cls(cameras=cameras, blend_params=BlendParams(sigma=sigma), device=d))
        seen = []
        renderer.rasterizer.register_forward_hook(lambda module, args, result: seen.append(result))
        shim.PATCH_CALLS.clear()
        img = renderer(meshes)
        (img * grad_image).sum().backward()
        torch.cuda.synchronize()
        (frags,) = seen
        p2f, zbuf, dists = frags.pix_to_face.detach(), frags.zbuf.detach(), frags.dists.detach()
        gv = torch.cat([v.grad for v in verts_l])
        rec = {"calls": {k: list(v) for k, v in shim.PATCH_CALLS.items()}, "shape": list(img.shape),
               "covered": float((p2f[..., 0] >= 0).float().mean()), "grad_finite": bool(torch.isfinite(gv).all()),
               "grad_max": float(gv.abs().max())}
        if cls is SoftDepthShader:
            want = dr.soft_depth_restated(p2f, zbuf, dists, sigma, zfar)
            rec["error"] = float((img.detach().double() - want).abs().max())
            rec["bound"] = dr.output_bound(K, zfar, zbuf)
            rec["soft_pixels"] = float(((img.detach() - dr.hard_depth_restated(p2f, zbuf, zfar)).abs() > 1e-3).float().mean())
        else:
            rec["equal"] = bool(torch.equal(img.detach(), dr.hard_depth_restated(p2f, zbuf, zfar)))
        out[cls.__name__] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
