#!/usr/bin/env python
"""The scene of tests/golden/splatter_ref.npz (make_golden_splatter.py: render_case) rendered by the UNMODIFIED reference's
MeshRenderer(MeshRasterizer, SplatterPhongShader) on the GPU through pytorch3d_amd.shim.install(patch_python=True), in a process
of its own (the shim replaces sys.modules entries).  Prints one JSON line: deviations from the fixture and the patch record.
tests/test_gpu_splatter.py asserts on it."""
import json
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
    import numpy as np
    import torch

    import _util as U
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    shim.install(ref_root, patch_python=True)
    from pytorch3d.renderer import (BlendParams, FoVPerspectiveCameras, Materials, MeshRasterizer, MeshRenderer, PointLights,
                                    RasterizationSettings, SplatterPhongShader, TexturesVertex, look_at_view_transform)
    from pytorch3d.structures import Meshes

    g = np.load(os.path.join(U.GOLDEN, "splatter_ref.npz"))
    d = torch.device("cuda:0")
    nv, nf = g["render_num_verts"].tolist(), g["render_num_faces"].tolist()
    verts = torch.from_numpy(g["render_verts"]).to(d).split(nv)
    faces_packed = torch.from_numpy(g["render_faces"])
    cols = torch.from_numpy(g["render_verts_colors"]).to(d).split(nv)
    faces, off = [], 0
    for i, n in enumerate(nf):
        faces.append((faces_packed[off:off + n] - sum(nv[:i])).to(d))
        off += n
    verts_l = [v.clone().requires_grad_(True) for v in verts]
    cols_l = [c.clone().requires_grad_(True) for c in cols]
    meshes = Meshes(verts=verts_l, faces=faces, textures=TexturesVertex(verts_features=cols_l))
    R, T = look_at_view_transform(dist=2.7, elev=torch.from_numpy(g["render_elev"]), azim=torch.from_numpy(g["render_azim"]))
    cameras = FoVPerspectiveCameras(R=R, T=T, znear=1.0, zfar=100.0, device=d)
    settings = RasterizationSettings(image_size=40, blur_radius=0.0, faces_per_pixel=4, bin_size=0)
    lights = PointLights(location=((1.5, 2.0, -2.0), (-2.0, 1.0, -1.5)), ambient_color=((0.4, 0.4, 0.4),),
                         diffuse_color=((0.5, 0.4, 0.6),), specular_color=((0.3, 0.3, 0.3),), device=d)
    materials = Materials(shininess=24.0, device=d)
    blend = BlendParams(sigma=0.5, background_color=(0.2, 0.3, 0.4))
    renderer = MeshRenderer(MeshRasterizer(cameras=cameras, raster_settings=settings),
                            SplatterPhongShader(cameras=cameras, lights=lights, materials=materials, blend_params=blend, device=d))
    shim.PATCH_CALLS.clear()
    img = renderer(meshes)
    (img * torch.from_numpy(g["render_grad_image"]).to(d)).sum().backward()
    gv = torch.cat([v.grad for v in verts_l]).cpu()
    gc = torch.cat([c.grad for c in cols_l]).cpu()

    def dev(a, b):
        return float((a - b).abs().max()), float(b.abs().max())

    print(json.dumps({"calls": {k: list(v) for k, v in shim.PATCH_CALLS.items()},
                      "image": dev(img.detach().cpu(), torch.from_numpy(g["render_image"])),
                      "grad_verts": dev(gv, torch.from_numpy(g["render_grad_verts"])),
                      "grad_verts_colors": dev(gc, torch.from_numpy(g["render_grad_verts_colors"])),
                      "covered": float((img[..., 3] > 0).float().mean())}))


if __name__ == "__main__":
    main()
