#!/usr/bin/env python
"""The UNMODIFIED reference's Meshes and MeshRenderer(MeshRasterizer, SoftPhongShader) on the GPU through
pytorch3d_amd.shim.install(patch_python=True), in a process of its own (the shim replaces sys.modules entries): what the patched
Meshes._compute_vertex_normals does -- fused count, agreement with the reference's method, the incidence list handed on by
offset_verts, the CPU fallback, the restore -- and one small render whose gradient to per-vertex offsets passes through the vertex
normals, with the patch and with only that one method restored.  Prints one JSON line; tests/test_gpu_mesh_normals.py asserts on it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAME = "Meshes._compute_vertex_normals"


def main():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    ref_root = next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage)
                     if c and os.path.isdir(os.path.join(c, "pytorch3d", "renderer"))), None)
    if ref_root is None:
        print(json.dumps({"skipped": "the reference's Python package is not on this machine"}))
        return
    import torch

    import _util as U
    import mesh_normals_case as C
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    shim.install(ref_root, patch_python=True)
    from pytorch3d.renderer import (BlendParams, FoVPerspectiveCameras, MeshRasterizer, MeshRenderer, PointLights, RasterizationSettings,
                                    SoftPhongShader, TexturesVertex, look_at_view_transform)
    from pytorch3d.structures import Meshes

    d = torch.device("cuda:0")
    out = {}
    patched = Meshes._compute_vertex_normals
    orig = patched.__wrapped__

    def calls():
        return list(shim.PATCH_CALLS.get(NAME, [0, 0]))

    # ---- the method itself, on the input of the kernel tests --------------------------------------------------------------------
    verts, faces, _ = C.build_input()
    truth = C.restated_forward(verts.double(), faces)[0]
    out["reference_cpu_error"] = float((C.reference_verts_normals(verts, faces).double() - truth).abs().max())
    m = Meshes(verts=[verts.to(d)], faces=[faces.to(d)])
    before = calls()
    ours = m.verts_normals_packed()
    out["fused_calls"] = calls()[0] - before[0]
    m.verts_normals_packed()  # cached: neither computed nor counted again
    out["calls_when_cached"] = calls()[0] - before[0] - out["fused_calls"]
    m_ref = Meshes(verts=[verts.to(d)], faces=[faces.to(d)])
    orig(m_ref)
    out["patched_vs_reference_method"] = float((ours - m_ref._verts_normals_packed).abs().max())
    out["patched_vs_truth"] = float((ours.double().cpu() - truth).abs().max())

    # ---- offset_verts hands the incidence list on -------------------------------------------------------------------------------
    gen = torch.Generator().manual_seed(3)
    off = (0.01 * torch.randn(verts.shape, generator=gen)).to(d)
    kept = m.__dict__["_p3d_amd_vert_incidence"]
    before = calls()
    m2 = m.offset_verts(off)
    n2 = m2.verts_normals_packed()
    kept2 = m2.__dict__["_p3d_amd_vert_incidence"]
    out["offset_fused_calls"] = calls()[0] - before[0]
    out["offset_reuses_list"] = bool(kept2[1] is kept[1] and kept2[2] is kept[2])
    moved = (verts.to(d) + off).cpu()  # the float32 sum the mesh holds
    truth2 = C.restated_forward(moved.double(), faces)[0]
    out["offset_vs_truth"] = float((n2.double().cpu() - truth2).abs().max())
    out["offset_reference_cpu_error"] = float((C.reference_verts_normals(moved, faces).double() - truth2).abs().max())

    # ---- a mesh on the CPU takes the reference's method -------------------------------------------------------------------------
    before = calls()
    n_cpu = Meshes(verts=[verts], faces=[faces]).verts_normals_packed()
    out["cpu_fallback_calls"] = calls()[1] - before[1]
    out["cpu_fused_calls"] = calls()[0] - before[0]
    out["cpu_equals_reference_formula"] = bool(torch.equal(n_cpu, C.reference_verts_normals(verts, faces)))

    # ---- end to end: the gradient of a SoftPhong render to per-vertex offsets ---------------------------------------------------
    v, f = U.ico_sphere(1)
    R, T = look_at_view_transform(dist=2.7, elev=10.0, azim=20.0)
    cameras = FoVPerspectiveCameras(R=R, T=T, device=d)
    settings = RasterizationSettings(image_size=32, blur_radius=1e-4, faces_per_pixel=4)
    lights = PointLights(location=[[1.0, 2.0, 3.0]], device=d)
    renderer = MeshRenderer(MeshRasterizer(cameras=cameras, raster_settings=settings),
                            SoftPhongShader(cameras=cameras, lights=lights, blend_params=BlendParams(sigma=1e-4, gamma=1e-4), device=d))
    colors = (0.3 + 0.7 * torch.rand(v.shape, generator=gen)).to(d)
    g_img = torch.randn(1, 32, 32, 4, generator=gen).to(d)

    def grad_of_offsets():
        mesh = Meshes(verts=[v.to(d)], faces=[f.to(d)], textures=TexturesVertex(verts_features=[colors]))
        offsets = torch.zeros(v.shape, device=d, requires_grad=True)
        before = calls()
        img = renderer(mesh.offset_verts(offsets))
        (img * g_img).sum().backward()
        torch.cuda.synchronize()
        return offsets.grad.clone(), calls()[0] - before[0]

    g_patched, n_fused = grad_of_offsets()
    Meshes._compute_vertex_normals = orig  # only this one method restored
    try:
        g_restored, n_fused_restored = grad_of_offsets()
    finally:
        Meshes._compute_vertex_normals = patched
    out["render"] = {"fused_calls": n_fused, "fused_calls_when_restored": n_fused_restored,
                     "max_diff": float((g_patched - g_restored).abs().max()), "largest": float(g_restored.abs().max()),
                     "finite": bool(torch.isfinite(g_patched).all())}

    # ---- restore --------------------------------------------------------------------------------------------------------------------
    shim.uninstall_python_patches()
    out["restored"] = bool(Meshes._compute_vertex_normals is orig)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
