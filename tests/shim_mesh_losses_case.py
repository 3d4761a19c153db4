#!/usr/bin/env python
"""The UNMODIFIED reference's pytorch3d.loss.mesh_edge_loss / mesh_laplacian_smoothing / mesh_normal_consistency through
pytorch3d_amd.shim, in a process of its own (the shim replaces sys.modules entries).  Prints one JSON line.

    --cpu-reference   no GPU: the reference's functions in float32 on the CPU on the batch of tests/mesh_losses_case.py (values,
                      gradients, edges_packed) -- the float32 formulation that scales the gates of the tests
    (default)         on the GPU: shim.install() alone runs the reference's normal consistency (the host find_verts operator); with
                      patch_python=True the three are fused, agree with the originals, the topology is handed on by offset_verts, a CPU
                      mesh and method="cot" fall back, uninstall restores; one SoftPhong fitting step with the three regularisers.
tests/test_gpu_mesh_losses.py and tests/mesh_losses_case.py read the line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("mesh_edge_loss", "mesh_laplacian_smoothing", "mesh_normal_consistency")


def _reference_root():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    return next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "loss"))), None)


def _call(loss_mod, name, meshes):
    """One of the cases of mesh_losses_case.LOSSES (+ cot, cotcurv) with the functions of `loss_mod`."""
    import mesh_losses_case as C

    if name in ("edge", "edge_target"):
        return loss_mod.mesh_edge_loss(meshes, C.TARGET if name == "edge_target" else 0.0)
    if name == "normal":
        return loss_mod.mesh_normal_consistency(meshes)
    return loss_mod.mesh_laplacian_smoothing(meshes, "uniform" if name == "laplacian" else name)


def cpu_reference(ref_root):
    import torch

    import mesh_losses_case as C
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    shim.install(ref_root)
    import pytorch3d.loss as loss_mod
    from pytorch3d.structures import Meshes

    verts, faces = C.build_batch()
    out = {"losses": {}}
    for name in C.LOSSES + ("cot", "cotcurv"):
        v = [x.clone().requires_grad_(True) for x in verts]
        m = Meshes(verts=v, faces=faces)
        loss = _call(loss_mod, name, m)
        grads = torch.autograd.grad(loss, v, allow_unused=True)
        grads = [g if g is not None else torch.zeros_like(x) for g, x in zip(grads, v)]
        out["losses"][name] = {"loss": float(loss.detach()), "grad": torch.cat(grads, 0).reshape(-1).tolist()}
    out["edges_packed"] = Meshes(verts=verts, faces=faces).edges_packed().tolist()
    print(json.dumps(out))


def gpu_report(ref_root):
    import torch

    import _util as U
    import mesh_losses_case as C
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim
    from pytorch3d_amd import mesh_losses as ours

    d = torch.device("cuda:0")
    out = {}
    verts, faces = C.build_batch()
    tables = C.brute_tables(verts, faces)

    # ---- shim.install() alone: the reference's own normal consistency runs (the host find_verts operator) -------------------------
    shim.install(ref_root)
    import pytorch3d.loss as loss_mod
    from pytorch3d.structures import Meshes

    t_loss, _, gate, _, rec = C.gates("normal", verts, faces, tables)
    plain = loss_mod.mesh_normal_consistency(Meshes(verts=[x.to(d) for x in verts], faces=[x.to(d) for x in faces]))
    out["install_alone"] = {"error": abs(float(plain.detach()) - t_loss), "gate": gate, **rec}

    # ---- patch_python=True -----------------------------------------------------------------------------------------------------
    shim.install(ref_root, patch_python=True)
    patched = {n: getattr(loss_mod, n) for n in NAMES}
    out["patched_everywhere"] = all(getattr(patched[n], "__p3d_amd__", False) and getattr(sys.modules["pytorch3d.loss." + n], n) is patched[n]
                                    for n in NAMES)

    def calls():
        return {n: list(shim.PATCH_CALLS.get(n, [0, 0])) for n in NAMES}

    def evaluate(fn_of, name, mesh_verts):
        m = Meshes(verts=mesh_verts, faces=[x.to(mesh_verts[0].device) for x in faces])
        loss = _call(fn_of, name, m)
        grads = torch.autograd.grad(loss, mesh_verts)
        return float(loss.detach()), torch.cat(list(grads), 0).cpu(), m

    class Originals:
        pass

    for n in NAMES:
        setattr(Originals, n, staticmethod(patched[n].__wrapped__))
    before = calls()
    out["cases"] = {}
    for name in C.LOSSES:
        t_loss, t_grad, gate_l, gate_g, rec = C.gates(name, verts, faces, tables)
        l_p, g_p, _ = evaluate(loss_mod, name, [x.to(d).requires_grad_(True) for x in verts])
        l_o, g_o, _ = evaluate(Originals, name, [x.to(d).requires_grad_(True) for x in verts])
        out["cases"][name] = {"patched_loss_error": abs(l_p - t_loss), "original_loss_error": abs(l_o - t_loss), "loss_gate": gate_l,
                              "patched_grad_error": float((g_p.double() - t_grad).abs().max()),
                              "original_grad_error": float((g_o.double() - t_grad).abs().max()), "grad_gate": gate_g,
                              "loss_difference": abs(l_p - l_o), "grad_difference": float((g_p - g_o).abs().max()), **rec}
    after = calls()
    out["fused_calls"] = {n: after[n][0] - before[n][0] for n in NAMES}
    out["fallback_calls"] = {n: after[n][1] - before[n][1] for n in NAMES}

    # ---- offset_verts hands the topology on ------------------------------------------------------------------------------------
    m = Meshes(verts=[x.to(d) for x in verts], faces=[x.to(d) for x in faces])
    loss_mod.mesh_edge_loss(m)
    kept = m.__dict__.get(ours._TOPOLOGY_KEY)
    m2 = m.offset_verts(torch.full((tables["V"], 3), 0.01, device=d))
    loss_mod.mesh_normal_consistency(m2)
    kept2 = m2.__dict__.get(ours._TOPOLOGY_KEY)
    out["offset_hands_topology_on"] = bool(kept is not None and kept2 is not None and kept2[1] is kept[1])

    # ---- a CPU mesh and method="cot" fall back -----------------------------------------------------------------------------------
    before = calls()
    m_cpu = Meshes(verts=verts, faces=faces)
    for n in NAMES:
        getattr(loss_mod, n)(m_cpu)
    loss_mod.mesh_laplacian_smoothing(m, "cot")
    after = calls()
    out["cpu_fallback_calls"] = {n: after[n][1] - before[n][1] for n in NAMES}
    out["cpu_fused_calls"] = {n: after[n][0] - before[n][0] for n in NAMES}

    # ---- a mesh of vertices alone inside the batch (0 edges: weight 1 / 0) is fused and finite; a face that names a vertex twice
    # ---- goes to the reference --------------------------------------------------------------------------------------------------
    lone_v, lone_f = C.build_with_a_mesh_of_vertices_alone()
    lone_tables = C.brute_tables(lone_v, lone_f)
    lone_f32 = C.package_formulation(lone_v, lone_f)
    before = calls()
    out["vertices_alone"] = {}
    for name in C.LOSSES:
        _, t_grad, _, gate_g, _ = C.gates(name, lone_v, lone_f, lone_tables, f32=lone_f32)
        mv = [x.to(d).requires_grad_(True) for x in lone_v]
        loss = _call(loss_mod, name, Meshes(verts=mv, faces=[x.to(d) for x in lone_f]))
        g = torch.cat(list(torch.autograd.grad(loss, mv)), 0).cpu()
        out["vertices_alone"][name] = {"finite": bool(torch.isfinite(g).all()), "grad_error": float((g.double() - t_grad).abs().max()),
                                       "grad_gate": gate_g, "rows_of_the_lone_vertices": float(g[:3].abs().max())}
    after = calls()
    out["vertices_alone_fused_calls"] = sum(after[n][0] - before[n][0] for n in NAMES)
    before = calls()
    twice = Meshes(verts=[verts[0].to(d)], faces=[torch.cat([faces[0], torch.tensor([[0, 1, 1]])], 0).to(d)])
    for n in NAMES:
        getattr(loss_mod, n)(twice)
    after = calls()
    out["repeated_vertex_fallback_calls"] = {n: after[n][1] - before[n][1] for n in NAMES}
    out["repeated_vertex_fused_calls"] = sum(after[n][0] - before[n][0] for n in NAMES)

    # ---- one fitting step: SoftPhong image term + the three regularisers -------------------------------------------------------
    from pytorch3d.renderer import (BlendParams, FoVPerspectiveCameras, MeshRasterizer, MeshRenderer, PointLights, RasterizationSettings,
                                    SoftPhongShader, TexturesVertex, look_at_view_transform)

    v, f = U.ico_sphere(1)
    gen = torch.Generator().manual_seed(3)
    R, T = look_at_view_transform(dist=2.7, elev=10.0, azim=20.0)
    cameras = FoVPerspectiveCameras(R=R, T=T, device=d)
    settings = RasterizationSettings(image_size=32, blur_radius=1e-4, faces_per_pixel=4)
    renderer = MeshRenderer(MeshRasterizer(cameras=cameras, raster_settings=settings),
                            SoftPhongShader(cameras=cameras, lights=PointLights(location=[[1.0, 2.0, 3.0]], device=d),
                                            blend_params=BlendParams(sigma=1e-4, gamma=1e-4), device=d))
    colors = (0.3 + 0.7 * torch.rand(v.shape, generator=gen)).to(d)
    target = torch.rand(1, 32, 32, 4, generator=gen).to(d)
    start = (v + 0.03 * torch.randn(v.shape, generator=gen)).to(d)

    def step():
        mesh = Meshes(verts=[start], faces=[f.to(d)], textures=TexturesVertex(verts_features=[colors]))
        offsets = torch.zeros(v.shape, device=d, requires_grad=True)
        moved = mesh.offset_verts(offsets)
        before = calls()
        loss = ((renderer(moved) - target) ** 2).mean() + 1.0 * loss_mod.mesh_edge_loss(moved) + 0.01 * loss_mod.mesh_normal_consistency(
            moved) + 1.0 * loss_mod.mesh_laplacian_smoothing(moved, method="uniform")
        loss.backward()
        torch.cuda.synchronize()
        after = calls()
        return offsets.grad.clone(), sum(after[n][0] - before[n][0] for n in NAMES)

    g_patched, n_fused = step()
    ours_entries = [p for p in shim._PATCHED if getattr(p[3], "__name__", None) in NAMES]
    for owner, attr, orig, _new in ours_entries:  # only the three losses restored
        setattr(owner, attr, orig)
    try:
        g_restored, n_fused_restored = step()
        g_again, _ = step()  # the image term's backward adds with float atomics: what two runs of the SAME code differ by
    finally:
        for owner, attr, _orig, new in ours_entries:
            setattr(owner, attr, new)
    # the regularisers' own gates on this mesh (offsets are zero: the vertices are `start`), weighted as in the loss
    step_v, step_f = [start.cpu()], [f]
    step_tables, step_f32 = C.brute_tables(step_v, step_f), C.package_formulation(step_v, step_f)
    reg = {name: C.gates(name, step_v, step_f, step_tables, f32=step_f32)[3] for name in ("edge", "laplacian", "normal")}
    out["step"] = {"fused_calls": n_fused, "fused_calls_when_restored": n_fused_restored, "finite": bool(torch.isfinite(g_patched).all()),
                   "max_diff": float((g_patched - g_restored).abs().max()), "largest": float(g_restored.abs().max()),
                   "same_code_twice": float((g_again - g_restored).abs().max()),
                   "regulariser_gates": 1.0 * reg["edge"] + 1.0 * reg["laplacian"] + 0.01 * reg["normal"]}

    # ---- restore ---------------------------------------------------------------------------------------------------------------
    shim.uninstall_python_patches()
    out["restored"] = all(getattr(loss_mod, n) is patched[n].__wrapped__ and getattr(sys.modules["pytorch3d.loss." + n], n) is patched[n].__wrapped__
                          for n in NAMES)
    print(json.dumps(out))


def main():
    ref_root = _reference_root()
    if ref_root is None:
        print(json.dumps({"skipped": "the reference's Python package is not on this machine"}))
        return
    if "--cpu-reference" in sys.argv:
        cpu_reference(ref_root)
    else:
        gpu_report(ref_root)


if __name__ == "__main__":
    main()
