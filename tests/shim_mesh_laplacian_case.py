#!/usr/bin/env python
"""The UNMODIFIED reference's pytorch3d.loss.mesh_laplacian_smoothing("cot" / "cotcurv"), pytorch3d.ops.cot_laplacian and
pytorch3d.ops.taubin_smoothing through pytorch3d_amd.shim with patch_python=True, on the GPU, in a process of its own (the shim
replaces sys.modules entries).  Prints one JSON line, read by tests/test_gpu_mesh_laplacian.py:

  * both names are rebound in every module that holds them (pytorch3d.ops, the defining modules, the loss module's global);
  * the reference's loss for "cot" / "cotcurv" -- the patched loss counts a fallback, its predicate stays method == "uniform" -- finds
    cot_laplacian served by the kernels (PATCH_CALLS["cot_laplacian"] fused) and stays within the gates of tests/mesh_laplacian_case.py;
  * taubin_smoothing(m) runs fused, within the gates, and returns the reference's Meshes without textures;
  * a CPU mesh, a face that names one vertex twice and an input that wants a gradient fall back; uninstall restores both names."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("cot_laplacian", "taubin_smoothing")
CASE = "batch"


def _reference_root():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    return next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "loss"))), None)


def gpu_report(ref_root):
    import torch

    import mesh_laplacian_case as C
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    d = torch.device("cuda:0")
    out = {}
    verts_list, faces_list = C.cases()[CASE]
    verts, faces, _, _ = C.packed(verts_list, faces_list)
    shim.install(ref_root, patch_python=True)
    import pytorch3d.loss as loss_mod
    import pytorch3d.ops as ops_mod
    from pytorch3d.structures import Meshes

    holders = {"cot_laplacian": ("pytorch3d.ops", "pytorch3d.ops.laplacian_matrices", "pytorch3d.loss.mesh_laplacian_smoothing"),
               "taubin_smoothing": ("pytorch3d.ops", "pytorch3d.ops.mesh_filtering")}
    patched = {n: getattr(ops_mod, n) for n in NAMES}
    out["patched_everywhere"] = all(getattr(patched[n], "__p3d_amd__", False) and all(getattr(sys.modules[h], n) is patched[n] for h in holders[n])
                                    for n in NAMES)

    def calls(names=NAMES):
        return {n: list(shim.PATCH_CALLS.get(n, [0, 0])) for n in names}

    def delta(before, after, which):
        return {n: after[n][which] - before[n][which] for n in before}

    def gpu_meshes(grad=False):
        v = [x.to(d).requires_grad_(grad) for x in verts_list]
        return Meshes(verts=v, faces=[f.to(d) for f in faces_list]), v

    # ---- the reference's loss for cot / cotcurv: cot_laplacian on the kernels ----------------------------------------------------
    before, loss_before = calls(), calls(("mesh_laplacian_smoothing",))
    out["losses"] = {}
    for method in C.METHODS:
        t_loss, t_grad, gate_l, gate_g, rec = C.loss_gates(CASE, method)
        m, v = gpu_meshes(grad=True)
        loss = loss_mod.mesh_laplacian_smoothing(m, method)
        grads = torch.autograd.grad(loss, [x for x in v if x.shape[0]])
        grad = torch.cat(list(grads), 0).cpu()
        out["losses"][method] = {"loss_error": abs(float(loss.detach()) - t_loss), "loss_gate": gate_l,
                                 "grad_error": float((grad.double() - t_grad).abs().max()), "grad_gate": gate_g, **rec}
    # ---- taubin_smoothing ----------------------------------------------------------------------------------------------------------
    edges = C.edges_of(faces, verts.shape[0])
    out["taubin"] = {}
    for it in C.TAUBIN_ITERS:
        m, _ = gpu_meshes()
        got = ops_mod.taubin_smoothing(m, C.LAMBD, C.MU, it) if it != 10 else ops_mod.taubin_smoothing(m)  # the defaults: 0.53, -0.53, 10
        out["taubin"][str(it)] = {"error": C.nan_aware_error(got.verts_packed().cpu(), C.taubin(verts, edges, it)), "gate": 4 * C.e32(CASE, f"taubin_{it}"),
                                  "is_reference_meshes": type(got) is Meshes and len(got) == len(verts_list), "no_textures": got.textures is None}
    after, loss_after = calls(), calls(("mesh_laplacian_smoothing",))
    out["fused_calls"], out["fallback_calls"] = delta(before, after, 0), delta(before, after, 1)
    out["loss_patch_counts_a_fallback"] = delta(loss_before, loss_after, 1)["mesh_laplacian_smoothing"]

    # ---- a CPU mesh, a repeated vertex and a gradient wanted fall back -----------------------------------------------------------
    def fallbacks(meshes, no_grad=True):
        before = calls()
        with torch.no_grad() if no_grad else torch.enable_grad():
            ops_mod.cot_laplacian(meshes.verts_packed(), meshes.faces_packed())
            ops_mod.taubin_smoothing(meshes, num_iter=1)
        after = calls()
        return delta(before, after, 1), delta(before, after, 0)

    out["cpu_fallback_calls"], out["cpu_fused_calls"] = fallbacks(Meshes(verts=verts_list, faces=faces_list))
    twice = Meshes(verts=[verts_list[0].to(d)], faces=[torch.cat([faces_list[0], torch.tensor([[0, 1, 1]])], 0).to(d)])
    out["repeated_fallback_calls"], out["repeated_fused_calls"] = fallbacks(twice)
    out["grad_wanted_fallback_calls"], _ = fallbacks(gpu_meshes(grad=True)[0], no_grad=False)

    # ---- restore ---------------------------------------------------------------------------------------------------------------
    shim.uninstall_python_patches()
    out["restored"] = all(getattr(sys.modules[h], n) is patched[n].__wrapped__ for n in NAMES for h in holders[n])
    print(json.dumps(out))


def main():
    ref_root = _reference_root()
    if ref_root is None:
        print(json.dumps({"skipped": "the reference's Python package is not on this machine"}))
        return
    gpu_report(ref_root)


if __name__ == "__main__":
    main()
