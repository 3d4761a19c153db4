#!/usr/bin/env python
"""The UNMODIFIED reference's `pytorch3d.ops.GraphConv` / `gather_scatter` / `vert_align` through pytorch3d_amd.shim, in a process of
its own (the shim replaces sys.modules entries).  argv[1]: the device ("cuda:0" by default).  Prints one JSON line that
tests/test_gpu_graph_conv.py and tests/test_gpu_vert_align.py read:
* plain install(): the reference's own GraphConv and GatherScatter run on `_C.gather_scatter`, directed and undirected, forward and
  backward to weights and input, and pass the gates of tests/mesh_refine_case.py on every gc_* / gs_* case; vert_align is left alone
  (no `_C` operator stands under it);
* patch_python=True: every module that holds the names sees the new functions; the gc_* cases again; and a refinement stage
  (vert_align of two maps, three GraphConv layers, Linear(., 3), offset_verts on a batch of ico_sphere(1) and ico_sphere(2)) passes
  the gates against the reference's CPU run of the same stage: MARGIN x that run's own float32 error against a float64 run (never
  below one float32 ulp of the quantity's largest value), PATCH_CALLS showing fused calls only;
* uninstall_python_patches() gives the reference's functions back."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("vert_align", "GraphConv.forward", "gather_scatter")


def _reference_root():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    return next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "ops"))), None)


def main():
    ref_root = _reference_root()
    if ref_root is None:
        print(json.dumps({"skipped": "the reference's Python package is not on this machine"}))
        return
    import importlib

    import torch

    import mesh_refine_case as C
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    d = torch.device(sys.argv[1] if len(sys.argv) > 1 else "cuda:0")
    out = {}

    def calls():
        return {n: list(shim.PATCH_CALLS.get(n, [0, 0])) for n in NAMES}

    # ---- plain install: the reference's own Python on the shim's operator ------------------------------------------------------------
    shim.install(ref_root)
    import pytorch3d.ops as ref_ops

    gc_mod = importlib.import_module("pytorch3d.ops.graph_conv")
    va_mod = importlib.import_module("pytorch3d.ops.vert_align")
    orig = {"gather_scatter": gc_mod.gather_scatter, "forward": gc_mod.GraphConv.forward, "vert_align": va_mod.vert_align}
    out["unpatched_is_the_reference"] = not any(getattr(f, "__p3d_amd__", False) or hasattr(f, "__wrapped__") for f in orig.values())

    def reference_layer(verts, edges, w0, b0, w1, b1, directed):
        layer = ref_ops.GraphConv(w0.shape[1], w0.shape[0], directed=directed)  # whatever forward the class has NOW
        params = {"w0.weight": w0, "w0.bias": b0, "w1.weight": w1, "w1.bias": b1}
        return torch.func.functional_call(layer, params, (verts, edges))

    def layer_misses():
        return [m for name in C.gc_cases() for m in C.gate(name, C.run_gc(name, reference_layer, d))]

    out["plain_misses"] = layer_misses()
    out["plain_gather_scatter_misses"] = [m for name in C.gs_cases() for m in C.gate(name, C.run_gs(name, gc_mod.gather_scatter, d))]
    out["plain_leaves_vert_align_alone"] = ref_ops.vert_align is orig["vert_align"]
    out["calls_before_patch"] = sum(sum(v) for v in calls().values())

    # ---- the refinement stage ---------------------------------------------------------------------------------------------------------
    from pytorch3d.structures import join_meshes_as_batch
    from pytorch3d.utils import ico_sphere

    gen = torch.Generator().manual_seed(31)
    maps = [torch.randn((2, 8, 14, 14), generator=gen), torch.randn((2, 16, 7, 7), generator=gen)]
    dims = [(27, 32), (32, 32), (32, 32)]
    weights = [torch.randn(s, generator=gen) * 0.3 for a, b in dims for s in ((b, a), (b,), (b, a), (b,))] + \
              [torch.randn((3, 32), generator=gen) * 0.3, torch.randn((3,), generator=gen) * 0.1]
    target = torch.randn((12 + 42 + 30 + 120, 3), generator=gen)[: 42 + 162]

    def stage(device, dtype, vert_align, graph_conv):
        """{quantity: tensor}: the refined vertices, and the gradients of <refined, target> to the maps and every weight."""
        meshes = join_meshes_as_batch([ico_sphere(1), ico_sphere(2)]).to(device)
        meshes = meshes.scale_verts(0.8)
        leaves = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in maps + weights]
        f, w = leaves[:2], leaves[2:]
        verts = meshes.verts_padded().to(dtype)
        lookup = meshes if dtype == torch.float32 else _Padded(verts, meshes.verts_padded_to_packed_idx())
        x = torch.cat([vert_align(f, lookup, return_packed=True), meshes.verts_packed().to(dtype)], 1)
        edges = meshes.edges_packed()
        for i in range(3):
            x = torch.relu(graph_conv(x, edges, *w[4 * i:4 * i + 4], False))
        offsets = torch.nn.functional.linear(x, w[12], w[13])
        refined = meshes.offset_verts(offsets.float()).verts_packed() if dtype == torch.float32 else meshes.verts_packed().to(dtype) + offsets
        grads = torch.autograd.grad((refined * target.to(device=device, dtype=dtype)).sum(), leaves)
        return dict(zip(["refined"] + ["g%d" % i for i in range(len(leaves))], (refined,) + grads))

    class _Padded:  # (Meshes is float32: the float64 run hands vert_align the padded tensor and the index directly)
        def __init__(self, padded, idx):
            self.padded, self.idx = padded, idx

        def verts_padded(self):
            return self.padded

        def verts_padded_to_packed_idx(self):
            return self.idx

    ours_gc = importlib.import_module("pytorch3d_amd.graph_conv")
    ours_va = importlib.import_module("pytorch3d_amd.vert_align")
    ref32 = stage(torch.device("cpu"), torch.float32, ref_ops.vert_align, reference_layer)   # the reference's CPU run
    ref64 = stage(torch.device("cpu"), torch.float64, ours_va.vert_align_torch, ours_gc.graph_conv)  # float64: the torch formulations

    # ---- patch_python -----------------------------------------------------------------------------------------------------------------
    shim.install(ref_root, patch_python=True)
    out["patched"] = bool(getattr(ref_ops.vert_align, "__p3d_amd__", False) and ref_ops.vert_align.__wrapped__ is orig["vert_align"]
                          and getattr(gc_mod.gather_scatter, "__p3d_amd__", False) and gc_mod.gather_scatter.__wrapped__ is orig["gather_scatter"]
                          and ref_ops.GraphConv.forward.__wrapped__ is orig["forward"] and va_mod.vert_align is ref_ops.vert_align)
    out["patched_misses"] = layer_misses()
    before = calls()
    got = stage(d, torch.float32, ref_ops.vert_align, reference_layer)
    after = calls()
    misses, figures = [], {}
    for q, want in ref32.items():
        w64 = ref64[q].detach()
        ref_err = (want.detach().double() - w64).abs().max().item()
        tol = max(C.MARGIN * ref_err, C.ulp32(w64.abs().max()))
        g = got[q].detach().cpu().double()
        errs = ((g - w64).abs().max().item(), (g - want.detach().double()).abs().max().item())
        figures[q] = [errs[0], errs[1], tol]
        if not (errs[0] <= tol and errs[1] <= tol):
            misses.append("%s: %.3g from float64, %.3g from the reference's CPU run, bound %.3g" % (q, errs[0], errs[1], tol))
    out["stage_misses"], out["stage_figures"] = misses, figures
    out["stage_fused_calls"] = {n: after[n][0] - before[n][0] for n in NAMES if after[n][0] - before[n][0]}
    out["stage_fallback_calls"] = sum(after[n][1] - before[n][1] for n in NAMES)

    # ---- restore ----------------------------------------------------------------------------------------------------------------------
    shim.uninstall_python_patches()
    out["restored"] = bool(gc_mod.gather_scatter is orig["gather_scatter"] and gc_mod.GraphConv.forward is orig["forward"]
                           and va_mod.vert_align is orig["vert_align"] and ref_ops.vert_align is orig["vert_align"]
                           and ref_ops.GraphConv.forward is orig["forward"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
