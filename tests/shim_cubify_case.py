#!/usr/bin/env python
"""The UNMODIFIED reference's `pytorch3d.ops.cubify` through pytorch3d_amd.shim, in a process of its own (the shim replaces sys.modules
entries).  argv[1]: the device ("cuda:0" by default; "cpu" runs everything on the torch formulation).  Prints one JSON line that
tests/test_cpu_cubify.py and tests/test_gpu_cubify.py read:
* plain install(): no `_C` operator stands under cubify, so the reference's function is left alone, in both holders -- the module
  pytorch3d.ops.cubify and the package pytorch3d.ops, which copied the name;
* patch_python=True: both holders carry the replacement; every fixture case on the device equals the fixture (torch.equal on the
  Meshes' lists and the TexturesAtlas); PATCH_CALLS counts float32 GPU calls as fused and CPU / float64 calls as fallbacks; on a GPU
  the result feeds pytorch3d_amd.vert_align and sample_points_from_meshes;
* uninstall_python_patches() gives the reference's function back to both holders."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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

    import cubify_case as C
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    d = torch.device(sys.argv[1] if len(sys.argv) > 1 else "cuda:0")
    out = {}

    def calls():
        return list(shim.PATCH_CALLS.get("cubify", [0, 0]))

    def lists(meshes):
        return meshes.verts_list(), meshes.faces_list(), None if meshes.textures is None else meshes.textures.atlas_list()

    shim.install(ref_root)
    import pytorch3d.ops as ref_ops

    module = importlib.import_module("pytorch3d.ops.cubify")
    orig = module.cubify
    out["plain_leaves_cubify_alone"] = bool(ref_ops.cubify is orig and not getattr(orig, "__p3d_amd__", False))
    out["plain_misses"] = C.misses(lists(ref_ops.cubify(*C.inputs("solid3")[:2])), C.expected("solid3"), "solid3")
    out["calls_before_patch"] = sum(calls())

    shim.install(ref_root, patch_python=True)
    out["patched"] = bool(getattr(module.cubify, "__p3d_amd__", False) and module.cubify.__wrapped__ is orig and ref_ops.cubify is module.cubify)
    before = calls()
    out["device_misses"] = C.failures(lambda v, t, f, a: lists(ref_ops.cubify(v, t, feats=f, align=a)), device=d)
    mid = calls()
    out["host_misses"] = C.failures(lambda v, t, f, a: lists(ref_ops.cubify(v, t, feats=f, align=a)), names=["g2345_center_p7", "feats_center"])
    v, t, f, a = C.inputs("g2532_corner_p3", d)
    want = C.restate(v.double(), t, f, a)
    out["float64_misses"] = C.misses(lists(module.cubify(v.double(), t, align=a)), want, "float64")
    after = calls()
    out["device_calls"] = [mid[0] - before[0], mid[1] - before[1]]
    out["host_and_float64_calls"] = [after[0] - mid[0], after[1] - mid[1]]
    out["cases"] = len(C.cases())

    if d.type == "cuda":
        import pytorch3d_amd as p3d

        voxels, thresh, _, _ = C.inputs("g2345_topleft_p7", d)
        meshes = ref_ops.cubify(voxels, thresh)
        pooled = p3d.vert_align(torch.rand((len(meshes), 4, 6, 6), device=d), meshes)
        samples = p3d.sample_points_from_meshes(meshes, 50)
        out["feeds"] = [list(pooled.shape), list(samples.shape), bool(torch.isfinite(pooled).all() and torch.isfinite(samples).all())]

    shim.uninstall_python_patches()
    out["restored"] = bool(module.cubify is orig and ref_ops.cubify is orig)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
