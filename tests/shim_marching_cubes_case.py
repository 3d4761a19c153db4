#!/usr/bin/env python
"""The UNMODIFIED reference's `pytorch3d.ops.marching_cubes` through pytorch3d_amd.shim, in a process of its own (the shim replaces
sys.modules entries).  argv[1]: the device ("cuda:0" by default, "cpu").  Prints one JSON line that tests/test_cpu_marching_cubes.py and
tests/test_gpu_marching_cubes.py read:
* plain install(): the reference's own function, untouched in its one holder -- the module pytorch3d.ops.marching_cubes; the package
  pytorch3d.ops does not copy the name, there `marching_cubes` is the module --, runs over `_C.marching_cubes` of the shim: on CPU
  tensors it returns the fixture's records, on a GPU the device contract (the restatement's device form; its torch.unique finds every
  id once);
* patch_python=True: the module carries the batched replacement, the same results, PATCH_CALLS counts float32 GPU calls as fused and
  CPU calls as fallbacks;
* uninstall_python_patches() gives the reference's function back, and it still runs;
* on a GPU the result feeds the reference's Meshes, sample_points_from_meshes and mesh_laplacian_smoothing."""
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

    import marching_cubes_case as C
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    d = torch.device(sys.argv[1] if len(sys.argv) > 1 else "cuda:0")
    contract = "device" if d.type == "cuda" else "cpu"
    out = {"cases": len(C.cases())}

    def calls():
        return list(shim.PATCH_CALLS.get("marching_cubes", [0, 0]))

    shim.install(ref_root)
    import pytorch3d.ops as ref_ops

    module = importlib.import_module("pytorch3d.ops.marching_cubes")
    orig = module.marching_cubes
    out["plain_is_the_reference_function"] = bool(ref_ops.marching_cubes is module and not getattr(orig, "__p3d_amd__", False))
    out["plain_misses"] = C.failures(lambda v, i, l: module.marching_cubes(v, i, l), contract, device=d)
    out["calls_before_patch"] = sum(calls())

    shim.install(ref_root, patch_python=True)
    out["patched"] = bool(getattr(module.marching_cubes, "__p3d_amd__", False) and module.marching_cubes.__wrapped__ is orig
                          and ref_ops.marching_cubes is module)
    before = calls()
    out["patched_misses"] = C.failures(lambda v, i, l: module.marching_cubes(v, i, l), contract, device=d)
    after = calls()
    out["patched_calls"] = [after[0] - before[0], after[1] - before[1]]

    if d.type == "cuda":
        structures = importlib.import_module("pytorch3d.structures")
        loss = importlib.import_module("pytorch3d.loss")
        vol, iso = C.inputs("rand579", d)
        verts, faces = module.marching_cubes(vol, iso)
        meshes = structures.Meshes(verts=verts, faces=faces)
        samples = ref_ops.sample_points_from_meshes(meshes, 50)
        smooth = loss.mesh_laplacian_smoothing(meshes)
        out["feeds"] = [list(samples.shape), bool(torch.isfinite(samples).all() and torch.isfinite(smooth))]

    shim.uninstall_python_patches()
    out["restored"] = bool(module.marching_cubes is orig and ref_ops.marching_cubes is module)
    out["restored_misses"] = C.failures(lambda v, i, l: module.marching_cubes(v, i, l), contract, names=["rand345", "mixed_empty"], device=d)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
