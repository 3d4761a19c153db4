#!/usr/bin/env python
"""The UNMODIFIED reference's `Pointclouds.estimate_normals` / `pytorch3d.ops.estimate_pointcloud_normals` through
pytorch3d_amd.shim, in a process of its own (the shim replaces sys.modules entries).  argv[1]: "cuda:0" (default) or "cpu".  Prints
one JSON line that tests/test_gpu_point_frames.py reads:
* plain install(): the two functions are the reference's own, nothing is counted;
* patch_python=True: every module that holds the names sees the new functions; the reference's Pointclouds.estimate_normals(
  neighborhood_size=50, assign_to_self=True), which resolves `ops.estimate_pointcloud_normals` at call time, goes through the
  kernel (PATCH_CALLS), and what it stores equals the package's direct call bit for bit; float64 clouds are counted as fallbacks;
* uninstall_python_patches() gives the reference's functions back."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("estimate_pointcloud_normals", "estimate_pointcloud_local_coord_frames")
MODULES = ("pytorch3d.ops.points_normals", "pytorch3d.ops")


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

    import point_frames_case as C
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd as p3d
    import pytorch3d_amd.shim as shim

    d = torch.device(sys.argv[1] if len(sys.argv) > 1 else "cuda:0")
    out = {}

    def calls():
        return {n: list(shim.PATCH_CALLS.get(n, [0, 0])) for n in NAMES}

    shim.install(ref_root)
    ref_mod = importlib.import_module("pytorch3d.ops.points_normals")
    importlib.import_module("pytorch3d.ops")
    orig = {n: getattr(ref_mod, n) for n in NAMES}
    out["unpatched_is_the_reference"] = not any(getattr(f, "__p3d_amd__", False) for f in orig.values())
    out["calls_before_patch"] = sum(sum(v) for v in calls().values())

    shim.install(ref_root, patch_python=True)
    from pytorch3d.structures import Pointclouds

    out["patched_everywhere"] = bool(all(getattr(getattr(sys.modules[m], n), "__p3d_amd__", False) and
                                         getattr(sys.modules[m], n).__wrapped__ is orig[n] for n in NAMES for m in MODULES))
    pts, lengths = C.inputs(("sphere", 50))
    clouds = Pointclouds([pts[n, :int(length)].to(d) for n, length in enumerate(lengths)])
    before = calls()
    stored = clouds.estimate_normals(neighborhood_size=50, assign_to_self=True)
    after = calls()
    direct = p3d.estimate_pointcloud_normals(C.Clouds(pts.to(d), lengths.to(d)), neighborhood_size=50)
    out["estimate_normals_equal"] = bool(torch.equal(stored, direct) and torch.equal(clouds.normals_padded(), direct))
    out["estimate_normals_nonzero"] = bool(direct.abs().sum() > 0)
    out["fused_calls"] = {n: after[n][0] - before[n][0] for n in NAMES}
    out["fallback_calls"] = {n: after[n][1] - before[n][1] for n in NAMES}
    import pytorch3d.ops as ref_ops

    before = calls()
    ref_ops.estimate_pointcloud_local_coord_frames(pts.to(d).double()[:1, :60], neighborhood_size=8)
    out["float64_counted_as_fallback"] = calls()[NAMES[1]][1] - before[NAMES[1]][1]

    shim.uninstall_python_patches()
    out["restored"] = bool(all(getattr(sys.modules[m], n) is orig[n] for n in NAMES for m in MODULES))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
