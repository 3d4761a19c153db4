#!/usr/bin/env python
"""The UNMODIFIED reference's `pytorch3d.ops.iterative_closest_point` / `corresponding_points_alignment` through pytorch3d_amd.shim,
in a process of its own (the shim replaces sys.modules entries).  argv[1]: "cuda:0" (default) or "cpu".  Prints one JSON line that
tests/test_gpu_points_alignment.py reads:
* plain install(): the two functions are the reference's own, nothing is counted;
* patch_python=True: every module that holds the names sees the new functions; a call on tensors and a call on the reference's
  Pointclouds go through the kernels (PATCH_CALLS), return the REFERENCE's ICPSolution / SimilarityTransform classes and, for
  Pointclouds, a Pointclouds made by update_padded, and equal the package's direct call bit for bit; float64 clouds are counted as
  fallbacks;
* uninstall_python_patches() gives the reference's functions back."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("iterative_closest_point", "corresponding_points_alignment")
MODULES = ("pytorch3d.ops.points_alignment", "pytorch3d.ops")


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

    import points_alignment_case as C
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd as p3d
    import pytorch3d_amd.shim as shim

    d = torch.device(sys.argv[1] if len(sys.argv) > 1 else "cuda:0")
    out = {}

    def calls():
        return {n: list(shim.PATCH_CALLS.get(n, [0, 0])) for n in NAMES}

    shim.install(ref_root)
    ref_mod = importlib.import_module("pytorch3d.ops.points_alignment")
    importlib.import_module("pytorch3d.ops")
    orig = {n: getattr(ref_mod, n) for n in NAMES}
    out["unpatched_is_the_reference"] = not any(getattr(f, "__p3d_amd__", False) for f in orig.values())
    out["calls_before_patch"] = sum(sum(v) for v in calls().values())

    shim.install(ref_root, patch_python=True)
    import pytorch3d.ops as ref_ops
    from pytorch3d.structures import Pointclouds

    out["patched_everywhere"] = bool(all(getattr(getattr(sys.modules[m], n), "__p3d_amd__", False) and
                                         getattr(sys.modules[m], n).__wrapped__ is orig[n] for n in NAMES for m in MODULES))
    case = ("icp_scale", "130x70", 0)
    inputs = C.icp_inputs(case)
    X, Y = inputs["X"].to(d), inputs["Y"].to(d)
    before = calls()
    sol = ref_ops.iterative_closest_point(X, Y, estimate_scale=True)
    direct = p3d.iterative_closest_point(X, Y, estimate_scale=True)
    out["icp_equal"] = bool(torch.equal(sol.Xt, direct.Xt) and torch.equal(sol.rmse, direct.rmse) and len(sol.t_history) == len(direct.t_history)
                            and all(torch.equal(a, b) for a, b in zip(sol.RTs, direct.RTs)) and sol.converged == direct.converged)
    out["icp_types"] = bool(type(sol) is ref_mod.ICPSolution and type(sol.RTs) is ref_mod.SimilarityTransform
                            and all(type(t) is ref_mod.SimilarityTransform for t in sol.t_history))
    ragged = C.icp_inputs(("icp_ragged", "hetero", 0))
    clouds = [Pointclouds([ragged[k][n, :int(m)].to(d) for n, m in enumerate(ragged[ln])]) for k, ln in (("X", "lengths1"), ("Y", "lengths2"))]
    got = ref_ops.iterative_closest_point(*clouds)
    want = p3d.iterative_closest_point(C.Clouds(clouds[0].points_padded(), clouds[0].num_points_per_cloud()),
                                       C.Clouds(clouds[1].points_padded(), clouds[1].num_points_per_cloud()))
    out["pointclouds_updated"] = bool(isinstance(got.Xt, Pointclouds) and torch.equal(got.Xt.points_padded(), want.Xt.points_padded())
                                      and len(got.t_history) == len(want.t_history))
    align = C.align_inputs(("weights", "rand", 0))
    a = ref_ops.corresponding_points_alignment(align["X"].to(d), align["Y"].to(d), weights=align["weights"].to(d), estimate_scale=True)
    b = p3d.corresponding_points_alignment(align["X"].to(d), align["Y"].to(d), weights=align["weights"].to(d), estimate_scale=True)
    out["align_equal"] = bool(type(a) is ref_mod.SimilarityTransform and all(torch.equal(s, t) for s, t in zip(a, b)))
    after = calls()
    out["fused_calls"] = {n: after[n][0] - before[n][0] for n in NAMES}
    out["fallback_calls"] = {n: after[n][1] - before[n][1] for n in NAMES}
    before = calls()
    ref_ops.corresponding_points_alignment(align["X"].to(d).double(), align["Y"].to(d).double())
    out["float64_counted_as_fallback"] = calls()[NAMES[1]][1] - before[NAMES[1]][1]

    shim.uninstall_python_patches()
    out["restored"] = bool(all(getattr(sys.modules[m], n) is orig[n] for n in NAMES for m in MODULES))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
