#!/usr/bin/env python
"""`pytorch3d._C.points_to_volumes_forward / _backward` of pytorch3d_amd.shim, and on the CPU the UNMODIFIED reference's
`pytorch3d.ops.add_pointclouds_to_volumes` / `add_points_features_to_volume_densities_features` on top of them, in a process of its
own (the shim replaces sys.modules entries).  argv[1]: "cuda" (default) or "cpu".  Prints one JSON line that
tests/test_gpu_points_to_volumes.py / tests/test_cpu_points_to_volumes.py read:
* both flavours of the shim module have the two operators, and they give the golden of tests/golden/points_to_volumes_ref.npz
  (lattice cases: bit-equal; random cases: within the bound of the float64 restatement);
* "cpu" only -- the reference is imported in this leg alone --: under plain install() the reference's own functions run on those
  operators, forward and backward, and give the golden; patch_python=True rebinds both functions in every module that holds the
  names, the golden again, PATCH_CALLS shows what ran, `_python=True` still reaches the reference's Python twin, and
  uninstall_python_patches() gives the reference's functions back."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("add_pointclouds_to_volumes", "add_points_features_to_volume_densities_features")
HOLDERS = ("pytorch3d.ops.points_to_volumes", "pytorch3d.ops")


def _reference_root():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    return next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "ops"))), None)


def _judged(case, inp, got):
    import points_to_volumes_case as C

    try:
        C.judge(case, inp, got)
        return True
    except AssertionError as e:
        print("MISMATCH", e, file=sys.stderr)
        return False


def main():
    import contextlib

    import torch

    import points_to_volumes_case as C
    import pytorch3d_amd.shim as shim

    device = sys.argv[1] if len(sys.argv) > 1 else "cuda"
    d = torch.device("cuda:0" if device == "cuda" else "cpu")
    out = {}
    cases = [c for c in C.all_cases() if c[1] in ("mixed_grids", "contended", "ragged")]

    # ---- the operators of the shim module, both flavours (no reference needed) -------------------------------------------------------
    out["operators_exist"], ok = {}, True
    for flavour in ("ctypes", "pybind"):
        try:
            mod = shim.make_module(flavour)
        except Exception as e:  # noqa: BLE001 -- the pybind flavour is optional (no host compiler): reported, not hidden
            out["operators_exist"][flavour] = repr(e)
            continue
        out["operators_exist"][flavour] = bool(callable(getattr(mod, "points_to_volumes_forward", None))
                                               and callable(getattr(mod, "points_to_volumes_backward", None)))
        with contextlib.redirect_stdout(sys.stderr):
            for case in cases:
                inp = C.inputs(case)
                ok = _judged(case, inp, C.run_operators(case, inp, d, mod.points_to_volumes_forward, mod.points_to_volumes_backward)) and ok
    out["operators_match_fixture"] = ok
    if device != "cpu":
        print(json.dumps(out))
        return

    # ---- the reference's own Python on the shim's operators (CPU leg only) -----------------------------------------------------------
    ref_root = _reference_root()
    if ref_root is None:
        print(json.dumps({"skipped": "the reference's Python package is not on this machine"}))
        return
    import importlib

    import run_reference_suite as rrs

    rrs._stub_missing_packages()

    def through(fn_tensors, fn_clouds):
        good = True
        with contextlib.redirect_stdout(sys.stderr):
            for case in cases:
                if C.inputs(case)["point_weight"] != 1.0:  # (the public functions add with weight 1)
                    continue
                inp = C.inputs(case)
                mode, align = case[2], case[3]
                pts, feats = inp["points_3d"].clone().requires_grad_(True), inp["features"].clone().requires_grad_(True)
                feat, dens = fn_tensors(pts, feats, inp["densities"].clone(), inp["volume_features"].clone(), mode=mode, mask=inp["mask"],
                                        grid_sizes=inp["grid_sizes"], rescale_features=False, align_corners=align)
                torch.autograd.backward((dens, feat), (inp["grad_densities"], inp["grad_features"]))
                got = {"densities": dens.detach(), "features": feat.detach(), "grad_points_features": feats.grad}
                if mode == "trilinear":
                    got["grad_points_3d"] = pts.grad
                good = _judged(case, inp, got) and good
                if case[0] == "lattice":
                    clouds, vols = C.stand_ins(inp, align)
                    res = fn_clouds(clouds, vols, mode=mode, rescale_features=False)
                    z = C.fixture()
                    good = good and torch.equal(res.densities(), z[C.key(case, "densities")]) and \
                        torch.equal(res.features(), z[C.key(case, "features")])
        return bool(good)

    def calls():
        return {n: list(shim.PATCH_CALLS.get(n, [0, 0])) for n in NAMES}

    shim.install(ref_root)
    import pytorch3d.ops as ref_ops

    ref_mod = importlib.import_module("pytorch3d.ops.points_to_volumes")
    orig = {n: getattr(ref_mod, n) for n in NAMES}
    out["unpatched_is_the_reference"] = not any(getattr(f, "__p3d_amd__", False) for f in orig.values())
    out["plain_reference_matches_fixture"] = through(ref_ops.add_points_features_to_volume_densities_features, ref_ops.add_pointclouds_to_volumes)
    out["calls_before_patch"] = sum(sum(v) for v in calls().values())

    shim.install(ref_root, patch_python=True)
    out["patched_everywhere"] = bool(all(getattr(getattr(sys.modules[m], n), "__p3d_amd__", False) for n in NAMES for m in HOLDERS)
                                     and all(getattr(ref_mod, n).__wrapped__ is orig[n] for n in NAMES))
    before = calls()
    out["patched_matches_fixture"] = through(ref_ops.add_points_features_to_volume_densities_features, ref_ops.add_pointclouds_to_volumes)
    after = calls()
    out["fused_calls"] = {n: after[n][0] - before[n][0] for n in NAMES}
    out["fallback_calls"] = {n: after[n][1] - before[n][1] for n in NAMES}
    # `_python=True` asks for the reference's Python twin, a different function: it must still be reached (half to even: 0, 2, 2)
    pts = torch.tensor([[[-0.75, -1.0, -1.0], [-0.25, -1.0, -1.0], [0.25, -1.0, -1.0]]])
    _, dens = ref_mod.add_points_features_to_volume_densities_features(pts, torch.ones(1, 3, 1), torch.zeros(1, 1, 5, 5, 5),
                                                                       torch.zeros(1, 1, 5, 5, 5), mode="nearest", _python=True)
    out["python_twin_still_the_reference"] = dens[0, 0, 0, 0].tolist() == [1.0, 0.0, 2.0, 0.0, 0.0]

    shim.uninstall_python_patches()
    out["restored"] = bool(all(getattr(sys.modules[m], n) is orig[n] for n in NAMES for m in HOLDERS))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
