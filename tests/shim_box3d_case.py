#!/usr/bin/env python
"""The UNMODIFIED reference's `pytorch3d.ops.box3d_overlap` through pytorch3d_amd.shim, in a process of its own (the shim replaces
sys.modules entries).  argv[1]: "cuda:0" (default) or "cpu".  Prints one JSON line that tests/test_gpu_box3d.py /
tests/test_cpu_box3d.py read:
* plain install(): the reference's own function (its four input checks, its autograd node) runs on `_C.iou_box3d` and passes the
  gates of tests/box3d_case.py on every case; its backward raises the reference's ValueError; its input checks raise;
* patch_python=True: every module that holds the name sees the new function, the gates again, PATCH_CALLS shows what ran;
* uninstall_python_patches() gives the reference's function back."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HOLDERS = ("pytorch3d.ops.iou_box3d", "pytorch3d.ops")


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

    import box3d_case as C
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    d = torch.device(sys.argv[1] if len(sys.argv) > 1 else "cuda:0")
    z = C.fixture()
    out = {}

    def misses(fn):
        bad = []
        for name in C.all_cases():
            b1, b2 = C.inputs(name, z)
            vol, iou = fn(b1.to(d), b2.to(d))
            bad += [] if vol.device.type == d.type else ["%s: result on %s" % (name, vol.device)]
            bad += C.gate(name, vol, iou, z)
        return bad

    def raises(fn, b, message):
        try:
            fn(b, b)
        except ValueError as e:
            return message in str(e)
        return False

    sheared, flat = C.bad_boxes()

    # ---- plain install: the reference's own Python on the shim's operator ------------------------------------------------------------
    shim.install(ref_root)
    import pytorch3d.ops as ref_ops

    orig = importlib.import_module(HOLDERS[0]).box3d_overlap
    out["unpatched_is_the_reference"] = not getattr(orig, "__p3d_amd__", False) and ref_ops.box3d_overlap is orig
    out["plain_misses"] = misses(ref_ops.box3d_overlap)
    b1, b2 = C.inputs("random_3x5")
    vol, _ = ref_ops.box3d_overlap(b1.to(d).requires_grad_(True), b2.to(d))
    try:
        vol.sum().backward()
        out["plain_backward_raises"] = False
    except ValueError as e:
        out["plain_backward_raises"] = "box3d_overlap backward is not supported" in str(e)
    out["plain_checks_raise"] = bool(raises(ref_ops.box3d_overlap, sheared.to(d), "Plane vertices are not coplanar")
                                     and raises(ref_ops.box3d_overlap, flat.to(d), "Planes have zero areas"))
    out["calls_before_patch"] = sum(shim.PATCH_CALLS.get("box3d_overlap", [0, 0]))

    # ---- patch_python ----------------------------------------------------------------------------------------------------------------
    shim.install(ref_root, patch_python=True)
    from pytorch3d.ops import box3d_overlap

    out["patched_everywhere"] = bool(all(getattr(sys.modules[m].box3d_overlap, "__p3d_amd__", False) for m in HOLDERS)
                                     and box3d_overlap.__wrapped__ is orig)
    before = list(shim.PATCH_CALLS.get("box3d_overlap", [0, 0]))
    out["patched_misses"] = misses(box3d_overlap)
    after = list(shim.PATCH_CALLS.get("box3d_overlap", [0, 0]))
    out["fused_calls"], out["fallback_calls"] = after[0] - before[0], after[1] - before[1]
    out["patched_checks_raise"] = bool(raises(box3d_overlap, sheared.to(d), "Plane vertices are not coplanar")
                                       and raises(box3d_overlap, flat.to(d), "Planes have zero areas"))

    # ---- restore ---------------------------------------------------------------------------------------------------------------------
    shim.uninstall_python_patches()
    out["restored"] = bool(all(sys.modules[m].box3d_overlap is orig for m in HOLDERS))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
