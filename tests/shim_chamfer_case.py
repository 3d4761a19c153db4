#!/usr/bin/env python
"""The UNMODIFIED reference's `from pytorch3d.loss import chamfer_distance` / `from pytorch3d.ops import knn_points` through
pytorch3d_amd.shim with patch_python=True, on the GPU, in a process of its own (the shim replaces sys.modules entries).  Prints one
JSON line that tests/test_gpu_chamfer.py reads: results against tests/golden/chamfer_ref.npz for tensors and Pointclouds-shaped
inputs, what PATCH_CALLS counted, and that uninstall_python_patches() gives the reference's stub-bound knn_points back."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("knn_points", "chamfer_distance")


def _reference_root():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    return next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "loss"))), None)


def main():
    ref_root = _reference_root()
    if ref_root is None:
        print(json.dumps({"skipped": "the reference's Python package is not on this machine"}))
        return
    import torch

    import chamfer_case as C
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    shim.install(ref_root, patch_python=True)
    from pytorch3d.loss import chamfer_distance
    from pytorch3d.ops import knn_points

    d = torch.device("cuda:0")
    z = C.fixture()
    out = {}
    mods = {"knn_points": ("pytorch3d.ops.knn", "pytorch3d.ops", "pytorch3d.loss.chamfer"),
            "chamfer_distance": ("pytorch3d.loss.chamfer", "pytorch3d.loss")}
    out["patched_everywhere"] = all(getattr(getattr(sys.modules[m], n), "__p3d_amd__", False) for n, ms in mods.items() for m in ms)
    out["patched_everywhere"] = bool(out["patched_everywhere"] and getattr(knn_points, "__p3d_amd__", False)
                                     and getattr(chamfer_distance, "__p3d_amd__", False))

    def calls():
        return {n: list(shim.PATCH_CALLS.get(n, [0, 0])) for n in NAMES}

    # ---- qualifying inputs: tensors and Pointclouds-shaped objects ------------------------------------------------------------------
    before = calls()
    p1, p2 = z[C.knn_key("pad", "p1")].to(d), z[C.knn_key("pad", "p2")].to(d)
    l1, l2 = C.lengths_tensor([70, 1, 33]).to(d), C.lengths_tensor([130, 64, 5]).to(d)
    got = knn_points(p1, p2, lengths1=l1, lengths2=l2, K=8)
    want_idx, want_d = z[C.knn_key("pad", "idx", 8, 2)], z[C.knn_key("pad", "dists", 8, 2)]
    out["knn_idx_equal"] = bool(torch.equal(got.idx.cpu(), want_idx))
    out["knn_dists_error"] = float(((got.dists.cpu() - want_d).abs() - 2e-6 * want_d.abs()).max())
    out["chamfer"] = {}
    for name in ("red_mean_mean", "weights_sum_none", "hetero"):  # tensors, tensors with weights, duck-typed clouds
        x, y, args, kw = C.chamfer_inputs(name, device=d)
        result = chamfer_distance(*args, **kw)
        gx, gy = torch.autograd.grad(C.scalarise(result), (x, y))
        want = z[C.cham_key(name, "out0")]
        wgx, wgy = z[C.cham_key(name, "grad_x")], z[C.cham_key(name, "grad_y")]
        out["chamfer"][name] = {
            "error": float((result[0].detach().cpu() - want).abs().max()), "tolerance": 1e-4 * max(1e-3, float(want.abs().max())),
            "grad_error": max(float((gx.cpu() - wgx).abs().max()), float((gy.cpu() - wgy).abs().max())),
            "grad_tolerance": 1e-4 * max(1e-3, float(wgx.abs().max()), float(wgy.abs().max()))}
    after = calls()
    out["fused_calls"] = {n: after[n][0] - before[n][0] for n in NAMES}
    out["fallbacks_in_fused_part"] = sum(after[n][1] - before[n][1] for n in NAMES)

    # ---- D = 5: the package's torch formulation (counted as fallbacks), on the GPU --------------------------------------------------
    before = calls()
    q1, q2 = z[C.knn_key("d5", "p1")].to(d), z[C.knn_key("d5", "p2")].to(d)
    got5 = knn_points(q1, q2, K=32)
    loss5, _ = chamfer_distance(q1, q2)
    idx64 = C.brute64(q1.cpu(), q2.cpu(), None, None, 1, 2)[0][..., 0], C.brute64(q2.cpu(), q1.cpu(), None, None, 1, 2)[0][..., 0]
    want5 = float(C.chamfer_restated(q1.cpu().double(), q2.cpu().double(), None, None, *idx64))
    out["d5_matches"] = bool(torch.equal(got5.idx.cpu(), z[C.knn_key("d5", "idx", 32, 2)]) and abs(float(loss5) - want5) <= 1e-5 * want5)
    after = calls()
    out["d5_fallback_calls"] = {n: after[n][1] - before[n][1] for n in NAMES}
    out["d5_fused_calls"] = sum(after[n][0] - before[n][0] for n in NAMES)

    # ---- restore: the reference's own knn_points ends in the stub again ----------------------------------------------------------------
    patched = knn_points
    shim.uninstall_python_patches()
    import pytorch3d.loss.chamfer as ref_chamfer
    import pytorch3d.ops as ref_ops

    out["restored"] = bool(ref_ops.knn_points is patched.__wrapped__ and ref_chamfer.knn_points is patched.__wrapped__
                           and not getattr(ref_chamfer.chamfer_distance, "__p3d_amd__", False))
    try:
        ref_ops.knn_points(p1, p2, K=1)
        out["reference_raises_again"] = False
    except NotImplementedError:
        out["reference_raises_again"] = True
    print(json.dumps(out))


if __name__ == "__main__":
    main()
