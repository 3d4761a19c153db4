#!/usr/bin/env python
"""The UNMODIFIED reference's `from pytorch3d.loss import point_mesh_face_distance, point_mesh_edge_distance` through
pytorch3d_amd.shim, in a process of its own (the shim replaces sys.modules entries).  Prints one JSON line that
tests/test_gpu_point_mesh.py (GPU, the default) and tests/test_cpu_point_mesh.py (`--cpu`) read:
  plain     the reference's own functions under shim.install(): they end in the eight `_C.*_dist_*` operators
  patched   the same calls under shim.install(patch_python=True): the fused nodes, with what PATCH_CALLS counted (GPU only)
  restored  uninstall_python_patches() gives the reference's functions back (GPU only)
Losses and gradients go out as lists; the readers compare them with tests/golden/point_mesh_ref.npz."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("point_mesh_face_distance", "point_mesh_edge_distance")
CASES = ("ico2", "ragged")


def _reference_root():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    return next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "loss"))), None)


def run_cases(device, face_fn, edge_fn):
    import torch

    import point_mesh_case as C
    from pytorch3d.structures import Meshes, Pointclouds

    z = C.fixture()
    out = {}
    for name in CASES:
        out[name] = {}
        for tag, fn in (("face", face_fn), ("edge", edge_fn)):
            verts, faces, points = C.mesh_inputs(z, name, device=device)
            loss = fn(Meshes(verts=verts, faces=faces), Pointclouds(points=points))
            grads = torch.autograd.grad(loss, verts + points)
            out[name][tag] = {"loss": float(loss), "grads": [g.cpu().tolist() for g in grads]}
    return out


def main():
    ref_root = _reference_root()
    if ref_root is None:
        print(json.dumps({"skipped": "the reference's Python package is not on this machine"}))
        return
    import torch

    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    cpu = "--cpu" in sys.argv
    device = torch.device("cpu" if cpu else "cuda:0")
    shim.install(ref_root)
    import pytorch3d.loss as ref_loss
    import pytorch3d.loss.point_mesh_distance as ref_pm

    originals = {n: getattr(ref_pm, n) for n in NAMES}
    out = {"plain_is_reference": all(not getattr(f, "__p3d_amd__", False) for f in originals.values())}
    out["plain"] = run_cases(device, ref_pm.point_mesh_face_distance, ref_pm.point_mesh_edge_distance)
    if cpu:
        print(json.dumps(out))
        return

    shim.install(ref_root, patch_python=True)
    out["patched_everywhere"] = all(getattr(getattr(m, n), "__p3d_amd__", False) for m in (ref_pm, ref_loss) for n in NAMES)

    def calls():
        return {n: list(shim.PATCH_CALLS.get(n, [0, 0])) for n in NAMES}

    before = calls()
    out["patched"] = run_cases(device, ref_loss.point_mesh_face_distance, ref_loss.point_mesh_edge_distance)
    after = calls()
    out["fused_calls"] = {n: after[n][0] - before[n][0] for n in NAMES}
    out["fallbacks_in_fused_part"] = sum(after[n][1] - before[n][1] for n in NAMES)
    # CPU batches under the patch: the package's torch formulation, counted as fallbacks
    before = calls()
    out["patched_cpu"] = run_cases(torch.device("cpu"), ref_loss.point_mesh_face_distance, ref_loss.point_mesh_edge_distance)
    after = calls()
    out["cpu_fallback_calls"] = {n: after[n][1] - before[n][1] for n in NAMES}
    out["cpu_fused_calls"] = sum(after[n][0] - before[n][0] for n in NAMES)

    shim.uninstall_python_patches()
    out["restored"] = all(getattr(m, n) is originals[n] for m in (ref_pm, ref_loss) for n in NAMES)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
