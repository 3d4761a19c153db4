#!/usr/bin/env python
"""The UNMODIFIED reference's `from pytorch3d.ops import sample_points_from_meshes` through pytorch3d_amd.shim, in a process of its own
(the shim replaces sys.modules entries).  argv[1]: "cuda" (default) or "cpu".  Prints one JSON line that
tests/test_gpu_sample_points.py / tests/test_cpu_sample_points.py read: without patch_python nothing changes; with it every module
that holds the name sees the new function, a reference Meshes batch gives the golden of tests/golden/sample_points_ref.npz (textures of
a TexturesVertex batch included, on the GPU), PATCH_CALLS moves, and uninstall_python_patches() gives the reference's function back."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAME = "sample_points_from_meshes"
# every reference module that holds the name: the defining one and pytorch3d.ops, which re-exports it.  pytorch3d.loss is NOT among
# them -- no module of the reference's loss package imports the sampler (its users call pytorch3d.ops.sample_points_from_meshes)
MODULES = ("pytorch3d.ops.sample_points_from_meshes", "pytorch3d.ops")


def _reference_root():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    return next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "ops"))), None)


def main():
    ref_root = _reference_root()
    if ref_root is None:
        print(json.dumps({"skipped": "the reference's Python package is not on this machine"}))
        return
    import numpy as np
    import torch

    import run_reference_suite as rrs
    import sample_points_case as C

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    d = torch.device(sys.argv[1] if len(sys.argv) > 1 else "cuda:0")
    out = {}
    shim.install(ref_root)
    import pytorch3d.loss  # noqa: F401 -- loaded before the patch, like a user's program
    import pytorch3d.ops as ref_ops
    from pytorch3d.renderer.mesh.textures import TexturesVertex
    from pytorch3d.structures import Meshes

    original = ref_ops.sample_points_from_meshes
    out["unpatched_is_the_reference"] = not getattr(original, "__p3d_amd__", False)
    shim.install(ref_root, patch_python=True)
    from pytorch3d.ops import sample_points_from_meshes

    out["loss_never_held_it"] = not hasattr(pytorch3d.loss, NAME)
    out["patched_everywhere"] = bool(all(getattr(getattr(sys.modules[m], NAME), "__p3d_amd__", False) for m in MODULES)
                                     and sample_points_from_meshes.__wrapped__ is original)

    g = C.golden()
    verts_list, faces_list = C.ragged_batch()
    feats = torch.from_numpy(g["features"])
    nv = [v.shape[0] for v in verts_list]
    feats_list = list(torch.split(feats, nv, 0))
    before = list(shim.PATCH_CALLS.get(NAME, [0, 0]))
    try:
        for S in (64, 257):
            u = torch.from_numpy(g["uniforms_%d" % S]).to(d)
            meshes = Meshes(verts=[v.to(d) for v in verts_list], faces=[f.to(d) for f in faces_list])
            samples, normals, idx = sample_points_from_meshes(meshes, S, return_normals=True, uniforms=u, return_face_idxs=True)
            bary = np.where((idx.cpu().numpy() >= 0)[..., None], C.formulation_weights32(g["uniforms_%d" % S]), 0.0).astype(np.float32)
            textures = None
            if d.type == "cuda":  # (the shim's operator surface refuses CPU tensors: TexturesVertex.sample_textures ends in it)
                valid = [int(n) for n in g["texture_meshes"]]
                tm = Meshes(verts=[verts_list[n].to(d) for n in valid], faces=[faces_list[n].to(d) for n in valid],
                            textures=TexturesVertex(verts_features=[feats_list[n].to(d) for n in valid]))
                s3, t3 = sample_points_from_meshes(tm, S, return_textures=True, uniforms=u[valid])
                assert torch.equal(s3, samples[valid])
                textures = np.zeros((5, S, 3), dtype=np.float32)
                textures[valid] = t3.cpu().numpy()
            C.gate_ragged(S, samples.cpu().numpy(), normals.cpu().numpy(), idx.cpu().numpy(), bary, textures, g)
        out["golden_ok"] = True
    except AssertionError as e:
        out["golden_ok"], out["golden_error"] = False, repr(e)
    after = list(shim.PATCH_CALLS.get(NAME, [0, 0]))
    out["fused_calls"], out["fallback_calls"] = after[0] - before[0], after[1] - before[1]

    shim.uninstall_python_patches()
    import pytorch3d.ops.sample_points_from_meshes  # noqa: F401

    out["restored"] = bool(all(getattr(sys.modules[m], NAME) is original for m in MODULES))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
