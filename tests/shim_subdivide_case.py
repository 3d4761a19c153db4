#!/usr/bin/env python
"""The UNMODIFIED reference's SubdivideMeshes and ico_sphere through pytorch3d_amd.shim, in a process of its own; one JSON line for
tests/test_gpu_subdivide.py.  ico_sphere's vertices are compared bit for bit with the unpatched reference on the SAME GPU (its closing
normalisation is torch's own and rounds differently on the CPU), its faces with the CPU."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch

    import run_reference_suite as rrs
    import subdivide_case as C

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    ref_root = next(c for c in (os.environ.get("P3D_REFERENCE_ROOT"), os.path.join(ROOT, "oracle", "_ref", "reference_py")) if c and os.path.isdir(c))
    shim.install(ref_root)
    from pytorch3d.ops import SubdivideMeshes
    from pytorch3d.structures import Meshes
    from pytorch3d.utils import ico_sphere

    d = torch.device("cuda:0")
    orig = (SubdivideMeshes.forward, SubdivideMeshes.subdivide_faces)

    def run(device, homogeneous=False):
        results = []
        for name in C.cases() if not homogeneous else ["tetrahedron"]:
            verts, faces, feats = C.inputs(name, device)
            if homogeneous:
                verts, faces, feats = [verts[0], verts[0] * 2, verts[0] + 1], faces * 3, torch.cat([feats, feats * 3, feats - 1])
            meshes = Meshes(verts=verts, faces=faces)
            new_meshes, new_feats = (SubdivideMeshes(meshes) if homogeneous else SubdivideMeshes())(meshes, feats)
            results.append([t.cpu() for t in new_meshes.verts_list() + new_meshes.faces_list() + [new_feats]])
        return results

    want = run("cpu") + run("cpu", True)
    sphere, sphere_gpu = ico_sphere(3), ico_sphere(3, d)  # (its last step, the normalisation, is torch's own: compared on one device)
    calls = lambda key: list(shim.PATCH_CALLS.get(key, [0, 0]))  # noqa: E731
    shim.install(ref_root, patch_python=True)
    got = run(d) + run(d, True)
    out = {"misses": [i for i, (a, b) in enumerate(zip(got, want)) if len(a) != len(b) or not all(torch.equal(x, y) for x, y in zip(a, b))],
           "forwards": len(got), "forward_calls": calls("SubdivideMeshes.forward"), "faces_calls": calls("SubdivideMeshes.subdivide_faces")}
    fast = ico_sphere(3, d)
    out["ico_sphere_equal"] = bool(torch.equal(fast.verts_packed(), sphere_gpu.verts_packed()) and torch.equal(fast.faces_packed().cpu(), sphere.faces_packed()))
    out["ico_sphere_cpu_close"] = bool(torch.allclose(fast.verts_packed().cpu(), sphere.verts_packed(), rtol=0, atol=2.0 ** -22))
    before = calls("SubdivideMeshes.forward")
    out["ico_sphere_calls"] = [before[0] - out["forward_calls"][0], before[1] - out["forward_calls"][1]]  # three levels
    run("cpu", True)
    after = calls("SubdivideMeshes.forward")
    out["cpu_forward_calls"] = [after[0] - before[0], after[1] - before[1]]
    shim.uninstall_python_patches()
    out["restored"] = bool((SubdivideMeshes.forward, SubdivideMeshes.subdivide_faces) == orig)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
