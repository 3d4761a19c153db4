#!/usr/bin/env python
"""python tests/golden/make_golden_subdivide.py -> tests/golden/subdivide_ref.npz: what the reference's Meshes (edges_packed,
faces_packed_to_edges_packed, num_edges_per_mesh) and SubdivideMeshes()(meshes, feats) return on the CPU for the cases of
tests/subdivide_case.py, from P3D_REFERENCE_ROOT or oracle/_ref/reference_py behind a plain shim.install().  The loop restatement of
the case file has to agree with every recorded tensor, or nothing is written."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import subdivide_case as C  # noqa: E402


def main():
    import run_reference_suite as rrs

    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    ref_root = next(c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "ops")))
    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    shim.install(ref_root)
    from pytorch3d.ops import SubdivideMeshes
    from pytorch3d.structures import Meshes

    out, wrong = {}, []
    for name in C.cases():
        verts, faces, feats = C.inputs(name)
        meshes = Meshes(verts=verts, faces=faces)
        new_meshes, new_feats = SubdivideMeshes()(meshes, feats)
        rec = {"edges": meshes.edges_packed(), "face_edges": meshes.faces_packed_to_edges_packed(),
               "num_edges": meshes.num_edges_per_mesh().to(torch.int64), "new_verts": new_meshes.verts_packed(),
               "new_faces": torch.cat(new_meshes.faces_list(), 0), "new_num_verts": new_meshes.num_verts_per_mesh(),
               "new_num_faces": new_meshes.num_faces_per_mesh(), "new_feats": new_feats}
        for key, value in rec.items():
            out[f"{name}/{key}"] = value.numpy()
        want = C.restate(verts, faces, feats)
        got = dict(rec, new_verts=list(rec["new_verts"].split(rec["new_num_verts"].tolist(), 0)),
                   new_faces=list(rec["new_faces"].split(rec["new_num_faces"].tolist(), 0)))
        wrong += C.misses(got, want, name)
    if wrong:
        raise SystemExit("the restatement and the reference differ: " + ", ".join(wrong))
    np.savez_compressed(C.GOLDEN, **out)
    print("wrote", C.GOLDEN, os.path.getsize(C.GOLDEN), "bytes,", len(C.cases()), "cases")


if __name__ == "__main__":
    main()
