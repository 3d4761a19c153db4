"""Golden fixture for cubify, recorded FROM THE REFERENCE's own Python on the CPU (build container only).

    python tests/golden/make_golden_cubify.py   ->  tests/golden/cubify_ref.npz

Imports the unmodified reference package (the staged copy under oracle/_ref/reference_py, or P3D_REFERENCE_ROOT) under plain
pytorch3d_amd.shim.install(), which leaves `pytorch3d.ops.cubify` alone, and records for every case of tests/cubify_case.py the inputs
(voxels, thresh, align, feats) and what the reference's function returns on CPU tensors: the vertex and face lists packed, the per-mesh
sizes, whether the lists hold 1-D empties, and the TexturesAtlas values.  Nothing of pytorch3d_amd computes anything here.  Asserted
below: what the case file's header promises (56 / 108 for the solid block, 8 / 12 per isolated voxel, the empties' shapes) and that
the nested-loop restatement of tests/cubify_case.py equals every record.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import cubify_case as C
    import run_reference_suite as rrs

    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    ref_root = next(c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "ops")))
    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    shim.install(ref_root)
    from pytorch3d.ops import cubify

    assert not getattr(cubify, "__p3d_amd__", False)  # (its __wrapped__ is torch.no_grad's)
    data = {}
    for name in C.cases():
        voxels, thresh, feats, align = C.build_inputs(name)
        meshes = cubify(voxels, thresh, feats=feats, align=align)
        verts, faces = meshes.verts_list(), meshes.faces_list()
        one_d = all(v.dim() == 1 for v in verts)
        assert one_d == (sum(f.shape[0] for f in faces) == 0) and (one_d or all(v.dim() == 2 and f.dim() == 2 for v, f in zip(verts, faces)))
        data[name + "/voxels"], data[name + "/thresh"], data[name + "/align"] = voxels.numpy(), np.float64(thresh), np.str_(align)
        data[name + "/ndim"] = np.int64(1 if one_d else 2)
        data[name + "/nv"] = np.array([v.shape[0] for v in verts], np.int64)
        data[name + "/nf"] = np.array([f.shape[0] for f in faces], np.int64)
        data[name + "/verts"] = torch.cat([v.reshape(-1, 3) for v in verts]).numpy()
        faces_packed = torch.cat([f.reshape(-1, 3) for f in faces])
        assert faces_packed.dtype == torch.int64 and data[name + "/verts"].dtype == np.float32
        data[name + "/faces"] = faces_packed.numpy()
        if feats is not None:
            data[name + "/feats"] = feats.numpy()
        if meshes.textures is not None:
            atlas = meshes.textures.atlas_list()
            assert all(a.shape[1:3] == (1, 1) for a in atlas)
            data[name + "/tex"] = torch.cat([a.reshape(a.shape[0], -1) for a in atlas]).numpy()
    assert (data["solid3/nv"].tolist(), data["solid3/nf"].tolist()) == ([56], [108])
    assert data["checker/nf"].tolist() == [12 * 32, 12 * 32] and data["all_empty/ndim"] == 1 and data["some_empty/nf"][0::2].tolist() == [0, 0, 0]
    assert data["some_empty/nf"][1::2].min() > 0 and "feats_center/tex" in data and data["thresh07/nf"].min() > 0
    np.savez_compressed(C.FIXTURE, **data)
    C._FIXTURE = None
    wrong = [m for name in C.cases() for m in C.misses(C.restate(*C.inputs(name)), C.expected(name), name)]
    assert wrong == [], wrong
    print("wrote %s: %d cases, %d bytes" % (C.FIXTURE, len(C.cases()), os.path.getsize(C.FIXTURE)))


if __name__ == "__main__":
    main()
