"""Golden fixture for box3d_overlap, generated FROM THE REFERENCE's own CPU operator (build container only; needs scipy).

    python tests/golden/make_golden_box3d.py   ->  tests/golden/box3d_ref.npz

The generator compiles the reference's csrc/iou_box3d/iou_box3d_cpu.cpp with a binding of a few lines (BINDING below, the generator's
own) through torch.utils.cpp_extension.load into a build directory OUTSIDE the repository and records for every case of
tests/box3d_case.py <case>/vol and <case>/iou, the operator's float32 outputs.  For the random and rot families it also records an
INDEPENDENT float64 figure, <case>/vol64 and <case>/iou64: the boxes' twelve half-spaces in float64, a Chebyshev centre by linear
programming, scipy's HalfspaceIntersection and the volume of the ConvexHull of its vertices (0 where the half-spaces have no interior);
and err/<family> = the reference's own largest |float32 - float64| over the family, for vol and for iou.  The reference's two test-data
files are stored as plain arrays: objectron/boxes1, boxes2 (float32, in the reference's corner order), objectron/expected_vol,
expected_iou (the recorded Objectron figures), real/boxes1 = boxes2 and real/expected_iou = identity.
Nothing of pytorch3d_amd is in the loop.

Asserted here (SEED of the case file was picked so):
* every random case with more than one pair has overlapping and disjoint pairs, and no pair's Chebyshev radius (negative: a gap) lies within 1e-5 x the scale of 0:
  the float64 figure never rests on a near-touching configuration;
* the reference's CPU operator meets the Objectron arrays and the real boxes' identity under the defaults of its own assertClose
  (rtol 1e-5, atol 1e-8), as tests/test_iou_box3d.py asks.
"""
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

REFERENCE = os.environ.get("P3D_REFERENCE_ROOT", "/root/reference")
OBJECTRON_TO_REFERENCE_ORDER = [0, 4, 6, 2, 1, 5, 7, 3]  # the corner permutation the reference's test applies to the Objectron boxes

BINDING = """
#include <torch/extension.h>
std::tuple<at::Tensor, at::Tensor> IoUBox3DCpu(const at::Tensor& boxes1, const at::Tensor& boxes2);
PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) { m.def("iou_box3d", &IoUBox3DCpu); }
"""


def reference_operator():
    from torch.utils.cpp_extension import load

    build_dir = os.path.join(tempfile.gettempdir(), "p3d_ref_iou_box3d")
    os.makedirs(build_dir, exist_ok=True)
    binding = os.path.join(build_dir, "binding.cpp")
    with open(binding, "w") as f:
        f.write(BINDING)
    csrc = os.path.join(REFERENCE, "pytorch3d", "csrc")
    ext = load(name="p3d_ref_iou_box3d", sources=[os.path.join(csrc, "iou_box3d", "iou_box3d_cpu.cpp"), binding],
               extra_include_paths=[csrc], build_directory=build_dir, extra_cflags=["-O2"], verbose=False)
    return ext.iou_box3d


def halfspaces(box):
    """(6, 4) float64 rows [n, d] with n . x + d <= 0 inside: a face is the four corners that share one coordinate of the unit box."""
    import box3d_case as C

    unit = np.array(C.UNIT_BOX)
    centre = box.mean(0)
    rows = []
    for axis in range(3):
        for side in (0, 1):
            p = box[unit[:, axis] == side]
            n = np.cross(p[1] - p[0], p[2] - p[0])
            n = n / np.linalg.norm(n)
            d = -float(n @ p.mean(0))
            if n @ centre + d > 0:
                n, d = -n, -d
            rows.append(np.append(n, d))
    return np.array(rows)


def intersection_volume(box1, box2):
    """(float64 volume, Chebyshev radius) of the intersection of two boxes given as (8, 3) float64 corners."""
    from scipy.optimize import linprog
    from scipy.spatial import ConvexHull, HalfspaceIntersection

    hs = np.concatenate([halfspaces(box1), halfspaces(box2)])
    A, b = hs[:, :3], hs[:, 3]
    res = linprog(c=[0, 0, 0, -1], A_ub=np.hstack([A, np.ones((len(A), 1))]), b_ub=-b, bounds=[(None, None)] * 4)  # (a negative radius: disjoint by that much)
    assert res.status == 0, res.message
    radius = float(res.x[3])
    if radius <= 1e-9:
        return 0.0, radius
    verts = HalfspaceIntersection(hs, res.x[:3]).intersections
    return float(ConvexHull(verts).volume), radius


def float64_figures(b1, b2):
    from scipy.spatial import ConvexHull

    b1, b2 = b1.double().numpy(), b2.double().numpy()
    vol = np.zeros((len(b1), len(b2)))
    radius = np.zeros_like(vol)
    for i, x in enumerate(b1):
        for j, y in enumerate(b2):
            vol[i, j], radius[i, j] = intersection_volume(x, y)
    v1 = np.array([ConvexHull(x).volume for x in b1])[:, None]
    v2 = np.array([ConvexHull(y).volume for y in b2])[None, :]
    return vol, vol / (v1 + v2 - vol), radius


def main():
    import box3d_case as C

    op = reference_operator()
    out, err = {}, {}
    # the reference's test data, as plain arrays
    obj = torch.load(os.path.join(REFERENCE, "tests", "data", "objectron_vols_ious.pt"))
    idx = torch.tensor(OBJECTRON_TO_REFERENCE_ORDER)
    out["objectron/boxes1"] = obj["boxes1"].float().index_select(1, idx)
    out["objectron/boxes2"] = obj["boxes2"].float().index_select(1, idx)
    out["objectron/expected_vol"], out["objectron/expected_iou"] = obj["vols"].float(), obj["ious"].float()
    with open(os.path.join(REFERENCE, "tests", "data", "real_boxes.pkl"), "rb") as f:
        real = pickle.load(f)
    out["real/boxes1"] = torch.stack([torch.FloatTensor(real["verts1"]), torch.FloatTensor(real["verts2"])])
    out["real/boxes2"] = out["real/boxes1"].clone()
    out["real/expected_vol"], out["real/expected_iou"] = torch.zeros(2, 2), torch.eye(2)
    for name in C.all_cases():
        fam = C.family(name)
        b1, b2 = C.inputs(name, out)
        vol, iou = op(b1.contiguous(), b2.contiguous())
        out[name + "/vol"], out[name + "/iou"] = vol, iou
        line = "%-28s %s overlapping %d of %d" % (name, tuple(vol.shape), int((vol > 0).sum()), vol.numel())
        if fam in ("objectron", "real"):
            assert torch.allclose(iou, out[name + "/expected_iou"], rtol=1e-5, atol=1e-8), name
            assert fam == "real" or torch.allclose(vol, out[name + "/expected_vol"], rtol=1e-5, atol=1e-8), name
        elif fam != "lattice":
            vol64, iou64, radius = float64_figures(b1, b2)
            out[name + "/vol64"], out[name + "/iou64"] = torch.from_numpy(vol64), torch.from_numpy(iou64)
            if fam.startswith("random"):
                scale = 0.05 if fam == "random_small" else 1.0
                assert not (np.abs(radius) < 1e-5 * scale).any(), (name, "a near-touching pair: pick another SEED")
                assert vol.numel() == 1 or ((vol64 > 0).any() and (vol64 == 0).any()), (name, "pick another SEED")
                assert ((vol64 > 0) == (vol.numpy() > 0)).all(), (name, "the reference and the float64 figure disagree on overlap")
            e = (float(np.abs(vol.double().numpy() - vol64).max()), float(np.abs(iou.double().numpy() - iou64).max()))
            err[fam] = tuple(max(a, b) for a, b in zip(err.get(fam, (0.0, 0.0)), e))
            line += "  reference's error vol %.3g iou %.3g" % e
        else:
            line += "  vol %s iou %s" % (vol.flatten().tolist(), iou.flatten().tolist())
        print(line)
    for fam, e in err.items():
        out["err/" + fam] = torch.tensor(e, dtype=torch.float64)
        print("err/%s" % fam, e)
    np.savez_compressed(C.FIXTURE, **{k: v.numpy() for k, v in out.items()})
    print("wrote", C.FIXTURE, os.path.getsize(C.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
