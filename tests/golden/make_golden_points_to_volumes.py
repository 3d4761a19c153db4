"""Golden fixture for points_to_volumes, generated FROM THE REFERENCE's own CPU operator (build container only).

    python tests/golden/make_golden_points_to_volumes.py   ->  tests/golden/points_to_volumes_ref.npz

The generator compiles the reference's csrc/points_to_volumes/points_to_volumes_cpu.cpp with a binding of a few lines (BINDING below,
the generator's own) through torch.utils.cpp_extension.load into a build directory OUTSIDE the repository, loads the reference's
pytorch3d/ops/points_to_volumes.py on top of it, and records for every case of tests/points_to_volumes_case.py
* <case>/densities, <case>/features: the volumes after the reference's own autograd function (`_points_to_volumes`, with the
  case's point_weight) on non-zero initial volumes;
* <case>/grad_points_3d (trilinear), <case>/grad_points_features: its autograd gradients for the case's upstream gradients.
Nothing of pytorch3d_amd is in the loop; the inputs are redrawn from seeds by the tests, so the file holds outputs only.

Asserted here (SEED of the case file was picked so):
* random cases: no float64 location within 1e-6 (relative) of an integer, or of a half in nearest mode;
* lattice cases: the locations are multiples of 1/4 and cover what the tests are about (halves, (-1, 0), below -1, exactly
  grid - 1, beyond it, on every axis), and every partial sum of grad_points_3d stays exact in float32;
* where the compiled operator and the reference's Python twin (`_python=True`) agree by construction -- align_corners=True, the
  whole tensor as the grid, the points with a location below 0 masked out and, in nearest mode, those at an exact half too --
  they agree on the lattice cases bit for bit.
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

REFERENCE = os.environ.get("P3D_REFERENCE_ROOT", "/root/reference")

BINDING = """
#include <torch/extension.h>
void PointsToVolumesForwardCpu(const torch::Tensor& points_3d, const torch::Tensor& points_features,
                               const torch::Tensor& volume_densities, const torch::Tensor& volume_features,
                               const torch::Tensor& grid_sizes, const torch::Tensor& mask, const float point_weight,
                               const bool align_corners, const bool splat);
void PointsToVolumesBackwardCpu(const torch::Tensor& points_3d, const torch::Tensor& points_features, const torch::Tensor& grid_sizes,
                                const torch::Tensor& mask, const float point_weight, const bool align_corners, const bool splat,
                                const torch::Tensor& grad_volume_densities, const torch::Tensor& grad_volume_features,
                                const torch::Tensor& grad_points_3d, const torch::Tensor& grad_points_features);
PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("points_to_volumes_forward", &PointsToVolumesForwardCpu);
  m.def("points_to_volumes_backward", &PointsToVolumesBackwardCpu);
}
"""


def reference_module():
    """The reference's pytorch3d/ops/points_to_volumes.py over its own CPU operator, without importing the rest of the package."""
    from torch.utils.cpp_extension import load

    build_dir = os.path.join(tempfile.gettempdir(), "p3d_ref_points_to_volumes")
    os.makedirs(build_dir, exist_ok=True)
    binding = os.path.join(build_dir, "binding.cpp")
    with open(binding, "w") as f:
        f.write(BINDING)
    csrc = os.path.join(REFERENCE, "pytorch3d", "csrc")
    ext = load(name="p3d_ref_points_to_volumes", sources=[os.path.join(csrc, "points_to_volumes", "points_to_volumes_cpu.cpp"), binding],
               extra_include_paths=[csrc], build_directory=build_dir, extra_cflags=["-O2"], verbose=False)
    pkg = types.ModuleType("pytorch3d")
    pkg.__path__ = []
    pkg._C = ext
    sys.modules["pytorch3d"], sys.modules["pytorch3d._C"] = pkg, ext
    spec = importlib.util.spec_from_file_location("pytorch3d_ops_points_to_volumes",
                                                  os.path.join(REFERENCE, "pytorch3d", "ops", "points_to_volumes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_reference(ref, case, inp, mask=None, python=False):
    """(points, features, (volume_features, volume_densities)) of the reference.  The compiled operator goes through the reference's
    own autograd function with the case's point_weight (its public function always passes 1); `python`: the public function with
    `_python=True`, which has no point_weight and always rescales."""
    import points_to_volumes_case as C

    mode, align = case[2], case[3]
    pts = inp["points_3d"].clone().requires_grad_(mode == "trilinear" and not python)
    feats = inp["features"].clone().requires_grad_(not python)
    dens, vfeat = inp["densities"].clone(), inp["volume_features"].clone()
    mask = C.full_mask(inp) if mask is None else mask
    if python:
        return pts, feats, ref.add_points_features_to_volume_densities_features(
            pts, feats, dens, vfeat, mode=mode, mask=mask, grid_sizes=inp["grid_sizes"], align_corners=align, _python=True)
    dens, vfeat = ref._points_to_volumes(pts, feats, dens, vfeat, inp["grid_sizes"], inp["point_weight"], mask, align, mode == "trilinear")
    return pts, feats, (vfeat, dens)


def check_coverage(C, cases):
    """The lattice cases together hold what the tests are about."""
    seen = set()
    for case in cases:
        inp = C.inputs(case)
        loc = C.locations(case, inp)
        assert torch.equal(loc * 4, (loc * 4).round()), case
        grid = inp["grid_sizes"][:, [2, 1, 0]][:, None, :].double()
        live = (inp["mask"] if inp["mask"] is not None else torch.ones(loc.shape[:2])) != 0
        for axis in range(3):
            a, g = loc[..., axis][live], grid.expand_as(loc)[..., axis][live]
            tags = {"half": (a - a.floor()) == 0.5, "in(-1,0)": (a > -1) & (a < 0), "below-1": a < -1, "grid-1": a == g - 1, "beyond": a > g - 1}
            seen |= {(case[2], axis, t) for t, m in tags.items() if bool(m.any())}
        assert C.exact_grad_bound(case, inp) < 2 ** 24, (case, C.exact_grad_bound(case, inp))
    want = {(mode, axis, t) for mode in ("trilinear", "nearest") for axis in range(3) for t in ("half", "in(-1,0)", "below-1", "grid-1", "beyond")}
    assert want <= seen, sorted(want - seen)


def check_python_twin(ref, C, case):
    """The compiled operator against `_python=True` where both are the same function; True when the case qualifies."""
    inp = C.inputs(case)
    dims = tuple(inp["densities"].shape[2:])
    if not case[3] or any(tuple(g) != dims for g in inp["grid_sizes"].tolist()):
        return False
    loc = C.locations(case, inp)
    keep = (loc >= 0).all(2)
    if case[2] == "nearest":
        keep &= ((loc - loc.floor()) != 0.5).all(2)
    mask = keep.float() * (inp["mask"] if inp["mask"] is not None else 1.0)
    if mask.sum() == 0:  # (a cloud of one point that lies below 0)
        return False
    inp = dict(inp, point_weight=1.0)  # (the twin has no point_weight)
    _, _, (feat, dens) = run_reference(ref, case, inp, mask=mask)
    with torch.no_grad():
        _, _, (feat_py, dens_py) = run_reference(ref, case, inp, mask=mask, python=True)
    rescaled = feat / dens.clamp(1e-4 if case[2] == "trilinear" else 1.0)
    assert torch.equal(dens.detach(), dens_py) and torch.equal(rescaled.detach(), feat_py), case
    return True


def main():
    import points_to_volumes_case as C

    ref = reference_module()
    cases = C.all_cases()
    check_coverage(C, [c for c in cases if c[0] == "lattice"])
    print("python twin agrees on", sum(check_python_twin(ref, C, c) for c in cases if c[0] == "lattice"), "lattice runs")
    out = {}
    for case in cases:
        inp = C.inputs(case)
        if case[0] == "random":
            gap = C.smallest_gap(case, inp)
            assert gap >= C.MIN_GAP, (case, gap, "pick another SEED")
        pts, feats, (feat, dens) = run_reference(ref, case, inp)
        grads = torch.autograd.grad((dens, feat), (pts, feats) if pts.requires_grad else (feats,),
                                    (inp["grad_densities"], inp["grad_features"]))
        out[C.key(case, "densities")], out[C.key(case, "features")] = dens.detach(), feat.detach()
        out[C.key(case, "grad_points_features")] = grads[-1]
        if pts.requires_grad:
            out[C.key(case, "grad_points_3d")] = grads[0]
        print(C.case_id(case), "touched voxels", int((dens.detach() != inp["densities"]).sum()), "of", dens.numel())
    np.savez_compressed(C.FIXTURE, **{k: v.numpy() for k, v in out.items()})
    print("wrote", C.FIXTURE, os.path.getsize(C.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
