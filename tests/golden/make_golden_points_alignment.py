"""Golden fixture for iterative_closest_point / corresponding_points_alignment, generated FROM THE REFERENCE's own code on the CPU (build
container only).

    python tests/golden/make_golden_points_alignment.py   ->  tests/golden/points_alignment_ref.npz

The generator compiles the reference's csrc/knn/knn_cpu.cpp with a binding of a few lines (BINDING below, the generator's own)
through torch.utils.cpp_extension.load into a build directory OUTSIDE the repository -- as it is, and once more inside a namespace
with `float` read as `double`, because the operator's accessors are float-only and the yardstick is a float64 run -- and loads the
reference's pytorch3d/ops/points_alignment.py, ops/utils.py, ops/knn.py and structures/utils.py on top of it, without the rest of the
package.  Every case of tests/points_alignment_case.py runs through the reference's function in float64 (the truth) and in float32
(the yardstick); what is recorded and what is asserted per seed is listed in that file's docstring.  Nothing of pytorch3d_amd is in
the loop.
"""
import importlib
import os
import sys
import tempfile
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

REFERENCE = os.environ.get("P3D_REFERENCE_ROOT", "/root/reference")

BINDING = """
#include <torch/extension.h>
#include <cmath>
#include <cstdlib>
#include <queue>
#include <tuple>
std::tuple<at::Tensor, at::Tensor> KNearestNeighborIdxCpu(const at::Tensor& p1, const at::Tensor& p2, const at::Tensor& lengths1,
                                                          const at::Tensor& lengths2, const int norm, const int K);
namespace f64 {
using std::abs;
#define float double
#include "knn/knn_cpu.cpp"
#undef float
}  // namespace f64
std::tuple<at::Tensor, at::Tensor> knn_points_idx(const at::Tensor& p1, const at::Tensor& p2, const at::Tensor& l1, const at::Tensor& l2,
                                                   const int norm, const int K, const int version) {
  return p1.scalar_type() == at::kDouble ? f64::KNearestNeighborIdxCpu(p1, p2, l1, l2, norm, K) : KNearestNeighborIdxCpu(p1, p2, l1, l2, norm, K);
}
PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) { m.def("knn_points_idx", &knn_points_idx); }
"""


def reference_module():
    """The reference's points_alignment module over its own CPU nearest neighbours, without importing the rest of the package."""
    from torch.utils.cpp_extension import load

    build_dir = os.path.join(tempfile.gettempdir(), "p3d_ref_points_alignment")
    os.makedirs(build_dir, exist_ok=True)
    binding = os.path.join(build_dir, "binding.cpp")
    with open(binding, "w") as f:
        f.write(BINDING)
    csrc = os.path.join(REFERENCE, "pytorch3d", "csrc")
    ext = load(name="p3d_ref_points_alignment", sources=[os.path.join(csrc, "knn", "knn_cpu.cpp"), binding], extra_include_paths=[csrc],
               build_directory=build_dir, extra_cflags=["-O2"], verbose=False)
    for name, sub in (("pytorch3d", None), ("pytorch3d.ops", "ops"), ("pytorch3d.structures", "structures")):
        mod = types.ModuleType(name)
        mod.__path__ = [] if sub is None else [os.path.join(REFERENCE, "pytorch3d", sub)]  # (no __init__ runs)
        sys.modules[name] = mod
    sys.modules["pytorch3d"]._C = ext
    sys.modules["pytorch3d._C"] = ext
    sys.modules["pytorch3d.ops"].knn_points = importlib.import_module("pytorch3d.ops.knn").knn_points
    return importlib.import_module("pytorch3d.ops.points_alignment")


class Recorder:
    """Wraps knn_points and torch.svd where the reference's module looks them up: keeps the neighbour indices of every iteration and
    the singular values of the last decomposition."""

    def __init__(self, ref):
        self.idx, self.S = [], None
        knn, svd = ref.knn_points, torch.svd

        def knn_points(*a, **k):
            out = knn(*a, **k)
            self.idx.append(out.idx[:, :, 0].clone())
            return out

        def recording_svd(*a, **k):
            out = svd(*a, **k)
            self.S = out[1].detach().clone()
            return out

        ref.knn_points = knn_points
        torch.svd = recording_svd  # (the module calls torch.svd(...): looked up at the call)

    def reset(self):
        self.idx, self.S = [], None


def sigma_ok(S, planar):
    g12 = bool(((S[:, 0] - S[:, 1]) >= C.SIGMA_GAP * S[:, 0]).all())
    g23 = bool(((S[:, 1] - S[:, 2]) >= C.SIGMA_GAP * S[:, 0]).all())
    return g12 and (planar or g23)


def try_align(ref, rec, case, seed):
    d = C.align_inputs(case, seed)
    runs = {}
    for dtype in (torch.float64, torch.float32):
        rec.reset()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            runs[dtype] = C.align_values(C.run_align(ref.corresponding_points_alignment, case, dtype=dtype, seed=seed))
        if dtype == torch.float64:
            S = rec.S
    live = torch.ones(3, dtype=torch.bool) if d["weights"] is None else d["weights"].sum(1) > 0
    if not sigma_ok(S[live], case[0] == "planar"):
        return "singular value gaps"
    r64 = runs[torch.float64]
    err = C.errors(runs[torch.float32], r64)
    print("align", C.case_id(case), "seed", seed, "S", [["%.3g" % v for v in row] for row in S.tolist()], {k: "%.3g" % v for k, v in err.items()})
    out = {q + "64": r64[q] for q in C.ALIGN_QUANTITIES}
    out.update(seed=torch.tensor(seed), checksum=C.checksum(d), err32=torch.tensor([err[q] for q in C.ALIGN_QUANTITIES], dtype=torch.float64))
    return out


def icp_replay(d, sol, idx):
    """From the float64 run: (smallest relative gap between the nearest and the next distinct distance over the iterations and live
    rows, relative rmse decrease per iteration (b,) each)."""
    X, Y = d["X"].double(), d["Y"].double()
    b, P1, _ = X.shape
    l1 = d["lengths1"] if d["lengths1"] is not None else torch.full((b,), P1)
    l2 = d["lengths2"] if d["lengths2"] is not None else torch.full((b,), Y.shape[1])
    hetero = bool(((l2 < Y.shape[1]).any() or (l1 < P1).any()) and (l1 != l2).any())
    mask = (torch.arange(P1)[None] < l1[:, None]).double() if hetero else torch.ones(b, P1, dtype=torch.float64)
    current = d["init"]
    gap, relative, prev = float("inf"), [], None
    for k, t in enumerate(sol.t_history):
        Xt = X if current is None else current[2].double()[:, None, None] * torch.bmm(X, current[0].double()) + current[1].double()[:, None]
        for n in range(b):
            dist = torch.cdist(Xt[n, :int(l1[n])], Y[n, :int(l2[n])]).sort(dim=1).values
            first = dist[:, :1]
            nxt = torch.where(dist > first, dist, torch.full_like(dist, float("inf"))).min(1).values
            gap = min(gap, float(((nxt - first[:, 0]) / nxt).min()))
        nn = torch.gather(Y, 1, idx[k][:, :, None].expand(-1, -1, 3))
        new = t.s[:, None, None] * torch.bmm(X, t.R) + t.T[:, None]
        rmse = ((((new - nn) ** 2).sum(2) * mask).sum(1) / mask.sum(1).clamp(1e-9)).sqrt()
        relative.append(torch.ones(b, dtype=torch.float64) if prev is None else (prev - rmse) / prev)
        prev = rmse
        current = (t.R, t.T, t.s)
    return gap, relative


def try_icp(ref, rec, case, seed):
    d = C.icp_inputs(case, seed)
    variant = case[1]
    rec.reset()
    s64 = C.run_icp(ref.iterative_closest_point, case, dtype=torch.float64, seed=seed)
    idx64, S = rec.idx, rec.S
    rec.reset()
    s32 = C.run_icp(ref.iterative_closest_point, case, dtype=torch.float32, seed=seed)
    idx32 = rec.idx
    its = len(s64.t_history)
    if len(s32.t_history) != its or s32.converged != s64.converged:
        return "float32 iteration count (%d / %d)" % (len(s32.t_history), its)
    if not all(torch.equal(a, b) for a, b in zip(idx64, idx32)):
        return "float32 neighbours"
    if s64.converged == (variant in C.UNCONVERGED):
        return "converged flag"
    if not sigma_ok(S, False):
        return "singular value gaps"
    gap, relative = icp_replay(d, s64, idx64)
    if gap < C.MIN_GAP:
        return "distance gap %.3g" % gap
    thr = d["kwargs"]["relative_rmse_thr"]
    if variant not in C.FREE_COUNT:
        if not (bool((relative[-1] <= thr / 10).all()) and its >= 3 and bool((relative[-2] >= 10 * thr).any())):
            return "the count is a coin toss"
    first = [min([k for k in range(its) if float(relative[k][n]) <= thr], default=its) for n in range(3)]
    if variant == "200x300" and len(set(first)) < 2:
        return "the clouds converge together"
    v64 = C.icp_values(s64)
    err = C.errors(C.icp_values(s32), v64)
    print("icp", C.case_id(case), "seed", seed, "iterations", its, "per cloud", first, "gap %.3g" % gap, {k: "%.3g" % v for k, v in err.items()})
    out = {q + "64": v64[q] for q in C.ICP_QUANTITIES}
    out.update(seed=torch.tensor(seed), checksum=C.checksum(d), iterations=torch.tensor(its), converged=torch.tensor(bool(s64.converged)),
               idx=torch.stack(idx64).to(torch.int16), first=torch.tensor(first),
               err32=torch.tensor([err[q] for q in C.ICP_QUANTITIES], dtype=torch.float64))
    return out


def main():
    global C
    import points_alignment_case as C

    ref = reference_module()
    rec = Recorder(ref)
    out = {}
    tried, skipped = {}, {}
    for kind, cases, attempt in (("align", C.ALIGN_CASES, try_align), ("icp", C.ICP_CASES, try_icp)):
        for case in cases:
            start = C.SEED0 + 1000 * case[2]
            for seed in range(start, start + 40):
                tried[case[0]] = tried.get(case[0], 0) + 1
                got = attempt(ref, rec, case, seed)
                if not isinstance(got, str):
                    break
                skipped[case[0]] = skipped.get(case[0], 0) + 1
                print(kind, C.case_id(case), "seed", seed, "skipped:", got)
            else:
                raise AssertionError("no seed for " + C.case_id(case))
            out.update({C.key(kind, case, k): v for k, v in got.items()})
    for family, n in tried.items():
        assert 2 * skipped.get(family, 0) <= n, ("more than half of the seeds of %s were skipped" % family, skipped[family], n)
    print("tried", tried, "skipped", skipped)
    np.savez_compressed(C.FIXTURE, **{k: v.numpy() for k, v in out.items()})
    print("wrote", C.FIXTURE, os.path.getsize(C.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
