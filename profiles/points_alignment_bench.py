#!/usr/bin/env python
"""iterative_closest_point on one MI355X: pytorch3d_amd.iterative_closest_point (csrc/points_alignment.hip) against what the same call
ran before the kernels existed -- the UNMODIFIED reference's iterative_closest_point under shim.install(patch_python=True) with the
alignment left to the reference: this package's knn_points kernel, then the reference's own corresponding_points_alignment chain
(wmean, bmm, torch.svd, det, bmm), its transform, rmse and host reads.  The script rebinds the reference module's
`corresponding_points_alignment` to the reference's own function to get that state back (output kept as
profiles/points_alignment_mi355x.txt).  Needs the staged reference package (oracle/_ref/reference_py, or P3D_REFERENCE_ROOT).

    python profiles/points_alignment_bench.py [--out FILE]

Shapes b x P1 x P2: 1 x 10 000 x 10 000, 8 x 5000 x 5000, 64 x 1024 x 1024; Y an anisotropic Gaussian blob, X noisy samples of it
moved by a rotation of 9 to 23 degrees and a shift.  Per shape:
  iterations       what the two take to converge at the default threshold (a run each, not timed): [ours, baseline]
  wall_ms          [min, median, max] over REPS calls with max_iterations = ITERS and relative_rmse_thr = -1 (no run converges: both do
                   exactly ITERS iterations on the same inputs), perf_counter around the call and a device synchronise; the two
                   alternate inside the loop.  per_iteration_ms: the median over ITERS.  baseline_over_ours: the medians' quotient
  max_dR, max_dXt  the largest difference between the two results after those ITERS iterations
  kernels_ms       the library's own event timing per kernel, per iteration (median over REPS calls): where an iteration's device time goes
  split            the waves per workgroup the search chose (from its launch rule)"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PREWARM = 2
REPS = 7
ITERS = 20
SHAPES = ((1, 10000, 10000), (8, 5000, 5000), (64, 1024, 1024))
KERNELS = ("icp_match", "icp_means", "icp_moments", "icp_solve", "icp_rmse", "icp_finish")


def wall(fns, reps):
    """{name: [min, median, max] wall ms} of the callables, alternating, each call ended by a device synchronise."""
    import torch

    for _ in range(PREWARM):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t) * 1e3)
    return {name: [round(min(v), 3), round(statistics.median(v), 3), round(max(v), 3)] for name, v in ms.items()}


def clouds(b, P1, P2, device):
    import torch

    import points_alignment_case as C

    gen = torch.Generator().manual_seed(b * 100003 + P1)
    Xs, Ys = [], []
    for n in range(b):
        y = torch.randn(P2, 3, generator=gen) * torch.tensor([1.0, 0.6, 0.3])
        x = y[torch.randint(0, P2, (P1,), generator=gen)] + 0.02 * torch.randn(P1, 3, generator=gen)
        Xs.append(C.move(x, C.rotation(n % 5, (n + 2) % 5), (0.05, -0.03, 0.04), 1.0)), Ys.append(y)
    return torch.stack(Xs).to(device), torch.stack(Ys).to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import run_reference_suite as rrs

    if not torch.cuda.is_available():
        sys.exit("points_alignment_bench: no GPU (the numbers of this script are device and wall times on one)")
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    ref_root = next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "ops"))), None)
    if ref_root is None:
        sys.exit("points_alignment_bench: the reference's Python package is not staged (the baseline is its function)")
    rrs._stub_missing_packages()
    import pytorch3d_amd as p3d
    import pytorch3d_amd.shim as shim
    from pytorch3d_amd import _lib

    shim.install(ref_root, patch_python=True)
    ref_mod = importlib.import_module("pytorch3d.ops.points_alignment")
    reference_icp = ref_mod.iterative_closest_point.__wrapped__
    assert not getattr(reference_icp, "__p3d_amd__", False) and getattr(ref_mod.knn_points, "__p3d_amd__", False)
    ref_mod.corresponding_points_alignment = ref_mod.corresponding_points_alignment.__wrapped__  # the state before these kernels
    d = torch.device("cuda:0")
    lib = _lib.load()
    lines = ["iterative_closest_point on %s, torch %s; PREWARM %d, REPS %d, ITERS %d; wall ms per call as [min, median, max], each call "
             "ended by a device synchronise" % (torch.cuda.get_device_name(0), torch.__version__, PREWARM, REPS, ITERS)]

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for b, P1, P2 in SHAPES:
        X, Y = clouds(b, P1, P2, d)
        natural = [len(fn(X, Y).t_history) for fn in (p3d.iterative_closest_point, reference_icp)]
        fixed = dict(max_iterations=ITERS, relative_rmse_thr=-1.0)
        ours = lambda: p3d.iterative_closest_point(X, Y, **fixed)  # noqa: E731
        baseline = lambda: reference_icp(X, Y, **fixed)  # noqa: E731
        got, want = ours(), baseline()
        assert len(got.t_history) == len(want.t_history) == ITERS and not got.converged and not want.converged
        rec = {"shape": [b, P1, P2], "iterations": natural,
               "max_dR": float((got.RTs.R - want.RTs.R).abs().max()), "max_dXt": float((got.Xt - want.Xt).abs().max())}
        del got, want
        times = wall({"ours": ours, "baseline": baseline}, REPS)
        rec["wall_ms"], rec["baseline_wall_ms"] = times["ours"], times["baseline"]
        rec["per_iteration_ms"] = round(times["ours"][1] / ITERS, 4)
        rec["baseline_per_iteration_ms"] = round(times["baseline"][1] / ITERS, 4)
        rec["baseline_over_ours"] = round(times["baseline"][1] / times["ours"][1], 2)
        lib.p3d_profile_enable(1)
        lib.p3d_profile_reset()
        per = {k: [] for k in KERNELS}
        for _ in range(REPS):
            ours()
            snap = _lib.profile_snapshot()
            for k in KERNELS:
                per[k].append(snap[k][1] / snap[k][0])
            lib.p3d_profile_reset()
        lib.p3d_profile_enable(0)
        rec["kernels_ms"] = {k: round(statistics.median(v), 4) for k, v in per.items()}
        blocks, simds, tiles, split = b * ((P1 + 63) // 64), 4 * torch.cuda.get_device_properties(0).multi_processor_count, (P2 + 511) // 512, 1
        while split < 8 and blocks * 2 * split <= simds and 2 * split <= tiles:
            split *= 2
        rec["split"] = split
        emit(rec)
        del X, Y
        torch.cuda.empty_cache()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
