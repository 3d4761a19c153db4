#!/usr/bin/env python
"""estimate_pointcloud_local_coord_frames on one MI355X: the kernel of csrc/point_frames.hip against what the same call cost before
it existed, and against this package's own torch formulation (output kept as profiles/point_frames_mi355x.txt).

    python profiles/point_frames_bench.py [--out FILE]        the driver: every step below in a child process of its own
    python profiles/point_frames_bench.py --step NAME          one step, in this process

The driver runs each step under its own time limit and stops at the first one that fails or runs out of time; it reads nothing
outside the repository but the staged reference package (oracle/_ref/reference_py, or P3D_REFERENCE_ROOT).  Legs:
  kernel       pytorch3d_amd.estimate_pointcloud_local_coord_frames (float32 GPU clouds: one launch after the recentring)
  parent       the UNMODIFIED reference function under shim.install(patch_python=True) with the two rebindings of
               pytorch3d.ops.points_normals taken out again: the reference's Python on this package's knn_points, which is what the
               call ran on the commit before the kernel (K = 50 > P3D_KNN_MAX_K goes to the chunked sort, K = 16 to csrc/knn.hip)
  formulation  the package's torch formulation (the kernel path switched off for the leg)
A leg whose first (untimed) run takes longer than SLOW seconds is reported from that single run and not repeated.  One cloud of
10^6 points with K = 50 has the kernel leg only: the parent's path there is 250 000 chunked sorts, minutes per run.
Random points on a noisy unit sphere.  Device events around each call, WARMUP warm-up runs untimed, then REPS timed, the legs taking
turns; min / median / max are reported, peak memory is torch.cuda.max_memory_allocated over a leg's own runs.  The scan bound: a
pair costs 9 VALU instructions (3 sub, 3 mul, 2 add, 1 cmp) of 4 cycles per wave of 64 queries; 1024 SIMDs at 2.4 GHz.
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP, REPS, SLOW = 2, 10, 5.0
# name: (time limit of the step in seconds, (N, P, K), legs)
STEPS = {
    "32x4096_k50": (300, (32, 4096, 50), ("kernel", "parent", "formulation")),
    "32x4096_k16": (300, (32, 4096, 16), ("kernel", "parent", "formulation")),
    "1x100000_k50": (420, (1, 100000, 50), ("kernel", "parent", "formulation")),
    "1x100000_k16": (300, (1, 100000, 16), ("kernel", "parent", "formulation")),
    "1x1000000_k50": (420, (1, 1000000, 50), ("kernel",)),  # parent / formulation: 250 000 chunked sorts of 4 rows, minutes per run
    "1x1000000_k16": (420, (1, 1000000, 16), ("kernel", "parent")),
}


def _reference_root():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    return next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "ops"))), None)


def run_step(name):
    import torch

    import pytorch3d_amd as p3d

    _, (N, P, K), legs = STEPS[name]
    d = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1)
    pts = torch.randn(N, P, 3, generator=gen)
    pts = (pts / pts.norm(dim=2, keepdim=True) * (1 + 0.01 * torch.randn(N, P, 1, generator=gen))).to(d)
    PN = importlib.import_module("pytorch3d_amd.points_normals")
    fns = {}
    if "kernel" in legs:
        fns["kernel"] = lambda: p3d.estimate_pointcloud_local_coord_frames(pts, K)
    if "formulation" in legs:
        def formulation():
            keep = PN.kernel_path
            PN.kernel_path = lambda *a, **k: False
            try:
                return p3d.estimate_pointcloud_local_coord_frames(pts, K)
            finally:
                PN.kernel_path = keep
        fns["formulation"] = formulation
    if "parent" in legs and _reference_root() is not None:
        import run_reference_suite as rrs

        rrs._stub_missing_packages()
        import pytorch3d_amd.shim as shim

        shim.install(_reference_root(), patch_python=True)
        ref = importlib.import_module("pytorch3d.ops.points_normals")
        theirs = ref.estimate_pointcloud_local_coord_frames.__wrapped__  # the reference's own function, knn_points stays patched
        fns["parent"] = lambda: theirs(pts, K)
    out = {"shape": [N, P, K], "times_ms": {}, "peak_bytes": {}, "single_run": []}
    slow = set()
    for leg, fn in fns.items():  # first run: code objects, allocator; decides whether the leg is repeated
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        first = time.perf_counter() - t0
        out["peak_bytes"][leg] = int(torch.cuda.max_memory_allocated())
        if leg == "kernel":
            kernel_res = res
        elif leg == "parent" and "kernel" in fns:  # the same estimate: normals up to sign where both are defined
            dots = (res[1][..., 0] * kernel_res[1][..., 0]).sum(-1).abs()
            out["parent_vs_kernel_median_1_minus_dot"] = float((1 - dots).median())
        del res
        if first > SLOW:
            slow.add(leg)
            out["times_ms"][leg] = [first * 1e3]
            out["single_run"].append(leg)
    times = {leg: [] for leg in fns if leg not in slow}
    for i in range(WARMUP + REPS):
        for leg in times:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fns[leg]()
            b.record()
            b.synchronize()
            if i >= WARMUP:
                times[leg].append(a.elapsed_time(b))
    out["times_ms"].update(times)
    out["scan_bound_ms"] = N * P * (P / 64.0) * 9 * 4 / (1024 * 2.4e9) * 1e3
    print(json.dumps(out))


def kernel_vgprs():
    """{demangled kernel: (VGPRs, occupancy)} of csrc/point_frames.hip from the build's resource record."""
    from pytorch3d_amd import build as lib_build

    with open(lib_build.LIB + ".resources.json") as f:
        rec = json.load(f)
    return {lib_build.demangle(k).split("(")[0]: (v["vgprs"], v["agprs"], v["vgpr_spill"], v["occupancy"]) for k, v in sorted(rec.items())
            if v.get("source") == "point_frames.hip"}


def fixture_tolerances():
    import point_frames_case as C

    z = C.fixture()
    return {C.case_id(c): [float(v) for v in z[C.key(c, "tol")]] for c in C.all_cases()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_frames_mi355x.txt"))
    args = ap.parse_args()
    if args.step:
        return run_step(args.step)
    lines = ["estimate_pointcloud_local_coord_frames: csrc/point_frames.hip against the parent commit's path and the torch formulation",
             "one MI355X, device events, %d warm-up + %d timed runs per leg, legs taking turns; ms as min / median / max" % (WARMUP, REPS),
             "kernel: the public function (float64 cloud mean, recentring, one launch).  parent: NOT a run of the parent commit but the",
             "reference's own function on this package's knn_points, which is what that commit ran (the docstring of the script).",
             "1x1000000_k50 has NO baseline: the parent's path there is 250 000 chunked sorts, minutes per run; formulation likewise.", ""]
    for name, (limit, shape, _) in STEPS.items():
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append("%s: ran out of its %d s; stopping here" % (name, limit))
            break
        if res.returncode != 0:
            lines.append("%s: failed (exit %d): %s" % (name, res.returncode, res.stderr.strip()[-400:]))
            break
        rec = json.loads(res.stdout.strip().splitlines()[-1])
        lines.append("%s  (N, P, K) = %s   scan-only VALU bound %.3f ms" % (name, tuple(rec["shape"]), rec["scan_bound_ms"]))
        med = {}
        for leg, ts in rec["times_ms"].items():
            med[leg] = statistics.median(ts)
            note = "  (ONE run: the first, untimed-warm-up run was above %.0f s)" % SLOW if leg in rec["single_run"] else ""
            lines.append("  %-12s %10.3f / %10.3f / %10.3f ms   peak memory %8.1f MiB%s"
                         % (leg, min(ts), med[leg], max(ts), rec["peak_bytes"][leg] / 2 ** 20, note))
        if "kernel" in med:
            lines.append("  kernel / scan bound %.2f" % (med["kernel"] / rec["scan_bound_ms"])
                         + "".join("   %s / kernel %.1f x" % (leg, med[leg] / med["kernel"]) for leg in med if leg != "kernel"))
        if "parent_vs_kernel_median_1_minus_dot" in rec:
            lines.append("  normals, parent against kernel: median 1 - |dot| %.3g" % rec["parent_vs_kernel_median_1_minus_dot"])
        lines.append("")
        print("\n".join(lines[-8:]), flush=True)
        with open(args.out, "w") as f:  # kept after every step: a later step that runs out of time loses nothing
            f.write("\n".join(lines) + "\n")
    lines.append("registers of the kernels (VGPRs, AGPRs, spilled VGPRs, waves / SIMD): " + json.dumps(kernel_vgprs()))
    lines.append("")
    lines.append("tolerances recorded in tests/golden/point_frames_ref.npz (the reference's own float32 against float64 figures: cov, curv, "
                 "flat, vec, ortho; the tests allow 4 x max(these, float32 eps)):")
    for k, v in fixture_tolerances().items():
        lines.append("  %-16s %s" % (k, "  ".join("%.3g" % x for x in v)))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
