#!/usr/bin/env python
"""chamfer_distance and knn_points on one MI355X: the kernels of csrc/knn.hip against this package's own torch formulation on the same
GPU (output kept as profiles/chamfer_mi355x.txt).

    python profiles/chamfer_bench.py [--out FILE]            the driver: every step below in a child process of its own
    python profiles/chamfer_bench.py --step NAME              one step, in this process

The driver runs each step under its own time limit and stops at the first one that fails or runs out of time; it reads nothing
outside the repository.  The baseline is the torch formulation of pytorch3d_amd/knn.py (forced by switching knn.kernel_path off for
that leg): the reference's device KNN kernel is not among the binaries this repository builds for checking.  Shapes: 64 clouds of
5000 x 5000 points and one such cloud, D = 3, random points, forward + backward to both clouds.  Device events around each step,
warm-up iterations untimed, the legs alternating, medians.  The per-kernel times come from the library's built-in timing
(p3d_profile_*) in separate, untimed iterations.

The K = 1 forward against the VALU issue bound: its inner loop is VALU_PER_8_PAIRS vector instructions per 8 pairs per wave (counted
in the disassembly of knn_kernel<3, 2, 1>: per pair 3 sub, 3 mul, 2 add, 1 cmp, 2 cndmask and 1 mov of the wave-uniform index into a
VGPR; +1 for the LDS address), one wave-instruction issues in 4 cycles on one of 4 x 256 SIMDs at CLOCK_GHZ.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_PER_8_PAIRS = 97
SIMDS = 4 * 256
CLOCK_GHZ = 2.4
P = 5000

# name: (time limit of the step in seconds, clouds, what)
STEPS = {
    "chamfer_64": (240, 64, "chamfer"),
    "chamfer_1": (120, 1, "chamfer"),
    "knn8_64": (240, 64, "knn8"),
    "knn8_1": (120, 1, "knn8"),
}


def alternate(legs, warmup, iters):
    """legs: {name: (step, timed iterations or None for `iters`)}; {name: [ms, ...]}, the legs taking turns."""
    import torch

    times = {name: [] for name in legs}
    for i in range(warmup + iters):
        for name, (step, own) in legs.items():
            if own is not None and i >= warmup + own:
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step()
            b.record()
            b.synchronize()
            if i >= warmup:
                times[name].append(a.elapsed_time(b))
    return times


def run_step(name):
    import torch

    import pytorch3d_amd as p3d
    from pytorch3d_amd import _lib
    from pytorch3d_amd import knn as knn_mod

    _, N, what = STEPS[name]
    d = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    x0, y0 = torch.rand(N, P, 3, generator=gen).to(d), torch.rand(N, P, 3, generator=gen).to(d)
    kernel_path = knn_mod.kernel_path

    def step_of(fused, ordered=False):
        def step():
            knn_mod.kernel_path = kernel_path if fused else (lambda *a: False)
            torch.use_deterministic_algorithms(ordered)
            try:
                x, y = x0.clone().requires_grad_(True), y0.clone().requires_grad_(True)
                if what == "chamfer":
                    loss, _ = p3d.chamfer_distance(x, y)
                else:
                    loss = p3d.knn_points(x, y, K=8).dists.sum()
                loss.backward()
            finally:
                knn_mod.kernel_path = kernel_path
                torch.use_deterministic_algorithms(False)
        return step

    # the torch formulation sorts N x P x P distances in chunks: seconds per step at 64 clouds, so it gets fewer timed iterations
    legs = {"kernels (atomic scatter)": (step_of(True), None), "kernels (ordered scatter)": (step_of(True, True), None),
            "torch formulation": (step_of(False), 3 if N > 1 else 10)}
    times = alternate(legs, 2, 20)
    out = {"step": name, "N": N, "legs": {k: {"median": statistics.median(t), "min": min(t), "max": max(t), "iters": len(t)} for k, t in times.items()}}
    lib = _lib.load()
    for label, ordered in (("atomic", False), ("ordered", True)):
        lib.p3d_profile_reset()
        lib.p3d_profile_enable(1)
        try:
            for _ in range(5):
                step_of(True, ordered)()
            torch.cuda.synchronize()
            snap = _lib.profile_snapshot()
        finally:
            lib.p3d_profile_enable(0)
        out["kernels_" + label] = {k: [n, ms / n] for k, (n, ms) in sorted(snap.items())}
    if what == "chamfer":
        bound_ms = N * P * P / 64 / 8 * VALU_PER_8_PAIRS * 4 / (SIMDS * CLOCK_GHZ * 1e9) * 1e3
        out["k1_forward_bound_ms"] = bound_ms
        out["k1_forward_ms"] = out["kernels_atomic"]["chamfer_forward_k1"][1]
    print(json.dumps(out))


def report(rec):
    lines = [f"{rec['step']}: {rec['N']} x {P} x {P}, D = 3, forward + backward, ms per step: median (min .. max) [timed iterations]"]
    for leg, t in rec["legs"].items():
        lines.append(f"  {leg:<28s} {t['median']:10.3f}  ({t['min']:.3f} .. {t['max']:.3f}) [{t['iters']}]")
    base = rec["legs"]["torch formulation"]["median"]
    lines.append(f"  {'torch / kernels (atomic)':<28s} {base / rec['legs']['kernels (atomic scatter)']['median']:10.1f} x")
    for label in ("atomic", "ordered"):
        lines.append(f"  per launch, {label} scatter (ms, mean of the launches of 5 steps):")
        for k, (n, ms) in rec["kernels_" + label].items():
            lines.append(f"    {k:<36s} {ms:9.4f}  x{n // 5} per step")
    if "k1_forward_ms" in rec:
        lines.append(f"  K = 1 forward: {rec['k1_forward_ms']:.4f} ms per launch; the 4-cycle VALU issue bound of its loop "
                     f"({VALU_PER_8_PAIRS} instructions per 8 pairs, {SIMDS} SIMDs, {CLOCK_GHZ} GHz) is {rec['k1_forward_bound_ms']:.4f} ms: "
                     f"the launch takes {rec['k1_forward_ms'] / rec['k1_forward_bound_ms']:.2f} of it")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=sorted(STEPS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        run_step(args.step)
        return
    lines = ["chamfer_distance / knn_points (K = 8): csrc/knn.hip against the package's torch formulation on the same GPU"]
    for name, (limit, _, _) in STEPS.items():
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append(f"{name}: no result within {limit} s; stopped here")
            break
        if res.returncode != 0:
            lines.append(f"{name}: exit status {res.returncode}; stopped here\n{res.stderr[-2000:]}")
            break
        lines += report(json.loads(res.stdout.strip().splitlines()[-1]))
        print("\n".join(lines), flush=True)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
