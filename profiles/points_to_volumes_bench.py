#!/usr/bin/env python
"""points_to_volumes on one MI355X: the atomic and the ordered forward of csrc/points_to_volumes.hip and the backward, against this
package's own torch formulation on the same GPU (output kept as profiles/points_to_volumes_mi355x.txt).

    python profiles/points_to_volumes_bench.py [--out FILE]    the driver: every step below in a child process of its own
    python profiles/points_to_volumes_bench.py --step NAME      one step, in this process

The driver runs each step under its own time limit and stops at the first one that fails or runs out of time; it reads nothing
outside the repository.  The baseline is the torch formulation of pytorch3d_amd/points_to_volumes.py (index_put_ with accumulate on
the GPU): it stands in for the reference's `_python=True`, the only thing a user could run before these kernels; the reference's
compiled operator is not among the binaries this repository builds for checking.  Points uniform in [-1.05, 1.05]^3 (a few percent
outside the cube), align_corners=True, point_weight 1, the operators called directly on preallocated volumes (the forward adds in
place; forward + backward also zero-fills the two gradient buffers, as the autograd node does).  The ordered leg runs under
torch.use_deterministic_algorithms(True) and includes the keys kernel and torch's stable sort.  20 untimed warm-up iterations of
every leg (code objects, allocator, clocks), then 20 timed ones (the formulation gets 5), the legs alternating, device events
around each call; medians with the spread.  The atomic-issue bound of a forward is samples * (1 + C) / 20e9 s, samples = 8 per
point for trilinear and 1 for nearest: profiles/microbench/global_atomic_mi355x.txt has 20 G lane-atomics/s when every lane hits
another row.
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ATOMICS_PER_SECOND = 20e9

# name: (time limit of the step in seconds, mode, N, P, C, grid side)
STEPS = {
    "trilinear_8x100000_c3_64": (300, "trilinear", 8, 100000, 3, 64),
    "trilinear_1x1000000_c3_128": (300, "trilinear", 1, 1000000, 3, 128),
    "nearest_1x1000000_c3_128": (300, "nearest", 1, 1000000, 3, 128),
    "trilinear_8x100000_c32_64": (420, "trilinear", 8, 100000, 32, 64),
}


def alternate(legs, warmup, iters):
    """legs: {name: (step, timed iterations or None for `iters`)}; {name: [ms, ...]}, the legs taking turns."""
    import torch

    times = {name: [] for name in legs}
    for i in range(warmup + iters):
        for name, (step, own) in legs.items():
            if own is not None and (i >= warmup + own or (i < warmup and i >= 2)):  # (a slow leg warms up twice)
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

    from pytorch3d_amd import _C

    _, mode, N, P, C, side = STEPS[name]
    splat = mode == "trilinear"
    d = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    m = importlib.import_module("pytorch3d_amd.points_to_volumes")
    pts = (torch.rand(N, P, 3, generator=gen) * 2.1 - 1.05).to(d)
    feats = torch.rand(N, P, C, generator=gen).to(d)
    grid = torch.tensor([[side] * 3] * N, device=d)
    mask = torch.ones(N, P, device=d)
    dens, vol = torch.zeros(N, 1, side, side, side, device=d), torch.zeros(N, C, side, side, side, device=d)
    gd, gv = torch.randn(N, 1, side, side, side, device=d), torch.randn(N, C, side, side, side, device=d)

    def forward(op):
        op(pts, feats, dens, vol, grid, mask, 1.0, True, splat)

    def both(fwd, bwd):
        fwd(pts, feats, dens, vol, grid, mask, 1.0, True, splat)
        gp, gf = torch.zeros_like(pts), torch.zeros_like(feats)
        bwd(pts, feats, grid, mask, 1.0, True, splat, gd, gv, gp, gf)

    def strict(fn):
        def step():
            torch.use_deterministic_algorithms(True)
            try:
                fn()
            finally:
                torch.use_deterministic_algorithms(False)
        return step

    kf, kb = m.points_to_volumes_forward_op, m.points_to_volumes_backward_op
    tf, tb = m.torch_points_to_volumes_forward, m.torch_points_to_volumes_backward
    legs = {"kernel, atomic, forward": (lambda: forward(kf), None),
            "kernel, ordered, forward": (strict(lambda: forward(kf)), None),
            "kernels, atomic, forward + backward": (lambda: both(kf, kb), None),
            "kernels, ordered, forward + backward": (strict(lambda: both(kf, kb)), None),
            "torch formulation, forward": (lambda: forward(tf), 5),
            "torch formulation, forward + backward": (lambda: both(tf, tb), 5)}
    before = dict(_C.POINTS_TO_VOLUMES_CALLS)
    times = alternate(legs, 20, 20)
    ran = {k: _C.POINTS_TO_VOLUMES_CALLS[k] - before[k] for k in before}
    assert ran["atomic"] == 80 and ran["ordered"] == 80, ran  # each form ran where it was asked for
    samples = N * P * (8 if splat else 1)
    print(json.dumps({"step": name, "mode": mode, "shape": (N, P, C, side), "bound_ms": 1e3 * samples * (1 + C) / ATOMICS_PER_SECOND,
                      "legs": {k: {"median": statistics.median(t), "min": min(t), "max": max(t), "iters": len(t)}
                               for k, t in times.items()}}))


def vgprs():
    """{demangled kernel: (VGPRs, occupancy)} of csrc/points_to_volumes.hip from the build's resource record."""
    from pytorch3d_amd import build

    try:
        with open(build.LIB + ".resources.json") as f:
            rec = json.load(f)
    except OSError:
        return {}
    return {build.demangle(k).split("(")[0].replace("void ", ""): (v["vgprs"], v["occupancy"])
            for k, v in sorted(rec.items()) if v.get("source") == "points_to_volumes.hip"}


def report(rec):
    N, P, C, side = rec["shape"]
    lines = [f"{rec['step']}: {rec['mode']}, {N} clouds x {P} points, C = {C}, into {side}^3; ms per call: median (min .. max) "
             "[timed iterations]"]
    for leg, t in rec["legs"].items():
        lines.append(f"  {leg:<44s} {t['median']:10.3f}  ({t['min']:.3f} .. {t['max']:.3f}) [{t['iters']}]")
    lines.append(f"  {'atomic-issue bound of the forward (ms)':<44s} {rec['bound_ms']:10.3f}")
    for form in ("atomic", "ordered"):
        lines.append(f"  {form + ' forward / bound':<44s} {rec['legs']['kernel, ' + form + ', forward']['median'] / rec['bound_ms']:10.2f} x")
    for tail in ("forward", "forward + backward"):
        k = rec["legs"]["kernel, atomic, forward" if tail == "forward" else "kernels, atomic, forward + backward"]["median"]
        lines.append(f"  {'torch formulation / atomic, ' + tail:<44s} {rec['legs']['torch formulation, ' + tail]['median'] / k:10.1f} x")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.step:
        run_step(args.step)
        return
    lines = ["points_to_volumes on one MI355X (profiles/points_to_volumes_bench.py): csrc/points_to_volumes.hip against the package's torch",
             "formulation on the same GPU.  Device events, 20 warm-up iterations untimed, the legs alternating."]
    for name, (limit, *_rest) in STEPS.items():
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=limit)
        if res.returncode != 0:
            lines.append(f"{name}: FAILED with exit status {res.returncode}; the steps behind it were not run")
            lines.append(res.stderr[-2000:])
            break
        lines += [""] + report(json.loads(res.stdout.strip().splitlines()[-1]))
    regs = vgprs()
    if regs:
        lines += ["", "kernel: VGPRs, waves per SIMD (the compiler's record)"] + [f"  {k:<60s} {v[0]:4d} {v[1]:3d}" for k, v in regs.items()]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    if any("FAILED" in line for line in lines):
        sys.exit(1)


if __name__ == "__main__":
    main()
