#!/usr/bin/env python
"""sample_farthest_points and ball_query on one MI355X: the kernels of csrc/fps_ball.hip against this package's own torch formulation
on the same GPU (output kept as profiles/fps_ball_mi355x.txt).

    python profiles/fps_ball_bench.py [--out FILE]            the driver: every step below in a child process of its own
    python profiles/fps_ball_bench.py --step NAME              one step, in this process

The driver runs each step under its own time limit and stops at the first one that fails or runs out of time; it reads nothing
outside the repository.  The baseline is the torch formulation of pytorch3d_amd/sample_farthest_points.py / ball_query.py (forced by
switching the module's kernel_path off for that leg): the reference's device kernels for these two operators are not among the
binaries this repository builds for checking.  Random points in the unit cube, D = 3.  Device events around each step, 2 warm-up
iterations untimed, 20 timed (the formulation of the sampling -- a dozen launches per selected point -- gets 3), the legs
alternating, medians.  The VGPR counts are the compiler's, read from the build's resource record.
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

# name: (time limit of the step in seconds, what, shape)
STEPS = {
    "fps_32x4096_1024": (240, "fps", (32, 4096, 1024)),
    "fps_1x16384_2048": (240, "fps", (1, 16384, 2048)),     # the top of the register form
    "fps_1x100000_2048": (300, "fps", (1, 100000, 2048)),   # the workspace form
    "ball_32x1024x4096_k64": (240, "ball", (32, 1024, 4096, 64, 0.2)),
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

    _, what, shape = STEPS[name]
    d = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    # (importlib: the package re-exports the functions of these names over the sub-modules)
    mod = importlib.import_module("pytorch3d_amd." + ("sample_farthest_points" if what == "fps" else "ball_query"))
    kernel_path = mod.kernel_path

    def forced(fused, fn):
        def step():
            mod.kernel_path = kernel_path if fused else (lambda *a: False)
            try:
                fn()
            finally:
                mod.kernel_path = kernel_path
        return step

    if what == "fps":
        N, P, K = shape
        pts = torch.rand(N, P, 3, generator=gen).to(d)
        fn = lambda: p3d.sample_farthest_points(pts, None, K)  # noqa: E731
        legs = {"kernel": (forced(True, fn), None), "torch formulation": (forced(False, fn), 3)}
    else:
        N, P1, P2, K, radius = shape
        a0, b0 = torch.rand(N, P1, 3, generator=gen).to(d), torch.rand(N, P2, 3, generator=gen).to(d)
        fwd = lambda: p3d.ball_query(a0, b0, K=K, radius=radius, return_nn=False)  # noqa: E731

        def both():
            a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
            p3d.ball_query(a, b, K=K, radius=radius, return_nn=False).dists.sum().backward()

        legs = {"kernel, forward": (forced(True, fwd), None), "kernels, forward + backward": (forced(True, both), None),
                "torch formulation, forward": (forced(False, fwd), 5), "torch formulation, forward + backward": (forced(False, both), 5)}
    times = alternate(legs, 2, 20)
    out = {"step": name, "what": what, "shape": shape,
           "legs": {k: {"median": statistics.median(t), "min": min(t), "max": max(t), "iters": len(t)} for k, t in times.items()}}
    if what == "ball":
        hits = (p3d.ball_query(a0, b0, K=K, radius=radius, return_nn=False).idx >= 0).sum(2).float()
        out["hits_mean"], out["rows_full"] = float(hits.mean()), float((hits == K).float().mean())
    print(json.dumps(out))


def vgprs():
    """{demangled kernel: VGPRs} of csrc/fps_ball.hip from the build's resource record."""
    from pytorch3d_amd import build

    try:
        with open(build.LIB + ".resources.json") as f:
            rec = json.load(f)
    except OSError:
        return {}
    return {build.demangle(k).split("(")[0].replace("void ", ""): (v["vgprs"], v["occupancy"], v["lds"])
            for k, v in sorted(rec.items()) if v.get("source") == "fps_ball.hip"}


def report(rec):
    lines = []
    if rec["what"] == "fps":
        N, P, K = rec["shape"]
        lines.append(f"{rec['step']}: {N} clouds of {P} points -> {K} samples each, ms per call: median (min .. max) [timed iterations]")
    else:
        N, P1, P2, K, radius = rec["shape"]
        lines.append(f"{rec['step']}: {N} x {P1} queries x {P2} points, K = {K}, radius {radius} ({rec['hits_mean']:.1f} hits per row, "
                     f"{100 * rec['rows_full']:.0f} % of the rows full), ms per call: median (min .. max) [timed iterations]")
    for leg, t in rec["legs"].items():
        lines.append(f"  {leg:<40s} {t['median']:10.3f}  ({t['min']:.3f} .. {t['max']:.3f}) [{t['iters']}]")
    if rec["what"] == "fps":
        k, base = rec["legs"]["kernel"]["median"], rec["legs"]["torch formulation"]["median"]
        lines.append(f"  {'kernel, per step of the chain (us)':<40s} {1e3 * k / rec['shape'][2]:10.3f}")
        lines.append(f"  {'torch formulation / kernel':<40s} {base / k:10.1f} x")
    else:
        for tail in ("forward", "forward + backward"):
            k = rec["legs"]["kernel, forward" if tail == "forward" else "kernels, forward + backward"]["median"]
            lines.append(f"  {'torch / kernels, ' + tail:<40s} {rec['legs']['torch formulation, ' + tail]['median'] / k:10.1f} x")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=sorted(STEPS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        run_step(args.step)
        return
    lines = ["sample_farthest_points / ball_query: csrc/fps_ball.hip against the package's torch formulation on the same GPU",
             "(the reference's device kernels for these operators are not among the binaries this repository builds for checking)"]
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
        print("\n".join(lines[-8:]), flush=True)
    lines.append("VGPRs / waves per SIMD / LDS bytes of the kernels (the compiler's resource report of the build):")
    for k, (v, occ, lds) in vgprs().items():
        lines.append(f"  {k:<48s} {v:4d} {occ:3d} {lds:6d}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
