#!/usr/bin/env python
"""knn_points on large 3D clouds on one MI355X: the grid search of csrc/knn_grid.hip against the scan of all pairs of csrc/knn.hip,
the same build, the same GPU, the same process (output kept as profiles/knn_grid_mi355x.txt).

    python profiles/knn_grid_bench.py [--out FILE]       the driver: every shape below in a child process of its own
    python profiles/knn_grid_bench.py --step NAME         one shape, in this process

The driver runs each shape under its own time limit and stops at the first one that fails or runs out of time; it reads nothing
outside the repository.  The public knn_points, forward and forward + backward to both clouds, K in {1, 8, 32}, three seeded
distributions: uniform in a cube, the surface of a sphere, eight Gaussian clusters with 1 % far outliers.  The legs are chosen by
knn.GRID_MIN_P2 (0: the grid; None: all pairs, the parent's kernel untouched).  Before any timing the two legs' idx and dists are
compared with torch.equal on the timed inputs, and the step fails where they differ.  A window is `reps` calls between two device
events, the second one synchronised, reps chosen from the warm-up call so that a window lasts at least WINDOW_MS; WINDOWS windows
per leg, the legs alternating; per call the median and the spread (min .. max) of the windows.  A leg whose call takes more than
SLOW_MS is timed in windows of one call, twice.

Last, the threshold: the smallest swept P of the 1 x P x P shapes from which on the grid is faster than all pairs in every
distribution, K and mode by more than the spread of the pair -- the grid's slowest window below the scan's fastest.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW_MS, WINDOWS, SLOW_MS = 50.0, 5, 250.0
KS = (1, 8, 32)
CLOUDS = ("cube", "sphere", "clusters")
# name: (time limit in seconds, N, P)
STEPS = {"p4096": (300, 1, 4096), "p16384": (300, 1, 16384), "p65536": (300, 1, 65536), "p262144": (400, 1, 262144),
         "p1000000": (900, 1, 1000000), "batch8_p32768": (400, 8, 32768)}


def cloud(kind, N, P, gen):
    import torch

    if kind == "cube":
        return torch.rand(N, P, 3, generator=gen)
    if kind == "sphere":
        v = torch.randn(N, P, 3, generator=gen)
        return v / v.norm(dim=2, keepdim=True).clamp_min(1e-12)
    centres = torch.rand(N, 8, 3, generator=gen)
    pick = torch.randint(0, 8, (N, P), generator=gen)
    x = torch.gather(centres, 1, pick[..., None].expand(-1, -1, 3)) + 0.03 * torch.randn(N, P, 3, generator=gen)
    far = torch.rand(N, P, generator=gen) < 0.01
    return torch.where(far[..., None], 100.0 * (torch.rand(N, P, 3, generator=gen) - 0.5), x)


def run_step(name):
    import torch

    import pytorch3d_amd as p3d
    from pytorch3d_amd import knn as knn_mod

    _, N, P = STEPS[name]
    d = torch.device("cuda:0")
    out = {"step": name, "N": N, "P": P, "rows": []}

    def call(x0, y0, K, grid, backward):
        knn_mod.GRID_MIN_P2 = 0 if grid else None
        try:
            if not backward:
                return p3d.knn_points(x0, y0, K=K)
            x, y = x0.clone().requires_grad_(True), y0.clone().requires_grad_(True)
            res = p3d.knn_points(x, y, K=K)
            res.dists.sum().backward()
            return res
        finally:
            knn_mod.GRID_MIN_P2 = None

    def window(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    for kind in CLOUDS:
        gen = torch.Generator().manual_seed(len(kind))
        x0, y0 = cloud(kind, N, P, gen).to(d), cloud(kind, N, P, gen).to(d)
        for K in KS:
            for backward in (False, True):
                legs = {"grid": lambda: call(x0, y0, K, True, backward), "all pairs": lambda: call(x0, y0, K, False, backward)}
                ours, base = legs["grid"](), legs["all pairs"]()
                if not (torch.equal(ours.idx, base.idx) and torch.equal(ours.dists, base.dists)):
                    raise SystemExit(f"{name} {kind} K={K}: idx or dists of the two legs differ")
                del ours, base
                torch.cuda.synchronize()
                first = {leg: window(fn, 1) for leg, fn in legs.items()}  # warm: the second call of the shape
                reps = {leg: max(1, min(500, math.ceil(WINDOW_MS / max(t, 1e-3)))) for leg, t in first.items()}
                count = {leg: 2 if first[leg] > SLOW_MS else WINDOWS for leg in legs}
                times = {leg: [] for leg in legs}
                for i in range(WINDOWS):
                    for leg, fn in legs.items():
                        if i < count[leg]:
                            times[leg].append(window(fn, reps[leg]))
                out["rows"].append({"cloud": kind, "K": K, "backward": backward, "reps": reps,
                                    "ms": {leg: [statistics.median(t), min(t), max(t), len(t)] for leg, t in times.items()}})
    print(json.dumps(out))


def report(rec):
    lines = [f"{rec['step']}: {rec['N']} x {rec['P']} x {rec['P']}; idx and dists of the two legs bit-equal on every row; ms per call: "
             "median (min .. max) [windows x calls]"]
    for row in rec["rows"]:
        g, a = row["ms"]["grid"], row["ms"]["all pairs"]
        verdict = "grid" if g[2] < a[1] else ("all pairs" if a[2] < g[1] else "within the spread")
        lines.append(f"  {row['cloud']:<9s} K={row['K']:<3d} {'fwd+bwd' if row['backward'] else 'forward':<8s}"
                     f" grid {g[0]:10.3f} ({g[1]:.3f} .. {g[2]:.3f}) [{g[3]} x {row['reps']['grid']}]"
                     f"   all pairs {a[0]:10.3f} ({a[1]:.3f} .. {a[2]:.3f}) [{a[3]} x {row['reps']['all pairs']}]"
                     f"   {a[0] / g[0]:8.2f} x   faster: {verdict}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=sorted(STEPS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        run_step(args.step)
        return
    lines = ["knn_points on 3D clouds: the grid search of csrc/knn_grid.hip against the scan of all pairs of csrc/knn.hip, same GPU"]
    wins = {}
    for name, (limit, N, P) in STEPS.items():
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append(f"{name}: no result within {limit} s; stopped here")
            break
        if res.returncode != 0:
            lines.append(f"{name}: exit status {res.returncode}; stopped here\n{res.stdout[-500:]}\n{res.stderr[-2000:]}")
            break
        rec = json.loads(res.stdout.strip().splitlines()[-1])
        lines += report(rec)
        if N == 1:
            wins[P] = all(r["ms"]["grid"][2] < r["ms"]["all pairs"][1] for r in rec["rows"])
        print("\n".join(lines[-19:]), flush=True)
    good = [P for P in sorted(wins) if all(wins[Q] for Q in wins if Q >= P)]
    lines.append(f"threshold (1 x P x P): the grid is faster on every row from P = {good[0]} on" if good else
                 "threshold (1 x P x P): no swept P from which on the grid is faster on every row")
    print(lines[-1], flush=True)
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
