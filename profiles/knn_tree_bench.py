#!/usr/bin/env python
"""knn_points on 3D clouds on one MI355X: the tree search of csrc/knn_tree.hip against the grid search of csrc/knn_grid.hip and the
scan of all pairs of csrc/knn.hip, the same build, the same GPU, the same process (output kept as
profiles/knn_tree_mi355x.txt).

    python profiles/knn_tree_bench.py [--out FILE] [--only NAME,NAME]   the driver: every shape in a child process of its own
    python profiles/knn_tree_bench.py --step NAME                        one shape, in this process

The driver runs each shape under its own time limit and stops at the first one that fails or runs out of time; it reads nothing
outside the repository.  The public knn_points, forward, K in {1, 8, 32}, three seeded distributions: uniform in a cube, the surface
of a sphere, eight Gaussian clusters with 1 % far outliers (those of profiles/knn_grid_bench.py).  The legs are chosen by
knn.TREE_MIN_P2 and knn.GRID_MIN_P2 (0: that search; both None: all pairs, the parent's kernel untouched).  Before any timing the
three legs' idx and dists are compared with torch.equal on the timed inputs, and the step fails where they differ.  A window is
`reps` calls between two device events, the second one synchronised, reps chosen from the warm-up call so that a window lasts at
least WINDOW_MS; WINDOWS windows per leg, the legs alternating; per call the median and the spread (min .. max) of the windows.  A leg
whose call takes more than SLOW_MS is timed in windows of one call, twice.  The tree's build (bounds, keys, sort, boxes) and its
search are timed apart by the library's own launch scopes in a run of their own behind the windows, four calls.

Last, per batch size, the spread of the legs and the threshold: the smallest swept P from which on the tree is faster than all
pairs in every distribution and K by more than the spread of the pair -- the tree's slowest window below the scan's fastest.
knn.TREE_MIN_P2 is the threshold of the 1 x P x P shapes.  --only runs a part of the steps (the kept file is two runs, the 1 x P and
the 8 x P steps, put together; it says so in its second line).
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
LEGS = ("tree", "grid", "all pairs")
# name: (time limit in seconds, N, P)
STEPS = {"p4096": (200, 1, 4096), "p32768": (200, 1, 32768), "p262144": (300, 1, 262144), "p1000000": (600, 1, 1000000),
         "batch8_p4096": (200, 8, 4096), "batch8_p32768": (300, 8, 32768), "batch8_p262144": (600, 8, 262144),
         "batch8_p1000000": (1100, 8, 1000000)}


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
    from pytorch3d_amd import _lib
    from pytorch3d_amd import knn as knn_mod

    _, N, P = STEPS[name]
    d = torch.device("cuda:0")
    lib = _lib.load()
    out = {"step": name, "N": N, "P": P, "rows": []}

    def call(x0, y0, K, leg):
        shipped = knn_mod.TREE_MIN_P2, knn_mod.GRID_MIN_P2
        knn_mod.TREE_MIN_P2, knn_mod.GRID_MIN_P2 = (0 if leg == "tree" else None), (0 if leg == "grid" else None)
        try:
            return p3d.knn_points(x0, y0, K=K)
        finally:
            knn_mod.TREE_MIN_P2, knn_mod.GRID_MIN_P2 = shipped

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
            legs = {leg: (lambda leg=leg: call(x0, y0, K, leg)) for leg in LEGS}
            base = legs["all pairs"]()
            for leg in ("tree", "grid"):
                ours = legs[leg]()
                if not (torch.equal(ours.idx, base.idx) and torch.equal(ours.dists, base.dists)):
                    raise SystemExit(f"{name} {kind} K={K}: idx or dists of {leg} and all pairs differ")
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
            lib.p3d_profile_reset()
            lib.p3d_profile_enable(1)
            for _ in range(4):
                legs["tree"]()
            torch.cuda.synchronize()
            scopes = _lib.profile_snapshot()
            lib.p3d_profile_enable(0)
            out["rows"].append({"cloud": kind, "K": K, "reps": reps,
                                "ms": {leg: [statistics.median(t), min(t), max(t), len(t)] for leg, t in times.items()},
                                "scopes": {k: scopes[k][1] / scopes[k][0] for k in ("knn_tree_build", "knn_tree_search") if k in scopes}})
    print(json.dumps(out))


def report(rec):
    lines = [f"{rec['step']}: {rec['N']} x {rec['P']} x {rec['P']}, forward; idx and dists of the three legs bit-equal on every row; "
             "ms per call: median (min .. max) [windows x calls]; tree = build + search by the launch scopes"]
    for row in rec["rows"]:
        t, g, a = (row["ms"][leg] for leg in LEGS)
        verdict = "tree" if t[2] < a[1] else ("all pairs" if a[2] < t[1] else "within the spread")
        s = row["scopes"]
        lines.append(f"  {row['cloud']:<9s} K={row['K']:<3d}"
                     f" tree {t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f}) [{t[3]} x {row['reps']['tree']}]"
                     f" = {s.get('knn_tree_build', float('nan')):.3f} + {s.get('knn_tree_search', float('nan')):.3f}"
                     f"   grid {g[0]:9.3f} ({g[1]:.3f} .. {g[2]:.3f}) [{g[3]} x {row['reps']['grid']}]"
                     f"   all pairs {a[0]:9.3f} ({a[1]:.3f} .. {a[2]:.3f}) [{a[3]} x {row['reps']['all pairs']}]"
                     f"   vs all pairs {a[0] / t[0]:7.2f} x, vs grid {g[0] / t[0]:7.2f} x   faster of tree and all pairs: {verdict}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=sorted(STEPS))
    ap.add_argument("--only", default=None, help="comma-separated steps for the driver")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        run_step(args.step)
        return
    lines = ["knn_points on 3D clouds: the tree search of csrc/knn_tree.hip against the grid search of csrc/knn_grid.hip and the scan "
             "of all pairs of csrc/knn.hip, same GPU"]
    wins, spread = {}, {}  # per batch size N: {P: the tree wins every row}, the largest spread of a leg
    for name, (limit, N, P) in STEPS.items():
        if args.only and name not in args.only.split(","):
            continue
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
        spread[N] = max([spread.get(N, 0.0)] + [(r["ms"][leg][2] - r["ms"][leg][1]) / r["ms"][leg][0] for r in rec["rows"] for leg in LEGS])
        wins.setdefault(N, {})[P] = all(r["ms"]["tree"][2] < r["ms"]["all pairs"][1] for r in rec["rows"])
        print("\n".join(lines[-10:]), flush=True)
        if args.out:  # after every step: a later step that runs out of time loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    tail = len(lines)
    for N in sorted(wins):
        good = [P for P in sorted(wins[N]) if all(wins[N][Q] for Q in wins[N] if Q >= P)]
        lines.append(f"{N} x P x P: run-to-run spread of the legs at most {100.0 * spread[N]:.1f} % (max - min of a leg's windows over its "
                     "median); " + (f"the tree is faster than all pairs on every row from P = {good[0]} on" if good else
                                    "no swept P from which on the tree is faster than all pairs on every row"))
    print("\n".join(lines[tail:]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
