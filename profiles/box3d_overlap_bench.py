#!/usr/bin/env python
"""box3d_overlap on one MI355X: csrc/box3d.hip's two launches, the public function with its one host sync, and the library's host
loop as context (output kept as profiles/box3d_overlap_mi355x.txt).

    python profiles/box3d_overlap_bench.py [--out FILE]

Shapes: 64 x 64 and 1000 x 1000 random oriented boxes from the generator of tests/box3d_case.py (sides in [0.5, 2], random rotation,
centres in [-1, 1]^3), and 1000 x 1000 axis-aligned boxes on a lattice of quarter units, the coplanar-heavy extreme.  Per shape:
  kernel     pytorch3d_amd._C.iou_box3d: the memset of the overflow counter, the LDS launch and the slab launch
  function   pytorch3d_amd.box3d_overlap on GPU tensors: the input checks, their one host sync, the kernels
  host       p3d_iou_box3d_host on min(N * M, HOST_PAIRS) pairs, serial, one core: microseconds per pair
and the overlapping fraction and the number of pairs the slab launch redid.  A last record runs the 1000 x 1000 random shape with
the LDS capacity lowered to 16, so that nearly every overlapping pair is redone from the workspace slab by the second launch's
P3D_BOX3D_SLAB_WAVES waves: what that launch costs when it does all the work.  Device events around each call, WARMUP untimed runs,
then REPS timed; min / median / max.  The issue bound next to it: vector instructions of the LDS kernel per pair are not counted by
this script; DESIGN.md 8.18 derives the estimate from the kernel's assembly.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP, REPS, HOST_PAIRS = 3, 30, 4096  # (the 64 x 64 shape: 10 x REPS, its call is tens of microseconds)


def boxes(kind, n, gen):
    import torch

    import box3d_case as C

    if kind == "random":
        return C.random_boxes(n, gen).float()
    lo = torch.randint(-4, 5, (n, 1, 3), generator=gen).double() / 4
    side = torch.randint(2, 9, (n, 1, 3), generator=gen).double() / 4
    return (lo + torch.tensor(C.UNIT_BOX, dtype=torch.float64)[None] * side).float()


def timed(fn, reps):
    import torch

    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), statistics.median(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import pytorch3d_amd as p3d
    from pytorch3d_amd import _C

    if not torch.cuda.is_available():
        sys.exit("box3d_overlap_bench: no GPU (the numbers of this script are device times)")
    d = torch.device("cuda:0")
    lines = ["box3d_overlap on %s, torch %s; WARMUP %d, REPS %d, device events; ms as min / median / max"
             % (torch.cuda.get_device_name(0), torch.__version__, WARMUP, REPS)]
    for kind, n in (("random", 64), ("random", 1000), ("axis_aligned", 1000)):
        gen = torch.Generator().manual_seed(3)
        b1, b2 = boxes(kind, n, gen), boxes(kind, n, gen)
        g1, g2 = b1.to(d), b2.to(d)
        vol, iou, redone = _C.iou_box3d(g1, g2, return_overflow=True)
        rec = {"shape": "%s %d x %d" % (kind, n, n), "overlapping_fraction": round(float((vol > 0).float().mean()), 4),
               "pairs_redone_in_slab_launch": int(redone)}
        for _ in range(WARMUP):
            _C.iou_box3d(g1, g2), p3d.box3d_overlap(g1, g2)
        torch.cuda.synchronize()
        reps = REPS if n >= 1000 else 10 * REPS
        rec["kernel_ms"] = [round(x, 4) for x in timed(lambda: _C.iou_box3d(g1, g2), reps)]
        rec["function_ms"] = [round(x, 4) for x in timed(lambda: p3d.box3d_overlap(g1, g2), reps)]
        rec["kernel_ns_per_pair"] = round(rec["kernel_ms"][1] * 1e6 / (n * n), 2)
        rows = max(1, min(n, HOST_PAIRS // n))
        t = time.perf_counter()
        hv, _ = _C.iou_box3d_host(b1[:rows], b2)
        rec["host_us_per_pair_one_core"] = round((time.perf_counter() - t) * 1e6 / (rows * n), 2)
        rec["host_rows_equal_kernel_bits"] = bool(torch.equal(hv, vol[:rows].cpu()))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if (kind, n) == ("random", 1000):
            _, _, redone = _C.iou_box3d(g1, g2, lds_capacity=16, return_overflow=True)
            low = {"shape": "random 1000 x 1000, LDS capacity 16", "pairs_redone_in_slab_launch": int(redone),
                   "kernel_ms": [round(x, 4) for x in timed(lambda: _C.iou_box3d(g1, g2, lds_capacity=16), 5)]}
            lines.append(json.dumps(low))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
