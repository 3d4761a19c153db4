#!/usr/bin/env python
"""Marching cubes on one MI355X: pytorch3d_amd.marching_cubes and marching_cubes_packed (csrc/marching_cubes.hip) and, as the baseline,
marching_cubes_torch -- the same device contract as a vectorised torch formulation on the same GPU, what a user would otherwise write;
it is NOT the kernels under test and not the reference's CUDA path, which this machine cannot run (output kept as
profiles/marching_cubes_mi355x.txt).

    python profiles/marching_cubes_bench.py [--out FILE]

Forward only.  Shapes: a sphere's signed distance at 1 x 128^3, 8 x 128^3 and 1 x 256^3, and at 64 x 32^3; 50 % noise (randn at
isolevel 0: nearly every cube emits) at 8 x 128^3.  Per shape:
  wall_ms          [min, median, max] over REPS calls of the public function, perf_counter around the call and a device synchronise
                   (the call's host read of the counts is inside); packed_wall_ms: marching_cubes_packed; torch_wall_ms: the baseline;
                   the three alternate inside the loop
  peak_MB          torch.cuda.max_memory_allocated over one call above what was allocated before it; torch_peak_MB likewise
  verts, faces     what comes out; equal: the kernels' packed result against the baseline's, torch.equal on all four tensors
  count_ms, emit_ms  the library's own event timing around the two entries (classify + carry; vertices + faces), median over REPS
  count_MB, emit_MB  the bytes each entry cannot avoid: count reads the grid and writes a word per lattice point (8 N L); emit reads
                   the words twice and writes 20 V + 24 F (8 N L + 20 V + 24 F; its gathers of neighbouring words and of the grid at
                   the vertices are not counted)
  count_x, emit_x  entry time over the time of those bytes at COPY_GBS, the rate of a 1 GiB device-to-device copy measured first
                   (read + write bytes over event time)"""
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
CASES = (("sphere", (1, 128, 128, 128)), ("sphere", (8, 128, 128, 128)), ("sphere", (1, 256, 256, 256)), ("sphere", (64, 32, 32, 32)),
         ("noise", (8, 128, 128, 128)))


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


def peak_mb(fn):
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return round(peak / 1e6, 1)


def copy_rate():
    """GB/s of a 1 GiB device-to-device copy, read + write bytes over the median event time of 9 copies."""
    import torch

    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    ms = []
    for _ in range(9):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return 2 * src.numel() * 4 / (statistics.median(ms) * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import marching_cubes_case as C
    import pytorch3d_amd as p3d
    from pytorch3d_amd import _lib

    if not torch.cuda.is_available():
        sys.exit("marching_cubes_bench: no GPU (the numbers of this script are device and wall times on one)")
    d = torch.device("cuda:0")
    M = importlib.import_module("pytorch3d_amd.marching_cubes")
    lib = _lib.load()
    rate = copy_rate()
    lines = ["marching cubes on %s, torch %s; PREWARM %d, REPS %d; wall ms per call as [min, median, max], each call ended by a device "
             "synchronise; COPY_GBS %.0f (1 GiB device-to-device copy, read + write)" % (torch.cuda.get_device_name(0), torch.__version__,
                                                                                         PREWARM, REPS, rate)]

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for kind, shape in CASES:
        N, D, H, W = shape
        if kind == "sphere":
            vol = C.sphere(D).to(d).expand(N, D, H, W).contiguous()
        else:
            vol = torch.randn(shape, generator=torch.Generator().manual_seed(1)).to(d)
        assert M.kernel_path(vol)
        ours = lambda: p3d.marching_cubes(vol, 0.0)  # noqa: E731
        packed = lambda: p3d.marching_cubes_packed(vol, 0.0)  # noqa: E731
        baseline = lambda: p3d.marching_cubes_torch(vol, 0.0)  # noqa: E731
        got, want = packed(), baseline()
        V, F = int(got[2].sum()), int(got[3].sum())
        rec = {"field": kind, "shape": list(shape), "verts": V, "faces": F, "equal": all(bool(torch.equal(a, b)) for a, b in zip(got, want))}
        del got, want
        times = wall({"ours": ours, "packed": packed, "torch": baseline}, REPS)
        rec["wall_ms"], rec["packed_wall_ms"], rec["torch_wall_ms"] = times["ours"], times["packed"], times["torch"]
        rec["torch_over_packed"] = round(times["torch"][1] / times["packed"][1], 2)
        rec["peak_MB"], rec["torch_peak_MB"] = peak_mb(packed), peak_mb(baseline)
        lib.p3d_profile_enable(1)
        lib.p3d_profile_reset()
        count_ms, emit_ms = [], []
        for _ in range(REPS):
            packed()
            snap = _lib.profile_snapshot()
            count_ms.append(snap["marching_cubes_count"][1])
            emit_ms.append(snap["marching_cubes_emit"][1])
            lib.p3d_profile_reset()
        lib.p3d_profile_enable(0)
        L = N * D * H * W
        rec["count_ms"], rec["emit_ms"] = round(statistics.median(count_ms), 4), round(statistics.median(emit_ms), 4)
        rec["count_MB"], rec["emit_MB"] = round(8 * L / 1e6, 1), round((8 * L + 20 * V + 24 * F) / 1e6, 1)
        rec["count_x"] = round(rec["count_ms"] * 1e-3 / (8 * L / (rate * 1e9)), 2)
        rec["emit_x"] = round(rec["emit_ms"] * 1e-3 / ((8 * L + 20 * V + 24 * F) / (rate * 1e9)), 2)
        emit(rec)
        del vol
        torch.cuda.empty_cache()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
