#!/usr/bin/env python
"""cubify on one MI355X: the public pytorch3d_amd.cubify (csrc/cubify.hip) against the reference's own `pytorch3d.ops.cubify` -- the
torch chain a user runs today -- in the same process on the same inputs (output kept as profiles/cubify_mi355x.txt).

    python profiles/cubify_bench.py [--out FILE]

The reference's function comes from the staged reference package (oracle/_ref/reference_py, or P3D_REFERENCE_ROOT) under plain
pytorch3d_amd.shim.install(), which leaves cubify alone.  Shapes: 64 x 24^3 and 32 x 48^3 (the voxel head's sizes) and 8 x 128^3, each
with a ball-shaped occupancy (a shell of faces) and with 50 % random occupancy (faces everywhere), thresh 0.5, align "topleft".
Per shape and side:
  wall_ms        [min, median, max] over REPS calls, perf_counter around the call and a device synchronise (both sides end in a host
                 read, so wall time is what a caller waits for); the two sides alternate inside the loop
  peak_MB        torch.cuda.max_memory_allocated over one call, above what was allocated before it
  launches       kernels of one call, counted by torch.profiler (device activities); "not measured" where it gives none
and for cubify_packed, the same call without the Meshes object (whose constructor, the reference's own class in this process, checks
and copies per mesh -- most of the launches and of the wall time of a batch of many small meshes on either side): packed_wall_ms and
packed_launches
and for ours
  kernel_ms      the library's own event timing around the count and the emit entry (their 3 + 2 kernels), median over REPS calls
  compulsory_MB  the grid read once (4 N M), the exposure bytes written once and read twice (3 N M), the rank table written and
                 read (8 N L), the outputs (12 V + 24 F); M voxels and L lattice points per mesh
  GBs            compulsory bytes over kernel time, and that as a fraction of PEAK_GBS
Faces must be equal on both sides (torch.equal); the vertex VALUES are compared too and reported: the reference's GPU run divides on
the device, ours gathers the CPU's correctly rounded quotients (the contract of the CPU reference), so a last-bit difference there is
the reference's device arithmetic, not an error here."""
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

PREWARM = 3
PEAK_GBS = 8000.0  # MI355X HBM3E
SHAPES = ((64, 24, 24, 24), (32, 48, 48, 48), (8, 128, 128, 128))


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


def launches(fn):
    import torch

    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or "not measured"
    except Exception as e:  # the profiler is not what this script is about
        return "not measured (%s)" % type(e).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-reference", action="store_true")
    args = ap.parse_args()
    import torch

    import cubify_case as C
    import run_reference_suite as rrs
    import pytorch3d_amd as p3d
    from pytorch3d_amd import _lib

    if not torch.cuda.is_available():
        sys.exit("cubify_bench: no GPU (the numbers of this script are device and wall times on one)")
    d = torch.device("cuda:0")
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    ref_root = next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "ops"))), None)
    reference = None
    if ref_root is not None and not args.skip_reference:
        rrs._stub_missing_packages()
        import pytorch3d_amd.shim as shim

        shim.install(ref_root)
        reference = importlib.import_module("pytorch3d.ops.cubify").cubify
        assert not getattr(reference, "__p3d_amd__", False)
    M = importlib.import_module("pytorch3d_amd.cubify")
    lib = _lib.load()
    lines = ["cubify on %s, torch %s; PREWARM %d; wall ms per call as [min, median, max], each call ended by a device synchronise; "
             "reference: %s" % (torch.cuda.get_device_name(0), torch.__version__, PREWARM,
                                "the staged reference's pytorch3d.ops.cubify under plain shim.install()" if reference else "absent: not measured")]

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for shape in SHAPES:
        N, D, H, W = shape
        for kind in ("ball", "random"):
            voxels = (C.ball(shape) if kind == "ball" else torch.rand(shape, generator=torch.Generator().manual_seed(1))).to(d)
            reps = 31 if N * D * H * W < 4e6 else 9
            ours = lambda: p3d.cubify(voxels, 0.5)  # noqa: E731
            theirs = (lambda: reference(voxels, 0.5)) if reference else None
            assert M.kernel_path(voxels)
            packed = lambda: p3d.cubify_packed(voxels, 0.5)  # noqa: E731
            fns = {"ours": ours, "packed": packed}
            if theirs:
                fns["reference"] = theirs
            rec = {"shape": list(shape), "occupancy": kind, "reps": reps}
            got = p3d.cubify_packed(voxels, 0.5)
            V, F = int(got[2].sum()), int(got[3].sum())
            rec["verts"], rec["faces"] = V, F
            if theirs:
                want = theirs()
                wf, wv = torch.cat(want.faces_list()), torch.cat(want.verts_list())
                rec["faces_equal"] = bool(torch.equal(wf, got[1]))
                rec["verts_equal"] = bool(torch.equal(wv, got[0]))
                rec["verts_max_abs_diff"] = float((wv - got[0]).abs().max()) if wv.shape == got[0].shape else None
                del want, wf, wv
            del got
            times = wall(fns, reps)
            rec["wall_ms"] = times["ours"]
            rec["peak_MB"] = peak_mb(ours)
            rec["launches"] = launches(ours)
            rec["packed_wall_ms"], rec["packed_launches"] = times["packed"], launches(packed)
            if theirs:
                rec["reference_wall_ms"] = times["reference"]
                rec["reference_peak_MB"] = peak_mb(theirs)
                rec["reference_launches"] = launches(theirs)
                rec["speedup_wall_median"] = round(times["reference"][1] / times["ours"][1], 2)
            lib.p3d_profile_enable(1)
            lib.p3d_profile_reset()
            per_call = []
            for _ in range(reps):
                ours()
                snap = _lib.profile_snapshot()
                per_call.append(sum(ms for name, (n, ms) in snap.items() if name.startswith("cubify_")))
                lib.p3d_profile_reset()
            lib.p3d_profile_enable(0)
            rec["kernel_ms"] = round(statistics.median(per_call), 4)
            m, l = D * H * W, (D + 1) * (H + 1) * (W + 1)
            nbytes = 7 * N * m + 8 * N * l + 12 * V + 24 * F
            rec["compulsory_MB"] = round(nbytes / 1e6, 1)
            rec["GBs"] = round(nbytes / (rec["kernel_ms"] * 1e-3) / 1e9, 1)
            rec["fraction_of_hbm_peak"] = round(rec["GBs"] / PEAK_GBS, 4)
            emit(rec)
            del voxels
            torch.cuda.empty_cache()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
