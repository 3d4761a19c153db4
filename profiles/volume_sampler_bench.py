#!/usr/bin/env python
"""The VolumeSampler on one MI355X: csrc/volume_sample.hip against what ran before it (output kept as
profiles/volume_sampler_mi355x.txt).

    python profiles/volume_sampler_bench.py [--out FILE] [--shapes NAME,NAME]

Everything is timed through the UNMODIFIED reference's VolumeRenderer(NDCMultinomialRaysampler, EmissionAbsorptionRaymarcher) under
shim.install(patch_python=True), forward alone and forward + backward (loss = images.sum(), gradients to densities and features):
  fused      VolumeSampler.forward patched (pytorch3d_amd.volume_sampler: one node over the kernels, atomic backward)
  reference  the same call with VolumeSampler.forward restored to the reference's own (two grid_sample calls over materialised ray
             points): what ran before.  The raysampler and the (fused) raymarcher are the same on both sides.
  ordered    fused under torch.use_deterministic_algorithms(True): keys, stable sort, segmented sum (the reference raises there)
The sides of a shape ALTERNATE call by call in one process; every shape is warmed; device events around each call; min / median of
REPS.  peak_mb: torch.cuda.max_memory_allocated over one forward + backward of a side, above what was allocated before it.
kernel_ms: the library's own per-kernel events (p3d_profile_enable) in a separate pass -- the kernels alone.  floor_ms: the bytes the
forward must move -- both outputs, the lengths, and the volumes once -- at the 6.29 TB/s measured copy rate.
Shapes: the volume-fitting tutorial's (one 128^3 grid, Cd = 1, Cf = 3, shared by 10 cameras through expand, 128 x 128 rays x 150
points), the same with 10 separate grids, a shared 64^3 grid, and 64 x 64 = 4096 rays x 64 points per camera.
Not built, so not measured: merging the atomics of one destination inside the wave before they leave.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP, REPS, COPY_RATE = 3, 12, 6.29e12
# name: (grid side, separate grids, image side, points per ray, cameras)
SHAPES = {"tutorial-128-shared": (128, False, 128, 150, 10), "separate-128": (128, True, 128, 150, 10), "grid-64-shared": (64, False, 128, 150, 10),
          "rays-4096x64": (128, False, 64, 64, 10)}


def alternate(sides, reps):
    import torch

    ms = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: [round(min(v), 3), round(statistics.median(v), 3)] for k, v in ms.items()}


def kernel_ms(fn, reps=5):
    import torch

    from pytorch3d_amd import _lib

    lib = _lib.load()
    lib.p3d_profile_reset()
    lib.p3d_profile_enable(1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    snap = _lib.profile_snapshot()
    lib.p3d_profile_enable(0)
    return {k: round(total / max(n, 1), 4) for k, (n, total) in snap.items() if k.startswith("volume_sample")}


def peak_mb(fn):
    import torch

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    import torch

    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    shim.install(next(c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d"))), patch_python=True)
    from pytorch3d.renderer import FoVPerspectiveCameras, NDCMultinomialRaysampler, VolumeRenderer, look_at_view_transform
    from pytorch3d.renderer.implicit import raymarching
    from pytorch3d.renderer.implicit import renderer as ref_renderer
    from pytorch3d.structures import Volumes

    d = torch.device("cuda:0")
    vs_cls = ref_renderer.VolumeSampler
    patched = vs_cls.forward
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "warmup": WARMUP, "reps": REPS})]
    print(lines[0], flush=True)
    for name in args.shapes.split(","):
        S, separate, side, P, cams = SHAPES[name]
        gen = torch.Generator().manual_seed(5)
        nv = cams if separate else 1
        dens = (0.1 * torch.rand((nv, 1, S, S, S), generator=gen)).to(d).requires_grad_(True)
        feats = torch.rand((nv, 3, S, S, S), generator=gen).to(d).requires_grad_(True)
        R, T = look_at_view_transform(dist=2.7, elev=torch.linspace(0, 60, cams), azim=torch.linspace(-180, 180, cams))
        cameras = FoVPerspectiveCameras(R=R, T=T, device=d)
        renderer = VolumeRenderer(raysampler=NDCMultinomialRaysampler(image_width=side, image_height=side, n_pts_per_ray=P, min_depth=0.1, max_depth=3.0),
                                  raymarcher=raymarching.EmissionAbsorptionRaymarcher())

        def volumes():
            if separate:
                return Volumes(densities=dens, features=feats, voxel_size=3.0 / S)
            return Volumes(densities=dens.expand(cams, -1, -1, -1, -1), features=feats.expand(cams, -1, -1, -1, -1), voxel_size=3.0 / S)

        def forward(reference=False):
            vs_cls.forward = patched.__wrapped__ if reference else patched
            try:
                return renderer(cameras=cameras, volumes=volumes())[0]
            finally:
                vs_cls.forward = patched

        def step(reference=False):
            return torch.autograd.grad(forward(reference).sum(), (dens, feats))

        def ordered_step():
            torch.use_deterministic_algorithms(True)
            try:
                return step()
            finally:
                torch.use_deterministic_algorithms(False)

        def fwd_only(reference=False):
            with torch.no_grad():
                return forward(reference)

        for _ in range(WARMUP):
            step(), step(True), fwd_only(), fwd_only(True)
        ordered_step()
        a, b = step(), step(True)
        agree = [round(float((x - y).abs().max() / y.abs().max()), 9) for x, y in zip(a, b)]
        del a, b
        rec = {"shape": name, "grid": S, "grids": nv, "cameras": cams, "rays": side * side, "points": P,
               "forward_ms": alternate({"fused": fwd_only, "reference": lambda: fwd_only(True)}, REPS),
               "step_ms": alternate({"fused": step, "reference": lambda: step(True), "ordered": ordered_step}, REPS),
               "peak_mb": {"fused": peak_mb(step), "reference": peak_mb(lambda: step(True)), "ordered": peak_mb(ordered_step)},
               "kernel_ms": {"atomic": kernel_ms(step), "ordered": kernel_ms(ordered_step)},
               "floor_ms": round((cams * side * side * P * (1 + 3 + 1) + nv * 4 * S ** 3) * 4 / COPY_RATE * 1e3, 4),
               "grad_rel_difference_fused_vs_reference": agree, "patch_calls": list(shim.PATCH_CALLS.get("VolumeSampler.forward", [0, 0]))}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del dens, feats, renderer
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
