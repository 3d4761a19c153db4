#!/usr/bin/env python
"""mesh_laplacian_smoothing "cot" / "cotcurv" and taubin_smoothing on one MI355X (output kept as
profiles/mesh_laplacian_mi355x.txt).

    python profiles/mesh_laplacian_bench.py [--warmup 5] [--iters 20] [--out FILE]

Two inputs: the config-3 batch (tests/_util.hetero_batch(64, seed=0): 64 meshes) and the single cow (tests/golden/cow_ref.npz).  A step
is what a fitting loop does: new vertices = vertices + offsets, the loss, backward to the offsets.  Legs, ALTERNATING, device events
around each step, `warmup` untimed + `iters` timed iterations per leg, medians with their spread:
    fused          pytorch3d_amd.mesh_laplacian_smoothing(PackedMeshes, method): the autograd node over csrc/mesh_laplacian.hip
    formulation    what the same call ran before the kernels existed: the package's torch formulation on the GPU (about thirty small
                   launches, four index_adds with float atomics) -- mesh_losses._torch_laplacian, unchanged
    uniform        the uniform Laplacian's node, for the ratio
and, where the reference's Python package is on the machine (oracle/_ref/reference_py or P3D_REFERENCE_ROOT), under
shim.install(patch_python=True) on the reference's Meshes:
    reference      pytorch3d.loss.mesh_laplacian_smoothing with its own cot_laplacian (the patch taken out for the leg)
    ref + patch    the same function finding cot_laplacian served by the kernels (what the drop-in gains)
taubin_smoothing, 10 iterations: fused (PackedMeshes) against the reference's own function on its Meshes.
Then the kernels one by one (the library's profile hooks over `iters` steps) beside their compulsory bytes at the copy rate this run
measures (a 256 MB device-to-device copy, read + write counted).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def alternate(legs, warmup, iters):
    import torch

    times = {name: [] for name in legs}
    for i in range(warmup + iters):
        for name, step in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step()
            b.record()
            b.synchronize()
            if i >= warmup:
                times[name].append(a.elapsed_time(b))
    return times


def copy_rate(torch, d):
    """GB/s of a 256 MB device-to-device copy, bytes read + bytes written."""
    src = torch.empty(64 * 2 ** 20, dtype=torch.float32, device=d).normal_()
    dst = torch.empty_like(src)
    t = alternate({"copy": lambda: dst.copy_(src)}, 3, 10)["copy"]
    return 2 * src.numel() * 4 / (statistics.median(t) * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import _util as U
    import pytorch3d_amd as p3d
    from pytorch3d_amd import _lib, mesh_losses

    d = torch.device("cuda:0")
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    ref_root = next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "loss"))), None)
    ref = None
    if ref_root is not None:
        import run_reference_suite as rrs

        rrs._stub_missing_packages()
        import pytorch3d_amd.shim as shim

        shim.install(ref_root, patch_python=True)
        import importlib

        import pytorch3d.ops as ref_ops
        from pytorch3d.structures import Meshes

        loss_module = importlib.import_module("pytorch3d.loss.mesh_laplacian_smoothing")  # (pytorch3d.loss names the function so)
        ref = {"loss": loss_module.mesh_laplacian_smoothing.__wrapped__, "module": loss_module, "cot_patched": ref_ops.cot_laplacian,
               "cot_original": ref_ops.cot_laplacian.__wrapped__, "taubin": ref_ops.taubin_smoothing.__wrapped__, "Meshes": Meshes}
    rate = copy_rate(torch, d)
    lines = [f"{torch.cuda.get_device_name(0)}; {args.warmup} warm-up + {args.iters} timed iterations per leg, legs alternating, device events, "
             f"ms per step: median (min .. max); copy rate {rate:.0f} GB/s (256 MB device-to-device, read + write)"]
    record = {"copy_GBps": rate}

    def row(title, name, t):
        out = {"median": statistics.median(t), "min": min(t), "max": max(t)}
        lines.append(f"  {title:<34s} {name:<12s} {out['median']:9.3f}  ({out['min']:.3f} .. {out['max']:.3f})")
        return out

    def bench(title, verts, faces):
        mesh = p3d.PackedMeshes([x.to(d) for x in verts], [x.to(d) for x in faces])
        V, F = mesh.verts_packed().shape[0], mesh.faces_packed().shape[0]
        topo = mesh_losses.topology_of(mesh)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        mesh_losses.cot_tables_of(mesh.faces_packed(), V, topo)
        b.record()
        b.synchronize()
        E = topo.E
        lines.append(f"{title}: {len(mesh)} meshes, V = {V}, F = {F}, E = {E} (cot_tables, once per topology: {a.elapsed_time(b):.1f} ms)")
        rec = record.setdefault(title, {"V": V, "F": F, "E": E})
        faces_long = mesh.faces_packed().long()
        ref_mesh = ref["Meshes"](verts=[x.to(d) for x in verts], faces=[x.to(d) for x in faces]) if ref else None

        def ours_step(method):
            def step():
                offsets = torch.zeros((V, 3), device=d, requires_grad=True)
                p3d.mesh_laplacian_smoothing(mesh.update_verts_packed(mesh.verts_packed() + offsets), method).backward()
            return step

        def formulation_step(method):
            def step():
                offsets = torch.zeros((V, 3), device=d, requires_grad=True)
                mesh_losses._torch_laplacian(mesh.verts_packed() + offsets, topo, method, faces_long).backward()
            return step

        def reference_step(method, cot):
            def step():
                ref["module"].cot_laplacian = cot
                try:
                    offsets = torch.zeros((V, 3), device=d, requires_grad=True)
                    ref["loss"](ref_mesh.offset_verts(offsets), method).backward()
                finally:
                    ref["module"].cot_laplacian = ref["cot_patched"]
            return step

        for method in ("cot", "cotcurv"):
            legs = {"fused": ours_step(method), "formulation": formulation_step(method), "uniform": ours_step("uniform")}
            if ref:
                legs["reference"] = reference_step(method, ref["cot_original"])
                legs["ref + patch"] = reference_step(method, ref["cot_patched"])
            times = alternate(legs, args.warmup, args.iters)
            out = {name: row(f"mesh_laplacian_smoothing ({method})", name, t) for name, t in times.items()}
            lines.append(f"  {'':<34s} formulation / fused {out['formulation']['median'] / out['fused']['median']:.2f} x; fused / uniform "
                         f"{out['fused']['median'] / out['uniform']['median']:.2f} x"
                         + (f"; reference / fused {out['reference']['median'] / out['fused']['median']:.2f} x; reference / (ref + patch) "
                            f"{out['reference']['median'] / out['ref + patch']['median']:.2f} x" if ref else ""))
            rec[method] = out
        legs = {"fused": lambda: p3d.taubin_smoothing(mesh, 0.53, -0.53, 10)}
        if ref:
            legs["reference"] = lambda: ref["taubin"](ref_mesh, 0.53, -0.53, 10)
        with torch.no_grad():
            times = alternate(legs, args.warmup, args.iters)
        out = {name: row("taubin_smoothing (10 iterations)", name, t) for name, t in times.items()}
        if ref:
            lines.append(f"  {'':<34s} reference / fused {out['reference']['median'] / out['fused']['median']:.2f} x")
        rec["taubin"] = out
        # the kernels one by one
        nbytes = {"mesh_cot_weights": 12 * V + 24 * F + 16 * F + 4 * E + 12 * F + 12 * F + 4 * E,
                  "mesh_cot_laplacian_forward (cot)": 12 * V + 4 * V + 8 * E + 8 * E + 4 * E + 4 * V + 20 * V,
                  "mesh_cot_laplacian_forward (cotcurv)": 12 * V + 4 * V + 8 * E + 8 * E + 4 * E + 4 * V + 20 * V + 4 * V + 12 * F + 4 * F,
                  "mesh_cot_laplacian_backward": 20 * V + 4 * E + 4 * V + 8 * E + 8 * E + 12 * V,
                  "mesh_taubin_smoothing (20 half-steps)": 20 * (12 * V + 4 * V + 8 * E + 12 * V)}
        lib = _lib.load()
        for method in ("cot", "cotcurv"):
            lib.p3d_profile_reset()
            lib.p3d_profile_enable(1)
            try:
                step = ours_step(method)
                for _ in range(args.iters):
                    step()
                if method == "cot":
                    for _ in range(args.iters):
                        p3d.taubin_smoothing(mesh, 0.53, -0.53, 10)
                ran = _lib.profile_snapshot()
            finally:
                lib.p3d_profile_enable(0)
            for name, (n, ms) in sorted(ran.items()):
                key = next((k for k in (name, f"{name} ({method})", f"{name} (20 half-steps)") if k in nbytes), None)
                if key is None or (method == "cotcurv" and key in ("mesh_cot_weights", "mesh_cot_laplacian_backward")):
                    continue
                floor = nbytes[key] / (rate * 1e9) * 1e3
                lines.append(f"  kernel {key:<40s} {ms / n:8.4f} ms per call; compulsory {nbytes[key] / 1e6:7.2f} MB = {floor:.4f} ms at the copy rate")
                rec.setdefault("kernels", {})[key] = {"ms": ms / n, "bytes": nbytes[key], "floor_ms": floor}

    bench("config-3 batch", *U.hetero_batch(64, seed=0))
    g = np.load(os.path.join(U.GOLDEN, "cow_ref.npz"))
    bench("single cow", [torch.from_numpy(g["verts_ndc"]).float()], [torch.from_numpy(g["faces"]).long()])
    lines.append(f"calls: {mesh_losses.CALLS}")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(record))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
