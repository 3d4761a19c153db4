#!/usr/bin/env python
"""The three mesh regularisers on one MI355X: the reference's own functions against the patched ones (output kept as
profiles/mesh_losses_mi355x.txt).

    python profiles/mesh_losses_bench.py [--warmup 5] [--iters 20] [--out FILE]

Needs the reference's Python package (oracle/_ref/reference_py, staged by __graft_entry__.build(), or P3D_REFERENCE_ROOT).  Two
inputs: the config-3 batch (tests/_util.hetero_batch(64, seed=0): 64 meshes) and the single cow (tests/golden/cow_ref.npz).  One
process, shim.install(patch_python=True); a step is what a fitting loop does: mesh.offset_verts(offsets) (the patched, lean one on
both sides, so the reference's caches of edges_packed / laplacian_packed and this package's tables are both inherited from the mesh
built once outside the loop), the loss, backward to the offsets.  Baseline: the reference's functions (the `__wrapped__` originals of
the three patches); its mesh_normal_consistency calls `_C.mesh_normal_consistency_find_verts`, which the shim serves on the host --
before that operator existed the baseline of that row raised NotImplementedError, so there is no earlier number to compare with.
Device events around each step, `warmup` untimed + `iters` timed iterations per leg, the two sides ALTERNATING, medians.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("mesh_edge_loss", "mesh_laplacian_smoothing", "mesh_normal_consistency")


def alternate(legs, warmup, iters):
    """legs: {name: step}; returns {name: [ms, ...]} of `iters` timed iterations each, the legs taking turns."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    ref_root = next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "loss"))), None)
    if ref_root is None:
        sys.exit("the reference's Python package is not on this machine (oracle/_ref/reference_py or P3D_REFERENCE_ROOT)")
    import numpy as np
    import torch

    import _util as U
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim
    from pytorch3d_amd import mesh_losses as ours

    shim.install(ref_root, patch_python=True)
    import pytorch3d.loss as loss_mod
    from pytorch3d.structures import Meshes

    d = torch.device("cuda:0")
    fused = {n: getattr(loss_mod, n) for n in NAMES}
    reference = {n: fused[n].__wrapped__ for n in NAMES}
    lines = [f"{torch.cuda.get_device_name(0)}; {args.warmup} warm-up + {args.iters} timed iterations per leg, legs alternating, device events, "
             "ms per offset_verts + loss + backward: median (min .. max)"]
    record = {}

    def bench(title, verts, faces):
        mesh = Meshes(verts=[x.to(d) for x in verts], faces=[x.to(d) for x in faces])
        V = mesh.verts_packed().shape[0]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        topo = ours.topology_of(mesh)
        b.record()
        b.synchronize()
        lines.append(f"{title}: {len(mesh)} meshes, V = {V}, F = {mesh.faces_packed().shape[0]}, E = {topo.E}, P = {topo.P} "
                     f"(mesh_loss_topology, once per topology: {a.elapsed_time(b):.1f} ms)")
        record[title] = {"V": V, "F": int(mesh.faces_packed().shape[0]), "E": topo.E, "P": topo.P}

        def step_of(fns, which):
            def step():
                offsets = torch.zeros((V, 3), device=d, requires_grad=True)
                moved = mesh.offset_verts(offsets)
                loss = 0.0
                if "mesh_edge_loss" in which:
                    loss = loss + fns["mesh_edge_loss"](moved)
                if "mesh_laplacian_smoothing" in which:
                    loss = loss + fns["mesh_laplacian_smoothing"](moved, method="uniform")
                if "mesh_normal_consistency" in which:
                    loss = loss + 0.01 * fns["mesh_normal_consistency"](moved)
                loss.backward()
            return step

        for row, which in (("mesh_edge_loss", NAMES[:1]), ("mesh_laplacian_smoothing (uniform)", NAMES[1:2]), ("mesh_normal_consistency", NAMES[2:]),
                           ("the three together", NAMES)):
            times = alternate({"reference": step_of(reference, which), "fused": step_of(fused, which)}, args.warmup, args.iters)
            out = {}
            for name, t in times.items():
                out[name] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
                lines.append(f"  {row:<36s} {name:<10s} {out[name]['median']:9.3f}  ({out[name]['min']:.3f} .. {out[name]['max']:.3f})")
            lines.append(f"  {'':<36s} {'ref/fused':<10s} {out['reference']['median'] / out['fused']['median']:9.2f} x")
            record[title][row] = out

    bench("config-3 batch", *U.hetero_batch(64, seed=0))
    g = np.load(os.path.join(U.GOLDEN, "cow_ref.npz"))
    bench("single cow", [torch.from_numpy(g["verts_ndc"]).float()], [torch.from_numpy(g["faces"]).long()])
    calls = {n: shim.PATCH_CALLS.get(n) for n in NAMES}
    lines.append(f"patch calls [fused, fallback]: {calls}")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(record))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
