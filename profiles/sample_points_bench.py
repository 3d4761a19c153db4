#!/usr/bin/env python
"""sample_points_from_meshes on one MI355X: the kernels of csrc/sample_points.hip against the reference's own torch chain on the same GPU
(output kept as profiles/sample_points_mi355x.txt).

    python profiles/sample_points_bench.py [--warmup 5] [--iters 30] [--out FILE]

Needs the reference's Python package (oracle/_ref/reference_py, staged by __graft_entry__.build(), or P3D_REFERENCE_ROOT).  One
process, shim.install(patch_python=True); the reference legs call the functions the patch replaced (their __wrapped__ originals).
What the reference sampler itself looks up -- mesh_face_areas_normals, packed_to_padded, both ending in `_C` operators, and the
Meshes accessors -- is not touched by patch_python (checked at start-up), so its leg is the chain that runs under plain
shim.install().  Shared by BOTH legs of "sample + chamfer": the mesh comes from the patched offset_verts, and chamfer_distance is this
package's.  Two inputs: the config-3 batch (tests/_util.hetero_batch(64, seed=0): 64 meshes) and the single cow
(tests/golden/cow_ref.npz), 10 000 samples per mesh.

  sample + chamfer   forward + backward of sample_points_from_meshes(mesh, 10000, return_normals=True) followed by chamfer_distance
                     to a fixed target cloud WITH normals (so that both outputs carry a gradient).  chamfer_distance is this package's
                     in both legs (the reference's ends in _C.knn_points_idx, which the shim does not serve): only the sampler differs.
  fitting step       what the reference's mesh-fitting tutorial does each step: offset_verts, sample 10 000 points, chamfer_distance
                     with normals off, mesh_edge_loss + mesh_normal_consistency + mesh_laplacian_smoothing, backward.  "patched": every
                     piece as shim.install(patch_python=True) binds it; "unpatched": the reference's offset_verts, sampler and three
                     regularisers (chamfer_distance again this package's, for the reason above).

Device events around each step, warm-up iterations untimed (they also bring the clocks up), the legs alternating, medians.  The
per-kernel times come from the library's built-in timing (p3d_profile_*) in separate, untimed iterations.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

S = 10000
REGULARISERS = ("mesh_edge_loss", "mesh_normal_consistency", "mesh_laplacian_smoothing")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
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
    import pytorch3d_amd as p3d
    import pytorch3d_amd.shim as shim
    from pytorch3d_amd import _lib

    shim.install(ref_root, patch_python=True)
    import pytorch3d.loss as loss_mod
    import pytorch3d.ops as ops_mod
    from pytorch3d.structures import Meshes

    d = torch.device("cuda:0")
    fused_sample = ops_mod.sample_points_from_meshes
    ref_sample = fused_sample.__wrapped__
    fused_reg = {n: getattr(loss_mod, n) for n in REGULARISERS}
    ref_reg = {n: fused_reg[n].__wrapped__ for n in REGULARISERS}
    import pytorch3d.ops.sample_points_from_meshes  # noqa: F401 -- the module, for the names the reference sampler looks up

    ref_module = sys.modules["pytorch3d.ops.sample_points_from_meshes"]
    for callee in ("mesh_face_areas_normals", "packed_to_padded"):
        assert not getattr(getattr(ref_module, callee), "__p3d_amd__", False), callee + " is patched: the reference leg is not the plain chain"
    ref_offset = next(orig for owner, attr, orig, _ in shim._PATCHED if owner is Meshes and attr == "offset_verts")
    lines = [f"{torch.cuda.get_device_name(0)}; {S} samples per mesh; {args.warmup} warm-up + {args.iters} timed iterations per leg, legs "
             "alternating, device events, ms per step: median (min .. max)"]
    record = {}

    def bench(title, verts, faces):
        mesh = Meshes(verts=[x.to(d) for x in verts], faces=[x.to(d) for x in faces])
        N, V, F = len(mesh), mesh.verts_packed().shape[0], mesh.faces_packed().shape[0]
        with torch.no_grad():  # a fixed target: points and normals of the same surfaces, moved a little
            target, target_normals = fused_sample(mesh, S, return_normals=True, generator=torch.Generator(device=d).manual_seed(0))
            target = target + 0.02
        for fn in fused_reg.values():  # the tables of the regularisers: once per topology, outside the timed steps
            fn(mesh)
        lines.append(f"{title}: {N} meshes, V = {V}, F = {F}")
        record[title] = {"N": N, "V": V, "F": F}

        def sample_chamfer(sample):
            def step():
                offsets = torch.zeros((V, 3), device=d, requires_grad=True)
                moved = mesh.offset_verts(offsets)
                points, normals = sample(moved, S, return_normals=True)
                loss, loss_normals = p3d.chamfer_distance(points, target, x_normals=normals, y_normals=target_normals)
                (loss + 0.1 * loss_normals).backward()
            return step

        def fitting(sample, reg, offset):
            def step():
                offsets = torch.zeros((V, 3), device=d, requires_grad=True)
                moved = offset(mesh, offsets)
                loss, _ = p3d.chamfer_distance(sample(moved, S), target)
                loss = loss + reg["mesh_edge_loss"](moved) + 0.01 * reg["mesh_normal_consistency"](moved)
                loss = loss + 0.1 * reg["mesh_laplacian_smoothing"](moved, method="uniform")
                loss.backward()
            return step

        rows = (("sample + chamfer (normals), fwd + bwd", {"reference": sample_chamfer(ref_sample), "kernels": sample_chamfer(fused_sample)}),
                ("fitting step", {"unpatched": fitting(ref_sample, ref_reg, ref_offset),
                                  "patched": fitting(fused_sample, fused_reg, Meshes.offset_verts)}))
        for row, legs in rows:
            times = alternate(legs, args.warmup, args.iters)
            out = {}
            for name, t in times.items():
                out[name] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
                lines.append(f"  {row:<40s} {name:<10s} {out[name]['median']:9.3f}  ({out[name]['min']:.3f} .. {out[name]['max']:.3f})")
            base, ours = list(out)
            lines.append(f"  {'':<40s} {base + ' / ' + ours:<22s} {out[base]['median'] / out[ours]['median']:9.2f} x")
            record[title][row] = out
        lib = _lib.load()
        lib.p3d_profile_reset()
        lib.p3d_profile_enable(1)
        try:
            for _ in range(5):
                sample_chamfer(fused_sample)()
            torch.cuda.synchronize()
            snap = _lib.profile_snapshot()
        finally:
            lib.p3d_profile_enable(0)
            lib.p3d_profile_reset()
        lines.append("  per launch in sample + chamfer, kernels leg (ms, mean of the launches of 5 steps):")
        for k, (n, ms) in sorted(snap.items()):
            lines.append(f"    {k:<40s} {ms / n:9.4f}  x{n / 5:g} per step")
        record[title]["launches"] = {k: [n, ms / n] for k, (n, ms) in snap.items()}

    bench("config-3 batch", *U.hetero_batch(64, seed=0))
    g = np.load(os.path.join(U.GOLDEN, "cow_ref.npz"))
    bench("single cow", [torch.from_numpy(g["verts_ndc"]).float()], [torch.from_numpy(g["faces"]).long()])
    lines.append(f"patch calls [fused, fallback]: {{'sample_points_from_meshes': {shim.PATCH_CALLS.get('sample_points_from_meshes')}}}")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(record))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
