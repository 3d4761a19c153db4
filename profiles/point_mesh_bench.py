#!/usr/bin/env python
"""point_mesh_face_distance / point_mesh_edge_distance on one MI355X: the kernels of csrc/point_mesh.hip against this package's own
torch formulation on the same GPU (output kept as profiles/point_mesh_mi355x.txt).

    python profiles/point_mesh_bench.py [--out FILE]            the driver: every step below in a child process of its own
    python profiles/point_mesh_bench.py --step NAME              one step, in this process

The driver runs each step under its own time limit and stops at the first one that fails or runs out of time; it reads nothing
outside the repository.  The baseline is the torch formulation of pytorch3d_amd/point_mesh.py (forced by switching
point_mesh.kernel_path off for that leg): the reference's device kernels for these operators are not among the binaries this
repository builds for checking, so no figure is given for them.  Shapes: one cow (tests/golden/cow_ref.npz: 5856 faces) against
10 000 points, 8 x ico_sphere(4) against 5000 points each, and the 64 meshes of the bench batch (tests/_util.py: hetero_batch)
against 5000 points each; the points lie near the surfaces.  Forward + backward to vertices and points of BOTH losses.  Device events
around each step, 2 warm-up iterations untimed, the legs alternating, medians.  The per-kernel times come from the library's built-in
timing (p3d_profile_*) in separate, untimed iterations.  On the single mesh a leg with the split over waves forced to 1 shows what
the split is worth.

The forwards against the VALU issue bound: VALU_PER_PAIR vector instructions per pair per wave (counted in the disassembly of the
inner loops), one wave-instruction issues in 4 cycles on one of 4 x 256 SIMDs at CLOCK_GHZ.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# vector instructions of the innermost loop (four pairs per trip) / 4, from the gfx950 assembly of pm_forward_kernel<query, target>:
# 758, 742, 190 and 186 per trip; five IEEE divisions per triangle pair and one per segment pair are ~11 of them each
VALU_PER_PAIR = {"point_face_forward": 190, "face_point_forward": 186, "point_edge_forward": 48, "edge_point_forward": 47}
SIMDS = 4 * 256
CLOCK_GHZ = 2.4

# name: (time limit of the step in seconds, timed iterations of the torch formulation)
STEPS = {"cow_1": (180, 5), "ico4_8": (240, 3), "batch_64": (360, 1)}


def meshes_of(name):
    import numpy as np
    import torch

    import _util as U

    if name == "cow_1":
        with np.load(os.path.join(ROOT, "tests", "golden", "cow_ref.npz")) as z:
            return [torch.from_numpy(z["verts_world"]).float()], [torch.from_numpy(z["faces"]).long()], 10000
    if name == "ico4_8":
        v, f = U.ico_sphere(4)
        return [v.float() * (1.0 + 0.05 * i) for i in range(8)], [f.long()] * 8, 5000
    verts, faces = U.hetero_batch(64, seed=0, torus_div=1.0)
    return [v.float() for v in verts], [f.long() for f in faces], 5000


def alternate(legs, warmup, iters):
    """legs: {name: (step, timed iterations or None for `iters`)}; {name: [ms, ...]}, the legs taking turns."""
    import torch

    times = {name: [] for name in legs}
    for i in range(warmup + iters):
        for name, (step, own) in legs.items():
            if own is not None and i >= min(warmup, 1) + own:
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step()
            b.record()
            b.synchronize()
            if i >= (warmup if own is None else min(warmup, 1)):
                times[name].append(a.elapsed_time(b))
    return times


def run_step(name):
    import torch

    import pytorch3d_amd as p3d
    from pytorch3d_amd import _lib
    from pytorch3d_amd import point_mesh as pm

    _, base_iters = STEPS[name]
    d = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    verts0, faces0, P = meshes_of(name)
    points0 = []
    for v in verts0:  # near the surface: vertices drawn with replacement, moved by 5 % of the mesh's size
        pick = torch.randint(0, v.shape[0], (P,), generator=gen)
        points0.append((v[pick] + 0.05 * float(v.abs().max()) * torch.randn(P, 3, generator=gen)).to(d))
    verts0, faces0 = [v.to(d) for v in verts0], [f.to(d) for f in faces0]
    kernel_path = pm.kernel_path
    template = p3d.PackedMeshes(verts0, faces0)
    p3d.point_mesh_edge_distance(template, p3d.PackedPointclouds(points0))  # builds the topology's tables once (host syncs)
    from pytorch3d_amd import mesh_losses

    pairs = {"face": sum(P * f.shape[0] for f in faces0), "edge": P * int(mesh_losses.topology_of(template).num_edges.sum())}

    def step_of(fused, ordered=False, split=0):
        def step():
            pm.kernel_path = kernel_path if fused else (lambda *a: False)
            pm.SPLIT = split
            torch.use_deterministic_algorithms(ordered)
            try:
                vp = template.verts_packed().detach().clone().requires_grad_(True)
                meshes = template.update_verts_packed(vp)
                pts = [p.clone().requires_grad_(True) for p in points0]
                pcls = p3d.PackedPointclouds(pts)
                loss = p3d.point_mesh_face_distance(meshes, pcls) + p3d.point_mesh_edge_distance(meshes, pcls)
                loss.backward()
            finally:
                pm.kernel_path, pm.SPLIT = kernel_path, 0
                torch.use_deterministic_algorithms(False)
        return step

    legs = {"kernels (atomic scatter)": (step_of(True), None), "kernels (ordered scatter)": (step_of(True, True), None)}
    if len(verts0) == 1:
        legs["kernels, split forced to 1"] = (step_of(True, split=1), None)
    legs["torch formulation"] = (step_of(False), base_iters)
    times = alternate(legs, 2, 20)
    out = {"step": name, "N": len(verts0), "P": P, "faces": [int(f.shape[0]) for f in faces0], "pairs_face": pairs["face"], "pairs_edge": pairs["edge"],
           "legs": {k: {"median": statistics.median(t), "min": min(t), "max": max(t), "iters": len(t)} for k, t in times.items()}}
    lib = _lib.load()
    variants = [("atomic", False, 0), ("ordered", True, 0)] + ([("split1", False, 1)] if len(verts0) == 1 else [])
    for label, ordered, split in variants:
        lib.p3d_profile_reset()
        lib.p3d_profile_enable(1)
        try:
            for _ in range(5):
                step_of(True, ordered, split)()
            torch.cuda.synchronize()
            snap = _lib.profile_snapshot()
        finally:
            lib.p3d_profile_enable(0)
        out["kernels_" + label] = {k: [n, ms / n] for k, (n, ms) in sorted(snap.items())}
    print(json.dumps(out))


def report(rec):
    faces = rec["faces"]
    lines = [f"{rec['step']}: {rec['N']} meshes ({min(faces)} .. {max(faces)} faces, {sum(faces)} in all) x {rec['P']} points each, both losses, "
             "forward + backward, ms per step: median (min .. max) [timed iterations]"]
    for leg, t in rec["legs"].items():
        lines.append(f"  {leg:<28s} {t['median']:10.3f}  ({t['min']:.3f} .. {t['max']:.3f}) [{t['iters']}]")
    base = rec["legs"]["torch formulation"]["median"]
    lines.append(f"  {'torch / kernels (atomic)':<28s} {base / rec['legs']['kernels (atomic scatter)']['median']:10.1f} x")
    for label in ("atomic", "ordered", "split1"):
        if "kernels_" + label not in rec:
            continue
        lines.append(f"  per launch, {label} (ms, mean of the launches of 5 steps):")
        for k, (n, ms) in rec["kernels_" + label].items():
            lines.append(f"    {k:<36s} {ms:9.4f}  x{n // 5} per step")
    for k in VALU_PER_PAIR:
        ms = rec["kernels_atomic"].get(k, [0, None])[1]
        if ms:
            bound = rec["pairs_face" if "face" in k else "pairs_edge"] / 64 * VALU_PER_PAIR[k] * 4 / (SIMDS * CLOCK_GHZ * 1e9) * 1e3
            lines.append(f"  {k}: {ms:.4f} ms per launch; the 4-cycle VALU issue bound of its loop ({VALU_PER_PAIR[k]} instructions per pair, "
                         f"{SIMDS} SIMDs, {CLOCK_GHZ} GHz) is {bound:.4f} ms: the launch takes {ms / bound:.2f} of it")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=sorted(STEPS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        run_step(args.step)
        return
    lines = ["point_mesh_face_distance + point_mesh_edge_distance: csrc/point_mesh.hip against the package's torch formulation on the same GPU"]
    for name, (limit, _) in STEPS.items():
        print("step", name, "...", flush=True)
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append(f"{name}: no result within {limit} s; stopped here")
            break
        if res.returncode != 0:
            lines.append(f"{name}: exit status {res.returncode}; stopped here\n{res.stderr[-2000:]}")
            break
        lines += report(json.loads(res.stdout.strip().splitlines()[-1]))
        keep(lines, args.out)
    keep(lines, args.out)


def keep(lines, out):
    """Print what there is so far and (re)write the output file: a step that runs out of time later loses nothing."""
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)) or ".", exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
