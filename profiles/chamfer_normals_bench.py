#!/usr/bin/env python
"""chamfer_distance with normals on one MI355X: the single node of csrc/chamfer_normals.hip against the general form of
pytorch3d_amd/chamfer.py on the same GPU (output kept as profiles/chamfer_normals_mi355x.txt).

    python profiles/chamfer_normals_bench.py [--out FILE]            the driver: every step below in a child process of its own
    python profiles/chamfer_normals_bench.py --step NAME              one step, in this process

The driver runs each step under its own time limit and stops at the first one that fails or runs out of time; it reads nothing
outside the repository.  The baseline is what the call did before the node existed: two knn_points(K = 1) on csrc/knn.hip, knn_gather,
F.cosine_similarity and the torch arithmetic around them, differentiated by autograd (chamfer.fused_normals_path switched off for
that leg).  Shapes: 64 and 1 clouds of 5000 x 5000 random points with random unit normals, and 64 x 10 000 x 10 000 samples and
normals that sample_points_from_meshes drew from two batches of spheres.  Forward + backward to both clouds and both normals.
Device events around each step, warm-up iterations untimed, the legs alternating, medians.  Launches per step are counted by
torch.profiler in an untimed step.  The forward kernel at every split and knn_kernel<3, 2, 1> on the same clouds (both
directions: two launches, added) come from the library's built-in timing (p3d_profile_*) in separate, untimed iterations.
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

# name: (time limit of the step in seconds, clouds, points per cloud, from meshes)
STEPS = {
    "random_64x5000": (240, 64, 5000, False),
    "random_1x5000": (120, 1, 5000, False),
    "sampled_64x10000": (300, 64, 10000, True),
}


class Spheres:
    """N latitude-longitude spheres of different radii: what sample_points_from_meshes reads of a batch of meshes."""

    def __init__(self, N, device, rings=24, shift=0.0):
        import torch

        t, p = torch.meshgrid(torch.linspace(0.05, math.pi - 0.05, rings), torch.linspace(0, 2 * math.pi, 2 * rings + 1)[:-1], indexing="ij")
        unit = torch.stack([t.sin() * p.cos(), t.sin() * p.sin(), t.cos()], 2).reshape(-1, 3)
        i, j = torch.meshgrid(torch.arange(rings - 1), torch.arange(2 * rings), indexing="ij")
        a, b = i * 2 * rings + j, i * 2 * rings + (j + 1) % (2 * rings)
        faces = torch.cat([torch.stack([a, b, a + 2 * rings], 2), torch.stack([b, b + 2 * rings, a + 2 * rings], 2)]).reshape(-1, 3)
        V, self.F, self.N = unit.shape[0], faces.shape[0], N
        radii = 1.0 + 0.25 * torch.arange(N)[:, None, None] / max(N, 1)
        self.verts = ((unit[None] * radii).reshape(-1, 3) + shift).to(device)
        self.faces = (faces[None] + V * torch.arange(N)[:, None, None]).reshape(-1, 3).to(device)
        self.first = (torch.arange(N) * self.F).to(device)
        self.count = torch.full((N,), self.F).to(device)

    def __len__(self):
        return self.N

    def isempty(self):
        return False

    def verts_packed(self):
        return self.verts

    def faces_packed(self):
        return self.faces

    def mesh_to_faces_packed_first_idx(self):
        return self.first

    def num_faces_per_mesh(self):
        return self.count


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


def run_step(name):
    import torch

    import pytorch3d_amd as p3d
    from pytorch3d_amd import _C, _lib
    from pytorch3d_amd import chamfer as chamfer_mod

    _, N, P, sampled = STEPS[name]
    d = torch.device("cuda:0")
    gen = torch.Generator(device=d).manual_seed(0)
    if sampled:
        x0, xn0 = p3d.sample_points_from_meshes(Spheres(N, d), P, return_normals=True, generator=gen)
        y0, yn0 = p3d.sample_points_from_meshes(Spheres(N, d, shift=0.02), P, return_normals=True, generator=gen)
    else:
        x0, y0 = torch.rand(N, P, 3, generator=gen, device=d), torch.rand(N, P, 3, generator=gen, device=d)
        xn0, yn0 = (torch.nn.functional.normalize(torch.randn(N, P, 3, generator=gen, device=d), dim=2) for _ in range(2))
    fused_path = chamfer_mod.fused_normals_path

    def step_of(fused):
        def step():
            chamfer_mod.fused_normals_path = fused_path if fused else (lambda *a: False)
            try:
                leaves = [t.clone().requires_grad_(True) for t in (x0, y0, xn0, yn0)]
                loss, loss_normals = p3d.chamfer_distance(leaves[0], leaves[1], x_normals=leaves[2], y_normals=leaves[3])
                (loss + 0.1 * loss_normals).backward()
            finally:
                chamfer_mod.fused_normals_path = fused_path
        return step

    legs = {"general form (before)": step_of(False), "one node": step_of(True)}
    times = alternate(legs, 3, 20)
    out = {"step": name, "N": N, "P": P, "legs": {k: {"median": statistics.median(t), "min": min(t), "max": max(t), "iters": len(t)} for k, t in times.items()}}
    out["launches"] = {}
    for leg, step in legs.items():
        try:
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                step()
                torch.cuda.synchronize()
            out["launches"][leg] = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
        except Exception as e:  # the count is a note beside the times, not what the step is for
            out["launches"][leg] = "n/a (%s)" % type(e).__name__
    lib = _lib.load()
    out["forward_ms"] = {}
    for split in (0, 1, 2, 4, 8):
        lib.p3d_profile_reset()
        lib.p3d_profile_enable(1)
        try:
            for _ in range(5):
                _C.chamfer_normals_forward(x0, y0, xn0, yn0, split=split)
                if split == 0:
                    _C.knn_points_idx(x0, y0, None, None, 2, 1)
                    _C.knn_points_idx(y0, x0, None, None, 2, 1)
                    step_of(True)()
            torch.cuda.synchronize()
            snap = _lib.profile_snapshot()
        finally:
            lib.p3d_profile_enable(0)
        out["forward_ms"]["split %d" % split if split else "split chosen"] = snap["chamfer_normals_forward"][1] / snap["chamfer_normals_forward"][0]
        if split == 0:
            out["forward_ms"]["knn_kernel<3, 2, 1>, two launches"] = 2 * snap["knn_forward_k1"][1] / snap["knn_forward_k1"][0]
            out["kernels"] = {k: [n, ms / n] for k, (n, ms) in sorted(snap.items()) if k.startswith("chamfer_normals")}
    print(json.dumps(out))


def report(rec):
    lines = [f"{rec['step']}: {rec['N']} x {rec['P']} x {rec['P']}, D = 3, forward + backward, ms per step: median (min .. max) [timed iterations]"]
    for leg, t in rec["legs"].items():
        lines.append(f"  {leg:<28s} {t['median']:10.3f}  ({t['min']:.3f} .. {t['max']:.3f}) [{t['iters']}]   launches per step: {rec['launches'][leg]}")
    before, node = (rec["legs"][k]["median"] for k in ("general form (before)", "one node"))
    lines.append(f"  {'before / one node':<28s} {before / node:10.2f} x")
    lines.append("  forward launch (ms, mean of 5):")
    for k, ms in rec["forward_ms"].items():
        lines.append(f"    {k:<36s} {ms:9.4f}")
    lines.append("  per launch of the node (ms, mean):")
    for k, (n, ms) in rec["kernels"].items():
        lines.append(f"    {k:<36s} {ms:9.4f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=sorted(STEPS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        run_step(args.step)
        return
    lines = ["chamfer_distance with normals: csrc/chamfer_normals.hip against the general form on csrc/knn.hip, same GPU"]
    for name, (limit, *_rest) in STEPS.items():
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append(f"{name}: no result within {limit} s; stopped here")
            break
        if res.returncode != 0:
            lines.append(f"{name}: exit status {res.returncode}; stopped here\n{res.stderr[-2000:]}")
            break
        lines += report(json.loads(res.stdout.strip().splitlines()[-1]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
