#!/usr/bin/env python
"""SubdivideMeshes, forward + backward, against the reference's own module (staged package, plain shim.install()) in one process.

    python profiles/subdivide_bench.py > profiles/subdivide_mi355x.txt

Shapes: batches of ico_sphere(4 .. 6) and a batch of cubified balls of different radii (heterogeneous), features of width 3 and 128.
Every repetition gets fresh mesh objects, so both sides build the edges of a topology they have not seen -- what a step after cubify
or marching_cubes pays.  Pre-warmed, 31 repetitions, each ended by a device synchronise: [min, median, max] in ms for both sides; peak
memory of a step; kernel launches of a step (torch.profiler); and the forward kernel alone against its compulsory traffic
(V + 2 E + V + E) D 4 bytes per tensor plus 8 E bytes of edges."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REPS = 31


def timed(step, make):
    for _ in range(3):
        step(make())
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        arg = make()
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        step(arg)
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end))
    return [min(times), statistics.median(times), max(times)]


def launches(step, arg):
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step(arg)
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as e:  # noqa: BLE001
        return "n/a (%s)" % type(e).__name__


def peak(step, arg):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step(arg)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd as p3d
    import pytorch3d_amd.shim as shim
    from pytorch3d_amd import _C
    from pytorch3d_amd import subdivide_meshes as M

    shim.install(os.environ.get("P3D_REFERENCE_ROOT") or os.path.join(ROOT, "oracle", "_ref", "reference_py"))
    from pytorch3d.ops import SubdivideMeshes as RefSubdivide
    from pytorch3d.structures import Meshes
    from pytorch3d.utils import ico_sphere

    d = torch.device("cuda:0")
    shapes = {}
    for level, batch in ((4, 16), (5, 8), (6, 4)):
        s = ico_sphere(level)
        shapes[f"ico_sphere({level}) x {batch}"] = ([s.verts_packed().to(d)] * batch, [s.faces_packed().to(d)] * batch)
    z, y, x = torch.meshgrid(*[torch.arange(32.0)] * 3, indexing="ij")
    balls = torch.stack([((x - 15.5) ** 2 + (y - 15.5) ** 2 + (z - 15.5) ** 2 <= r * r).float() for r in (6, 8, 9, 10, 11, 12, 13, 14)]).to(d)
    cubes = p3d.cubify(balls, 0.5)
    shapes["cubified balls 32^3 x 8"] = (cubes.verts_list(), cubes.faces_list())

    a = torch.empty(2 ** 26, device=d)
    copy_ms = timed(lambda t: t.copy_(a), lambda: torch.empty_like(a))[1]
    rate = 2 * a.numel() * 4 / copy_ms / 1e6
    print(f"device copy rate {rate:.0f} GB/s ({REPS} repetitions of a 256 MiB copy, median)")
    del a
    for name, (verts, faces) in shapes.items():
        V, F = sum(v.shape[0] for v in verts), sum(f.shape[0] for f in faces)
        for D in (3, 128):
            feats = torch.randn((V, D), device=d)

            def fresh(cls):
                vs = [v.clone().requires_grad_(True) for v in verts]
                return cls(vs, [f.clone() for f in faces]) if cls is p3d.PackedMeshes else cls(verts=vs, faces=[f.clone() for f in faces])

            def step(module):
                def run(meshes):
                    new_meshes, new_feats = module(meshes, feats.requires_grad_(True))
                    (new_meshes.verts_packed().sum() + new_feats.sum()).backward()
                return run

            ours, ref = step(p3d.SubdivideMeshes()), step(RefSubdivide())
            t_ours, t_ref = timed(ours, lambda: fresh(p3d.PackedMeshes)), timed(ref, lambda: fresh(Meshes))
            E = M.mesh_edges_build(torch.cat(faces), [V], [F]).E if len(verts) == 1 else M._edges_of(fresh(p3d.PackedMeshes)).E
            t = M._edges_of(p3d.PackedMeshes(verts, faces))
            xs = [torch.cat(verts), feats]
            t_fwd = timed(lambda _: _C.subdivide_forward(xs, t.edges, t.vert_first, t.first_edge, t.V, t.E), lambda: None)[1]
            floor_bytes = (V + 2 * E + V + E) * (3 + D) * 4 + 8 * E
            verdict = "below" if t_ours[1] < t_ref[0] else "NOT below"
            print(f"{name}, D = {D}: V = {V}, F = {F}, E = {E}")
            print("  fused      fwd + bwd [min, median, max] ms: [%.3f, %.3f, %.3f]   launches %s   peak %.1f MiB" %
                  (*t_ours, launches(ours, fresh(p3d.PackedMeshes)), peak(ours, fresh(p3d.PackedMeshes))))
            print("  reference  fwd + bwd [min, median, max] ms: [%.3f, %.3f, %.3f]   launches %s   peak %.1f MiB" %
                  (*t_ref, launches(ref, fresh(Meshes)), peak(ref, fresh(Meshes))))
            print(f"  fused median {verdict} the reference's minimum ({t_ref[0] / t_ours[1]:.1f} x)")
            print("  forward kernel (verts + feats, one launch) %.4f ms; compulsory %.2f MB = %.4f ms at the copy rate: %.1f x its floor" %
                  (t_fwd, floor_bytes / 1e6, floor_bytes / rate / 1e6, t_fwd / (floor_bytes / rate / 1e6)))


if __name__ == "__main__":
    main()
