#!/usr/bin/env python
"""point_mesh_face_distance / point_mesh_edge_distance on one MI355X: the grid search of csrc/point_mesh_grid.hip for the two
point-query forwards against the scan of all pairs of csrc/point_mesh.hip, the same build, the same GPU, the same process
(output kept as profiles/point_mesh_grid_mi355x.txt).

    python profiles/point_mesh_grid_bench.py [--out FILE]     the driver: every shape below in a child process of its own
    python profiles/point_mesh_grid_bench.py --step NAME       one shape, in this process

The driver runs each shape under its own time limit and stops at the first one that fails or runs out of time; it reads nothing
outside the repository.  The public losses, forward only and forward + backward to vertices and points.  Shapes: the three of
profiles/point_mesh_mi355x.txt (one cow x 10 000 points, 8 x ico_sphere(4) x 5000, the 64 meshes of the bench batch x 5000) and
ico_sphere(6) (81 920 faces, 122 880 edges) x 100 000 points.  Point distributions, seeded:
    near   vertices drawn with replacement, moved by 1 % of the mesh's size (a scan of the surface)
    box2   uniform in twice the mesh's bounding box
    bad    `near` with 1 % of the points 50 sizes away, and four faces added to the mesh that span its whole box
The legs are chosen by point_mesh.GRID_MIN_TARGETS (0: the grid; None: all pairs, the parent's kernels untouched); the two
target-query forwards and the backward are the same kernels in both.  Before any timing the two legs' losses, and dists and idxs of
both point-query operators, are compared with torch.equal on the timed inputs; the step fails where they differ.  A window is
`reps` calls between two device events, the second one synchronised, reps chosen from the warm call so that a window lasts at least
WINDOW_MS; WINDOWS windows per leg, the legs alternating; per call the median and the spread (min .. max) of the windows.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

WINDOW_MS, WINDOWS = 50.0, 5
CLOUDS = ("near", "box2", "bad")
# name: (time limit in seconds, points per mesh)
STEPS = {"cow_1": (240, 10000), "ico4_8": (240, 5000), "batch_64": (400, 5000), "ico6_1": (400, 100000)}


def meshes_of(name):
    import numpy as np
    import torch

    import _util as U

    if name == "cow_1":
        with np.load(os.path.join(ROOT, "tests", "golden", "cow_ref.npz")) as z:
            return [torch.from_numpy(z["verts_world"]).float()], [torch.from_numpy(z["faces"]).long()]
    if name == "ico4_8":
        v, f = U.ico_sphere(4)
        return [v.float() * (1.0 + 0.05 * i) for i in range(8)], [f.long()] * 8
    if name == "ico6_1":
        v, f = U.ico_sphere(6)
        return [v.float()], [f.long()]
    verts, faces = U.hetero_batch(64, seed=0, torus_div=1.0)
    return [v.float() for v in verts], [f.long() for f in faces]


def scene(name, kind, P, gen):
    """(verts list, faces list, points list) on the CPU."""
    import torch

    verts, faces = meshes_of(name)
    points = []
    for i, v in enumerate(verts):
        lo, hi = v.min(0).values, v.max(0).values
        size = float((hi - lo).max())
        if kind == "box2":
            points.append((lo + hi) / 2 + (torch.rand(P, 3, generator=gen) - 0.5) * 2.0 * (hi - lo))
            continue
        p = v[torch.randint(0, v.shape[0], (P,), generator=gen)] + 0.01 * size * torch.randn(P, 3, generator=gen)
        if kind == "bad":
            far = torch.rand(P, generator=gen) < 0.01
            p = torch.where(far[:, None], p + 50.0 * size * (torch.rand(P, 3, generator=gen) - 0.5), p)
            V = v.shape[0]
            corners = torch.stack([lo, torch.stack([hi[0], lo[1], lo[2]]), torch.stack([lo[0], hi[1], hi[2]]), hi])
            verts[i] = torch.cat([v, corners], 0)
            faces[i] = torch.cat([faces[i], V + torch.tensor([[0, 1, 2], [1, 2, 3], [0, 1, 3], [0, 2, 3]])], 0)
        points.append(p)
    return verts, faces, points


def run_step(name):
    import torch

    import pytorch3d_amd as p3d
    from pytorch3d_amd import _C, mesh_losses
    from pytorch3d_amd import point_mesh as pm

    _, P = STEPS[name]
    d = torch.device("cuda:0")
    out = {"step": name, "rows": []}

    def window(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    for kind in CLOUDS:
        gen = torch.Generator().manual_seed(len(kind) + len(name))
        verts0, faces0, points0 = scene(name, kind, P, gen)
        faces0 = [f.to(d) for f in faces0]
        leaves = {}
        for grad in (False, True):
            verts = [v.to(d).requires_grad_(grad) for v in verts0]
            points = [p.to(d).requires_grad_(grad) for p in points0]
            leaves[grad] = (verts + points, p3d.PackedMeshes(verts, faces0), p3d.PackedPointclouds(points))
            p3d.point_mesh_edge_distance(*leaves[grad][1:])  # builds the topology's tables once (host syncs)
        meshes, pcls = leaves[False][1:]
        topo = mesh_losses.topology_of(meshes)
        out[kind] = {"faces": int(meshes.faces_packed().shape[0]), "edges": int(topo.num_edges.sum()), "points": len(points0) * P}

        def call(loss_fn, grid, backward):
            pm.GRID_MIN_TARGETS = 0 if grid else None
            try:
                ls, m, c = leaves[backward]
                loss = loss_fn(m, c)
                if backward:
                    for t in ls:
                        t.grad = None
                    loss.backward()
                return loss.detach()
            finally:
                pm.GRID_MIN_TARGETS = None

        # bit-equality of the operators on the timed inputs
        pts, pfirst = pcls.points_packed(), pcls.cloud_to_packed_first_idx()
        tris = meshes.verts_packed()[meshes.faces_packed()]
        segs = meshes.verts_packed()[topo.edges.long()]
        sfirst = torch.cumsum(topo.num_edges.long(), 0) - topo.num_edges.long()
        for direction, prims, first in (("point_face", tris, meshes.mesh_to_faces_packed_first_idx()), ("point_edge", segs, sfirst)):
            a = _C.point_mesh_forward(direction, pts, pfirst, prims, first, P)
            b = _C.point_mesh_grid_forward(direction, pts, pfirst, prims, first, P)
            if not (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])):
                raise SystemExit(f"{name} {kind} {direction}: dists or idxs of the two legs differ")
        for tag, loss_fn in (("face", p3d.point_mesh_face_distance), ("edge", p3d.point_mesh_edge_distance)):
            for backward in (False, True):
                legs = {"grid": lambda: call(loss_fn, True, backward), "all pairs": lambda: call(loss_fn, False, backward)}
                ours, base = legs["grid"](), legs["all pairs"]()
                if not torch.equal(ours, base):
                    raise SystemExit(f"{name} {kind} {tag}: the losses of the two legs differ")
                torch.cuda.synchronize()
                first = {leg: window(fn, 1) for leg, fn in legs.items()}  # warm: the second call of the shape
                reps = {leg: max(1, min(500, math.ceil(WINDOW_MS / max(t, 1e-3)))) for leg, t in first.items()}
                times = {leg: [] for leg in legs}
                for _ in range(WINDOWS):
                    for leg, fn in legs.items():
                        times[leg].append(window(fn, reps[leg]))
                out["rows"].append({"cloud": kind, "loss": tag, "backward": backward, "reps": reps,
                                    "ms": {leg: [statistics.median(t), min(t), max(t), len(t)] for leg, t in times.items()}})
    print(json.dumps(out))


def report(rec):
    lines = [f"{rec['step']}: " + "; ".join(f"{k}: {rec[k]['faces']} faces, {rec[k]['edges']} edges, {rec[k]['points']} points" for k in CLOUDS),
             "  losses, dists and idxs of the two legs bit-equal on every row; ms per call: median (min .. max) [windows x calls]"]
    for row in rec["rows"]:
        g, a = row["ms"]["grid"], row["ms"]["all pairs"]
        verdict = "grid" if g[2] < a[1] else ("all pairs" if a[2] < g[1] else "within the spread")
        lines.append(f"  {row['cloud']:<5s} {row['loss']:<5s} {'fwd+bwd' if row['backward'] else 'forward':<8s}"
                     f" grid {g[0]:9.3f} ({g[1]:.3f} .. {g[2]:.3f}) [{g[3]} x {row['reps']['grid']}]"
                     f"   all pairs {a[0]:9.3f} ({a[1]:.3f} .. {a[2]:.3f}) [{a[3]} x {row['reps']['all pairs']}]"
                     f"   {a[0] / g[0]:7.2f} x   faster: {verdict}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=sorted(STEPS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        run_step(args.step)
        return
    lines = ["point-mesh losses: the grid search of csrc/point_mesh_grid.hip (point-query forwards) against the scan of all pairs, same GPU"]
    wins = {}
    for name, (limit, _) in STEPS.items():
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append(f"{name}: no result within {limit} s; stopped here")
            break
        if res.returncode != 0:
            lines.append(f"{name}: exit status {res.returncode}; stopped here\n{res.stdout[-500:]}\n{res.stderr[-2000:]}")
            break
        rec = json.loads(res.stdout.strip().splitlines()[-1])
        lines += report(rec)
        wins[name] = all(r["ms"]["grid"][2] < r["ms"]["all pairs"][1] for r in rec["rows"])
        print("\n".join(lines[-14:]), flush=True)
    lines.append("shapes on which the grid is faster on every row: " + (", ".join(n for n, w in wins.items() if w) or "none"))
    print(lines[-1], flush=True)
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
