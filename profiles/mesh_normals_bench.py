#!/usr/bin/env python
"""Face and vertex normals on one MI355X, the reference's torch chain (what ran before csrc/normals.hip) against the fused nodes
(output kept as profiles/mesh_normals_mi355x.txt).

    python profiles/mesh_normals_bench.py [--warmup 5] [--iters 20] [--out FILE]

The config-3 batch (tests/_util.hetero_batch(64, seed=0): 64 meshes).  Same process, device events around each forward + backward,
`warmup` untimed + `iters` timed iterations per leg, the two formulations ALTERNATING iteration by iteration, medians.
  1  vertex normals forward + backward to the vertices: Meshes._compute_vertex_normals' chain (gather, cross, 3 x index_add,
     normalize; torch autograd) against pytorch3d_amd.verts_normals with the incidence list built once outside the loop
  2  face areas + normals forward + backward: the torch formulation of pytorch3d_amd/_aux_ops.py against pytorch3d_amd.face_areas_normals
  3  pytorch3d_amd.phong_shading forward + backward on config-3 fragments (512^2, K = 8, point lights) with the vertex normals DERIVED
     from the vertices inside the step (not a detached leaf as in profiles/bench_configs.py), chain against fused node
"""
import argparse
import json
import math
import os
import statistics
import sys
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_verts_normals(verts, faces):
    import torch

    fv = verts[faces]
    fn = torch.cross(fv[:, 2] - fv[:, 1], fv[:, 0] - fv[:, 1], dim=1)
    s = torch.zeros_like(verts)
    for j in range(3):
        s = s.index_add(0, faces[:, j], fn)
    return torch.nn.functional.normalize(s, eps=1e-6, dim=1)


class _TorchFaceAreasNormals:
    """The autograd node the reference builds over `_C.face_areas_normals_*` (ops/mesh_face_areas_normals.py), on the torch formulation."""

    @staticmethod
    def make():
        import torch

        from pytorch3d_amd import _aux_ops

        cross = _aux_ops._cross

        class Node(torch.autograd.Function):
            @staticmethod
            def forward(ctx, verts, faces):
                ctx.save_for_backward(verts, faces)
                c = cross(verts, faces)
                norm = c.norm(dim=1)
                return norm / 2.0, c / norm.clamp_min(1e-6)[:, None]

            @staticmethod
            def backward(ctx, ga, gn):
                verts, faces = ctx.saved_tensors
                return torch_face_backward(ga, gn, verts, faces), None

        return Node


def torch_face_backward(grad_areas, grad_normals, verts, faces):
    """pytorch3d_amd/_aux_ops.py: face_areas_normals_backward's torch formulation, reached by switching the dispatch off."""
    from pytorch3d_amd import _aux_ops

    keep = _aux_ops.fused_face_areas_normals
    _aux_ops.fused_face_areas_normals = lambda *a: False
    try:
        return _aux_ops.face_areas_normals_backward(grad_areas, grad_normals, verts, faces)
    finally:
        _aux_ops.fused_face_areas_normals = keep


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
    ap.add_argument("--skip-phong", action="store_true")
    args = ap.parse_args()
    import torch

    import _util as U
    import pytorch3d_amd as p3d
    from pytorch3d_amd import shading as sh

    d = torch.device("cuda:0")
    verts, faces = U.hetero_batch(64, seed=0)
    m3 = p3d.PackedMeshes([x.to(d) for x in verts], [x.to(d) for x in faces])
    vp, fp = m3.verts_packed().detach(), m3.faces_packed()
    V, F = vp.shape[0], fp.shape[0]
    gen = torch.Generator(device=d).manual_seed(0)
    lines = [f"{torch.cuda.get_device_name(0)}; config-3 batch: 64 meshes, V = {V}, F = {F}; {args.warmup} warm-up + {args.iters} timed "
             "iterations per leg, legs alternating, device events, ms per forward + backward: median (min .. max)"]
    record = {"V": V, "F": F}

    def report(title, times):
        row = {}
        for name, t in times.items():
            row[name] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
            lines.append(f"  {title:<34s} {name:<12s} {row[name]['median']:8.3f}  ({row[name]['min']:.3f} .. {row[name]['max']:.3f})")
        lines.append(f"  {'':<34s} {'torch/fused':<12s} {row['torch']['median'] / row['fused']['median']:8.2f} x")
        record[title] = row

    # ---- 1. vertex normals ----------------------------------------------------------------------------------------------------
    g_n = torch.randn((V, 3), generator=gen, device=d)
    inc = p3d.vert_incidence(fp, V)

    def vn(fn):
        def step():
            v = vp.clone().requires_grad_(True)
            fn(v).backward(g_n)
        return step

    report("vertex normals fwd+bwd", alternate({"torch": vn(lambda v: torch_verts_normals(v, fp)),
                                                "fused": vn(lambda v: p3d.verts_normals(v, fp, inc))}, args.warmup, args.iters))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    p3d.vert_incidence(fp, V)
    b.record()
    b.synchronize()
    lines.append(f"  (vert_incidence, once per topology: {a.elapsed_time(b):.3f} ms)")

    # ---- 2. face areas and normals ----------------------------------------------------------------------------------------------
    g_a, g_fn = torch.randn((F,), generator=gen, device=d), torch.randn((F, 3), generator=gen, device=d)
    node = _TorchFaceAreasNormals.make()

    def fa(fn):
        def step():
            v = vp.clone().requires_grad_(True)
            torch.autograd.backward(list(fn(v)), [g_a, g_fn])
        return step

    report("face areas + normals fwd+bwd", alternate({"torch": fa(lambda v: node.apply(v, fp)), "fused": fa(lambda v: p3d.face_areas_normals(v, fp))},
                                                     args.warmup, args.iters))

    # ---- 3. phong_shading with derived normals ------------------------------------------------------------------------------------
    if not args.skip_phong:
        blur = math.log(1.0 / 1e-4 - 1.0) * 1e-4
        frag = p3d.rasterize_meshes(m3, image_size=512, blur_radius=blur, faces_per_pixel=8, perspective_correct=True, clip_barycentric_coords=True)
        p2f, bary = frag[0], frag[2].detach()
        FragS = namedtuple("FragS", "pix_to_face bary_coords")
        tex = torch.rand((64, 512, 512, 8, 3), generator=gen, device=d)
        g_col = torch.randn((64, 512, 512, 8, 3), generator=gen, device=d)
        r3 = lambda n=64: torch.rand((n, 3), generator=gen, device=d)
        lights = sh.Lights(r3(), r3(), r3(), location=torch.randn((64, 3), generator=gen, device=d) * 2)
        mats = sh.Materials(r3(1), r3(1), r3(1), torch.tensor([32.0], device=d))

        class Cam:
            c = torch.randn((64, 3), generator=gen, device=d) - torch.tensor([0.0, 0.0, 3.0], device=d)

            def get_camera_center(self):
                return self.c

        class Mesh:
            def __init__(self, v, n):
                self.v, self.n = v, n

            def verts_packed(self):
                return self.v

            def faces_packed(self):
                return fp

            def verts_normals_packed(self):
                return self.n

        def ph(fn):
            def step():
                v = vp.clone().requires_grad_(True)
                p3d.phong_shading(Mesh(v, fn(v)), FragS(p2f, bary), lights, Cam(), mats, tex).backward(g_col)
            return step

        report("phong_shading fwd+bwd, normals(v)", alternate({"torch": ph(lambda v: torch_verts_normals(v, fp)),
                                                               "fused": ph(lambda v: p3d.verts_normals(v, fp, inc))}, args.warmup, args.iters))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(record))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
