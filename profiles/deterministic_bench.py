#!/usr/bin/env python
"""What the deterministic backwards cost on one MI355X (csrc/ordered_bwd.hip): the ordered backward under
torch.use_deterministic_algorithms(True) next to the atomic backward of the same inputs, in the same process.

    python profiles/deterministic_bench.py [--warmup 5] [--iters 20] [--out FILE]

config 3: bench.py's batch -- 64 meshes, 512^2, K = 8, its upstream gradients -- both forms of the mesh backward:
  grad_face_verts (F,3,3) and grad_verts (V,3) through faces.
config 4: 1M points, 512^2, K = 10, r = 0.01: rasterize_points_backward, and the fused PointsRenderer backward (alpha).
Per leg: `atomic` (flag off, the forward's row cover where there is one), `ordered` end to end as a user gets it (the hit list --
torch.nonzero with its host sync, the stable sort -- the workspace allocation and the kernels), `ordered_kernels` (the C entry
alone on a list and a workspace made before).  One call between two device events on the stream; the legs alternate inside every
iteration; median (min .. max) of the timed iterations.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import math

    import _util as U
    import pytorch3d_amd as p3d
    from pytorch3d_amd import _C, _lib

    d = torch.device("cuda:0")
    lib = _lib.load()
    P_, S_ = _C._ptr, _C._stream

    def flagged(on, fn):
        def run():
            torch.use_deterministic_algorithms(on)
            try:
                return fn()
            finally:
                torch.use_deterministic_algorithms(False)
        return run

    # ---- config 3 ----------------------------------------------------------------------------------------------------------------
    B, H, K = 64, 512, 8
    blur = math.log(1.0 / 1e-4 - 1.0) * 1e-4
    verts, faces = U.hetero_batch(B, seed=0, torus_div=U.CONFIG3_TORUS_DIV)
    m = p3d.PackedMeshes([v.to(d) for v in verts], [f.to(d) for f in faces])
    fv = m.verts_packed()[m.faces_packed()].contiguous()
    fp = m.faces_packed().contiguous()
    F, V = int(fv.shape[0]), int(m.verts_packed().shape[0])
    nbr = torch.full((F,), -1, dtype=torch.int64, device=d)
    (p2f, _, _, _), cover = _C._rasterize_meshes_covered(fv, m.mesh_to_faces_packed_first_idx(), m.num_faces_per_mesh(), nbr, (H, H), blur, K, 32,
                                                          int(max(10000, F / 5)), True, True, False)
    gen = torch.Generator().manual_seed(231)
    gz = torch.randn((B, H, H, K), generator=gen).to(d)
    gb = torch.randn((B, H, H, K, 3), generator=gen).to(d)
    gd = torch.randn((B, H, H, K), generator=gen).to(d)
    hits = _C._sorted_hits(p2f)
    corners = _C._sorted_corners(fp, V)
    ws_f = _C._workspace(lib.p3d_rasterize_meshes_backward_ordered_workspace_bytes(F, 0, hits.numel()), d)
    ws_v = _C._workspace(lib.p3d_rasterize_meshes_backward_ordered_workspace_bytes(F, 1, hits.numel()), d)
    out_f = torch.empty((F, 3, 3), device=d)
    out_v = torch.empty((V, 3), device=d)

    def mesh_kernels(through):
        def run():
            rc = lib.p3d_rasterize_meshes_backward_ordered(
                P_(fv), P_(fp) if through else None, P_(p2f), P_(gz), P_(gb), P_(gd), P_(hits), hits.numel(), P_(corners) if through else None,
                corners.numel() if through else 0, F, V if through else 0, B, H, H, K, 1, 1, P_(out_v if through else out_f),
                P_(ws_v if through else ws_f), (ws_v if through else ws_f).numel(), S_(d))
            _lib.check(rc, "mesh ordered")
        return run

    # ---- config 4 ----------------------------------------------------------------------------------------------------------------
    gen = torch.Generator().manual_seed(0)
    NP, KP, r, C = 1_000_000, 10, 0.01, 3
    pts = torch.cat([torch.rand(NP, 2, generator=gen) * 2 - 1, torch.rand(NP, 1, generator=gen) * 2 + 0.5], 1).to(d)
    feats = torch.rand(NP, C, generator=gen).to(d)
    first = torch.zeros(1, dtype=torch.int64, device=d)
    count = torch.full((1,), NP, dtype=torch.int64, device=d)
    radius = torch.full((NP,), r, device=d)
    inv = _C.inv_r2_of(r)
    idx, _, dists, _ = _C.rasterize_points_composite(pts, first, count, (H, H), radius, feats, inv, KP, 32, 200000)
    pgz = torch.randn((1, H, H, KP), generator=gen).to(d)
    pgd = torch.randn((1, H, H, KP), generator=gen).to(d)
    gi = torch.randn((1, H, H, C), generator=gen).to(d)
    phits = _C._sorted_hits(idx)
    ws_p = _C._workspace(lib.p3d_rasterize_points_backward_ordered_workspace_bytes(phits.numel()), d)
    ws_s = _C._workspace(lib.p3d_rasterize_points_composite_backward_ordered_workspace_bytes(1, H, H, KP, C, phits.numel()), d)
    out_p = torch.empty((NP, 3), device=d)
    out_pf = torch.empty((NP, C), device=d)

    def points_kernels():
        _lib.check(lib.p3d_rasterize_points_backward_ordered(P_(pts), P_(idx), P_(pgz), P_(pgd), P_(phits), phits.numel(), NP, 1, H, H, KP, P_(out_p),
                                                             P_(ws_p), ws_p.numel(), S_(d)), "points ordered")

    def fused_kernels():
        _lib.check(lib.p3d_rasterize_points_composite_backward_ordered(0, P_(pts), P_(feats), P_(idx), P_(dists), P_(gi), P_(phits), phits.numel(), NP, C,
                                                                       1, H, H, KP, inv, P_(out_p), P_(out_pf), P_(ws_s), ws_s.numel(), S_(d)),
                   "fused ordered")

    mesh_f = lambda: _C.rasterize_meshes_backward(fv, p2f, gz, gb, gd, True, True, _cover=cover)  # noqa: E731
    mesh_v = lambda: _C._mesh_backward(fv, fp, V, p2f, gz, gb, gd, True, True, cover)  # noqa: E731
    pts_b = lambda: _C.rasterize_points_backward(pts, idx, pgz, pgd)  # noqa: E731
    fused_b = lambda: _C.rasterize_points_composite_backward(pts, feats, idx, dists, gi, inv)  # noqa: E731
    groups = [
        ("config3_mesh_backward_face_verts", flagged(False, mesh_f), flagged(True, mesh_f), mesh_kernels(False)),
        ("config3_mesh_backward_verts", flagged(False, mesh_v), flagged(True, mesh_v), mesh_kernels(True)),
        ("config4_points_backward", flagged(False, pts_b), flagged(True, pts_b), points_kernels),
        ("config4_points_composite_backward", flagged(False, fused_b), flagged(True, fused_b), fused_kernels),
    ]
    legs = []
    for name, atomic, ordered, kernels in groups:
        legs += [(name, "atomic", atomic), (name, "ordered", ordered), (name, "ordered_kernels", kernels)]
    times = {(n, k): [] for n, k, _ in legs}
    for it in range(args.warmup + args.iters):
        for n, k, fn in legs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= args.warmup:
                times[(n, k)].append(a.elapsed_time(b))
    lines = [f"# deterministic_bench: config 3 = {B} meshes, {F} faces, {V} vertices, {H}^2, K={K}, {hits.numel()} samples with a face; "
             f"config 4 = {NP} points, {H}^2, K={KP}, r={r}, {phits.numel()} entries with a point; {args.warmup} warm-up + {args.iters} timed "
             f"iterations, device events, median (min .. max) ms; {torch.cuda.get_device_name(0)}"]
    for name, _, _, _ in groups:
        med = {}
        rec = {"case": name}
        for k in ("atomic", "ordered", "ordered_kernels"):
            t = times[(name, k)]
            med[k] = statistics.median(t)
            rec[k] = {"ms": round(med[k], 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
        rec["ordered_over_atomic"] = round(med["ordered"] / med["atomic"], 2)
        rec["ordered_kernels_over_atomic"] = round(med["ordered_kernels"] / med["atomic"], 2)
        rec["list_sort_alloc_ms"] = round(med["ordered"] - med["ordered_kernels"], 4)
        lines.append(json.dumps(rec))
    # where the kernel time goes (the library's own per-launch events)
    lib.p3d_profile_reset()
    lib.p3d_profile_enable(1)
    for fn in (mesh_kernels(False), mesh_kernels(True), points_kernels, fused_kernels):
        fn()
    lib.p3d_profile_enable(0)
    lines.append(json.dumps({"ordered_launches_ms_each": {k: round(v[1] / v[0], 4) for k, v in _lib.profile_snapshot().items()}}))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
