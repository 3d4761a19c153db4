#!/usr/bin/env python
"""The mesh-refinement operators on one MI355X: GraphConv's neighbour sums (csrc/graph_conv.hip) and vert_align
(csrc/vert_align.hip) against the torch formulations the package ran before (output kept as
profiles/mesh_refine_mi355x.txt).

    python profiles/mesh_refine_bench.py [--out FILE]

Graphs: 32 x ico_sphere(4) (81 984 vertices, 245 760 edges) and the 64-mesh bench batch (tests/_util.hetero_batch, bench.py's
meshes), edges as Meshes.edges_packed gives them (unique, undirected).  Per graph:
  neighbor_sum      the kernel alone at D = 128, 3 and 512: ms, and its algorithmic bytes -- per row (1 + mean degree) reads and 1
                    write of D floats, plus the table -- as a fraction of PEAK_GBS
  gather_scatter    forward + backward at D = 128: ours against the scatter_add formulation (the reference's gather_scatter_python,
                    the only thing the parent commit could run on the GPU)
  graph_conv        one GraphConv(128 -> 128) layer, forward + backward to input and weights: ours against F.linear x 2 +
                    gather_scatter_python + add
  table build       graph_topology with its one checking sync, wall time
and a star graph (one hub joined to 100 000 leaves, D = 128): the hub's row is summed by one wave's lanes sequentially -- the figure
for the long-row case the kernel does not split.
vert_align: maps (32, 256, 56, 56) and (32, 512, 28, 28), NCHW and channels_last, the vertices of the 32 ico-spheres scaled into
[-1, 1]: forward, forward + backward as routed by default (which form of grad_feats ran is recorded), with the atomic form forced,
and with the ordered form under torch.use_deterministic_algorithms(True), against the reference's chain restated (F.grid_sample +
transpose + cat + gather).
Method: PREWARM untimed calls, then REPS timed loops of INNER calls between two device events; the median loop / INNER is reported,
min and max next to it.  Wall time (perf_counter around a synchronised loop) is given for the public functions as well."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PREWARM, REPS, INNER = 5, 15, 10
PEAK_GBS = 8000.0  # MI355X HBM3E


def timed(fn, inner=INNER, reps=REPS):
    """[min, median, max] ms per call from device events, and the wall ms per call of the median loop's kind."""
    import torch

    for _ in range(PREWARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    t = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t) * 1e3 / inner
    return [round(min(ms), 4), round(statistics.median(ms), 4), round(max(ms), 4)], round(wall, 4)


def unique_edges(faces):
    import torch

    e = torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    e = torch.stack([e.min(1).values, e.max(1).values], 1)
    return torch.unique(e, dim=0)


def batch_graph(verts, faces):
    """(packed verts, packed unique edges (E, 2) int64, first vertex of every mesh)."""
    import torch

    first, edges = 0, []
    for v, f in zip(verts, faces):
        edges.append(unique_edges(f.long()) + first)
        first += v.shape[0]
    return torch.cat(verts), torch.cat(edges)


def scatter_formulation(x, edges, directed=False):
    """pytorch3d/ops/graph_conv.py: gather_scatter_python."""
    import torch

    idx0 = edges[:, 0].view(-1, 1).expand(-1, x.shape[1])
    idx1 = edges[:, 1].view(-1, 1).expand(-1, x.shape[1])
    out = torch.zeros_like(x).scatter_add(0, idx0, x.gather(0, idx1))
    return out if directed else out.scatter_add(0, idx1, x.gather(0, idx0))


def fwd_bwd(fn, leaves, grad):
    import torch

    def run():
        out = fn(*leaves)
        torch.autograd.grad(out, leaves, grad)

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", help="graph | vert_align")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F

    import _util as U
    import pytorch3d_amd as p3d
    from pytorch3d_amd import _C
    import importlib

    VA = importlib.import_module("pytorch3d_amd.vert_align")

    if not torch.cuda.is_available():
        sys.exit("mesh_refine_bench: no GPU (the numbers of this script are device times)")
    d = torch.device("cuda:0")
    lines = ["mesh refinement operators on %s, torch %s; PREWARM %d, %d loops of %d calls, device events; ms per call as "
             "[min, median, max] of the loops, then wall ms" % (torch.cuda.get_device_name(0), torch.__version__, PREWARM, REPS, INNER)]

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    gen = torch.Generator().manual_seed(2)
    v4, f4 = U.ico_sphere(4)
    v4, f4 = torch.as_tensor(v4).float(), torch.as_tensor(f4)
    hv, hf = U.hetero_batch(64, seed=0)
    graphs = {"32 x ico_sphere(4)": batch_graph([v4] * 32, [f4] * 32), "bench batch of 64": batch_graph([torch.as_tensor(v).float() for v in hv], [torch.as_tensor(f) for f in hf])}
    if args.only in ("", "graph"):
        for label, (verts, edges) in graphs.items():
            V, E = verts.shape[0], edges.shape[0]
            edges_d = edges.to(d)
            t = time.perf_counter()
            topo = p3d.graph_topology(edges_d, V)
            torch.cuda.synchronize()
            first_build = (time.perf_counter() - t) * 1e3
            builds = []
            for _ in range(5):
                t = time.perf_counter()
                p3d.graph_topology(edges_d, V)
                torch.cuda.synchronize()
                builds.append((time.perf_counter() - t) * 1e3)
            rec = {"graph": label, "V": V, "E": E, "mean_degree": round(2 * E / V, 3), "table_build_wall_ms": round(statistics.median(builds), 3),
                   "table_build_first_call_ms": round(first_build, 3)}
            off, ent = topo.table()
            for D in (128, 3, 512):
                x = torch.randn((V, D), generator=gen).to(d)
                ms, _ = timed(lambda: _C.neighbor_sum(x, off, ent))
                nbytes = V * D * 4 * (2 + 2 * E / V) + (V + 1 + 2 * E) * 4
                rec["neighbor_sum_D%d_ms" % D] = ms
                # (the loops reread the same rows: whatever fits the 256 MiB Infinity Cache is served from there, and the figure can pass 1)
                rec["neighbor_sum_D%d_algorithmic_MB" % D] = round(nbytes / 1e6, 1)
                rec["neighbor_sum_D%d_fraction_of_hbm_peak" % D] = round(nbytes / (ms[1] * 1e-3) / 1e9 / PEAK_GBS, 4)
                base_ms, _ = timed(lambda: scatter_formulation(x, edges_d))
                rec["scatter_add_D%d_ms" % D] = base_ms
            x = torch.randn((V, 128), generator=gen).to(d).requires_grad_(True)
            g = torch.randn((V, 128), generator=gen).to(d)
            rec["gather_scatter_fwd_bwd_ms"], rec["gather_scatter_fwd_bwd_wall_ms"] = timed(fwd_bwd(lambda t: p3d.gather_scatter(t, edges_d), [x], g))
            rec["scatter_add_fwd_bwd_ms"], rec["scatter_add_fwd_bwd_wall_ms"] = timed(fwd_bwd(lambda t: scatter_formulation(t, edges_d), [x], g))
            w = [(torch.randn(s, generator=gen) * 0.05).to(d).requires_grad_(True) for s in ((128, 128), (128,), (128, 128), (128,))]
            rec["graph_conv_fwd_bwd_ms"], rec["graph_conv_fwd_bwd_wall_ms"] = timed(
                fwd_bwd(lambda t, w0, b0, w1, b1: p3d.graph_conv(t, edges_d, w0, b0, w1, b1), [x] + w, g))
            rec["reference_layer_fwd_bwd_ms"], rec["reference_layer_fwd_bwd_wall_ms"] = timed(
                fwd_bwd(lambda t, w0, b0, w1, b1: F.linear(t, w0, b0) + scatter_formulation(F.linear(t, w1, b1), edges_d), [x] + w, g))
            emit(rec)
        # the long row
        leaves = 100000
        star = torch.stack([torch.zeros(leaves, dtype=torch.int64), torch.arange(1, leaves + 1)], 1).to(d)
        topo = p3d.graph_topology(star, leaves + 1)
        x = torch.randn((leaves + 1, 128), generator=gen).to(d)
        ms, _ = timed(lambda: _C.neighbor_sum(x, *topo.table()), inner=3, reps=7)
        base_ms, _ = timed(lambda: scatter_formulation(x, star), inner=3, reps=7)
        emit({"graph": "star: one hub, 100000 leaves, D = 128", "neighbor_sum_ms": ms, "scatter_add_ms": base_ms})

    if args.only in ("", "vert_align"):
        verts = (v4 / v4.abs().max())[None].expand(32, -1, -1).contiguous()
        verts = (verts * (0.6 + 0.4 * torch.rand((32, 1, 1), generator=gen))).to(d).requires_grad_(True)
        for shape in ((32, 256, 56, 56), (32, 512, 28, 28)):
            for layout in ("NCHW", "channels_last"):
                feat = torch.randn(shape, generator=gen).to(d)
                if layout == "channels_last":
                    feat = feat.contiguous(memory_format=torch.channels_last)
                feat.requires_grad_(True)
                g = torch.randn((32, verts.shape[1], shape[1]), generator=gen).to(d)
                rec = {"vert_align": list(shape), "layout": layout, "rows": 32 * verts.shape[1]}
                with torch.no_grad():
                    rec["forward_ms"], rec["forward_wall_ms"] = timed(lambda: p3d.vert_align(feat, verts))
                    rec["chain_forward_ms"], rec["chain_forward_wall_ms"] = timed(lambda: VA.vert_align_torch(feat, verts))
                before = dict(_C.VERT_ALIGN_CALLS)
                rec["fwd_bwd_default_ms"], _ = timed(fwd_bwd(lambda f, v: p3d.vert_align(f, v), [feat, verts], g), inner=5)
                rec["default_grad_feats_path"] = "ordered" if _C.VERT_ALIGN_CALLS["ordered"] > before["ordered"] else "atomic"
                keep, _C.VERT_ALIGN_STRIDED_ORDERED_MIN_C = _C.VERT_ALIGN_STRIDED_ORDERED_MIN_C, 1 << 60  # the atomic form whatever the layout
                try:
                    rec["fwd_bwd_atomic_ms"], _ = timed(fwd_bwd(lambda f, v: p3d.vert_align(f, v), [feat, verts], g), inner=5)
                finally:
                    _C.VERT_ALIGN_STRIDED_ORDERED_MIN_C = keep
                rec["chain_fwd_bwd_ms"], _ = timed(fwd_bwd(lambda f, v: VA.vert_align_torch(f, v), [feat, verts], g), inner=5)
                torch.use_deterministic_algorithms(True)
                try:
                    rec["fwd_bwd_ordered_ms"], _ = timed(fwd_bwd(lambda f, v: p3d.vert_align(f, v), [feat, verts], g), inner=3, reps=7)
                finally:
                    torch.use_deterministic_algorithms(False)
                out_bytes = 32 * verts.shape[1] * shape[1] * 4
                rec["forward_output_GBs"] = round(out_bytes / (rec["forward_ms"][1] * 1e-3) / 1e9, 1)  # (4 corner reads per output float sit in cache)
                emit(rec)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
