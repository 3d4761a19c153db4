#!/usr/bin/env python
"""HarmonicEmbedding and the stratified ray depths on one MI355X: csrc/harmonic.hip against the torch chains that ran before it
(output kept as profiles/harmonic_mi355x.txt).

    python profiles/harmonic_bench.py [--out FILE] [--shapes NAME,NAME]

  fused   pytorch3d_amd.harmonic_embedding / stratified_depths: one autograd node / one launch over the kernels
  chain   harmonic_embedding_torch / stratified_depths_torch: the reference's formulation restated, what ran at the parent commit
The sides of a shape ALTERNATE call by call in one process; every shape is warmed; device events around each call; min / median of
REPS.  forward_ms: under no_grad.  step_ms: forward + backward, loss = sum(out * g) with a fixed g, gradients to x (and diag_cov).
peak_mb: torch.cuda.max_memory_allocated over one step of a side, above what was allocated before it.  kernel_ms: the library's own
per-kernel events (p3d_profile_enable) in a separate pass -- the kernels alone.  floor_ms: the bytes a kernel must move (forward: x
(+ diag_cov) in, the embedding out; backward: the embedding's gradient and x in, the gradients out; depths: uniforms in, depths out)
at the 6.29 TB/s measured copy rate.
Embedding shapes (dim 3, append_input, n = 10 and n = 4): 65 536 x 128 rows, 4096 x 64 rows, 65 536 x 128 rows with diag_cov.
Depth shapes: 10 x 128^2 rays x 150 points (the volume tutorial), 1024 rays x 64 points; the centres are the ray samplers' stride-0
expand of one linspace; both sides get the same pre-drawn uniforms, and `draw` times the call that draws for itself.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, REPS, COPY_RATE = 3, 12, 6.29e12
# name: (rows, n, diag_cov)
EMBEDDING_SHAPES = {"65536x128-n10": (65536 * 128, 10, False), "65536x128-n4": (65536 * 128, 4, False), "4096x64-n10": (4096 * 64, 10, False),
                    "4096x64-n4": (4096 * 64, 4, False), "65536x128-n10-cov": (65536 * 128, 10, True), "65536x128-n4-cov": (65536 * 128, 4, True)}
# name: (rays, points)
DEPTH_SHAPES = {"depths-10x128x128x150": (10 * 128 * 128, 150), "depths-1024x64": (1024, 64)}


def alternate(sides, reps):
    import torch

    ms = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: [round(min(v), 3), round(statistics.median(v), 3)] for k, v in ms.items()}


def kernel_ms(fn, prefix, reps=5):
    import torch

    from pytorch3d_amd import _lib

    lib = _lib.load()
    lib.p3d_profile_reset()
    lib.p3d_profile_enable(1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    snap = _lib.profile_snapshot()
    lib.p3d_profile_enable(0)
    return {k: round(total / max(n, 1), 4) for k, (n, total) in snap.items() if k.startswith(prefix)}


def peak_mb(fn):
    import torch

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=",".join(list(EMBEDDING_SHAPES) + list(DEPTH_SHAPES)))
    args = ap.parse_args()
    import importlib

    import torch

    import pytorch3d_amd as A

    H = importlib.import_module("pytorch3d_amd.harmonic_embedding")
    RS = importlib.import_module("pytorch3d_amd.raysampling")
    d = torch.device("cuda:0")
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "warmup": WARMUP, "reps": REPS})]
    print(lines[0], flush=True)

    def keep(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for name in args.shapes.split(","):
        if name in EMBEDDING_SHAPES:
            rows, n, with_cov = EMBEDDING_SHAPES[name]
            gen = torch.Generator(device=d).manual_seed(5)
            module = A.HarmonicEmbedding(n).to(d)
            f, W = module._frequencies, module.get_output_dim(3)
            x = (8 * torch.rand((rows, 3), generator=gen, device=d) - 4).requires_grad_(True)
            cov = (1e-2 * torch.rand((rows, 3), generator=gen, device=d)).requires_grad_(True) if with_cov else None
            g = torch.randn((rows, W), generator=gen, device=d)
            leaves = [x] + ([cov] if with_cov else [])
            assert H.kernel_path(x, f, cov, True)
            fns = {"fused": A.harmonic_embedding, "chain": H.harmonic_embedding_torch}

            def forward(side):
                with torch.no_grad():
                    return fns[side](x, f, cov, True)

            def step(side):
                return torch.autograd.grad(fns[side](x, f, cov, True), leaves, g)

            for _ in range(WARMUP):
                for side in fns:
                    forward(side), step(side)
            a, b = step("fused"), step("chain")
            agree = [round(float((p - q).abs().max() / q.abs().max()), 9) for p, q in zip(a, b)]
            out_agree = round(float((forward("fused") - forward("chain")).abs().max()), 9)
            del a, b
            in_bytes = rows * 3 * 4 * (2 if with_cov else 1)
            keep({"shape": name, "rows": rows, "n": n, "width": W, "diag_cov": with_cov,
                  "forward_ms": alternate({k: (lambda k=k: forward(k)) for k in fns}, REPS),
                  "step_ms": alternate({k: (lambda k=k: step(k)) for k in fns}, REPS),
                  "peak_mb": {k: peak_mb(lambda k=k: step(k)) for k in fns},
                  "kernel_ms": kernel_ms(lambda: step("fused"), "harmonic_embedding"),
                  "floor_ms": {"forward": round((in_bytes + rows * W * 4) / COPY_RATE * 1e3, 4),
                               "backward": round((2 * in_bytes + rows * W * 4) / COPY_RATE * 1e3, 4)},
                  "out_abs_difference_fused_vs_chain": out_agree, "grad_rel_difference_fused_vs_chain": agree})
            del x, cov, g
        else:
            rays, P = DEPTH_SHAPES[name]
            centers = torch.linspace(0.1, 3.0, P, device=d)[None].expand(rays, P)
            u = torch.rand((rays, P), device=d)
            fns = {"fused": A.stratified_depths, "chain": RS.stratified_depths_torch}
            assert RS.kernel_path(centers, u) and centers.stride(0) == 0
            for _ in range(WARMUP):
                for side in fns:
                    fns[side](centers, u), fns[side](centers)
            same = bool(torch.equal(fns["fused"](centers, u), fns["chain"](centers, u)))
            keep({"shape": name, "rays": rays, "points": P,
                  "given_uniforms_ms": alternate({k: (lambda k=k: fns[k](centers, u)) for k in fns}, REPS),
                  "draw_ms": alternate({k: (lambda k=k: fns[k](centers)) for k in fns}, REPS),
                  "peak_mb": {k: peak_mb(lambda k=k: fns[k](centers)) for k in fns},
                  "kernel_ms": kernel_ms(lambda: fns["fused"](centers, u), "stratified_depths"),
                  "floor_ms": round(2 * rays * P * 4 / COPY_RATE * 1e3, 4), "same_bits_fused_vs_chain": same})
            del centers, u
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
