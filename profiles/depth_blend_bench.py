#!/usr/bin/env python
"""The depth shaders' kernels on one MI355X (csrc/blend.hip: soft_depth / hard_depth, forward and backward) next to
softmax_rgb_blend's kernels on the same fragments -- the yardstick: the depth kernels move 16 B per slot where the softmax
blend moves 28 forward, and write 8 B per slot backward where it writes 20, so each is expected to take no longer than its
softmax counterpart in the same run -- and next to the torch chain a user without the shim patch runs (SoftDepthShader's
sigmoid / cat / cumsum / clamp / diff / sum in float32 with autograd), forward + backward, run over 16 images at a time
(torch.cumsum on ROCm refuses the launch for the (64, 512, 512, 9) tensor).

    python profiles/depth_blend_bench.py [--n 64] [--size 512] [--k 8] [--warmup 5] [--iters 20] [--out FILE]

Fragments: the recipe of tests/depth_restatement.py: depth_inputs ("prefix": 0..K valid leading slots per pixel, 35 % of
the slots interior, the others within a few sigma of an edge), NOT a rasterized scene: 8 seeded images repeated to the batch.
Every candidate is one C-ABI call between two device events; the candidates alternate inside every iteration and the
softmax legs run twice per iteration (`softmax_*` and `softmax_*_again`): the difference of their medians is the spread
of the run.  Compulsory bytes: soft forward npix (16 K + 4), soft backward npix (16 K + 4 + 8 K), hard forward one 32-byte
sector of pix_to_face and of zbuf per pixel + 4, hard backward one sector + 4 + 4 K; the peak is 8 TB/s.
Kernel times are confirmed by a separate `rocprofv3 --kernel-trace --stats -- python profiles/depth_blend_bench.py` run.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK = 8.0e12  # B/s


def torch_chain(p2f, zbuf, dists, sigma, zfar):
    """SoftDepthShader's formula with autograd-capable torch ops in float32"""
    N, H, W, K = p2f.shape
    prob = torch.sigmoid(-dists / sigma) * (p2f >= 0)
    one = torch.ones((N, H, W, 1), device=zbuf.device)
    z = torch.cat((zbuf, one * zfar), dim=3)
    c = torch.cat((prob, one), dim=3).cumsum(dim=3).clamp(max=1)
    w = c.diff(dim=3, prepend=torch.zeros((N, H, W, 1), device=zbuf.device))
    return (w * z).sum(dim=3).unsqueeze(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import depth_restatement as dr
    from pytorch3d_amd import _C, _lib

    d = torch.device("cuda:0")
    N, H, W, K = args.n, args.size, args.size, args.k
    sigma, gamma, zfar, znear = 1e-4, 1e-4, 100.0, 1.0
    gen = torch.Generator().manual_seed(3)
    base = min(8, N)
    reps = -(-N // base)
    p2f, zbuf, dists = (t.to(d).repeat(reps, 1, 1, 1)[:N].contiguous() for t in dr.depth_inputs(gen, base, H, W, K, sigma))
    classes = dr.pixel_classes(p2f[:base].cpu(), dists[:base].cpu(), sigma)
    npix = N * H * W
    colors = torch.rand(N, H, W, K, 3, device=d)
    g1 = torch.randn(N, H, W, 1, device=d)
    g4 = torch.randn(N, H, W, 4, device=d)
    depth = torch.empty(N, H, W, 1, device=d)
    rgba = torch.empty(N, H, W, 4, device=d)
    gd, gz, gc = torch.empty_like(dists), torch.empty_like(zbuf), torch.empty_like(colors)
    bg = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    lib = _lib.load()
    P, S = _C._ptr, _C._stream(d)

    def call(fn, *a):
        _lib.check(fn(*a), fn.__name__)

    def chain():
        # in chunks of 16 images: torch.cumsum refuses the launch for the 64-image tensor ("invalid configuration argument")
        for i in range(0, N, 16):
            z = zbuf[i:i + 16].detach().requires_grad_(True)
            x = dists[i:i + 16].detach().requires_grad_(True)
            torch_chain(p2f[i:i + 16], z, x, sigma, zfar).backward(g1[i:i + 16])

    softmax_fwd = lambda: call(lib.p3d_softmax_rgb_blend_forward, P(colors), P(p2f), P(dists), P(zbuf), sigma, gamma, bg, znear,  # noqa: E731
                               zfar, None, None, N, H * W, K, P(rgba), S)
    softmax_bwd = lambda: call(lib.p3d_softmax_rgb_blend_backward, P(g4), P(colors), P(p2f), P(dists), P(zbuf), sigma, gamma, bg,  # noqa: E731
                               znear, zfar, None, None, N, H * W, K, P(gc), P(gd), P(gz), S)
    sector = 32
    legs = [  # name, callable, compulsory bytes (None: not a single stream)
        ("soft_depth_fwd", lambda: call(lib.p3d_soft_depth_blend_forward, P(dists), P(zbuf), P(p2f), sigma, zfar, npix, K, P(depth), S),
         npix * (16 * K + 4)),
        ("softmax_fwd", softmax_fwd, npix * (28 * K + 16)),
        ("soft_depth_bwd", lambda: call(lib.p3d_soft_depth_blend_backward, P(g1), P(dists), P(zbuf), P(p2f), sigma, zfar, npix, K,
                                        P(gd), P(gz), S), npix * (16 * K + 4 + 8 * K)),
        ("softmax_bwd", softmax_bwd, npix * (28 * K + 16 + 20 * K)),
        ("hard_depth_fwd", lambda: call(lib.p3d_hard_depth_blend_forward, P(zbuf), P(p2f), zfar, npix, K, P(depth), S),
         npix * (2 * sector + 4)),
        ("hard_depth_bwd", lambda: call(lib.p3d_hard_depth_blend_backward, P(g1), P(p2f), npix, K, P(gz), S),
         npix * (sector + 4 + 4 * K)),
        ("softmax_fwd_again", softmax_fwd, npix * (28 * K + 16)),
        ("softmax_bwd_again", softmax_bwd, npix * (28 * K + 16 + 20 * K)),
        ("torch_chain_fwd_bwd", chain, None),
    ]
    times = {name: [] for name, _, _ in legs}
    for it in range(args.warmup + args.iters):
        for name, fn, _ in legs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= args.warmup:
                times[name].append(a.elapsed_time(b))
    lines = [f"# depth_blend_bench: N={N} {H}x{W} K={K} sigma={sigma} zfar={zfar}; recipe fragments (empty / unsaturated / "
             f"saturated by slot 0 / saturated later = " + " / ".join("%.2f" % c for c in classes) + f"); {args.warmup} warm-up + "
             f"{args.iters} timed iterations, device events, median (min .. max) ms; {torch.cuda.get_device_name(0)}"]
    med = {}
    for name, _, nbytes in legs:
        t = times[name]
        med[name] = statistics.median(t)
        rec = {"kernel": name, "ms": round(med[name], 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
        if nbytes is not None:
            rec.update(compulsory_gb=round(nbytes / 1e9, 3), tb_per_s=round(nbytes / med[name] / 1e9, 3),
                       of_hbm_peak=round(nbytes / (med[name] * 1e-3) / HBM_PEAK, 3))
        lines.append(json.dumps(rec))
    spread = {k: abs(med["softmax_" + k] - med["softmax_" + k + "_again"]) / med["softmax_" + k] for k in ("fwd", "bwd")}
    lines.append(json.dumps({"softmax_leg_spread": {k: round(v, 4) for k, v in spread.items()},
                             "soft_depth_fwd_over_softmax_fwd": round(med["soft_depth_fwd"] / med["softmax_fwd"], 3),
                             "soft_depth_bwd_over_softmax_bwd": round(med["soft_depth_bwd"] / med["softmax_bwd"], 3),
                             "torch_chain_over_fused_fwd_bwd": round(med["torch_chain_fwd_bwd"] /
                                                                     (med["soft_depth_fwd"] + med["soft_depth_bwd"]), 1)}))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
