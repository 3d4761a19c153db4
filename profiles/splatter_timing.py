#!/usr/bin/env python
"""SplatterPhongShader's blend on one MI355X: the fused kernels (pytorch3d_amd/splatter.py) against the reference's torch
SplatterBlender (pytorch3d/renderer/splatter_blend.py) on the same GPU, and the whole SplatterPhongShader forward + backward
unpatched vs patched (pytorch3d_amd.shim).  Fragments: BASELINE config 3's mesh generator (bench.build_batch), 512^2, K = 8,
rasterized by pytorch3d_amd.  One JSON line per case; a reference run that does not fit is recorded as out of memory.

    python profiles/splatter_timing.py [--n 8 64] [--fused-only] [--iters 5]

Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python profiles/splatter_timing.py --fused-only` run.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STAGE = os.path.join(ROOT, "oracle", "_ref", "reference_py")
HBM_PEAK = 8.0e12  # B/s


def bytes_fwd(N, H, W, K):  # per layer RGB, screen xyz, background flag; RGBA out
    return N * H * W * (K * (12 + 12 + 1) + 16)


def bytes_bwd(N, H, W, K):  # inputs twice (two passes), grad_out, the 96-byte record written and read, both gradients
    return N * H * W * (2 * K * 25 + 16 + 2 * 96 + K * 24)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / iters
    return round(ms, 3), round((torch.cuda.max_memory_allocated() - base) / 2**30, 3)


def attempt(fn, iters):
    try:
        ms, gb = timed(fn, iters)
        return {"ms": ms, "peak_gb_above_inputs": gb, "measured": True}
    except torch.cuda.OutOfMemoryError as e:
        torch.cuda.empty_cache()
        return {"measured": False, "result": "out of memory", "error": str(e).splitlines()[0][:200]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true")
    args = ap.parse_args()
    import bench
    import pytorch3d_amd as p3d

    d = torch.device("cuda:0")
    H = W = 512
    K = 8
    ref = None
    if not args.fused_only and os.path.isdir(os.path.join(STAGE, "pytorch3d", "renderer")):
        import run_reference_suite as rrs

        rrs._stub_missing_packages()
        import pytorch3d_amd.shim as shim

        shim.install(STAGE, patch_python=False)
        ref = shim
    for N in args.n:
        meshes, verts, faces, _ = bench.build_batch(N, 0, d)
        p2f, zbuf, bary, dists = p3d.rasterize_meshes(meshes, image_size=H, blur_radius=0.0, faces_per_pixel=K)
        mask = p2f < 0
        gen = torch.Generator().manual_seed(1)
        hh = torch.arange(H, device=d, dtype=torch.float32).view(1, H, 1, 1)
        ww = torch.arange(W, device=d, dtype=torch.float32).view(1, 1, W, 1)
        coords = torch.stack([(ww + 0.5).expand(N, H, W, K), (hh + 0.5).expand(N, H, W, K), zbuf], -1).contiguous()
        colors = torch.rand((N, H, W, K, 3), generator=gen).to(d)
        grad = torch.randn((N, H, W, 4), generator=gen).to(d)
        bp = p3d.BlendParams(sigma=0.5, background_color=(1.0, 1.0, 1.0))
        c = colors.clone().requires_grad_(True)
        x = coords.clone().requires_grad_(True)

        def fused_fwd():
            with torch.no_grad():
                p3d.splatter_blend(colors, coords, mask, bp)

        def fused_fwd_bwd():
            img = p3d.splatter_blend(c, x, mask, bp)
            img.backward(grad)

        row = {"case": f"blend N={N} {H}x{W} K={K}", "covered": round(float((p2f[..., 0] >= 0).float().mean()), 3),
               "fused_fwd": attempt(fused_fwd, args.iters), "fused_fwd_bwd": attempt(fused_fwd_bwd, args.iters),
               "algorithmic_bytes_fwd": bytes_fwd(N, H, W, K), "algorithmic_bytes_bwd": bytes_bwd(N, H, W, K)}
        if ref is not None:
            from pytorch3d.renderer import BlendParams
            from pytorch3d.renderer.splatter_blend import SplatterBlender

            class Ident:
                def transform_points_screen(self, p, image_size=None, with_xyflip=True):
                    return p.clone()

            rbp = BlendParams(sigma=0.5, background_color=(1.0, 1.0, 1.0))
            holder = {}

            def ref_fwd():
                with torch.no_grad():
                    if "b" not in holder:
                        holder["b"] = SplatterBlender((N, H, W, K), d)
                    holder["b"](colors, coords, Ident(), mask, rbp)

            def ref_fwd_bwd():
                if "b" not in holder:
                    holder["b"] = SplatterBlender((N, H, W, K), d)
                img = holder["b"](c, x.clone(), Ident(), mask, rbp)
                img.backward(grad)

            row["reference_fwd"] = attempt(ref_fwd, args.iters)
            row["reference_fwd_bwd"] = attempt(ref_fwd_bwd, args.iters)
            holder.clear()
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
            row = {"case": f"SplatterPhongShader fwd+bwd N={N} {H}x{W} K={K}",
                   **shader_case(ref, verts, faces, p2f, zbuf, bary, dists, grad, d, args.iters)}
        print(json.dumps(row), flush=True)
        del p2f, zbuf, bary, dists, coords, colors, c, x, mask, grad
        torch.cuda.empty_cache()


def shader_case(shim, verts, faces, p2f, zbuf, bary, dists, grad, d, iters):
    """SplatterPhongShader forward + backward on the fragments, the reference's own code vs the patched forward."""
    from pytorch3d.renderer import (BlendParams, FoVOrthographicCameras, Materials, PointLights, SplatterPhongShader,
                                    TexturesVertex)
    from pytorch3d.renderer.mesh.rasterizer import Fragments
    from pytorch3d.structures import Meshes

    vl = [v.to(d).requires_grad_(True) for v in verts]
    fl = [f.to(d) for f in faces]
    frags = Fragments(pix_to_face=p2f, zbuf=zbuf, bary_coords=bary, dists=dists)
    kw = dict(cameras=FoVOrthographicCameras(device=d), lights=PointLights(device=d), materials=Materials(device=d),
              blend_params=BlendParams(sigma=0.5, background_color=(1.0, 1.0, 1.0)))
    out = {}
    for mode in ("reference", "patched"):
        if mode == "patched":
            shim.patch_reference_python()
        shader = SplatterPhongShader(device=d, **kw)

        def step():  # a Meshes per step: its cached normals belong to one graph
            meshes = Meshes(verts=vl, faces=fl, textures=TexturesVertex(verts_features=[torch.full_like(v, 0.7) for v in vl]))
            img = shader(frags, meshes)
            img.backward(grad)

        out[mode] = attempt(step, iters)
        if mode == "patched":
            out["patched"]["calls"] = {k: v for k, v in shim.PATCH_CALLS.items() if k.startswith("Splatter")}
            shim.uninstall_python_patches()
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    main()
