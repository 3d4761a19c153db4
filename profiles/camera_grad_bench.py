#!/usr/bin/env python
"""What a training step costs on one MI355X once a CAMERA parameter requires grad.  Only interfaces that
exist before and after the camera gradients were fused, so the same file runs on either commit and the two outputs are the
comparison (profiles/camera_grad_mi355x.txt).

    python profiles/camera_grad_bench.py [--warmup 5] [--steps 20] [--windows 5] [--out FILE]

  world          pytorch3d_amd.rasterize_meshes_world, both matrix stacks (64, 4, 4) leaves that require grad, forward + backward
                 to the matrices and the vertices: config 3 (tests/_util.hetero_batch, 64 meshes, 512^2, K = 8), a camera per mesh
  mesh_dropin    the reference's MeshRasterizer under shim.install(patch_python=True), FoVOrthographicCameras whose T (64, 3)
                 requires grad, the same batch, forward + backward to T and the vertices
  points_dropin  the reference's PointsRenderer(PointsRasterizer, AlphaCompositor), config 4 (1M points, 512^2, K = 10,
                 r = 0.01), T (1, 3) requires grad, forward + backward to T, the points and the features
The two drop-in steps need the staged reference package (oracle/_ref/reference_py or P3D_REFERENCE_ROOT) and say so when it is
absent.  Every step is a process of its own under `timeout`, and a step that fails ends the run (as `a && b && c` would).
Per step: ~0.4 s of the same work untimed, `warmup` steps, then `windows` windows of `steps` steps, each between a host clock
and a device synchronise; ms per step as median (min .. max) of the windows.  Then 5 steps with the library's own per-launch
events on: the transform kernels' time per launch.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = ("world", "mesh_dropin", "points_dropin")
STEP_LIMIT_S = 240


def reference_root():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    return next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "renderer"))), None)


def measure(name, step, args, extra):
    import torch

    from pytorch3d_amd import _lib

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.4:
        step()
        torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    windows = []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / args.steps * 1e3)
    lib = _lib.load()
    lib.p3d_profile_reset()
    lib.p3d_profile_enable(1)
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    lib.p3d_profile_enable(0)
    kern = {k: round(ms / n, 4) for k, (n, ms) in sorted(_lib.profile_snapshot().items()) if k.startswith("transform")}
    rec = {"case": name, "ms_per_step": round(statistics.median(windows), 4), "min_ms": round(min(windows), 4), "max_ms": round(max(windows), 4),
           "windows": args.windows, "steps_per_window": args.steps, "transform_kernels_ms_per_launch": kern}
    rec.update(extra())
    print(json.dumps(rec))


def config3(d):
    import torch

    import _util as U

    B, H, K = 64, 512, 8
    verts, faces = U.hetero_batch(B, seed=0, torus_div=U.CONFIG3_TORUS_DIV)
    gen = torch.Generator().manual_seed(231)
    g_z = torch.randn((B, H, H, K), generator=gen).to(d)
    g_b = torch.randn((B, H, H, K, 3), generator=gen).to(d)
    g_d = torch.randn((B, H, H, K), generator=gen).to(d)
    rs = dict(image_size=H, blur_radius=math.log(1.0 / 1e-4 - 1.0) * 1e-4, faces_per_pixel=K, perspective_correct=True,
              clip_barycentric_coords=True)
    return [v.to(d) for v in verts], [f.to(d) for f in faces], (g_z, g_b, g_d), rs


def install_shim():
    import run_reference_suite as rrs  # the iopath / imageio stubs the reference's package needs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    shim.install(reference_root(), patch_python=True)
    return shim


def run_step(name, args):
    if name != "world" and reference_root() is None:
        print(json.dumps({"case": name, "skipped": "the reference's Python package is not on this machine"}))
        return
    import torch

    d = torch.device("cuda:0")
    if name == "world":
        import pytorch3d_amd as p3d

        verts, faces, grads, rs = config3(d)
        B = len(verts)
        vl = [v.clone().requires_grad_(True) for v in verts]
        meshes = p3d.PackedMeshes(vl, faces)
        # the batch is generated in NDC (x, y, view depth): identity cameras, one pair per mesh
        w2v = torch.eye(4, device=d)[None].repeat(B, 1, 1).requires_grad_(True)
        v2n = torch.eye(4, device=d)[None].repeat(B, 1, 1).requires_grad_(True)

        def step():
            w2v.grad = v2n.grad = None
            for v in vl:
                v.grad = None
            out = p3d.rasterize_meshes_world(meshes, w2v, v2n, **rs)
            torch.autograd.backward([out[1], out[2], out[3]], list(grads))

        measure(name, step, args, lambda: {"grad_finite": bool(torch.isfinite(w2v.grad).all() and torch.isfinite(v2n.grad).all()),
                                           "grad_w2v_abs_max": float(w2v.grad.abs().max())})
    elif name == "mesh_dropin":
        shim = install_shim()
        from pytorch3d.renderer import FoVOrthographicCameras, MeshRasterizer, RasterizationSettings
        from pytorch3d.structures import Meshes

        verts, faces, grads, rs = config3(d)
        mesh0 = Meshes(verts=verts, faces=faces)
        deform = torch.zeros((int(mesh0.verts_packed().shape[0]), 3), device=d, requires_grad=True)  # (as profiles/dropin_timing.py)
        T = torch.zeros((len(verts), 3), device=d, requires_grad=True)
        rast = MeshRasterizer(cameras=FoVOrthographicCameras(T=T, device=d), raster_settings=RasterizationSettings(**rs))

        def step():
            T.grad = deform.grad = None
            frag = rast(mesh0.offset_verts(deform))
            torch.autograd.backward([frag.zbuf, frag.bary_coords, frag.dists], list(grads))

        measure(name, step, args, lambda: {"grad_finite": bool(torch.isfinite(T.grad).all()), "grad_T_abs_max": float(T.grad.abs().max()),
                                           "patched_calls": {k: list(v) for k, v in shim.PATCH_CALLS.items() if k.startswith("MeshRasterizer")}})
    else:
        shim = install_shim()
        from pytorch3d.renderer import AlphaCompositor, FoVOrthographicCameras, PointsRasterizationSettings, PointsRasterizer, PointsRenderer
        from pytorch3d.structures import Pointclouds

        P, H, K, r, C = 1_000_000, 512, 10, 0.01, 3
        gen = torch.Generator().manual_seed(0)
        pts = torch.cat([torch.rand(P, 2, generator=gen) * 2 - 1, torch.rand(P, 1, generator=gen) * 2 + 0.5], 1).to(d).requires_grad_(True)
        feats = torch.rand(P, C, generator=gen).to(d).requires_grad_(True)
        g_img = torch.randn((1, H, H, C), generator=gen).to(d)
        T = torch.zeros((1, 3), device=d, requires_grad=True)
        settings = PointsRasterizationSettings(image_size=H, radius=r, points_per_pixel=K, bin_size=None)
        renderer = PointsRenderer(rasterizer=PointsRasterizer(cameras=FoVOrthographicCameras(T=T, device=d), raster_settings=settings),
                                  compositor=AlphaCompositor())

        def step():
            T.grad = pts.grad = feats.grad = None
            (renderer(Pointclouds(points=[pts], features=[feats])) * g_img).sum().backward()

        measure(name, step, args, lambda: {"grad_finite": bool(torch.isfinite(T.grad).all()), "grad_T_abs_max": float(T.grad.abs().max()),
                                           "patched_calls": {k: list(v) for k, v in shim.PATCH_CALLS.items() if k.startswith("Points")}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--step", choices=STEPS, default=None, help="run this one step in this process")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        run_step(args.step, args)
        return
    lines = [f"# camera_grad_bench: {args.warmup} warm-up steps, {args.windows} windows of {args.steps} steps, host clock to device synchronise, "
             "ms per step as median (min .. max) of the windows"]
    status = 0
    for name in STEPS:  # one process per step, each under its own time limit; the first failure ends the run
        res = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", name, "--warmup",
                              str(args.warmup), "--steps", str(args.steps), "--windows", str(args.windows)], stdout=subprocess.PIPE, text=True, cwd=ROOT)
        lines += [line for line in res.stdout.splitlines() if line.startswith("{")]
        if res.returncode != 0:
            lines.append(f"# step {name} ended with status {res.returncode}: nothing more was started")
            status = res.returncode
            break
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    sys.exit(status)


if __name__ == "__main__":
    main()
