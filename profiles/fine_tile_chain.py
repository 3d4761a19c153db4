#!/usr/bin/env python
"""Where an active tile's wave spends its life in mesh_fine, on the bench launch (BASELINE configs[2]).

    python profiles/ab_variant.py probe -DP3D_PROBE_CHAIN          (a library of its own, never the product)
    python profiles/fine_tile_chain.py pytorch3d_amd/libp3d_probe.so [--iters 5]

The probe build (csrc/raster_mesh.hip: P3D_PROBE_CHAIN) notes the shader clock of lane 0 of every wave of one workgroup in eight
(single-chunk tiles of the plan walk) at eleven points and adds the length of each phase to a small device buffer.  This script runs
the forward of the bench launch on that library, reads the buffer (p3d_probe_chain_read) and prints, per phase, the number of waves
that passed it, their mean time in it and its share of the wave's life.  The dependent global round trips of the head are the
phases "list indices" (one trip: the list) and "vertices" (one trip: the gather).
"""
import argparse
import ctypes
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

PHASES = ["entry", "CSR row known (flag, header, order; total, offset)", "list indices arrived", "vertices arrived", "staging published",
          "order done", "evaluation done", "past the trailing barrier", "pixel stores issued", "background rows known", "exit (fill issued)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib")
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()

    import _util as U
    import pytorch3d_amd as p3d
    from exp_measure import open_lib

    lib = open_lib(os.path.abspath(args.lib))
    lib.p3d_probe_chain_read.restype = None
    lib.p3d_probe_chain_read.argtypes = [ctypes.POINTER(ctypes.c_ulonglong)]
    d = torch.device("cuda:0")
    B, H, K = 64, 512, 8
    blur = math.log(1.0 / 1e-4 - 1.0) * 1e-4
    verts, faces = U.hetero_batch(B, seed=0, torus_div=1.0)
    m = p3d.PackedMeshes([v.to(d) for v in verts], [f.to(d) for f in faces])
    fv = m.verts_packed()[m.faces_packed()].contiguous()
    F = int(fv.shape[0])
    first, count = m.mesh_to_faces_packed_first_idx().contiguous(), m.num_faces_per_mesh().contiguous()
    nbr = torch.full((F,), -1, dtype=torch.int64, device=d)
    bin_size, M = 32, int(max(10000, F / 5))
    out = (torch.empty((B, H, H, K), dtype=torch.int64, device=d), torch.empty((B, H, H, K), device=d),
           torch.empty((B, H, H, K, 3), device=d), torch.empty((B, H, H, K), device=d))
    cover = torch.empty((B, H // 16, H // 16), dtype=torch.int32, device=d)
    ws = torch.empty((int(lib.p3d_rasterize_meshes_workspace_bytes(F, B, H, H, bin_size, M)),), dtype=torch.uint8, device=d)
    stream = ctypes.c_void_p(torch.cuda.current_stream(d).cuda_stream)

    def run():
        rc = lib.p3d_rasterize_meshes_ex(fv.data_ptr(), first.data_ptr(), count.data_ptr(), nbr.data_ptr(), F, B, H, H, blur, K, bin_size, M,
                                         1, 1, 0, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                                         cover.data_ptr(), 0, ws.data_ptr(), ws.numel(), stream)
        assert rc == 0, rc

    buf = (ctypes.c_ulonglong * 32)()
    run()
    torch.cuda.synchronize()
    lib.p3d_probe_chain_read(buf)  # (reads and clears: the warm-up does not count)
    for _ in range(args.iters):
        run()
    torch.cuda.synchronize()
    lib.p3d_probe_chain_read(buf)
    v = list(buf)
    waves, ticks = v[31], v[15]  # wave lives on the constant 100 MHz clock
    cyc = sum(v[1:11])
    if waves == 0 or ticks == 0:
        raise SystemExit("the probe counted nothing: is this a -DP3D_PROBE_CHAIN library?")
    mhz = cyc / ticks * 100.0
    print(f"probed waves {waves} ({args.iters} launches), mean life {cyc / waves:.0f} shader clocks = {ticks / waves / 100.0:.2f} us "
          f"(shader clock {mhz:.0f} MHz)")
    print(f"{'phase (time since the point before)':<52}{'waves':>9}{'clocks':>10}{'us':>8}{'share':>8}")
    for i in range(1, 11):
        n = v[16 + i]
        mean = v[i] / n if n else 0.0
        # share of the mean life: a phase that only some waves pass counts by how many did
        print(f"{PHASES[i]:<52}{n:>9}{mean:>10.0f}{mean / mhz:>8.2f}{100.0 * v[i] / cyc:>7.1f}%")


if __name__ == "__main__":
    main()
