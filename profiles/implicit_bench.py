#!/usr/bin/env python
"""sample_pdf and the raymarchers on one MI355X: csrc/implicit.hip against what ran before it (output kept as
profiles/implicit_mi355x.txt).

    python profiles/implicit_bench.py [--out FILE]

Raymarching: 4096 rays x 64 and x 128 points and 65 536 rays x 192 points, C = 3, densities 1 - exp(-relu(noise)) as a NeRF makes
them.  `fused` is pytorch3d_amd.ea_raymarch_unchecked (one node, two kernels), `chain` the reference's chain as ATen runs it on the
same GPU (pytorch3d_amd.implicit.ea_raymarch_torch, the same ops as raymarching.py) -- forward alone and forward + backward.  Neither
side has the bounds warning (two host syncs: measured on its own as `bounds_check_ms`).
sample_pdf: 4096 and 65 536 rows x 63 bins x 64 and 128 samples; `fused` is the in-place operator on given uniforms, `python_twin` the
reference's sample_pdf_python with det=True (no draw on either side) from the staged reference package, absent when that is not there.
The two sides of a shape ALTERNATE call by call in one process; every shape is warmed; device events around each call; min / median
of REPS.  kernel_ms: the library's own per-kernel events (p3d_profile_enable) in a separate pass; they hold the gap between two
event records too, so a kernel of a few microseconds reads long: --trace runs one shape's fused side alone for a kernel trace taken
from outside (the end of the record).  share: the algorithmic bytes --
every input read once, every output written once -- over the kernel time, as a share of the 6.29 TB/s measured copy rate.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP, REPS, COPY_RATE = 5, 40, 6.29e12


def alternate(sides, reps):
    """{name: (min, median) ms} of the callables in `sides`, called in turn."""
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
    return {k: [round(min(v), 4), round(statistics.median(v), 4)] for k, v in ms.items()}


def kernel_ms(fn, names, reps=10):
    """Mean ms per launch of the library's kernels `names` while fn runs (its own pass: the events serialise the stream)."""
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
    return {n: round(snap[n][1] / snap[n][0], 5) for n in names if n in snap}


def reference_python_twin():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    root = next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "renderer", "implicit"))), None)
    if root is None:
        return None
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    shim.install(root)
    from pytorch3d.renderer.implicit.sample_pdf import sample_pdf_python

    return sample_pdf_python


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, help="ea:RAYS:POINTS or pdf:ROWS:SAMPLES: only the fused side of that shape, 3 + 20 times, for a "
                    "kernel trace taken from outside (rocprofv3 --kernel-trace --stats -- python profiles/implicit_bench.py --trace ...)")
    args = ap.parse_args()
    import torch

    from pytorch3d_amd import implicit

    if not torch.cuda.is_available():
        sys.exit("implicit_bench: no GPU (the numbers of this script are device times)")
    d = torch.device("cuda:0")
    if args.trace:
        kind, a, b = args.trace.split(":")
        a, b, gen = int(a), int(b), torch.Generator().manual_seed(7)
        if kind == "ea":
            dens = (1.0 - torch.exp(-torch.relu(torch.randn(a, b, 1, generator=gen)))).to(d).requires_grad_(True)
            feats, g_out = torch.rand(a, b, 3, generator=gen).to(d).requires_grad_(True), torch.randn(a, 4, generator=gen).to(d)
            run = lambda: torch.autograd.grad(implicit.ea_raymarch_unchecked(dens, feats), (dens, feats), g_out)
        else:
            bins, weights = torch.cumsum(torch.rand(a, 64, generator=gen), 1).to(d), torch.rand(a, 63, generator=gen).to(d)
            u = torch.rand(a, b, generator=gen).to(d)
            run = lambda: implicit.sample_pdf_op(bins, weights, u.clone(), 1e-5)  # (the clone is a kernel of its own in the trace)
        for _ in range(23):
            run()
        torch.cuda.synchronize()
        return
    lines = ["implicit rendering on %s, torch %s; WARMUP %d, REPS %d, sides alternating, device events; ms as [min, median]"
             % (torch.cuda.get_device_name(0), torch.__version__, WARMUP, REPS)]

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for N, P, C in ((4096, 64, 3), (4096, 128, 3), (65536, 192, 3)):
        gen = torch.Generator().manual_seed(7)
        dens = (1.0 - torch.exp(-torch.relu(torch.randn(N, P, 1, generator=gen)))).to(d)
        feats = torch.rand(N, P, C, generator=gen).to(d)
        g_out = torch.randn(N, C + 1, generator=gen).to(d)

        def both(fn):
            def run():
                x, y = dens.detach().requires_grad_(True), feats.detach().requires_grad_(True)
                torch.autograd.grad(fn(x, y), (x, y), g_out)
            return run

        sides = {"fused_fwd": lambda: implicit.ea_raymarch_unchecked(dens, feats), "chain_fwd": lambda: implicit.ea_raymarch_torch(dens, feats),
                 "fused_fwd_bwd": both(implicit.ea_raymarch_unchecked), "chain_fwd_bwd": both(implicit.ea_raymarch_torch)}
        for _ in range(WARMUP):
            for fn in sides.values():
                fn()
        torch.cuda.synchronize()
        rec = {"shape": "ea_raymarch %d rays x %d points, C = %d" % (N, P, C)}
        rec.update(alternate(sides, REPS))
        rec["bounds_check_ms"] = alternate({"check": lambda: implicit._check_density_bounds(dens)}, REPS)["check"]
        k = kernel_ms(sides["fused_fwd_bwd"], ("ea_raymarch_forward", "ea_raymarch_backward"))
        fwd_bytes, bwd_bytes = 4 * (N * P * (1 + C) + N * (C + 1)), 4 * (2 * N * P * (1 + C) + N * (C + 1))
        rec["kernel_ms"] = k
        rec["share_of_copy_rate"] = {"forward": round(fwd_bytes / (k["ea_raymarch_forward"] * 1e-3) / COPY_RATE, 3),
                                     "backward": round(bwd_bytes / (k["ea_raymarch_backward"] * 1e-3) / COPY_RATE, 3)}
        rec["speedup_median"] = {"fwd": round(rec["chain_fwd"][1] / rec["fused_fwd"][1], 2), "fwd_bwd": round(rec["chain_fwd_bwd"][1] / rec["fused_fwd_bwd"][1], 2)}
        emit(rec)

    twin = reference_python_twin()
    for B in (4096, 65536):
        for S in (64, 128):
            n = 63
            gen = torch.Generator().manual_seed(9)
            bins = torch.cumsum(torch.rand(B, n + 1, generator=gen), 1).to(d)
            weights = torch.rand(B, n, generator=gen).to(d)
            u = torch.linspace(0.0, 1.0, S, device=d).expand(B, S).contiguous()
            out = u.clone()

            def fused():
                out.copy_(u)  # (the operator is in place: the copy is timed with it, the twin builds its uniforms too)
                implicit.sample_pdf_op(bins, weights, out, 1e-5)

            sides = {"fused": fused}
            if twin is not None:
                sides["python_twin"] = lambda: twin(bins, weights, S, det=True)
            for _ in range(WARMUP):
                for fn in sides.values():
                    fn()
            torch.cuda.synchronize()
            rec = {"shape": "sample_pdf %d rows x %d bins x %d samples" % (B, n, S)}
            rec.update(alternate(sides, REPS))
            k = kernel_ms(fused, ("sample_pdf_lds",))
            rec["kernel_ms"] = k
            rec["share_of_copy_rate"] = round(4 * B * (2 * n + 1 + 2 * S) / (k["sample_pdf_lds"] * 1e-3) / COPY_RATE, 3)
            if twin is not None:
                rec["speedup_median"] = round(rec["python_twin"][1] / rec["fused"][1], 2)
            else:
                rec["python_twin"] = "not measured: the reference package is not staged"
            emit(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
