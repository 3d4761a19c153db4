#!/usr/bin/env python
"""knn_points on feature clouds on one MI355X: csrc/knn_features.hip against what the same call ran before it existed, this package's
torch formulation (knn.torch_knn_forward / torch_knn_backward), on the same GPU in the same process (output kept as
profiles/knn_features_mi355x.txt).

    python profiles/knn_features_bench.py [--out FILE]       the driver: every shape below in a child process of its own
    python profiles/knn_features_bench.py --step NAME         one shape, in this process

The driver runs each shape under its own time limit and stops at the first one that fails or runs out of time; it reads nothing
outside the repository.  Normal noise, the public knn_points, forward and forward + backward to both clouds; the formulation leg is
forced by switching knn.feature_kernel_path off.  Device events around each call, warm-up iterations untimed, the legs alternating,
medians.  Before any timing the two legs' idx and dists are compared with torch.equal on the timed inputs.

Beside each time: the forward kernel's own time (the library's p3d_profile_* timing, separate untimed iterations) against the issue
bound of its matrix instructions -- ceil(D / 2) v_mfma_f32_32x32x2_f32 per 32 x 32 block of pairs, 16 passes of 4 cycles each, on 4 x
256 SIMDs at CLOCK_GHZ -- and the share of pairs that pass the screen.  That share is NOT a counter of the kernel: it is the screen
restated in torch (float32 matmul for the cross term, the kernel's bound E, the worst neighbour as it stands at the start of each
tile of 32 targets) on the first 128 queries of the first cloud.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIMDS = 4 * 256
CLOCK_GHZ = 2.4
QUEUES = (1, 2, 4, 8, 16, 20, 32)  # the register queues of the kernel: K rounds up to one of them

# name: (time limit in seconds, N, P, D, K, timed iterations of the formulation leg)
STEPS = {
    "edgeconv_d64": (300, 8, 4096, 64, 20, 3),
    "edgeconv_d128": (300, 8, 4096, 128, 20, 3),
    "edgeconv_d256": (400, 8, 4096, 256, 20, 3),
    "one_cloud_d32": (300, 1, 10000, 32, 8, 3),
    "batch64_d64": (300, 64, 1024, 64, 16, 3),
}


def screen_share(x, y, K):
    """The share of (query, target) pairs of x (Q, D), y (P, D) that the screen lets through: see the module docstring."""
    import torch

    D = x.shape[1]
    kq = next(q for q in QUEUES if q >= K)
    exact = ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    total = x.square().sum(1)[:, None] + y.square().sum(1)[None, :]
    s = total - 2.0 * (x @ y.t())
    bound = (8 * D + 24) * 2.0 ** -24 * total + 2.0 ** -100
    passed = 0
    for j0 in range(0, y.shape[0], 32):
        worst = exact[:, :j0].kthvalue(kq, dim=1).values[:, None] if j0 >= kq else torch.full_like(exact[:, :1], float("inf"))
        passed += int((~(s[:, j0:j0 + 32] - bound[:, j0:j0 + 32] > worst)).sum())
    return passed / exact.numel()


def run_step(name):
    import torch

    import pytorch3d_amd as p3d
    from pytorch3d_amd import _lib
    from pytorch3d_amd import knn as knn_mod

    _, N, P, D, K, base_iters = STEPS[name]
    d = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    x0, y0 = torch.randn(N, P, D, generator=gen).to(d), torch.randn(N, P, D, generator=gen).to(d)
    path = knn_mod.feature_kernel_path

    def step_of(fused, backward):
        def step():
            knn_mod.feature_kernel_path = path if fused else (lambda *a: False)
            try:
                if not backward:
                    return p3d.knn_points(x0, y0, K=K)
                x, y = x0.clone().requires_grad_(True), y0.clone().requires_grad_(True)
                p3d.knn_points(x, y, K=K).dists.sum().backward()
            finally:
                knn_mod.feature_kernel_path = path
        return step

    ours, base = step_of(True, False)(), step_of(False, False)()
    same = bool(torch.equal(ours.idx, base.idx) and torch.equal(ours.dists, base.dists))
    out = {"step": name, "N": N, "P": P, "D": D, "K": K, "same_bits": same, "legs": {}}
    for label, backward in (("forward", False), ("forward + backward", True)):
        legs = {"kernels": step_of(True, backward), "torch formulation": step_of(False, backward)}
        times = {k: [] for k in legs}
        for i in range(2 + 20):
            for leg, step in legs.items():
                if leg != "kernels" and i >= 2 + base_iters:
                    continue
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                step()
                b.record()
                b.synchronize()
                if i >= 2:
                    times[leg].append(a.elapsed_time(b))
        out["legs"][label] = {k: {"median": statistics.median(t), "min": min(t), "max": max(t), "iters": len(t)} for k, t in times.items()}
    lib = _lib.load()
    lib.p3d_profile_reset()
    lib.p3d_profile_enable(1)
    try:
        for _ in range(5):
            step_of(True, True)()
        torch.cuda.synchronize()
        snap = _lib.profile_snapshot()
    finally:
        lib.p3d_profile_enable(0)
    out["kernels"] = {k: [n, ms / n] for k, (n, ms) in sorted(snap.items())}
    blocks = N * -(-P // 32) * -(-P // 32)
    out["mfma_bound_ms"] = blocks * -(-D // 2) * 16 * 4 / (SIMDS * CLOCK_GHZ * 1e9) * 1e3
    out["screen_share"] = screen_share(x0[0, :128], y0[0], K)
    print(json.dumps(out))


def report(rec):
    lines = [f"{rec['step']}: {rec['N']} x {rec['P']} x {rec['P']}, D = {rec['D']}, K = {rec['K']}; idx and dists of the two legs "
             f"{'bit-equal' if rec['same_bits'] else 'DIFFER'}; ms per call: median (min .. max) [timed iterations]"]
    for label, legs in rec["legs"].items():
        for leg, t in legs.items():
            lines.append(f"  {label + ', ' + leg:<40s} {t['median']:10.3f}  ({t['min']:.3f} .. {t['max']:.3f}) [{t['iters']}]")
        lines.append(f"  {label + ', torch / kernels':<40s} {legs['torch formulation']['median'] / legs['kernels']['median']:10.1f} x")
    lines.append("  per launch (ms, mean of the launches of 5 forward + backward calls):")
    for k, (n, ms) in rec["kernels"].items():
        lines.append(f"    {k:<36s} {ms:9.4f}  x{n // 5} per call")
    fwd = rec["kernels"]["knn_features_forward"][1]
    lines.append(f"  forward kernel {fwd:.4f} ms; the issue bound of its matrix instructions ({SIMDS} SIMDs, {CLOCK_GHZ} GHz) is "
                 f"{rec['mfma_bound_ms']:.4f} ms: the launch takes {fwd / rec['mfma_bound_ms']:.2f} of it")
    lines.append(f"  share of pairs that pass the screen (restated in torch, 128 queries of cloud 0): {100 * rec['screen_share']:.2f} %")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=sorted(STEPS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        run_step(args.step)
        return
    lines = ["knn_points on feature clouds: csrc/knn_features.hip against the package's torch formulation on the same GPU"]
    for name, (limit, *_rest) in STEPS.items():
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append(f"{name}: no result within {limit} s; stopped here")
            break
        if res.returncode != 0:
            lines.append(f"{name}: exit status {res.returncode}; stopped here\n{res.stderr[-2000:]}")
            break
        lines += report(json.loads(res.stdout.strip().splitlines()[-1]))
        print("\n".join(lines[-14:]), flush=True)
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
