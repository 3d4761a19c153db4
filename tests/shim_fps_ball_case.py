#!/usr/bin/env python
"""The UNMODIFIED reference's `pytorch3d.ops.sample_farthest_points` / `pytorch3d.ops.ball_query` through pytorch3d_amd.shim, in a
process of its own (the shim replaces sys.modules entries).  argv[1]: "cuda" (default) or "cpu".  Prints one JSON line that
tests/test_gpu_fps_ball.py / tests/test_cpu_fps_ball.py read:
* plain install(): the reference's own functions run on `_C.sample_farthest_points` / `_C.ball_query` and give the golden of
  tests/golden/fps_ball_ref.npz; the reference's ball-query backward meets the `_C.knn_points_backward` stub;
* patch_python=True: every module that holds the names sees the new functions, the golden again, gradients flow, PATCH_CALLS shows
  what ran, and a PointNet++ set-abstraction step (sampling, then a ball query around the samples with return_nn) equals the
  package's torch formulation on the CPU;
* uninstall_python_patches() gives the reference's functions back."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MODULES = {"sample_farthest_points": ("pytorch3d.ops.sample_farthest_points", "pytorch3d.ops"),
           "ball_query": ("pytorch3d.ops.ball_query", "pytorch3d.ops")}


def _reference_root():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    return next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "ops"))), None)


def main():
    ref_root = _reference_root()
    if ref_root is None:
        print(json.dumps({"skipped": "the reference's Python package is not on this machine"}))
        return
    import importlib

    import torch

    import fps_ball_case as C
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    d = torch.device(sys.argv[1] if len(sys.argv) > 1 else "cuda:0")
    z = C.fixture()
    out = {}

    def dev(t):
        return None if t is None else t.to(d)

    def golden(fps, ball):
        """Both functions on every case of the fixture: (all indices equal, largest distance error beyond 2e-6 relative)."""
        same, err = True, 0.0
        for name, _, _, _, lengths, K in C.FPS_RANDOM:
            pts = z["fps/%s/points" % name].to(d)
            sel, idx = fps(pts, dev(C.lengths_tensor(lengths)), K if isinstance(K, int) else dev(C.k_arg(K)))
            same = same and torch.equal(idx.cpu(), z["fps/%s/idx" % name]) and torch.equal(sel.cpu(), z["fps/%s/sel" % name])
        for name in C.FPS_LATTICE:
            sel, idx = fps(z["fps/%s/points" % name].to(d), None, C.FPS_LATTICE_K[name])
            same = same and torch.equal(idx.cpu(), z["fps/%s/idx" % name]) and torch.equal(sel.cpu(), z["fps/%s/sel" % name])
        cases = [(n, l1, l2, K, r) for n, _, _, _, _, l1, l2, Ks, r in C.BALL_RANDOM for K in Ks]
        cases.append(("lattice", None, None, C.BALL_LATTICE_K, C.BALL_LATTICE_RADIUS))
        for name, l1, l2, K, radius in cases:
            res = ball(z["ball/%s/p1" % name].to(d), z["ball/%s/p2" % name].to(d), dev(C.lengths_tensor(l1)), dev(C.lengths_tensor(l2)),
                       K=K, radius=radius)
            want_i, want_d = z["ball/%s/idx/%d" % (name, K)], z["ball/%s/dists/%d" % (name, K)]
            same = same and torch.equal(res.idx.cpu(), want_i)
            err = max(err, float(((res.dists.detach().cpu() - want_d).abs() - 2e-6 * want_d.abs()).max()))
        return bool(same), err

    def calls():
        return {n: list(shim.PATCH_CALLS.get(n, [0, 0])) for n in MODULES}

    # ---- plain install: the reference's own Python on the shim's operators ---------------------------------------------------------
    shim.install(ref_root)
    import pytorch3d.ops as ref_ops

    orig = {n: getattr(importlib.import_module(ms[0]), n) for n, ms in MODULES.items()}
    out["unpatched_is_the_reference"] = not any(getattr(f, "__p3d_amd__", False) for f in orig.values())
    out["plain_golden_equal"], out["plain_golden_dists_error"] = golden(ref_ops.sample_farthest_points, ref_ops.ball_query)
    p1 = z["ball/ragged3/p1"].to(d).requires_grad_(True)
    p2 = z["ball/ragged3/p2"].to(d).requires_grad_(True)
    res = ref_ops.ball_query(p1, p2, K=5, radius=0.2)
    try:
        res.dists.sum().backward()
        out["plain_backward_meets_the_stub"] = False
    except NotImplementedError:
        out["plain_backward_meets_the_stub"] = True
    out["calls_before_patch"] = sum(sum(v) for v in calls().values())

    # ---- patch_python ----------------------------------------------------------------------------------------------------------------
    shim.install(ref_root, patch_python=True)
    from pytorch3d.ops import ball_query, sample_farthest_points

    out["patched_everywhere"] = bool(all(getattr(getattr(sys.modules[m], n), "__p3d_amd__", False) for n, ms in MODULES.items() for m in ms)
                                     and sample_farthest_points.__wrapped__ is orig["sample_farthest_points"]
                                     and ball_query.__wrapped__ is orig["ball_query"])
    before = calls()
    out["patched_golden_equal"], out["patched_golden_dists_error"] = golden(sample_farthest_points, ball_query)
    # a set-abstraction step of PointNet++: sample, then group the cloud around the samples
    gen = torch.Generator().manual_seed(5)
    cloud_cpu = torch.rand(3, 700, 3, generator=gen)
    lengths_cpu = torch.tensor([700, 333, 64])
    cloud = cloud_cpu.to(d).requires_grad_(True)
    centres, centre_idx = sample_farthest_points(cloud, lengths_cpu.to(d), K=48)
    groups = ball_query(centres, cloud, lengths1=None, lengths2=lengths_cpu.to(d), K=16, radius=0.25, return_nn=True)
    (groups.dists.sum() + groups.knn.sum()).backward()
    after = calls()
    # (importlib: the package re-exports the functions over the sub-modules of the same names)
    fps_mod = importlib.import_module("pytorch3d_amd.sample_farthest_points")
    ball_mod = importlib.import_module("pytorch3d_amd.ball_query")
    want_idx = fps_mod.torch_sample_farthest_points(cloud_cpu, lengths_cpu, None, None, 48)
    want_centres = fps_mod.masked_gather(cloud_cpu, want_idx)
    want_gi, want_gd = ball_mod.torch_ball_query_forward(want_centres, cloud_cpu, None, lengths_cpu, 16, 0.25)
    out["set_abstraction_equal"] = bool(torch.equal(centre_idx.cpu(), want_idx) and torch.equal(centres.detach().cpu(), want_centres)
                                        and torch.equal(groups.idx.cpu(), want_gi) and torch.equal(groups.dists.detach().cpu(), want_gd)
                                        and torch.equal(groups.knn.detach().cpu(), fps_mod.masked_gather(cloud_cpu, want_gi)))
    out["set_abstraction_grad_finite"] = bool(cloud.grad is not None and torch.isfinite(cloud.grad).all() and cloud.grad.abs().sum() > 0)
    out["fused_calls"] = {n: after[n][0] - before[n][0] for n in MODULES}
    out["fallback_calls"] = {n: after[n][1] - before[n][1] for n in MODULES}

    # ---- restore ---------------------------------------------------------------------------------------------------------------------
    shim.uninstall_python_patches()
    out["restored"] = bool(all(getattr(sys.modules[m], n) is orig[n] for n, ms in MODULES.items() for m in ms))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
