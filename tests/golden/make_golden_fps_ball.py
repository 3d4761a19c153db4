"""Golden fixture for sample_farthest_points / ball_query, generated FROM THE REFERENCE's own code on the CPU (build container only).

    python tests/golden/make_golden_fps_ball.py   ->  tests/golden/fps_ball_ref.npz

* fps/<case>/idx, sel: the reference's pytorch3d.ops.sample_farthest_points.sample_farthest_points_naive on the clouds of
  tests/fps_ball_case.py: FPS_RANDOM (start index 0) and on the lattice clouds FPS_LATTICE.
* ball/<case>/idx/<K>, dists/<K>: the reference's naive ball query (its tests/test_ball_query.py: TestBallQuery._ball_query_naive)
  on BALL_RANDOM and on the lattice case.
Nothing of pytorch3d_amd is in the loop.

The generator asserts, and SEED was picked so, that
* in the random FPS cases, at every step the largest and the second-largest minimum distance differ by a relative 1e-5 or more,
* in the random ball cases no pair has |dist2 - radius2| <= 1e-5 radius2:
under those conditions an implementation in float32 must reproduce the indices bit for bit.  The lattice cases carry no such
condition: integer coordinates with |c| <= 64 make every float32 operation exact.  They have ties at most steps (FPS: the lowest
index must win, and a cloud of coinciding points repeats index 0) and points at distance exactly `radius` (ball query: no hits).
"""
import importlib
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 0  # the first seed tried meets both conditions (smallest gaps 1.0e-3 and 7.7e-4)


def gaps(inputs, fps_idx):
    import fps_ball_case as C

    fps = min(C.fps_smallest_gap(inputs["fps/%s/points" % name], lengths, K, fps_idx[name]) for name, _, _, _, lengths, K in C.FPS_RANDOM)
    ball = min(C.ball_smallest_gap(inputs["ball/%s/p1" % name], inputs["ball/%s/p2" % name], l1, l2, radius)
               for name, _, _, _, _, l1, l2, _, radius in C.BALL_RANDOM)
    return fps, ball


def main():
    import fps_ball_case as C
    import make_golden as mg

    mg.bind_reference()
    from pytorch3d.ops.sample_farthest_points import sample_farthest_points_naive

    # the reference's tests are a package of their own (relative imports): loaded under a name that cannot meet this repository's tests/
    ref_tests = os.path.join(mg.REFERENCE, "tests")
    spec = importlib.util.spec_from_file_location("p3d_reference_tests", os.path.join(ref_tests, "__init__.py"),
                                                  submodule_search_locations=[ref_tests])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules["p3d_reference_tests"] = pkg
    spec.loader.exec_module(pkg)
    naive_ball = importlib.import_module("p3d_reference_tests.test_ball_query").TestBallQuery._ball_query_naive

    inputs = C.draw(SEED)
    out = dict(inputs)
    fps_idx = {}
    for name, N, P, D, lengths, K in C.FPS_RANDOM:
        sel, idx = sample_farthest_points_naive(inputs["fps/%s/points" % name], C.lengths_tensor(lengths), C.k_arg(K))
        fps_idx[name] = idx
        out["fps/%s/idx" % name], out["fps/%s/sel" % name] = idx, sel
    fps_gap, ball_gap = gaps(inputs, fps_idx)
    print("smallest relative gap: fps %.3g, ball %.3g" % (fps_gap, ball_gap))
    assert fps_gap >= C.MIN_GAP and ball_gap >= C.MIN_GAP, "pick another SEED"

    lattice = C.lattice_clouds()
    for name in C.FPS_LATTICE:
        sel, idx = sample_farthest_points_naive(lattice[name], None, C.FPS_LATTICE_K[name])
        out["fps/%s/points" % name], out["fps/%s/idx" % name], out["fps/%s/sel" % name] = lattice[name], idx, sel
        print(name, idx[0, -8:].tolist())

    for name, N, P1, P2, D, l1, l2, Ks, radius in C.BALL_RANDOM:
        for K in Ks:
            res = naive_ball(inputs["ball/%s/p1" % name], inputs["ball/%s/p2" % name], C.lengths_tensor(l1), C.lengths_tensor(l2), K, radius)
            out["ball/%s/idx/%d" % (name, K)], out["ball/%s/dists/%d" % (name, K)] = res.idx, res.dists
            hits = (res.idx >= 0).sum(2)
            print(name, K, "hits per row: min %d max %d" % (int(hits.min()), int(hits.max())))
    res = naive_ball(lattice["ball_p1"], lattice["ball_p2"], None, None, C.BALL_LATTICE_K, C.BALL_LATTICE_RADIUS)
    out["ball/lattice/p1"], out["ball/lattice/p2"] = lattice["ball_p1"], lattice["ball_p2"]
    out["ball/lattice/idx/%d" % C.BALL_LATTICE_K], out["ball/lattice/dists/%d" % C.BALL_LATTICE_K] = res.idx, res.dists
    print("lattice hits per row", (res.idx >= 0).sum(2)[0].tolist())

    arrays = {k: v.detach().cpu().numpy() for k, v in out.items()}
    np.savez_compressed(C.FIXTURE, **arrays)
    print("wrote", C.FIXTURE, os.path.getsize(C.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
