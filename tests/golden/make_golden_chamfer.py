"""Golden fixture for knn_points / chamfer_distance, generated FROM THE REFERENCE's own code on the CPU (build container only).

    python tests/golden/make_golden_chamfer.py   ->  tests/golden/chamfer_ref.npz

* idx / dists: the reference's naive nearest neighbours (its tests/test_knn.py: TestKNN._knn_points_naive) on the shapes of
  tests/chamfer_case.py: KNN_CASES, for every K and norm listed there.
* losses and gradients: the reference's pytorch3d.loss.chamfer_distance on CHAMFER_CASES -- every reduction pair, weights (also all
  zero), normals with abs_cosine both ways, single_directional, norm 1 and 2, a Pointclouds batch with an empty cloud.  For this
  process `chamfer.knn_points` is bound to "the naive indices + the reference's knn_gather + torch arithmetic", so that autograd
  differentiates the distances; nothing of pytorch3d_amd is in the loop.  The gradients are those of chamfer_case.scalarise(result).

The generator asserts that in every recorded case the relative gap between consecutive distances among each query's first
min(K, len2) + 1 neighbours is >= 1e-5 (more than 8 x the (D + 2) 2^-24 rounding of one distance for D <= 8): under that condition
an implementation in float32 must reproduce idx bit for bit.  SEED was picked so.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 4  # of the seeds 0 .. 4 the one with the largest smallest gap (1.6e-5); 0 and 3 miss the condition


def draw(seed):
    """Every input of the fixture from one generator: clouds in the unit cube scaled per cloud, unit normals."""
    import chamfer_case as C

    gen = torch.Generator().manual_seed(seed)
    out = {}
    for name, N, P1, P2, D, _, _, _, _ in C.KNN_CASES:
        out[C.knn_key(name, "p1")] = torch.rand(N, P1, D, generator=gen) * 2 - 1
        out[C.knn_key(name, "p2")] = torch.rand(N, P2, D, generator=gen) * 2 - 1
    for name, (N, P1, P2, D, _, _) in C.CHAMFER_CLOUDS.items():
        out["clouds/%s/x" % name] = torch.rand(N, P1, D, generator=gen) * 2 - 1
        out["clouds/%s/y" % name] = torch.rand(N, P2, D, generator=gen) * 2 - 1 + 0.1
        for key, P in (("xn", P1), ("yn", P2)):
            v = torch.randn(N, P, D, generator=gen)
            out["clouds/%s/%s" % (name, key)] = v / v.norm(dim=2, keepdim=True)
    return out


def smallest_gap_of(inputs):
    import chamfer_case as C

    worst = float("inf")
    for name, N, P1, P2, D, l1, l2, Ks, norms in C.KNN_CASES:
        for norm in norms:
            worst = min(worst, C.smallest_gap(inputs[C.knn_key(name, "p1")], inputs[C.knn_key(name, "p2")], l1, l2, max(Ks), norm))
    for name, (N, P1, P2, D, l1, l2) in C.CHAMFER_CLOUDS.items():
        x, y = inputs["clouds/%s/x" % name], inputs["clouds/%s/y" % name]
        for norm in (1, 2):
            worst = min(worst, C.smallest_gap(x, y, l1, l2, 1, norm), C.smallest_gap(y, x, l2, l1, 1, norm))
    return worst


def main():
    import chamfer_case as C
    import make_golden as mg

    mg.bind_reference()
    import importlib.util

    import pytorch3d.loss.chamfer as ref_chamfer
    import pytorch3d.ops.knn as ref_knn
    from pytorch3d.structures import Pointclouds

    # the reference's tests are a package of their own (relative imports): loaded under a name that cannot meet this repository's tests/
    ref_tests = os.path.join(mg.REFERENCE, "tests")
    spec = importlib.util.spec_from_file_location("p3d_reference_tests", os.path.join(ref_tests, "__init__.py"),
                                                  submodule_search_locations=[ref_tests])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules["p3d_reference_tests"] = pkg
    spec.loader.exec_module(pkg)
    TestKNN = importlib.import_module("p3d_reference_tests.test_knn").TestKNN

    inputs = draw(SEED)
    gap = smallest_gap_of(inputs)
    print("smallest relative gap between consecutive distances: %.3g" % gap)
    assert gap >= C.MIN_GAP, "pick another SEED"
    out = dict(inputs)

    for name, N, P1, P2, D, l1, l2, Ks, norms in C.KNN_CASES:
        p1, p2 = inputs[C.knn_key(name, "p1")], inputs[C.knn_key(name, "p2")]
        for K in Ks:
            for norm in norms:
                res = TestKNN._knn_points_naive(p1, p2, C.lengths_tensor(l1), C.lengths_tensor(l2), K, norm)
                out[C.knn_key(name, "idx", K, norm)], out[C.knn_key(name, "dists", K, norm)] = res.idx, res.dists

    def knn_points_by_autograd(p1, p2, lengths1=None, lengths2=None, norm=2, K=1, **_):
        naive = TestKNN._knn_points_naive(p1.detach(), p2.detach(), lengths1, lengths2, K, norm)
        near = ref_knn.knn_gather(p2, naive.idx, lengths2)
        diff = p1[:, :, None, :] - near
        d = (diff * diff).sum(3) if norm == 2 else diff.abs().sum(3)
        valid = C.valid_mask(lengths1, lengths2, p1.shape[0], p1.shape[1], p2.shape[1], K)
        return ref_knn._KNN(dists=d * valid.to(d.dtype), idx=naive.idx, knn=None)

    ref_chamfer.knn_points = knn_points_by_autograd
    for name, clouds, normals, weights, as_objects, _ in C.CHAMFER_CASES:
        x, y, (ax, ay), kw = C.chamfer_inputs_from(inputs, name)
        if as_objects:
            def listed(c):
                n = [int(v) for v in c.num_points_per_cloud()]
                pts = [c.points_padded()[i, :k] for i, k in enumerate(n)]
                nrm = None if c.normals_padded() is None else [c.normals_padded()[i, :k] for i, k in enumerate(n)]
                return Pointclouds(points=pts, normals=nrm)

            ax, ay = listed(ax), listed(ay)
        result = ref_chamfer.chamfer_distance(ax, ay, **kw)
        gx, gy = torch.autograd.grad(C.scalarise(result), (x, y), allow_unused=True)
        for i, t in enumerate(C.flatten(result)):
            out[C.cham_key(name, "out%d" % i)] = t
        out[C.cham_key(name, "has_normals")] = torch.tensor(result[1] is not None)
        out[C.cham_key(name, "grad_x")] = gx if gx is not None else torch.zeros_like(x)
        out[C.cham_key(name, "grad_y")] = gy if gy is not None else torch.zeros_like(y)
        print(name, [tuple(t.shape) for t in C.flatten(result)])

    arrays = {k: v.detach().cpu().numpy() for k, v in out.items()}
    np.savez_compressed(C.FIXTURE, **arrays)
    print("wrote", C.FIXTURE, os.path.getsize(C.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
