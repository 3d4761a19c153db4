"""The machinery of tests/test_gpu_loss_kernel_edges.py, proved on the CPU.

  1. The generated cases of that file with the package's float32 torch formulation (which CPU tensors take) in place of the kernels:
     the generators, the admission caps and the gates hold for a correct implementation.  Of the two shapes of the grid-stride part
     the nearest-neighbour one (1 048 876 queries against 8 targets) runs here too; the large mesh (1025 x 1025 vertices) does not --
     the float32 formulation of the four losses alone takes some ten seconds on a CPU -- and is replaced by the same generator at
     33 x 33.
  2. The vectorised float64 restatements the large shapes need against the brute-force ones on the existing small batches.
  3. The gates are not vacuous: five deliberately wrong answers, each of which must be rejected.
"""
import pytest
import torch

import chamfer_case as C


def _formulation(p1, p2, l1, l2, norm, K):
    from pytorch3d_amd import knn as knn_mod

    return knn_mod.torch_knn_forward(p1, p2, C.lengths_tensor(l1), C.lengths_tensor(l2), norm, K)


def _valid(shape, D, K):
    p1, p2, l1, l2 = C.edge_clouds(shape, D)
    return C.valid_mask(l1, l2, p1.shape[0], p1.shape[1], p2.shape[1], K)


# ---- A. every rung, ragged over tile and wave edges -------------------------------------------------------------------------------------
def test_the_generated_clouds_are_what_the_cases_need():
    for (shape, D) in [(s, d) for s in C.EDGE_SHAPES for d in (3, 2)]:
        p1, p2, l1, l2 = C.edge_clouds(shape, D)
        N, P1, P2, _, _ = C.EDGE_SHAPES[shape]
        assert p1.shape == (N, P1, D) and p2.shape == (N, P2, D)
        for n in range(N):
            assert bool(torch.isnan(p1[n, l1[n]:]).all()) and not bool(torch.isnan(p1[n, :l1[n]]).any())
            if l2[n] < P2:  # the decoys: every live query would find distance 0 past the length, up to the number of decoys
                assert torch.equal(p2[n, l2[n]], p1[n, 0])
    # one launch whose clouds scan 3, 1, 2 and 1 tiles; lengths2 on the tile edge and one to either side while P2 is larger
    assert [-(-l // C.TILE) for l in C.EDGE_SHAPES["rungs"][4]] == [3, 1, 2, 1] and C.EDGE_SHAPES["rungs"][2] == 2 * C.TILE + 6
    # K > lengths2 on the rungs 8, 16 and 32
    assert all(any(l < K for l in C.EDGE_SHAPES["short"][4]) for K in (8, 9, 16, 17, 32))
    assert {K for K in C.EDGE_KS if 9 <= K <= 16} == {9, 15, 16}


@pytest.mark.parametrize("K", C.EDGE_KS)
@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("D", [3, 2])
@pytest.mark.parametrize("shape", list(C.EDGE_SHAPES))
def test_formulation_passes_the_forward_contract_on_every_rung(shape, D, norm, K):
    p1, p2, l1, l2 = C.edge_clouds(shape, D)
    want_idx, want_d, ok, live = C.edge_truth(shape, D, norm, K)
    idx, dists = _formulation(p1, p2, l1, l2, norm, K)
    C.check_knn_forward("formulation %s D%d norm%d K%d" % (shape, D, norm, K), idx, dists, want_idx, want_d, ok, live, _valid(shape, D, K))


def test_the_vectorised_brute_force_equals_brute64_on_the_short_shape():
    for D in (3, 2):
        p1, p2, l1, l2 = C.edge_clouds("short", D)
        for norm in (2, 1):
            for K in C.EDGE_KS:
                want_idx, want_d, ok, live = C.edge_truth("short", D, norm, K)
                idx, dists, ok_v = C.brute64_device(p1, p2, l1, l2, K, norm)
                # rows past lengths1 hold NaN in p1: the vectorised pass sorts them too, the mask zeroes them
                assert torch.equal(idx, want_idx) and torch.equal(dists, want_d) and torch.equal(ok_v, ok), (D, norm, K)
    # and the admission, per query, is the rule smallest_gap states for a case: all admitted <=> the case's smallest gap >= MIN_GAP
    p1, p2, l1, l2 = C.edge_clouds("short", 3)
    for K in (1, 8, 32):
        ok = C.edge_truth("short", 3, 2, K)[2]
        live = C.live_rows(l1, 3, 70)
        assert bool(ok[live].all()) == (C.smallest_gap(p1, p2, l1, l2, K, 2) >= C.MIN_GAP)


@pytest.mark.parametrize("D,norm", C.EDGE_DN)
@pytest.mark.parametrize("shape,K", C.EDGE_BACKWARD)
def test_formulation_passes_the_backward_gates(shape, K, D, norm):
    """The gate is 4 x the formulation's own error, so the formulation passes by construction; what is checked is that the truth is
    finite with NaN in the padding rows, that the error is not 0 (a gate of 0) and the exact zeros of the padding."""
    from pytorch3d_amd import knn as knn_mod

    p1, p2, l1, l2 = C.edge_clouds(shape, D)
    idx = C.edge_truth(shape, D, norm, K)[0]
    g = torch.randn(idx.shape, generator=torch.Generator().manual_seed(17))
    truth, e32 = C.edge_backward_truth(p1, p2, l1, l2, idx, norm, g)
    assert all(bool(torch.isfinite(t).all()) for t in truth) and (norm == 1 or min(e32) > 0)
    grads = knn_mod.torch_knn_backward(p1, p2, C.lengths_tensor(l1), C.lengths_tensor(l2), idx, norm, g)
    C.check_knn_backward("formulation %s K%d D%d norm%d" % (shape, K, D, norm), grads, truth, e32, l1, l2)


# ---- B. runs in the scatter ---------------------------------------------------------------------------------------------------------------
def _scatter_cases():
    """name -> (p1, p2, K)"""
    out = {"star_d2": C.star_clouds_d2() + (1,)}
    for D in (2, 3):
        p1, p2, _ = C.few_targets_clouds(D)
        out["few_d%d_k2" % D] = (p1, p2, 2)
        out["few_d%d_k1" % D] = (p1, p2, 1)
    return out


def test_the_run_cases_hold_the_runs_they_are_for():
    p1, p2 = C.star_clouds_d2()
    assert p1.shape == (1, 300, 2) and p2.shape == (1, 1, 2)
    for D, per_wave in ((2, 32), (3, 21)):
        p1, p2, owner = C.few_targets_clouds(D)
        assert p1.shape == (1, 200, D) and p2.shape == (1, 3, D)
        idx1 = C.brute64(p1, p2, None, None, 1, 2)[0][0, :, 0]
        assert torch.equal(idx1, owner)
        runs = C.run_lengths(idx1)
        assert runs == list(C.RUN_BLOCKS) and max(runs) > per_wave and runs.count(1) >= 4
        # a run that lies across a wave's boundary, and a run of one that starts a wave's neighbourhood
        starts = torch.cumsum(torch.tensor([0] + runs[:-1]), 0).tolist()
        assert any(s // per_wave != (s + n - 1) // per_wave for s, n in zip(starts, runs))
        idx2 = C.brute64(p1, p2, None, None, 2, 2)[0][0].reshape(-1)
        assert set(C.run_lengths(idx2)) == {1, 2}  # K = 2: a hit's neighbour is the same query's other target
        assert C.smallest_gap(p1, p2, None, None, 2, 2) >= C.MIN_GAP


@pytest.mark.parametrize("name", list(_scatter_cases()))
def test_formulation_scatter_within_the_bound_and_a_scatter_that_keeps_only_the_last_hit_of_a_run_is_rejected(name):
    from pytorch3d_amd import knn as knn_mod

    p1, p2, K = _scatter_cases()[name]
    idx = C.brute64(p1, p2, None, None, K, 2)[0]
    g = torch.cos(torch.arange(idx.numel(), dtype=torch.float32)).reshape(idx.shape)
    truth, bound, terms = C.scatter_truth(p1, p2, idx[0], g[0])
    got = knn_mod.torch_knn_backward(p1, p2, None, None, idx, 2, g)[1][0].double()
    err = float((got - truth).abs().max())
    print(name, "formulation error %.3g" % err, "bound %.3g" % bound)
    assert err <= bound
    # the wrong answer: of every run of consecutive hits on one target only the last is added
    flat = idx[0].reshape(-1)
    last = torch.ones_like(flat, dtype=torch.bool)
    last[:-1] = flat[1:] != flat[:-1]
    wrong = torch.zeros_like(truth).index_add(0, flat[last], terms.reshape(-1, p1.shape[2])[last])
    err_wrong = float((wrong - truth).abs().max())
    print(name, "keeping the last hit of a run only: error %.3g" % err_wrong)
    assert err_wrong > bound


# ---- C. the second round of the chamfer sum ---------------------------------------------------------------------------------------------
def test_the_sum_shape_is_in_the_second_round():
    N, P1, P2, lx, ly = C.SUM_SHAPE
    assert C.tree_depth(P1) == 16 and C.tree_depth(16384) == 15 and C.tree_depth(lx[1]) == 16
    assert -(-lx[1] // 64) == 257 and -(-lx[1] // C.TILE) == 33


@pytest.mark.parametrize("kw", C.SUM_CASES, ids=lambda kw: C.sum_case_name(0, kw)[3:])
@pytest.mark.parametrize("D", [3, 2])
def test_formulation_passes_the_sum_gates_and_a_sum_of_the_first_256_partials_is_rejected(D, kw):
    N, P1, P2, lx, ly = C.SUM_SHAPE
    name = C.sum_case_name(D, kw)
    t = C.sum_truth(D, kw)
    assert all(C.check_sum_case("formulation " + name, t, *t["f32"]))
    # the wrong answer: the per-cloud sum of the x -> y direction stops after 256 wave partials = 16 384 queries
    w = torch.ones(N, dtype=torch.float64) if kw["weights"] is None else torch.tensor(kw["weights"], dtype=torch.float64)
    div = torch.tensor(lx, dtype=torch.float64) if kw["point_reduction"] == "mean" else torch.ones(N, dtype=torch.float64)
    per = t["per"] - t["terms_x"][:, 256 * 64:].sum(1) * w / div
    wrong = per if kw["batch_reduction"] is None else per.sum() * t["scale"]
    ok = C.check_sum_case("first 256 partials " + name, t, wrong, t["gx"], t["gy"])
    assert not ok[0], name


# ---- D. the second pass of the grid-stride loops: nearest neighbours ------------------------------------------------------------------------
@pytest.mark.parametrize("D,K", [(3, 2)])
def test_formulation_passes_on_the_large_cloud_and_a_gradient_without_the_items_past_the_cap_is_rejected(D, K):
    from pytorch3d_amd import knn as knn_mod

    p1, p2 = C.big_clouds(D)
    assert p1.shape[1] > C.STREAM_CAP and p1.shape[1] * K * 64 // (64 // D) > C.STREAM_CAP
    want_idx, want_d, ok = C.brute64_device(p1, p2, None, None, K, 2)
    live = torch.ones(p1.shape[:2], dtype=torch.bool)
    valid = C.valid_mask(None, None, 1, p1.shape[1], 8, K)
    idx, dists = knn_mod.torch_knn_forward(p1, p2, None, None, 2, K)
    C.check_knn_forward("formulation big D%d K%d" % (D, K), idx, dists, want_idx, want_d, ok, live, valid)
    g = torch.randn(want_idx.shape, generator=torch.Generator().manual_seed(17))
    truth, e32 = C.edge_backward_truth(p1, p2, None, None, want_idx, 2, g)
    grads = knn_mod.torch_knn_backward(p1, p2, None, None, want_idx, 2, g)
    C.check_knn_backward("formulation big D%d K%d" % (D, K), grads, truth, e32, None, None)
    # the wrong answer: one pass of the loops -- the queries past the cap get no gradient and give none
    short = knn_mod.torch_knn_backward(p1[:, :C.STREAM_CAP], p2, None, None, want_idx[:, :C.STREAM_CAP], 2, g[:, :C.STREAM_CAP])
    wrong = (torch.cat([short[0], torch.zeros(1, 300, D)], 1), short[1])
    for which, got, tr, e in zip(("grad_p1", "grad_p2"), wrong, truth, e32):
        err = float((got.double() - tr).abs().max())
        print("one pass only:", which, "error %.3g" % err, "gate %.3g" % (4 * e))
        assert err > 4 * e, which


# ---- the wrong neighbours ------------------------------------------------------------------------------------------------------------------
def _rejected(fn, *args):
    try:
        fn(*args)
    except AssertionError as e:
        return str(e) or "rejected"
    return None


@pytest.mark.parametrize("D,norm", [(3, 2), (2, 1)])
@pytest.mark.parametrize("K", [9, 15, 16])
def test_neighbours_from_a_queue_of_eight_are_rejected(K, D, norm):
    """K in 9..16 served by the capacity-8 queue: the slots 8.. never receive a neighbour (the kernel would write index 0, distance
    +inf or 0 there)."""
    for shape in C.EDGE_SHAPES:
        p1, p2, l1, l2 = C.edge_clouds(shape, D)
        want_idx, want_d, ok, live = C.edge_truth(shape, D, norm, K)
        idx, dists = _formulation(p1, p2, l1, l2, norm, K)
        idx[:, :, 8:], dists[:, :, 8:] = 0, 0.0
        why = _rejected(C.check_knn_forward, "queue of 8 %s K%d" % (shape, K), idx, dists, want_idx, want_d, ok, live, _valid(shape, D, K))
        assert why is not None, shape
        print(shape, K, "rejected:", why)


@pytest.mark.parametrize("D,norm", [(3, 2), (2, 1)])
@pytest.mark.parametrize("K", [1, 5, 32])
def test_a_search_that_reads_p2_past_lengths2_is_rejected(K, D, norm):
    for shape in C.EDGE_SHAPES:
        p1, p2, l1, l2 = C.edge_clouds(shape, D)
        want_idx, want_d, ok, live = C.edge_truth(shape, D, norm, K)
        idx, dists = _formulation(torch.nan_to_num(p1, nan=0.0), p2, l1, None, norm, K)
        why = _rejected(C.check_knn_forward, "P2 for lengths2 %s K%d" % (shape, K), idx, dists, want_idx, want_d, ok, live, _valid(shape, D, K))
        assert why is not None, shape
        print(shape, K, "rejected:", why)


# ---- C. the second round: point-mesh losses and regularisers ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["face", "edge"])
def test_formulation_passes_the_point_mesh_gates_and_a_sum_of_the_first_256_partials_is_rejected(tag):
    import point_mesh_case as PM

    t = PM.second_round_truth(tag)
    assert t["num_points"] == [30, 16500] and t["num_prims"] == ([16562, 20] if tag == "face" else [25025, 30])
    assert PM.sum_depth(t["n"]) == 18 and PM.sum_depth(16384) == 17  # 6 + 2 + 8 + 2: the second round
    for direction, r in t["directions"].items():
        assert r["max_queries"] > 256 * 64
        share = float(r["ok"].double().mean())
        print(tag, direction, "E %.3g, admitted %.4f" % (r["E"], share))
        assert share >= 1.0 - PM.MAX_DROPPED
    assert all(PM.check_second_round_loss("formulation " + tag, t, t["f32_loss"], t["f32_grad_verts"], t["f32_grad_points"]))
    # the wrong answer: each element's sum stops after 256 wave partials = 16 384 queries
    wrong = t["loss64"]
    for direction, r in t["directions"].items():
        counts = t["num_points"] if direction.startswith("point") else t["num_prims"]
        for (q0, q1), c in zip(PM.element_slices(counts), counts):
            wrong -= float(r["best64"][q0 + 256 * 64:q1].sum()) / (c * len(counts)) if c > 256 * 64 else 0.0
    ok = PM.check_second_round_loss("first 256 partials " + tag, t, wrong, t["grad_verts64"], t["grad_points64"])
    assert not ok[0]


def test_formulation_passes_the_regulariser_gates_beyond_65536_terms_and_a_sum_of_the_first_256_partials_is_rejected():
    import mesh_losses_case as ML
    import pytorch3d_amd as p3d
    from pytorch3d_amd import mesh_losses

    verts, faces = ML.second_round_batch()
    tables, tt = ML.brute_tables(verts, faces), ML.tensor_tables(verts, faces)
    assert tables["V"] == 66049 + 42 and len(tables["edges"]) == 197120 + 120 and len(tables["pairs"]) == 196096 + 120
    assert min(tables["V"], len(tables["edges"]), len(tables["pairs"])) > ML.SUM_CAP
    assert [ML.depth(n) for n in (tables["V"], len(tables["edges"]), len(tables["pairs"]))] == [18, 20, 19] and ML.depth(ML.SUM_CAP) == 17
    # the sorted tables are the definition's, here and on the small batch; so are the package's on the CPU
    for v, f, b in ((verts, faces, tables), ML.build_batch() + (None,)):
        b, s = b if b is not None else ML.brute_tables(v, f), (tt if b is not None else ML.tensor_tables(v, f))
        assert s["edges"].tolist() == [list(e) for e in b["edges"]] and s["pairs"].tolist() == [list(p) for p in b["pairs"]]
        assert s["edge_mesh"].tolist() == b["edge_mesh"] and s["pair_mesh"].tolist() == b["pair_mesh"] and s["vert_mesh"].tolist() == b["vert_mesh"]
        assert [s["adj_col"][s["adj_row"] == u].tolist() for u in range(0, b["V"], max(1, b["V"] // 50))] == b["adjacency"][::max(1, b["V"] // 50)]
        vv = torch.cat(v, 0).double()
        for name in ML.LOSSES:
            assert torch.equal(ML.terms(name, vv, b), ML.terms_vectorised(name, vv, s)), name
    t = mesh_losses.topology_of(p3d.PackedMeshes(verts, faces))
    assert torch.equal(t.edges.long(), tt["edges"]) and torch.equal(t.pairs.long(), tt["pairs"]) and torch.equal(t.adj.long(), tt["adj_col"])
    f32 = ML.package_formulation(verts, faces, names=ML.LOSSES)
    for name in ML.LOSSES:
        t_loss, t_grad, gate_l, gate_g, rec = ML.gates(name, verts, faces, tables, f32=f32)
        v_loss, v_grad, vgate_l, vgate_g, _ = ML.gates_vectorised(name, verts, tt, f32)
        assert (t_loss, gate_l, gate_g) == (v_loss, vgate_l, vgate_g) and torch.equal(t_grad, v_grad)
        err_l, err_g = abs(f32[name][0] - t_loss), float((f32[name][1].double() - t_grad).abs().max())
        first = float(ML.terms(name, torch.cat(verts, 0).double(), tables)[:ML.SUM_CAP].sum()) / tables["N"]
        print(f"{name}: formulation loss error {err_l:.2e} (gate {gate_l:.2e}), gradient {err_g:.2e} (gate {gate_g:.2e}); the first 256 partials "
              f"alone are {abs(first - t_loss):.2e} away (n = {rec['n']}, D = {rec['D']})")
        assert err_l <= gate_l and err_g <= gate_g and rec["E32_grad"] > 0
        assert abs(first - t_loss) > gate_l, name


# ---- D. the large mesh: the same generator at 33 x 33, and the restatements it needs ---------------------------------------------------------
def test_formulation_passes_the_gates_of_the_large_mesh_at_33_by_33():
    import mesh_losses_case as ML
    import mesh_normals_case as MN
    from pytorch3d_amd import _aux_ops

    assert ML.second_pass_mesh.__defaults__ == (1025,)
    n = 1025  # the counts of the full size, by the formulas of jittered_grid: every loop beyond one pass
    assert min(n * n, 2 * (n - 1) ** 2, 3 * (n - 1) ** 2 + 2 * (n - 1), 3 * (n - 1) ** 2 - 2 * (n - 1)) > ML.STREAM_CAP
    assert min(n * n, 2 * (n - 1) ** 2) == 1050625 and 3 * (n - 1) ** 2 + 2 * (n - 1) == 3147776
    assert (n - 1) ** 2 <= ML.STREAM_CAP  # ... and 1024 x 1024 vertices would not be
    v, f = ML.second_pass_mesh(33)
    tt, b = ML.tensor_tables([v], [f]), ML.brute_tables([v], [f])
    assert (tt["V"], f.shape[0], tt["edges"].shape[0], tt["pairs"].shape[0]) == (33 * 33, 2 * 32 * 32, 3 * 32 * 32 + 64, 3 * 32 * 32 - 64)
    assert tt["edges"].tolist() == [list(e) for e in b["edges"]] and tt["pairs"].tolist() == [list(p) for p in b["pairs"]]
    f32 = ML.package_formulation([v], [f], names=ML.LOSSES)
    for name in ML.LOSSES:
        t_loss, t_grad, gate_l, gate_g, rec = ML.gates_vectorised(name, [v], tt, f32)
        assert abs(f32[name][0] - t_loss) <= gate_l and float((f32[name][1].double() - t_grad).abs().max()) <= gate_g and gate_g > 0
    # vertex normals: the reference's float32 formulation against the vectorised truths
    g = torch.randn(v.shape, generator=torch.Generator().manual_seed(5))
    n64, sums64 = MN.restated_forward_vectorised(v.double(), f)
    auto_n, auto_g = MN.autograd_truth(v, f, g)
    assert float((n64 - auto_n).abs().max()) < 1e-13
    assert float((MN.restated_backward_vectorised(g.double(), v.double(), f, sums64) - auto_g).abs().max()) < 1e-9 * float(auto_g.abs().max())
    # face areas and normals: the package's formulation in float64 is the restatement's, to rounding
    gen = torch.Generator().manual_seed(9)
    ga, gn = torch.randn(f.shape[0], generator=gen), torch.randn(f.shape[0], 3, generator=gen)
    want = _aux_ops.face_areas_normals_backward(ga.double(), gn.double(), v.double(), f)
    got = MN.face_areas_normals_backward_restated(ga.double(), gn.double(), v.double(), f)
    assert float((got - want).abs().max()) < 1e-12 * float(want.abs().max())


def test_the_vectorised_normal_restatements_equal_the_loops_on_the_small_input():
    import mesh_normals_case as MN
    from pytorch3d_amd import _aux_ops

    v, f, eps = MN.build_input()
    g = torch.randn(v.shape, generator=torch.Generator().manual_seed(5)).double()
    n, sums = MN.restated_forward(v.double(), f)
    nv, sums_v = MN.restated_forward_vectorised(v.double(), f)
    assert torch.equal(n, nv) and torch.equal(sums, sums_v)
    assert torch.equal(MN.restated_backward(g, v.double(), f, sums), MN.restated_backward_vectorised(g, v.double(), f, sums))
    # the face operator: against the package's formulation in float64 (which tests/test_cpu_aux_ops.py pins to the reference's CPU
    # kernels), off the degenerate faces, where the clamp at 1e-6 makes the two differ by design
    gen = torch.Generator().manual_seed(9)
    ga, gn = torch.randn(f.shape[0], generator=gen).double(), torch.randn(f.shape[0], 3, generator=gen).double()
    a, nrm = MN.face_areas_normals_restated(v.double(), f)
    wa, wn = _aux_ops.face_areas_normals_forward(v.double(), f)
    assert torch.equal(a, wa) and torch.equal(nrm, wn)
    want = _aux_ops.face_areas_normals_backward(ga, gn, v.double(), f)
    got = MN.face_areas_normals_backward_restated(ga, gn, v.double(), f)
    assert float((got - want)[~eps].abs().max()) < 1e-12 * float(want[~eps].abs().max())
    # and the deviation is in it: without the c_x term the restatement would be the plain derivative, far from the reference's
    vv = v.double().clone().requires_grad_(True)
    (plain,) = torch.autograd.grad(list(MN.face_areas_normals_restated(vv, f)), vv, [ga, gn])
    assert float((plain - want)[~eps].abs().max()) > 1e-3 * float(want[~eps].abs().max())


# ---- E. the restated tree (tests/fixed_sum_case.py) on the torch formulations' distances ----------------------------------------------------
def test_the_restated_tree_is_a_sum_and_its_inputs_tell_it_from_a_chain():
    """What section E of the GPU file relies on, shown without the kernels: the restatement is within depth x 2^-24 x sum |term| of
    the float64 sum, it is not the left-to-right sum on the seeded inputs wherever TELLS_APART says so, and an empty segment is +0."""
    import numpy as np

    import fixed_sum_case as FS
    from pytorch3d_amd import knn as knn_mod
    from pytorch3d_amd import point_mesh as pm

    cases = []
    for name in FS.CHAMFER_LENGTHS:
        p1, p2, l1 = FS.chamfer_clouds(name)
        d = knn_mod.torch_knn_forward(p1, p2, l1, None, 2, 1)[1].reshape(2, -1).numpy()
        cases += [("chamfer " + name, d[n], -(-p1.shape[1] // 64), FS.CHAMFER_TELLS_APART[name][n]) for n in range(2)]
    for name in FS.POINT_EDGE_COUNTS:
        points, pfirst, segms, sfirst, w, max_points = FS.point_edge_case(name)
        d = pm.torch_forward("point_edge", points, pfirst, segms, sfirst)[0].numpy()
        ends = pfirst.tolist() + [points.shape[0]]
        cases += [("point_edge " + name, d[ends[n]:ends[n + 1]] * np.float32(w[n]), -(-max_points // 64), FS.POINT_EDGE_TELLS_APART[name][n])
                  for n in range(2)]
    for who, terms, per_segment, tells_apart in cases:
        tree, chain, exact = FS.tree_sum(terms, per_segment), FS.chain_sum(terms), float(terms.astype(np.float64).sum())
        depth = 6 + -(-per_segment // 256) + 8
        assert abs(float(tree) - exact) <= depth * 2.0 ** -24 * float(np.abs(terms).astype(np.float64).sum()), who
        assert bool((FS.bits(tree) != FS.bits(chain)).all()) == tells_apart, who
    assert FS.bits(FS.tree_sum(np.zeros(0, np.float32), 3)) == 0
