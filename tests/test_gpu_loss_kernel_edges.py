"""The structural paths of the loss kernels that the recorded fixtures are too small to reach, on the MI355X: csrc/knn.hip,
csrc/point_mesh.hip, csrc/mesh_losses.hip and csrc/normals.hip.

  A. knn_points forward and backward on every queue capacity (K = 1 .. 32: both ends and the inside of 1, 2, 4, 8, 16, 32), on ragged
     clouds that scan one, two and three tiles in ONE launch, with lengths2 on the tile edge below P2, distance-0 decoys in the p2
     padding and NaN in the p1 padding;
  B. runs of hits on one target in the scatter of the backward for D = 2 (32 hits per wave) and D = 3 (21);
  C. the second round of the three partial-sum kernels: more than 256 partials per cloud, element or batch;
  D. the second pass of the grid-stride loops: more than 1 048 576 queries, hits, vertices, faces, edges and pairs;
  E. the fixed tree of csrc/fixed_sum.h bit for bit: the chamfer and point-edge sums against a numpy float32 restatement of the
     header's comment (tests/fixed_sum_case.py), on inputs whose left-to-right sum has other bits.

Inputs come from seeded generators (tests/*_case.py); in A to D every yardstick is a float64 restatement from those files and
every gate is the one of the neighbouring test files (test_gpu_chamfer.py, test_gpu_point_mesh.py, test_gpu_mesh_losses.py,
test_gpu_mesh_normals.py), scaled by the error the package's float32 torch formulation makes on the CPU against the same truth.
tests/test_cpu_loss_kernel_edges.py proves the machinery: the formulation passes every gate and five wrong answers are rejected.
"""
import contextlib

import pytest
import torch

import chamfer_case as C

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


@contextlib.contextmanager
def _flag(on):
    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])


def _mode(ordered):
    return "ordered" if ordered else "atomic"


def _to(lengths):
    return None if lengths is None else C.lengths_tensor(lengths).to(_dev())


# ---- A. every rung, ragged over tile and wave edges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", C.EDGE_KS)
@pytest.mark.parametrize("norm", [2, 1])
@pytest.mark.parametrize("D", [3, 2])
@pytest.mark.parametrize("shape", list(C.EDGE_SHAPES))
def test_knn_forward_on_every_rung_over_ragged_tiles(shape, D, norm, K):
    import pytorch3d_amd as p3d
    from pytorch3d_amd import knn as knn_mod

    p1, p2, l1, l2 = C.edge_clouds(shape, D)
    want_idx, want_d, ok, live = C.edge_truth(shape, D, norm, K)
    a, b = p1.to(_dev()), p2.to(_dev())
    assert knn_mod.kernel_path(a, b, K)
    got = p3d.knn_points(a, b, _to(l1), _to(l2), norm=norm, K=K)
    valid = C.valid_mask(l1, l2, p1.shape[0], p1.shape[1], p2.shape[1], K)
    C.check_knn_forward("kernel %s D%d norm%d K%d" % (shape, D, norm, K), got.idx.cpu(), got.dists.cpu(), want_idx, want_d, ok, live, valid)


@pytest.fixture(scope="module")
def edge_backward_cases():
    """Per case: the upstream gradient, the float64 truth on the float64 indices and the float32 CPU formulation's errors against it
    -- computed once, never modified."""
    out = {}
    for shape, K in C.EDGE_BACKWARD:
        for D, norm in C.EDGE_DN:
            p1, p2, l1, l2 = C.edge_clouds(shape, D)
            idx = C.edge_truth(shape, D, norm, K)[0]
            g = torch.randn(idx.shape, generator=torch.Generator().manual_seed(17))
            out[(shape, K, D, norm)] = (idx, g) + C.edge_backward_truth(p1, p2, l1, l2, idx, norm, g)
    return out


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("D,norm", C.EDGE_DN)
@pytest.mark.parametrize("shape,K", C.EDGE_BACKWARD)
def test_knn_backward_on_the_rungs_over_ragged_tiles(edge_backward_cases, shape, K, D, norm, ordered):
    from pytorch3d_amd import _C

    idx, g, truth, e32 = edge_backward_cases[(shape, K, D, norm)]
    p1, p2, l1, l2 = C.edge_clouds(shape, D)
    with _flag(ordered):
        grads = _C.knn_points_backward(p1.to(_dev()), p2.to(_dev()), _to(l1), _to(l2), idx.to(_dev()), norm, g.to(_dev()))
    C.check_knn_backward("kernel %s K%d D%d norm%d %s" % (shape, K, D, norm, _mode(ordered)), grads, truth, e32, l1, l2)


# ---- B. runs in the scatter ---------------------------------------------------------------------------------------------------------------
def _scatter_cases():
    out = {"star_d2": C.star_clouds_d2() + (1,)}
    for D in (2, 3):
        p1, p2, _ = C.few_targets_clouds(D)
        out["few_d%d_k2" % D] = (p1, p2, 2)
        out["few_d%d_k1" % D] = (p1, p2, 1)
    return out


def _scatter_grad(name, ordered, stream=None):
    import pytorch3d_amd as p3d

    p1, p2, K = _scatter_cases()[name]
    ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    with ctx, _flag(ordered):
        a, b = p1.to(_dev()), p2.to(_dev()).requires_grad_(True)
        got = p3d.knn_points(a, b, K=K)
        g = torch.cos(torch.arange(got.idx.numel(), dtype=torch.float32)).reshape(got.idx.shape).to(_dev())
        (grad,) = torch.autograd.grad((got.dists * g).sum(), (b,))
    if stream is not None:
        stream.synchronize()
    return grad, got.idx


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("name", list(_scatter_cases()))
def test_runs_in_the_scatter_within_the_stars_bound(name, ordered):
    p1, p2, K = _scatter_cases()[name]
    idx = C.brute64(p1, p2, None, None, K, 2)[0]
    g = torch.cos(torch.arange(idx.numel(), dtype=torch.float32)).reshape(idx.shape)
    truth, bound, _ = C.scatter_truth(p1, p2, idx[0], g[0])
    grad, got_idx = _scatter_grad(name, ordered)
    assert torch.equal(got_idx.cpu(), idx)
    runs = C.run_lengths(idx[0].reshape(-1))
    err = float((grad.cpu().double()[0] - truth).abs().max())
    print(name, _mode(ordered), "runs up to %d hits, %d of one;" % (max(runs), runs.count(1)), "error %.3g" % err, "bound %.3g" % bound)
    assert err <= bound


def test_runs_in_the_scatter_repeat_their_bits_under_the_flag_on_two_runs_and_two_streams():
    torch.cuda.synchronize()
    for name in _scatter_cases():
        first = _scatter_grad(name, True)[0]
        torch.cuda.synchronize()
        again = _scatter_grad(name, True)[0]
        other = _scatter_grad(name, True, torch.cuda.Stream(device=_dev()))[0]
        torch.cuda.synchronize()
        assert torch.equal(first, again) and torch.equal(first, other), name


# ---- C. the second round of the partial sums: chamfer ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("kw", C.SUM_CASES, ids=lambda kw: C.sum_case_name(0, kw)[3:])
@pytest.mark.parametrize("D", [3, 2])
def test_chamfer_with_more_than_256_wave_partials_per_cloud(D, kw, ordered):
    import pytorch3d_amd as p3d

    N, P1, P2, lx, ly = C.SUM_SHAPE
    assert C.tree_depth(P1) == 16 and -(-lx[1] // 64) == 257  # the second round of segment_sum_kernel (csrc/fixed_sum.h), in both clouds
    t = C.sum_truth(D, kw)
    x, y, ckw = C.sum_inputs(D, kw, device=_dev())
    with _flag(ordered):
        result = p3d.chamfer_distance(x, y, **ckw)
        assert result[1] is None and type(result[0].grad_fn).__name__ == "_ChamferFusedBackward"
        gx, gy = torch.autograd.grad(C.scalarise(result), (x, y))
    ok = C.check_sum_case("kernel %s %s" % (C.sum_case_name(D, kw), _mode(ordered)), t, result[0], gx, gy)
    assert ok[0], "loss"
    assert ok[1], "grad_x"
    assert ok[2], "grad_y"


# ---- D. the second pass of the grid-stride loops: nearest neighbours ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_knn():
    """Per (D, K): the float64 neighbours (one vectorised pass on the GPU), the upstream gradient, the float64 gradients and the
    float32 CPU formulation's errors -- computed once, never modified."""
    out = {}
    for D, K in ((3, 1), (3, 2), (2, 1)):
        p1, p2 = C.big_clouds(D)
        idx, dists, ok = C.brute64_device(p1.to(_dev()), p2.to(_dev()), None, None, K, 2)
        idx, dists, ok = idx.cpu(), dists.cpu(), ok.cpu()
        g = torch.randn(idx.shape, generator=torch.Generator().manual_seed(17))
        out[(D, K)] = (idx, dists, ok, g) + C.edge_backward_truth(p1, p2, None, None, idx, 2, g)
    return out


@pytest.mark.parametrize("D,K", [(3, 1), (3, 2), (2, 1)])
def test_knn_backward_loops_go_round_twice(big_knn, D, K):
    import pytorch3d_amd as p3d
    from pytorch3d_amd import _C

    p1, p2 = C.big_clouds(D)
    idx, dists, ok, g, truth, e32 = big_knn[(D, K)]
    P1 = p1.shape[1]
    # the gather has one lane per query, the scatter one per hit and coordinate, 64 / D hits to a wave: both beyond one pass
    assert P1 > C.STREAM_CAP and -(-P1 * K // (64 // D)) * 64 > C.STREAM_CAP
    a, b = p1.to(_dev()), p2.to(_dev())
    got = p3d.knn_points(a, b, K=K)
    C.check_knn_forward("kernel big D%d K%d" % (D, K), got.idx.cpu(), got.dists.cpu(), idx, dists, ok, torch.ones(1, P1, dtype=torch.bool),
                        C.valid_mask(None, None, 1, P1, 8, K))
    for ordered in (False, True):
        junk = [torch.full((P1 * D,), float("nan"), device=_dev()) for _ in range(2)]  # what torch.empty hands out next
        del junk
        with _flag(ordered):
            grads = _C.knn_points_backward(a, b, None, None, idx.to(_dev()), 2, g.to(_dev()))
        assert bool(torch.isfinite(grads[0]).all()) and bool(torch.isfinite(grads[1]).all()), "an entry was not written"
        C.check_knn_backward("kernel big D%d K%d %s" % (D, K, _mode(ordered)), grads, truth, e32, None, None)


# ---- C. the second round of the partial sums: point-mesh losses -------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["face", "edge"])
def test_point_mesh_directions_with_more_than_16384_queries_in_an_element(tag):
    """The operators on the batch of the fused losses below, judged as test_gpu_point_mesh's larger shape: distances within 4 E,
    indices exact where the float64 gap is at least 16 E."""
    import point_mesh_case as PM
    from pytorch3d_amd import point_mesh as pm

    t = PM.second_round_truth(tag)
    points, prims = t["points"].to(_dev()), t["prims"].to(_dev())
    pfirst, sfirst = t["pfirst"].to(_dev()), t["sfirst"].to(_dev())
    for direction, r in t["directions"].items():
        assert r["max_queries"] > 256 * 64  # more than 256 waves of queries in one element
        assert pm.kernel_path(points, prims)
        d, i = getattr(pm, direction + "_dist_forward")(points, pfirst, prims, sfirst, r["max_queries"])
        err = float((d.cpu().double() - r["best64"]).abs().max())
        share = float(r["ok"].double().mean())
        print("%s: dist error %.3g (4 E = %.3g), admitted %d of %d" % (direction, err, 4 * r["E"], int(r["ok"].sum()), r["ok"].numel()))
        assert share >= 1.0 - PM.MAX_DROPPED
        assert torch.equal(i.cpu()[r["ok"]], r["want_i"][r["ok"]])
        assert err <= 4 * r["E"]


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("tag", ["face", "edge"])
def test_point_mesh_losses_with_more_than_256_wave_partials_in_an_element(tag, ordered):
    import point_mesh_case as PM
    import pytorch3d_amd as p3d

    t = PM.second_round_truth(tag)
    assert PM.sum_depth(t["n"]) == 18 and PM.sum_depth(256 * 64) == 17  # segment_sum_kernel (csrc/fixed_sum.h) takes a second round
    verts, faces, points, _ = PM.second_round_batch()
    with _flag(ordered):
        v, p = [x.to(_dev()).requires_grad_(True) for x in verts], [x.to(_dev()).requires_grad_(True) for x in points]
        meshes, pcls = p3d.PackedMeshes(v, [f.to(_dev()) for f in faces]), p3d.PackedPointclouds(p)
        loss = p3d.point_mesh_face_distance(meshes, pcls) if tag == "face" else p3d.point_mesh_edge_distance(meshes, pcls)
        assert type(loss.grad_fn).__name__.startswith("_PointMeshLoss")  # ONE autograd node
        grads = torch.autograd.grad(loss, v + p)
    ok = PM.check_second_round_loss("fused %s (%s)" % (tag, _mode(ordered)), t, loss, torch.cat(grads[:2], 0), torch.cat(grads[2:], 0))
    assert ok[0], "loss"
    assert ok[1], "gradients"


# ---- C. the second round of the partial sums: regularisers ------------------------------------------------------------------------------------
def _regulariser(name, meshes):
    import mesh_losses_case as ML
    import pytorch3d_amd as p3d

    if name in ("edge", "edge_target"):
        return p3d.mesh_edge_loss(meshes, ML.TARGET if name == "edge_target" else 0.0)
    if name == "normal":
        return p3d.mesh_normal_consistency(meshes)
    return p3d.mesh_laplacian_smoothing(meshes)


def _run_regulariser(name, verts, faces):
    import pytorch3d_amd as p3d

    v = [x.to(_dev()).requires_grad_(True) for x in verts]
    m = p3d.PackedMeshes(v, [x.to(_dev()) for x in faces])
    loss = _regulariser(name, m)
    return loss.detach(), torch.cat(list(torch.autograd.grad(loss, v)), 0), m


@pytest.fixture(scope="module")
def second_round_meshes():
    """The batch, its tables by the definition and the float32 formulation's results on the CPU -- computed once, never modified."""
    import mesh_losses_case as ML

    verts, faces = ML.second_round_batch()
    return {"verts": verts, "faces": faces, "tables": ML.brute_tables(verts, faces), "f32": ML.package_formulation(verts, faces, names=ML.LOSSES)}


def test_regulariser_tables_beyond_65536_rows_equal_the_definition(second_round_meshes):
    import mesh_losses_case as ML
    import pytorch3d_amd as p3d
    from pytorch3d_amd import mesh_losses

    b = second_round_meshes["tables"]
    assert b["V"] == 66049 + 42 and len(b["edges"]) == 197120 + 120 and len(b["pairs"]) == 196096 + 120
    assert min(b["V"], len(b["edges"]), len(b["pairs"])) > ML.SUM_CAP
    m = p3d.PackedMeshes([x.to(_dev()) for x in second_round_meshes["verts"]], [x.to(_dev()) for x in second_round_meshes["faces"]])
    t = mesh_losses.topology_of(m)
    assert t.edges.is_cuda and t.edges.tolist() == [list(e) for e in b["edges"]] and t.pairs.tolist() == [list(p) for p in b["pairs"]]
    off, adj = t.adj_offsets.tolist(), t.adj.tolist()
    assert [adj[off[v]:off[v + 1]] for v in range(t.V)] == b["adjacency"]


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("name", ["edge", "edge_target", "laplacian", "normal"])
def test_regularisers_with_more_than_256_partials(second_round_meshes, name, ordered):
    import mesh_losses_case as ML

    s = second_round_meshes
    t_loss, t_grad, gate_l, gate_g, rec = ML.gates(name, s["verts"], s["faces"], s["tables"], f32=s["f32"])
    assert rec["n"] > ML.SUM_CAP and rec["D"] == {"edge": 20, "edge_target": 20, "laplacian": 18, "normal": 19}[name]  # 17 up to 65 536 terms
    with _flag(ordered):
        loss, grad, _ = _run_regulariser(name, s["verts"], s["faces"])
    err_l, err_g = abs(float(loss) - t_loss), float((grad.cpu().double() - t_grad).abs().max())
    print(f"{name} ({_mode(ordered)}): loss {float(loss):.9g} (truth {t_loss:.9g}) error {err_l:.2e}, gate {gate_l:.2e} = 4 x {rec['E32_loss']:.2e} + "
          f"{rec['D']} x 2^-24 x {rec['S']:.3g}; gradient error {err_g:.2e}, gate {gate_g:.2e} = 4 x {rec['E32_grad']:.2e} (n = {rec['n']})")
    assert rec["E32_grad"] > 0
    assert err_l <= gate_l, (err_l, gate_l)
    assert err_g <= gate_g, (err_g, gate_g)


# ---- D. the second pass of the grid-stride loops: one large mesh -----------------------------------------------------------------------------
def _dirty_the_allocator(nbytes):
    """NaN-filled buffers handed back to the allocator: what torch.empty returns next holds NaN wherever a kernel does not write."""
    junk = [torch.full((max(nbytes // 4, 1),), float("nan"), device=_dev()) for _ in range(3)]
    del junk


@pytest.fixture(scope="module")
def large_mesh():
    """The 1025 x 1025 grid, its tables (sorted on the GPU) and the float32 formulation's results on the CPU -- computed once, never
    modified."""
    import time

    import mesh_losses_case as ML

    v, f = ML.second_pass_mesh()
    t0 = time.time()
    tt = ML.tensor_tables([v], [f], device=_dev())
    t1 = time.time()
    f32 = ML.package_formulation([v], [f], names=ML.LOSSES)
    print("large mesh: tables on the GPU %.1f s, the float32 formulation of the four losses on the CPU %.1f s" % (t1 - t0, time.time() - t1))
    counts = {"vertices": v.shape[0], "faces": f.shape[0], "edges": tt["edges"].shape[0], "pairs": tt["pairs"].shape[0]}
    assert counts == {"vertices": 1050625, "faces": 2097152, "edges": 3147776, "pairs": 3143680}
    assert min(counts.values()) > ML.STREAM_CAP  # every loop takes a second pass
    return {"verts": v, "faces": f, "tt": tt, "f32": f32}


@pytest.mark.parametrize("name", ["edge", "edge_target", "laplacian", "normal"])
def test_regulariser_loops_go_round_twice(large_mesh, name):
    import mesh_losses_case as ML

    s = large_mesh
    t_loss, t_grad, gate_l, gate_g, rec = ML.gates_vectorised(name, [s["verts"]], s["tt"], s["f32"])
    assert rec["n"] > ML.STREAM_CAP
    for ordered in (False, True):
        _dirty_the_allocator(s["verts"].numel() * 4)
        with _flag(ordered):
            loss, grad, _ = _run_regulariser(name, [s["verts"]], [s["faces"]])
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()), "an entry was not written"
        err_l, err_g = abs(float(loss) - t_loss), float((grad.cpu().double() - t_grad).abs().max())
        print(f"{name} ({_mode(ordered)}): loss error {err_l:.2e}, gate {gate_l:.2e} = 4 x {rec['E32_loss']:.2e} + {rec['D']} x 2^-24 x "
              f"{rec['S']:.3g}; gradient error {err_g:.2e}, gate {gate_g:.2e} = 4 x {rec['E32_grad']:.2e} (n = {rec['n']})")
        assert err_l <= gate_l, (err_l, gate_l)
        assert err_g <= gate_g, (err_g, gate_g)


def test_verts_normals_loops_go_round_twice(large_mesh):
    import mesh_normals_case as MN
    import pytorch3d_amd as p3d

    v, f = large_mesh["verts"], large_mesh["faces"]
    g = torch.randn(v.shape, generator=torch.Generator().manual_seed(5))
    vg, fg = v.to(_dev()), f.to(_dev())
    truth_n = MN.restated_forward_vectorised(vg.double(), fg)[0].cpu()
    truth_g = MN.autograd_truth(vg, fg, g.to(_dev()))[1].cpu()
    v32 = v.clone().requires_grad_(True)  # the reference's float32 formulation on the CPU: the scale of the gates
    ref_n = MN.reference_verts_normals(v32, f)
    (ref_g,) = torch.autograd.grad(ref_n, v32, g)
    e_n, e_g = float((ref_n.detach().double() - truth_n).abs().max()), float((ref_g.double() - truth_g).abs().max())
    assert e_n > 0 and e_g > 0
    for ordered in (False, True):
        _dirty_the_allocator(v.numel() * 4)
        with _flag(ordered):
            leaf = vg.clone().requires_grad_(True)
            n = p3d.verts_normals(leaf, fg)
            (grad,) = torch.autograd.grad(n, leaf, g.to(_dev()))
        assert bool(torch.isfinite(n).all()) and bool(torch.isfinite(grad).all()), "an entry was not written"
        err_n, err_g = float((n.detach().cpu().double() - truth_n).abs().max()), float((grad.cpu().double() - truth_g).abs().max())
        print(f"vertex normals ({_mode(ordered)}): {err_n:.2e}, gate {4 * e_n:.2e} = 4 x {e_n:.2e}; gradient {err_g:.2e}, gate {4 * e_g:.2e} = "
              f"4 x {e_g:.2e} (largest {float(truth_g.abs().max()):.2e})")
        assert err_n <= 4 * e_n
        assert err_g <= 4 * e_g


def test_face_areas_normals_loops_go_round_twice(large_mesh):
    import mesh_normals_case as MN
    import pytorch3d_amd as p3d
    from pytorch3d_amd import _aux_ops

    v, f = large_mesh["verts"], large_mesh["faces"]
    gen = torch.Generator().manual_seed(9)
    ga, gn = torch.randn(f.shape[0], generator=gen), torch.randn(f.shape[0], 3, generator=gen)
    vg, fg = v.to(_dev()), f.to(_dev())
    truth_a, truth_n = [t.cpu() for t in MN.face_areas_normals_restated(vg.double(), fg)]
    truth_g = MN.face_areas_normals_backward_restated(ga.to(_dev()).double(), gn.to(_dev()).double(), vg.double(), fg).cpu()
    f_a, f_n = _aux_ops.face_areas_normals_forward(v, f)  # the package's float32 torch formulation on the CPU: the scale of the gates
    f_g = _aux_ops.face_areas_normals_backward(ga, gn, v, f)
    e_a, e_n = float((f_a.double() - truth_a).abs().max()), float((f_n.double() - truth_n).abs().max())
    e_g = float((f_g.double() - truth_g).abs().max())
    assert min(e_a, e_n, e_g) > 0
    for ordered in (False, True):
        _dirty_the_allocator(f.numel() * 4)
        with _flag(ordered):
            leaf = vg.clone().requires_grad_(True)
            a, n = p3d.face_areas_normals(leaf, fg)
            (grad,) = torch.autograd.grad([a, n], leaf, [ga.to(_dev()), gn.to(_dev())])
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(n).all()) and bool(torch.isfinite(grad).all()), "an entry was not written"
        err_a, err_n = float((a.detach().cpu().double() - truth_a).abs().max()), float((n.detach().cpu().double() - truth_n).abs().max())
        err_g = float((grad.cpu().double() - truth_g).abs().max())
        print(f"face areas ({_mode(ordered)}): {err_a:.2e} (gate 4 x {e_a:.2e}), normals {err_n:.2e} (4 x {e_n:.2e}), gradient {err_g:.2e} "
              f"(4 x {e_g:.2e}; largest {float(truth_g.abs().max()):.2e})")
        assert err_a <= 4 * e_a
        assert err_n <= 4 * e_n
        assert err_g <= 4 * e_g


# ---- E. the fixed tree, bit for bit (csrc/fixed_sum.h restated by tests/fixed_sum_case.py) -----------------------------------------------------
def _assert_tree_bits(who, got, terms_per_segment, per_segment, tells_apart):
    """got[n] has the bits of the restated tree over terms_per_segment[n]; where the inputs tell the orders apart, not those of the
    left-to-right sum."""
    import numpy as np

    import fixed_sum_case as FS

    for n, terms in enumerate(terms_per_segment):
        want, chain = FS.tree_sum(terms, per_segment), FS.chain_sum(terms)
        print("%s segment %d: %d terms, %d partials, kernel %r tree %r left-to-right %r" % (who, n, len(terms), per_segment, float(got[n]), float(want), float(chain)))
        assert np.array_equal(FS.bits(got[n]), FS.bits(want)), (who, n)
        if tells_apart[n]:
            assert not np.array_equal(FS.bits(chain), FS.bits(want)), (who, n, "the inputs do not tell the tree from a chain")


@pytest.mark.parametrize("name", ["small", "second_step"])
def test_chamfer_cloud_sums_have_the_bits_of_the_documented_tree(name):
    import fixed_sum_case as FS
    from pytorch3d_amd import _lib, chamfer

    p1, p2, lengths1 = FS.chamfer_clouds(name)
    a, b = p1.to(_dev()), p2.to(_dev())
    with torch.cuda.device(_dev()):
        _, dists, sums = chamfer._direction_forward(_lib.load(), a, b, lengths1.to(_dev()), None, None, 2, False)
    dists, sums = dists.cpu().numpy(), sums.cpu().numpy()
    per_segment = -(-p1.shape[1] // 64)
    assert per_segment == {"small": 3, "second_step": 258}[name] and -(-int(lengths1.min()) // 64) == {"small": 1, "second_step": 257}[name]
    assert not dists[1, int(lengths1[1]):].any()  # a row past its cloud's length is +0: the terms are the whole padded row
    _assert_tree_bits("chamfer " + name, sums, [dists[n] for n in range(2)], per_segment, FS.CHAMFER_TELLS_APART[name])


@pytest.mark.parametrize("name", ["second_step", "empty_element"])
def test_point_edge_element_sums_have_the_bits_of_the_documented_tree(name):
    import numpy as np

    import fixed_sum_case as FS
    from pytorch3d_amd import _C

    points, pfirst, segms, sfirst, w, max_points = FS.point_edge_case(name)
    dists, _, sums = _C.point_mesh_forward("point_edge", points.to(_dev()), pfirst.to(_dev()), segms.to(_dev()), sfirst.to(_dev()),
                                           max_points, weights=w.to(_dev()), with_sums=True)
    dists, sums = dists.cpu().numpy(), sums.cpu().numpy()
    ends = pfirst.tolist() + [points.shape[0]]
    terms = [dists[ends[n]:ends[n + 1]] * np.float32(w[n]) for n in range(2)]  # one float32 multiplication
    per_segment = -(-max_points // 64)
    assert per_segment == {"second_step": 257, "empty_element": 3}[name]
    _assert_tree_bits("point_edge " + name, sums, terms, per_segment, FS.POINT_EDGE_TELLS_APART[name])
