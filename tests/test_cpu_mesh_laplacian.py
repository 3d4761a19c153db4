"""The cotangent Laplacian without a GPU: the fixture recorded from the reference (tests/golden/mesh_laplacian_ref.npz) against the
float64 truth of tests/mesh_laplacian_case.py, the package's torch formulations (mesh_laplacian_smoothing "cot" / "cotcurv",
cot_laplacian_torch, taubin_smooth_torch) inside the gates, the tables of cot_tables against a brute-force definition, and
deliberately wrong variants refused by the same gates.

Gates (mesh_laplacian_case.loss_gates): a gradient, a matrix entry, an inverse area or a smoothed vertex within FOUR times the
reference's own float32 error against the truth, per case and per quantity; a loss within four times its error plus D(n) 2^-24 S.
"""
import os
import re

import pytest
import torch

import _util as U
import mesh_laplacian_case as C

SMALL = C.SMALL


def _meshes(case, dtype=torch.float32, grad=False):
    import pytorch3d_amd as p3d

    verts_list, faces_list = C.cases()[case]
    v = [x.to(dtype).clone().requires_grad_(grad) for x in verts_list]
    return p3d.PackedMeshes(v, faces_list), v


def test_the_fixture_holds_the_references_results_and_their_errors():
    z = C.fixture()
    for case in C.cases():
        for q in ("L", "inv_areas", "taubin_1", "taubin_10", "loss_cot", "loss_cotcurv", "grad_cot_1", "grad_cot_0.37", "grad_cotcurv_1",
                  "grad_cotcurv_0.37"):
            assert C.e32(case, q) >= 0, (case, q)
        assert C.e32(case, "grad_cot_1") > 0 and C.e32(case, "grad_cotcurv_1") > 0
    for case in SMALL:
        verts, faces, nv, vert_mesh = C.packed(*C.cases()[case])
        for method in C.METHODS:
            t_loss, t_grad, _, _ = C.truth(case, method)
            assert abs(float(z[f"{case}/loss_{method}"]) - t_loss) <= C.e32(case, f"loss_{method}") * (1 + 1e-6) + 1e-12
            assert float((torch.from_numpy(z[f"{case}/grad_{method}"]).double() - t_grad).abs().max()) == C.e32(case, f"grad_{method}_1")
    assert os.path.getsize(C.GOLDEN) < 2 ** 20


@pytest.mark.parametrize("case", ("collinear", "coincident", "grid20"))
def test_the_vectorised_truth_equals_the_dense_loop(case):
    verts, faces, nv, vert_mesh = C.packed(*C.cases()[case])
    row, col, val, mag, ia = C.laplacian_entries(verts, faces)
    L, ia_dense = C.laplacian_dense(verts, faces)
    sparse = torch.zeros_like(L)
    sparse[row, col] = val
    assert float((sparse - L).abs().max()) <= 1e-12 * float(L.abs().max())
    assert float((ia - ia_dense).abs().max()) <= 1e-12 * float(ia.abs().max())
    # and the loss from the dense matrix, by autograd
    for method in C.METHODS:
        x = verts.double().clone().requires_grad_(True)
        rs = L.sum(1, keepdim=True)
        if method == "cot":
            r = (L @ x) * torch.where(rs > 0, 1.0 / rs, rs) - x
        else:
            r = (L @ x - rs * x) * (0.25 * ia_dense[:, None])
        loss = (r.norm(dim=1) / torch.tensor(nv, dtype=torch.float64)[vert_mesh]).sum() / len(nv)
        (g,) = torch.autograd.grad(loss, x)
        t_loss, t_grad, _, _ = C.truth(case, method)
        assert abs(float(loss) - t_loss) <= 1e-10 * max(1.0, abs(t_loss))
        assert float((g - t_grad).abs().max()) <= 1e-9 * max(1.0, float(t_grad.abs().max()))


def test_the_special_rows():
    """The lone vertex of the batch: "cot" r = -x with a non-zero gradient, "cotcurv" r = 0 with a zero gradient, Taubin a NaN row.
    The collinear face: area 1e-6 in both precisions, inverse vertex areas of 1e6 order.  The coincident pair: a row sum of exactly 0."""
    verts, faces, nv, vert_mesh = C.packed(*C.cases()["batch"])
    assert not bool((faces == C.LONE_VERTEX).any())
    for dtype in (torch.float32, torch.float64):
        x = verts.to(dtype)
        assert torch.equal(C.residual("cot", x, faces)[C.LONE_VERTEX], -x[C.LONE_VERTEX])
        assert torch.equal(C.residual("cotcurv", x, faces)[C.LONE_VERTEX], torch.zeros(3, dtype=dtype))
    assert float(C.truth("batch", "cot")[1][C.LONE_VERTEX].abs().max()) > 0
    assert float(C.truth("batch", "cotcurv")[1][C.LONE_VERTEX].abs().max()) == 0
    z = C.fixture()
    for it in C.TAUBIN_ITERS:
        nan_rows = torch.nonzero(torch.isnan(torch.from_numpy(z[f"batch/taubin_{it}"])).any(1)).flatten().tolist()
        assert nan_rows == [C.LONE_VERTEX]
    verts, faces, _, _ = C.packed(*C.cases()["collinear"])
    line = int(torch.nonzero((faces == 42).any(1))[0])  # the first face of the second mesh (ico_sphere(1) has 42 vertices)
    for dtype in (torch.float32, torch.float64):
        assert float(C.face_weights(verts.to(dtype), faces)[1][line]) == pytest.approx(1e-6, rel=1e-6)
    assert float(torch.from_numpy(z["collinear/inv_areas"])[43]) > 1e-1 and float(torch.from_numpy(z["collinear/inv_areas"]).max()) < 1e6 + 1
    verts, faces, _, _ = C.packed(*C.cases()["coincident"])
    for dtype in (torch.float32, torch.float64):
        cot, _ = C.face_weights(verts.to(dtype), faces)
        assert float(cot[-1][0]) == 0.0 and float(cot[-1][1]) == 0.0 and float(cot[-1][2]) > 1e5
        r = C.residual("cot", verts.to(dtype), faces)
        assert torch.equal(r[-1], -verts[-1].to(dtype))


@pytest.mark.parametrize("case", list(C.cases()))
@pytest.mark.parametrize("method", C.METHODS)
def test_the_torch_formulation_is_inside_the_gates(case, method):
    import pytorch3d_amd as p3d
    from pytorch3d_amd import mesh_losses

    for g in C.GRAD_OUTPUTS:
        t_loss, t_grad, gate_l, gate_g, rec = C.loss_gates(case, method, g)
        m, v = _meshes(case, grad=True)
        before = dict(mesh_losses.CALLS)
        loss = p3d.mesh_laplacian_smoothing(m, method)
        assert mesh_losses.CALLS["cot_torch"] == before["cot_torch"] + 1 and mesh_losses.CALLS["cot_fused"] == before["cot_fused"]
        grad = torch.cat(list(torch.autograd.grad(loss * g, [x for x in v if x.shape[0]])), 0)
        err_l, err_g = abs(float(loss) - t_loss), float((grad.double() - t_grad).abs().max())
        print(f"{case} {method} x {g:g}: loss error {err_l:.2e} (gate {gate_l:.2e}), gradient error {err_g:.2e} (gate {gate_g:.2e} = 4 x {rec['E32_grad']:.2e})")
        assert err_l <= gate_l and err_g <= gate_g


@pytest.mark.parametrize("case", list(C.cases()))
def test_cot_laplacian_torch_and_taubin_torch_inside_the_gates(case):
    import pytorch3d_amd as p3d

    verts, faces, nv, _ = C.packed(*C.cases()[case])
    L, inv_areas = p3d.cot_laplacian(verts, faces)
    assert not L.is_coalesced() and inv_areas.shape == (verts.shape[0], 1)  # the reference's layout on this path
    Lc = L.coalesce()
    row, col, val, _, ia = C.laplacian_entries(verts, faces)
    assert torch.equal(Lc.indices()[0], row) and torch.equal(Lc.indices()[1], col)
    assert float((Lc.values().double() - val).abs().max()) <= 4 * C.e32(case, "L")
    assert float((inv_areas.reshape(-1).double() - ia).abs().max()) <= 4 * C.e32(case, "inv_areas")
    z = C.fixture()
    if case in SMALL:  # the restated chain against the recorded reference: the same operations, the same bits or next to them
        assert float((Lc.values() - torch.from_numpy(z[f"{case}/L_values"])).abs().max()) <= 2 * C.e32(case, "L")
    edges = C.edges_of(faces, verts.shape[0])
    for it in C.TAUBIN_ITERS:
        got = p3d.taubin_smooth_torch(verts, edges, C.LAMBD, C.MU, it)
        err = C.nan_aware_error(got, C.taubin(verts, edges, it))
        print(f"{case} taubin x {it}: error {err:.2e}, gate 4 x {C.e32(case, f'taubin_{it}'):.2e}")
        assert err <= 4 * C.e32(case, f"taubin_{it}")
        if case in SMALL:
            assert C.nan_aware_error(got, torch.from_numpy(z[f"{case}/taubin_{it}"])) <= 2 * C.e32(case, f"taubin_{it}")
        m, _ = _meshes(case)
        out = p3d.taubin_smoothing(m, C.LAMBD, C.MU, it)
        assert isinstance(out, p3d.PackedMeshes) and C.nan_aware_error(out.verts_packed(), got) == 0.0
        assert out.faces_packed() is m.faces_packed()


WRONG = (("cot", "cot_not_over_4"), ("cotcurv", "cot_not_over_4"), ("cot", "plain_reciprocal"), ("cotcurv", "cotcurv_without_rowsum"))


@pytest.mark.parametrize("method,variant", WRONG)
def test_wrong_variants_are_refused(method, variant):
    """Each wrong formulation, in float32, misses a gate on the batch (NaN counts as a miss).  "cot" normalises by the row sum, so the
    factor 1 / 4 cancels there: "cot_not_over_4" must be caught for "cotcurv" and is caught for "cot" through the matrix entries."""
    verts, faces, nv, vert_mesh = C.packed(*C.cases()["batch"])
    t_loss, t_grad, gate_l, gate_g, _ = C.loss_gates("batch", method)
    loss, grad, _, _ = C.evaluate(method, verts, faces, nv, vert_mesh, dtype=torch.float32, variant=variant)
    good = C.evaluate(method, verts, faces, nv, vert_mesh, dtype=torch.float32)
    assert abs(good[0] - t_loss) <= gate_l and float((good[1].double() - t_grad).abs().max()) <= gate_g  # the right one passes
    inside = abs(loss - t_loss) <= gate_l and float((grad.double() - t_grad).abs().max()) <= gate_g
    if (method, variant) == ("cot", "cot_not_over_4"):
        cot4, _ = C.face_weights(verts, faces, over=1.0)
        cot, _ = C.face_weights(verts.double(), faces)
        assert float((cot4.double() - cot).abs().max()) > 4 * C.e32("batch", "L")
        return
    assert not inside, (method, variant, loss, t_loss)


def test_the_other_taubin_grouping_differs_in_bits_and_by_roundings_only():
    """The grouping c (L x / L 1) in place of the reference's (c L x) / L 1.  It was meant to be one of the variants the gates refuse;
    they cannot: the two groupings differ by one rounding per half-step, and after ten iterations in float32 both stay within the
    gate of 4 x the reference's error -- grid20 1.32e-6 against 1.24e-6 (gate 4.96e-6), fan200 4.98e-7 against 5.63e-7 (1.90e-6),
    collinear 5.80e-7 against 5.00e-7 (2.38e-6).  What is asserted: the right grouping passes, and the two differ in bits after one
    half-step pair, so a comparison of bits can tell them apart where a gate cannot."""
    for case in ("grid20", "fan200", "collinear"):
        verts, faces, _, _ = C.packed(*C.cases()[case])
        edges = C.edges_of(faces, verts.shape[0])
        want = C.taubin(verts, edges, 10)
        right = C.nan_aware_error(C.taubin(verts, edges, 10, dtype=torch.float32), want)
        wrong = C.nan_aware_error(C.taubin(verts, edges, 10, dtype=torch.float32, variant="taubin_grouping"), want)
        assert right <= 4 * C.e32(case, "taubin_10")
        assert not torch.equal(C.taubin(verts, edges, 1, dtype=torch.float32), C.taubin(verts, edges, 1, dtype=torch.float32, variant="taubin_grouping"))
        print(f"{case}: c (Lx / tw) error {wrong:.2e}, (c Lx) / tw error {right:.2e}, gate {4 * C.e32(case, 'taubin_10'):.2e}")


@pytest.mark.parametrize("case", SMALL)
def test_the_tables_equal_a_brute_force_definition(case):
    from pytorch3d_amd import mesh_losses

    verts, faces, nv, _ = C.packed(*C.cases()[case])
    V = verts.shape[0]
    m, _ = _meshes(case)
    t = mesh_losses.topology_of(m)
    c = mesh_losses.cot_tables_of(m.faces_packed(), V, t)
    assert t.cot is c and mesh_losses.cot_tables_of(m.faces_packed(), V, t) is c and c.adj is t.adj
    alone = mesh_losses.cot_tables(faces, V)  # without a topology: the same tables
    for name in ("adj_offsets", "adj", "adj_edge", "edge_corner_offsets", "edge_corners", "inc_offsets", "inc_corners"):
        a, b = getattr(c, name), getattr(alone, name)
        assert a.dtype == torch.int32 and a.is_contiguous() and torch.equal(a, b), name
    edges = C.edges_of(faces, V).tolist()
    index = {tuple(e): i for i, e in enumerate(edges)}
    assert c.E == len(edges) == t.E and c.F == faces.shape[0] and not c.repeated
    # adj_edge: the edge id of every slot
    off, adj, adj_edge = c.adj_offsets.tolist(), c.adj.tolist(), c.adj_edge.tolist()
    for v in range(V):
        for i in range(off[v], off[v + 1]):
            assert adj_edge[i] == index[(min(v, adj[i]), max(v, adj[i]))]
    # the corners of every edge, ascending (stable), and of every vertex
    by_edge, by_vert = [[] for _ in edges], [[] for _ in range(V)]
    for f, face in enumerate(faces.tolist()):
        for k in range(3):
            a, b = face[(k + 1) % 3], face[(k + 2) % 3]
            by_edge[index[(min(a, b), max(a, b))]].append(3 * f + k)
            by_vert[face[k]].append(3 * f + k)
    eo, ec = c.edge_corner_offsets.tolist(), c.edge_corners.tolist()
    assert [ec[eo[e]:eo[e + 1]] for e in range(c.E)] == by_edge
    io, ic = c.inc_offsets.tolist(), c.inc_corners.tolist()
    assert [ic[io[v]:io[v + 1]] for v in range(V)] == by_vert
    if case == "batch":
        assert sorted(len(x) for x in by_edge)[-1] == 3 and min(len(x) for x in by_edge) == 1  # non-manifold and boundary edges


def test_the_cache_per_faces_tensor():
    from pytorch3d_amd import mesh_losses

    mesh_losses.clear_cot_tables_cache()
    _, faces, _, _ = C.packed(*C.cases()["grid20"])
    a = mesh_losses.cot_tables_of(faces, 400)
    assert mesh_losses.cot_tables_of(faces, 400) is a
    faces[0, 0] += 0  # an in-place write: another _version
    assert mesh_losses.cot_tables_of(faces, 400) is not a
    assert mesh_losses.cot_tables_of(faces.clone(), 400) is not a


def test_value_errors():
    import pytorch3d_amd as p3d
    from pytorch3d_amd import mesh_losses

    m, _ = _meshes("grid20")
    with pytest.raises(ValueError, match="Method should be one of"):
        p3d.mesh_laplacian_smoothing(m, "cotan")
    verts = torch.rand(4, 3)
    twice = p3d.PackedMeshes([verts], [torch.tensor([[0, 1, 1], [1, 2, 3]])])
    for method in C.METHODS:
        with pytest.raises(ValueError, match="names one vertex twice"):
            p3d.mesh_laplacian_smoothing(twice, method)
    with pytest.raises(ValueError, match="names one vertex twice"):
        p3d.taubin_smoothing(twice)
    with pytest.raises(ValueError, match="need faces_packed"):
        mesh_losses.laplacian_smoothing(m.verts_packed(), mesh_losses.topology_of(m), "cot")
    assert mesh_losses.cot_tables(twice.faces_packed(), 4).repeated


def test_the_abi_declares_and_exports_the_entries():
    from pytorch3d_amd import _lib

    header = open(_lib.EXTENSION_HEADER_PATH).read()
    lib = _lib.load()
    for name in ("p3di_mesh_cot_laplacian_forward_workspace_bytes", "p3di_mesh_cot_weights", "p3di_mesh_cot_inv_areas",
                 "p3di_mesh_cot_laplacian_forward", "p3di_mesh_cot_laplacian_backward", "p3di_mesh_taubin_smoothing"):
        assert re.search(r"\b%s\(" % name, header) and name in _lib.EXTENSION_SYMBOLS and name not in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert lib.p3di_mesh_cot_laplacian_forward_workspace_bytes(257) == 8 and lib.p3di_mesh_cot_laplacian_forward_workspace_bytes(0) == 0
    null = None
    assert lib.p3di_mesh_cot_weights(null, null, null, null, -1, 0, 0, 1e-12, null, null, null, null) == _lib.ERR_INVALID_ARG
    assert lib.p3di_mesh_cot_weights(null, null, null, null, 0, 0, 0, 1e-12, null, null, null, null) == _lib.OK
    assert lib.p3di_mesh_taubin_smoothing(null, null, null, 0, 0, 0.5, 0.5, 0.5, 0.5, 1e-12, 1, null, null, null) == _lib.OK
    assert lib.p3di_mesh_taubin_smoothing(null, null, null, 5, 0, 0.5, 0.5, 0.5, 0.5, 1e-12, 1, null, null, null) == _lib.ERR_INVALID_ARG
    assert "mesh_laplacian.hip" in __import__("pytorch3d_amd.build", fromlist=["SOURCES"]).SOURCES
    assert U.ROOT
