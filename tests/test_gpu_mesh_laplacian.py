"""csrc/mesh_laplacian.hip on the MI355X: mesh_laplacian_smoothing "cot" / "cotcurv" forward and backward, cot_laplacian, taubin_smoothing
and the two patches of pytorch3d_amd.shim.

Inputs and yardsticks: tests/mesh_laplacian_case.py -- the five-mesh batch of the other regularisers, a collinear face, a coincident
pair, a fan of 200 faces round one vertex, a 20 x 20 grid and a 257 x 257 grid, each restated in float64 and differentiated by autograd.
Gates: a gradient, a matrix entry, an inverse area or a smoothed vertex within FOUR times the error the reference's own float32 code
makes on the CPU against that truth (tests/golden/mesh_laplacian_ref.npz, per case and per quantity); a loss within four times its
error plus D(n) 2^-24 S, D(n) = 8 + ceil(ceil(n / 256) / 256) + 8 the depth of the kernels' sum tree and S the float64 sum of the
absolute terms.
"""
import contextlib
import json
import os
import subprocess
import sys

import pytest
import torch

import _util as U
import mesh_laplacian_case as C

pytestmark = pytest.mark.gpu

CASES = list(C.cases())


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


@contextlib.contextmanager
def _profile():
    from pytorch3d_amd import _lib

    ran = {}
    _lib.load().p3d_profile_reset()
    _lib.load().p3d_profile_enable(1)
    try:
        yield ran
        ran.update(_lib.profile_snapshot())
    finally:
        _lib.load().p3d_profile_enable(0)


def _meshes(case, grad=False, dtype=torch.float32, device=None):
    import pytorch3d_amd as p3d

    d = _dev() if device is None else device
    verts_list, faces_list = C.cases()[case]
    v = [x.detach().to(device=d, dtype=dtype, copy=True).requires_grad_(grad) for x in verts_list]  # (never the case's own tensors)
    return p3d.PackedMeshes(v, [f.to(d) for f in faces_list]), v


def _run(case, method, grad_output=1.0):
    import pytorch3d_amd as p3d

    m, v = _meshes(case, grad=True)
    loss = p3d.mesh_laplacian_smoothing(m, method)
    grads = torch.autograd.grad(loss * grad_output if grad_output != 1.0 else loss, [x for x in v if x.shape[0]])
    return loss.detach(), torch.cat(list(grads), 0)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("method", C.METHODS)
def test_loss_and_gradient_within_the_gates(case, method):
    from pytorch3d_amd import mesh_losses

    for g in C.GRAD_OUTPUTS:
        t_loss, t_grad, gate_l, gate_g, rec = C.loss_gates(case, method, g)
        before = dict(mesh_losses.CALLS)
        with _profile() as ran:
            loss, grad = _run(case, method, g)
        assert {"mesh_cot_weights", "mesh_cot_laplacian_forward", "mesh_cot_laplacian_backward"} <= set(ran), f"the HIP kernels did not run: {sorted(ran)}"
        assert mesh_losses.CALLS["cot_fused"] == before["cot_fused"] + 1 and mesh_losses.CALLS["cot_torch"] == before["cot_torch"]
        assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
        err_l, err_g = abs(float(loss) - t_loss), float((grad.cpu().double() - t_grad).abs().max())
        print(f"{case} {method} x {g:g}: loss {float(loss):.9g} (truth {t_loss:.9g}) error {err_l:.2e}, gate {gate_l:.2e} = 4 x {rec['E32_loss']:.2e} + "
              f"{rec['D']} x 2^-24 x {rec['S']:.3g}; gradient error {err_g:.2e}, gate {gate_g:.2e} = 4 x {rec['E32_grad']:.2e} (n = {rec['n']}, "
              f"largest gradient {float(t_grad.abs().max()):.2e})")
        assert rec["E32_grad"] > 0
        assert err_l <= gate_l, (err_l, gate_l)
        assert err_g <= gate_g, (err_g, gate_g)
        if case == "batch":  # the vertex without a face: "cot" r = -x, a non-zero gradient; "cotcurv" r = 0, a zero gradient
            row = grad[C.LONE_VERTEX].cpu()
            assert (float(row.abs().max()) > 0) if method == "cot" else torch.equal(row, torch.zeros(3))


@pytest.mark.parametrize("method", C.METHODS)
def test_the_same_bits_on_two_runs_two_streams_and_under_the_strict_flag(method):
    for case in ("batch", "fan200"):
        first = _run(case, method)
        torch.cuda.synchronize()
        runs = {"a second call": _run(case, method)}
        side = torch.cuda.Stream(device=_dev())
        with torch.cuda.stream(side):
            runs["another stream"] = _run(case, method)
        side.synchronize()
        with _flag(True):  # nothing to refuse: no atomic in either direction; the tables are rebuilt under the flag too
            runs["the strict flag"] = _run(case, method)
        torch.cuda.synchronize()
        for how, (loss, grad) in runs.items():
            assert torch.equal(loss, first[0]), f"{case}: the loss differs with {how}"
            assert torch.equal(grad, first[1]), f"{case}: the gradient differs with {how}"


@pytest.mark.parametrize("case", CASES)
def test_cot_laplacian_values_and_inverse_areas(case):
    import pytorch3d_amd as p3d
    from pytorch3d_amd import mesh_losses

    verts, faces, _, _ = C.packed(*C.cases()[case])
    row, col, val, _, ia = C.laplacian_entries(verts, faces)
    before = dict(mesh_losses.CALLS)
    with _profile() as ran:
        L, inv_areas = p3d.cot_laplacian(verts.to(_dev()), faces.to(_dev()))
    assert {"mesh_cot_weights", "mesh_cot_inv_areas"} <= set(ran), sorted(ran)
    assert mesh_losses.CALLS["cot_laplacian_fused"] == before["cot_laplacian_fused"] + 1
    assert L.is_sparse and L.is_coalesced() and L.shape == (verts.shape[0],) * 2 and L.dtype == torch.float32 and L.is_cuda
    assert inv_areas.shape == (verts.shape[0], 1) and inv_areas.dtype == torch.float32
    assert torch.equal(L.indices()[0].cpu(), row) and torch.equal(L.indices()[1].cpu(), col)
    err_l = float((L.values().cpu().double() - val).abs().max())
    err_a = float((inv_areas.reshape(-1).cpu().double() - ia).abs().max())
    print(f"{case}: entries of L error {err_l:.2e}, gate 4 x {C.e32(case, 'L'):.2e}; inv_areas error {err_a:.2e}, gate 4 x {C.e32(case, 'inv_areas'):.2e}")
    assert err_l <= 4 * C.e32(case, "L") and err_a <= 4 * C.e32(case, "inv_areas")
    if case in ("batch", "collinear"):  # the dense form, as a user of the reference's uncoalesced L compares
        dense = torch.zeros((verts.shape[0],) * 2, dtype=torch.float64)
        dense[row, col] = val
        assert float((L.to_dense().cpu().double() - dense).abs().max()) <= 4 * C.e32(case, "L")
        again = p3d.cot_laplacian(verts.to(_dev()), faces.to(_dev()))  # other tensors: the tables are rebuilt, the same bits
        assert torch.equal(again[0].values(), L.values()) and torch.equal(again[1], inv_areas)


@pytest.mark.parametrize("case", CASES)
def test_taubin_smoothing(case):
    import pytorch3d_amd as p3d
    from pytorch3d_amd import mesh_filtering

    verts, faces, _, _ = C.packed(*C.cases()[case])
    edges = C.edges_of(faces, verts.shape[0])
    m, _ = _meshes(case)
    for it in C.TAUBIN_ITERS:
        want = C.taubin(verts, edges, it)
        before = dict(mesh_filtering.CALLS)
        with _profile() as ran:
            out = p3d.taubin_smoothing(m, C.LAMBD, C.MU, it)
        assert "mesh_taubin_smoothing" in ran and mesh_filtering.CALLS["fused"] == before["fused"] + 1, sorted(ran)
        # a PackedMeshes round trip: the same topology object, new vertices, the input untouched
        assert isinstance(out, p3d.PackedMeshes) and out.faces_packed() is m.faces_packed() and out.verts_packed() is not m.verts_packed()
        assert torch.equal(m.verts_packed().cpu(), verts)
        assert [tuple(x.shape) for x in out.verts_list()] == [tuple(x.shape) for x in C.cases()[case][0]]
        err = C.nan_aware_error(out.verts_packed().cpu(), want)
        print(f"{case} x {it}: error {err:.2e}, gate 4 x {C.e32(case, f'taubin_{it}'):.2e}")
        assert err <= 4 * C.e32(case, f"taubin_{it}")
        if case == "batch":  # the vertex without a neighbour: the reference's NaN row, and no other
            assert torch.nonzero(torch.isnan(out.verts_packed()).any(1)).flatten().tolist() == [C.LONE_VERTEX]
        assert torch.equal(p3d.taubin_smoothing(m, C.LAMBD, C.MU, it).verts_packed().isnan(), out.verts_packed().isnan())
        again = p3d.taubin_smoothing(m, C.LAMBD, C.MU, it).verts_packed()
        assert C.nan_aware_error(again.cpu(), out.verts_packed().cpu()) == 0.0  # the same bits on a second run
    zero = p3d.taubin_smoothing(m, C.LAMBD, C.MU, 0)
    assert torch.equal(zero.verts_packed(), m.verts_packed()) and zero.verts_packed() is not m.verts_packed()


def test_what_the_kernels_do_not_take_goes_to_the_formulation():
    import pytorch3d_amd as p3d
    from pytorch3d_amd import mesh_filtering, mesh_losses

    case = "grid20"
    verts, faces, _, _ = C.packed(*C.cases()[case])
    edges = C.edges_of(faces, verts.shape[0])
    want = C.taubin(verts, edges, 1)

    def counts():
        return dict(mesh_losses.CALLS), dict(mesh_filtering.CALLS)

    # float64 on the GPU and CPU tensors: the torch formulation of the loss
    for kw in ({"dtype": torch.float64}, {"device": torch.device("cpu")}):
        (a, _), (m, v) = counts(), _meshes(case, grad=True, **kw)
        loss = p3d.mesh_laplacian_smoothing(m, "cot")
        torch.autograd.grad(loss, v)
        (b, _) = counts()
        assert b["cot_torch"] == a["cot_torch"] + 1 and b["cot_fused"] == a["cot_fused"], kw
    t_loss = C.truth(case, "cot")[0]
    assert abs(float(p3d.mesh_laplacian_smoothing(_meshes(case, dtype=torch.float64)[0], "cot")) - t_loss) < 1e-8  # (the weight 1 / V_n is a float32 there: 2^-24 of the loss)
    # cot_laplacian: a gradient wanted, or the CPU: the chain (and the reference's uncoalesced layout)
    d = _dev()
    for v, f in ((verts.to(d).requires_grad_(True), faces.to(d)), (verts, faces)):
        (a, _) = counts()
        L, _ = p3d.cot_laplacian(v, f)
        (b, _) = counts()
        assert b["cot_laplacian_torch"] == a["cot_laplacian_torch"] + 1 and b["cot_laplacian_fused"] == a["cot_laplacian_fused"]
        assert not L.is_coalesced()
    with torch.no_grad():  # ... but not under no_grad: the reference's losses call it there
        (a, _) = counts()
        p3d.cot_laplacian(verts.to(d).requires_grad_(True), faces.to(d))
        assert counts()[0]["cot_laplacian_fused"] == a["cot_laplacian_fused"] + 1
    # taubin: vertices that require grad take the chain and autograd differentiates through the weights
    (_, a), (m, v) = counts(), _meshes(case, grad=True)
    out = p3d.taubin_smoothing(m, C.LAMBD, C.MU, 1)
    (_, b) = counts()
    assert b["chain"] == a["chain"] + 1 and b["fused"] == a["fused"] and out.verts_packed().requires_grad
    assert C.nan_aware_error(out.verts_packed().detach().cpu(), want) <= 4 * C.e32(case, "taubin_1")
    (g,) = torch.autograd.grad(out.verts_packed().square().sum(), v)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    for kw in ({"dtype": torch.float64}, {"device": torch.device("cpu")}):
        (_, a), (m, _) = counts(), _meshes(case, **kw)
        out = p3d.taubin_smoothing(m, C.LAMBD, C.MU, 1)
        assert counts()[1]["chain"] == a["chain"] + 1
        assert C.nan_aware_error(out.verts_packed().cpu(), want) <= 4 * C.e32(case, "taubin_1")
    # a repeated vertex is refused, an unknown method too
    twice = p3d.PackedMeshes([torch.rand(4, 3, device=d)], [torch.tensor([[0, 1, 1], [1, 2, 3]], device=d)])
    with pytest.raises(ValueError, match="names one vertex twice"):
        p3d.mesh_laplacian_smoothing(twice, "cotcurv")
    with pytest.raises(ValueError, match="Method should be one of"):
        p3d.mesh_laplacian_smoothing(_meshes(case)[0], "cotangent")


def test_the_tables_are_built_once_per_topology():
    import pytorch3d_amd as p3d
    from pytorch3d_amd import mesh_losses

    m, _ = _meshes("grid20")
    t = mesh_losses.topology_of(m)
    assert t.cot is None
    p3d.mesh_laplacian_smoothing(m)  # "uniform" alone pays nothing
    assert t.cot is None
    p3d.mesh_laplacian_smoothing(m, "cot")
    c = t.cot
    assert c is not None and c.adj is t.adj and c.adj_edge.is_cuda and c.adj_edge.dtype == torch.int32
    moved = m.update_verts_packed(m.verts_packed() + 0.01)
    p3d.mesh_laplacian_smoothing(moved, "cotcurv")
    assert mesh_losses.topology_of(moved).cot is c


# ---- the shim ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim_report():
    if not os.path.isdir(os.path.join(U.ROOT, "oracle", "_ref", "reference_py", "pytorch3d", "loss")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(U.ROOT, "tests", "shim_mesh_laplacian_case.py")], capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    print(json.dumps(rec))
    return rec


def test_the_references_cot_losses_and_taubin_run_on_the_kernels(shim_report):
    r = shim_report
    assert r["patched_everywhere"]
    for name, c in r["losses"].items():
        assert c["loss_error"] <= c["loss_gate"] and c["grad_error"] <= c["grad_gate"], (name, c)
    assert r["fused_calls"] == {"cot_laplacian": 2, "taubin_smoothing": 2}
    assert r["fallback_calls"] == {"cot_laplacian": 0, "taubin_smoothing": 0}
    assert r["loss_patch_counts_a_fallback"] == 2  # the patched loss keeps its predicate: "cot" / "cotcurv" are the reference's loss
    for it, c in r["taubin"].items():
        assert c["error"] <= c["gate"] and c["is_reference_meshes"] and c["no_textures"], (it, c)


def test_a_cpu_mesh_and_a_repeated_vertex_fall_back_and_uninstall_restores(shim_report):
    r = shim_report
    assert r["cpu_fallback_calls"] == {"cot_laplacian": 1, "taubin_smoothing": 1} and r["cpu_fused_calls"] == {"cot_laplacian": 0, "taubin_smoothing": 0}
    assert r["repeated_fallback_calls"] == {"cot_laplacian": 1, "taubin_smoothing": 1}
    assert r["repeated_fused_calls"] == {"cot_laplacian": 0, "taubin_smoothing": 0}
    assert r["grad_wanted_fallback_calls"] == {"cot_laplacian": 1, "taubin_smoothing": 1}
    assert r["restored"]
