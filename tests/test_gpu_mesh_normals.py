"""csrc/normals.hip on the MI355X: face areas / normals (forward, backward) and vertex normals in gather form (forward, backward).

Input (tests/mesh_normals_case.py): one packed batch of 433 vertices and 649 faces -- a noisy icosphere, a torus, a fan whose apex
has valence 200 and an "eps group" whose vertex sums are exactly zero (the max(|s|, 1e-6) branch both ways) -- plus the trivial
sizes F = 1 and V = 0 / F = 0.

  1. face areas / normals against the reference's CPU kernels (oracle/_ref/p3d_ref_cpu.so), gates of tests/test_cpu_aux_ops.py, through
     the ctypes and the pybind flavour; the backward under the strict deterministic flag;
  2. vertex normals forward against the float64 restatement; 3. backward against float64 autograd, regular vertices and eps group gated
     separately.  Gates of 2 and 3: FOUR times the error the reference's own float32 formulation makes against the same truth on
     this input on the CPU, computed here at run time -- the factor covers another order of summation over at most 200 terms
     (re-ordering the faces alone moves the reference's float32 result by 1.2e-7 on this input);
  4. bits: equal between two calls, two streams, a fresh and a pre-dirtied workspace, with the strict flag on and off;
  5. the patched Meshes._compute_vertex_normals and a SoftPhong render through it (a child process: tests/shim_mesh_normals_case.py);
  6. the reference's own tests/test_face_areas_normals.py through tests/run_reference_suite.py (a child process).
"""
import contextlib
import json
import os
import subprocess
import sys

import pytest
import torch

import _util as U
import mesh_normals_case as C
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = U.ROOT
STAGE = os.path.join(ROOT, "oracle", "_ref", "reference_py")


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


@pytest.fixture(scope="module")
def case():
    """The input, the truths and the reference's own float32 errors against them -- computed once, never modified."""
    verts, faces, eps = C.build_input()
    gen = torch.Generator().manual_seed(5)
    grad = torch.randn(verts.shape, generator=gen)
    truth_n = C.restated_forward(verts.double(), faces)[0]
    _, truth_g = C.autograd_truth(verts, faces, grad)
    # the reference's float32 formulation on the CPU: the scale of the gates
    v32 = verts.clone().requires_grad_(True)
    ref_n = C.reference_verts_normals(v32, faces)
    (ref_g,) = torch.autograd.grad(ref_n, v32, grad)
    c = {"verts": verts, "faces": faces, "eps": eps, "grad": grad, "truth_n": truth_n, "truth_g": truth_g,
         "ref_err_n": float((ref_n.detach().double() - truth_n).abs().max())}
    for name, group in (("regular", ~eps), ("eps", eps)):
        scale = float(truth_g[group].abs().max())
        c["scale_" + name] = scale
        c["ref_err_g_" + name] = float((ref_g.double() - truth_g)[group].abs().max()) / scale
    print(f"reference float32 on the CPU against the float64 truth: normals {c['ref_err_n']:.2e}; gradient relative to the group's "
          f"largest, regular {c['ref_err_g_regular']:.2e} (largest {c['scale_regular']:.2e}), eps group {c['ref_err_g_eps']:.2e} "
          f"(largest {c['scale_eps']:.2e})")
    assert c["ref_err_n"] > 0 and c["ref_err_g_regular"] > 0 and c["ref_err_g_eps"] > 0
    return c


def _on_gpu(c):
    d = _dev()
    return c["verts"].to(d), c["faces"].to(d)


# ---- 1. face areas and normals ---------------------------------------------------------------------------------------------------
def _ref():
    m = orc.ref_module()
    if m is None or not hasattr(m, "face_areas_normals_forward"):
        pytest.skip("oracle/_ref/p3d_ref_cpu.so not built")
    return m


def _face_ops(flavour):
    """The two face operators: of _aux_ops (ctypes), of the compiled module (pybind), or what shim.make_module("pybind") serves."""
    if flavour == "ctypes":
        from pytorch3d_amd import _aux_ops

        return _aux_ops
    if flavour == "pybind":
        from pytorch3d_amd import build_bind

        return build_bind.load()
    from pytorch3d_amd import shim

    return shim.make_module("pybind")


FLAVOURS = ["ctypes", "pybind", "make_module_pybind"]


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_face_areas_normals_match_the_reference_cpu_kernels(case, flavour):
    ref, ops = _ref(), _face_ops(flavour)
    from pytorch3d_amd import _aux_ops, _lib

    if flavour == "make_module_pybind":  # served from the compiled module, not the ctypes functions handed through
        assert ops.face_areas_normals_forward is not _aux_ops.face_areas_normals_forward
        assert ops.face_areas_normals_backward is not _aux_ops.face_areas_normals_backward

    v, f = case["verts"], case["faces"]
    vg, fg = _on_gpu(case)
    gen = torch.Generator().manual_seed(9)
    ga, gn = torch.randn(f.shape[0], generator=gen), torch.randn(f.shape[0], 3, generator=gen)
    want_a, want_n = ref.face_areas_normals_forward(v, f)
    want_g = ref.face_areas_normals_backward(ga, gn, v, f)
    assert float(want_a.min()) == 0.0, "the input holds a degenerate face"
    _lib.load().p3d_profile_reset()
    _lib.load().p3d_profile_enable(1)
    try:
        a, n = ops.face_areas_normals_forward(vg, fg)
        g = ops.face_areas_normals_backward(ga.to(vg.device), gn.to(vg.device), vg, fg)
        ran = _lib.profile_snapshot()
    finally:
        _lib.load().p3d_profile_enable(0)
    assert "face_areas_normals_forward" in ran and "face_areas_normals_backward" in ran, f"the HIP kernels did not run: {sorted(ran)}"
    if flavour == "make_module_pybind":
        # the compiled path ran: the same launches again with the ctypes operators made unusable
        from pytorch3d_amd import mesh_normals

        def unusable(*_):
            raise AssertionError("make_module('pybind') went through the ctypes operators")

        keep_mn = mesh_normals.face_areas_normals_forward, mesh_normals.face_areas_normals_backward
        mesh_normals.face_areas_normals_forward = mesh_normals.face_areas_normals_backward = unusable
        try:
            a2, _ = ops.face_areas_normals_forward(vg, fg)
            g2 = ops.face_areas_normals_backward(ga.to(vg.device), gn.to(vg.device), vg, fg)
        finally:
            mesh_normals.face_areas_normals_forward, mesh_normals.face_areas_normals_backward = keep_mn
        assert torch.equal(a2, a) and g2.shape == g.shape
        # and what is not float32 on the GPU still takes the torch formulation through the same module
        a_cpu, _ = ops.face_areas_normals_forward(v, f)
        assert torch.allclose(a_cpu, want_a, atol=1e-6)
    err_a, err_n = float((a.cpu() - want_a).abs().max()), float((n.cpu() - want_n).abs().max())
    err_g, scale = float((g.cpu() - want_g).abs().max()), float(want_g.abs().max())
    # the analytic derivative is NOT what the reference returns (its c_x-for-c_y term): the torch autograd of the forward differs
    v64 = v.double().requires_grad_(True)
    c = torch.cross(v64[f[:, 1]] - v64[f[:, 0]], v64[f[:, 2]] - v64[f[:, 0]], dim=1)
    nrm = c.norm(dim=1)
    (analytic,) = torch.autograd.grad([nrm / 2, c / nrm.clamp_min(1e-6)[:, None]], v64, [ga.double(), gn.double()])
    print(f"[{flavour}] areas {err_a:.2e}, normals {err_n:.2e} (gate 1e-6); backward {err_g:.2e} against the reference's CPU kernel, gate "
          f"{2e-5 * scale:.2e} = 2e-5 x {scale:.2e}; the analytic derivative is {float((analytic - want_g.double()).abs().max()):.2e} away from it")
    assert torch.allclose(a.cpu(), want_a, atol=1e-6) and torch.allclose(n.cpu(), want_n, atol=1e-6)
    assert torch.allclose(g.cpu(), want_g, atol=2e-5 * scale)
    # the degenerate face's gradients (1e6) set that scale: the same gate again on the other vertices alone, relative to their largest
    rest = ~case["eps"]
    gate_rest = 2e-5 * float(want_g[rest].abs().max())
    assert torch.allclose(g.cpu()[rest], want_g[rest], atol=gate_rest)
    # the c_x deviation is in the input: on those vertices the analytic derivative lies far outside the gate the kernel has to meet,
    # so a kernel that returned the analytic derivative would fail above
    away = float((analytic - want_g.double())[rest].abs().max())
    print(f"[{flavour}] regular vertices: gate {gate_rest:.2e}, the analytic derivative is {away:.2e} from the reference's")
    assert away > 100 * gate_rest, (away, gate_rest)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_face_normals_backward_under_the_strict_flag_repeats_its_bits_on_two_streams(case, flavour):
    ops = _face_ops(flavour)
    vg, fg = _on_gpu(case)
    gen = torch.Generator().manual_seed(9)
    ga, gn = torch.randn(fg.shape[0], generator=gen).to(vg.device), torch.randn(fg.shape[0], 3, generator=gen).to(vg.device)
    want = ops.face_areas_normals_backward(ga, gn, vg, fg)  # the atomic scatter: the value gate of the ordered one
    torch.cuda.synchronize()
    with _flag(True):
        first = ops.face_areas_normals_backward(ga, gn, vg, fg)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=vg.device)
        with torch.cuda.stream(side):
            second = ops.face_areas_normals_backward(ga, gn, vg, fg)
        side.synchronize()
    assert torch.equal(first, second)
    assert torch.allclose(first, want, atol=2e-5 * float(want.abs().max()))


def test_face_areas_normals_autograd_node_and_trivial_sizes(case):
    import pytorch3d_amd as p3d
    from pytorch3d_amd import _aux_ops, mesh_normals

    vg, fg = _on_gpu(case)
    d = vg.device
    gen = torch.Generator().manual_seed(9)
    ga, gn = torch.randn(fg.shape[0], generator=gen).to(d), torch.randn(fg.shape[0], 3, generator=gen).to(d)
    v = vg.clone().requires_grad_(True)
    a, n = p3d.face_areas_normals(v, fg)
    torch.autograd.backward([a, n], [ga, gn])
    raw = mesh_normals.face_areas_normals_backward(ga, gn, vg, fg)
    assert torch.allclose(v.grad, raw, atol=2e-5 * float(raw.abs().max()))  # (two atomic scatters: not bit-equal)
    # F = 1
    v1 = torch.tensor([[0.0, 0, 0], [2, 0, 0], [0, 3, 0]], device=d)
    f1 = torch.tensor([[0, 1, 2]], device=d)
    a1, n1 = mesh_normals.face_areas_normals_forward(v1, f1)
    assert a1.tolist() == [3.0] and n1.tolist() == [[0.0, 0.0, 1.0]]
    g1 = mesh_normals.face_areas_normals_backward(torch.ones(1, device=d), torch.zeros(1, 3, device=d), v1, f1)
    assert torch.allclose(g1.cpu(), torch.tensor([[-1.5, -1.0, 0.0], [1.5, 0.0, 0.0], [0.0, 1.0, 0.0]]), atol=1e-6)
    # an id out of range: that face is NaN, nothing else is
    a2, n2 = mesh_normals.face_areas_normals_forward(v1, torch.tensor([[0, 1, 2], [0, 1, 3]], device=d))
    assert a2[0].item() == 3.0 and torch.isnan(a2[1]).item() and bool(torch.isnan(n2[1]).all())
    # F = 0 and V = 0: empty outputs, the torch formulation behind the `_C` operators as before
    e_v, e_f = torch.zeros((0, 3), device=d), torch.zeros((0, 3), dtype=torch.int64, device=d)
    a0, n0 = mesh_normals.face_areas_normals_forward(v1, e_f)
    assert a0.shape == (0,) and n0.shape == (0, 3)
    assert float(mesh_normals.face_areas_normals_backward(a0, n0, v1, e_f).abs().max()) == 0.0
    a0, n0 = _aux_ops.face_areas_normals_forward(e_v, e_f)
    assert a0.shape == (0,) and n0.shape == (0, 3)
    assert _aux_ops.face_areas_normals_backward(a0, n0, e_v, e_f).shape == (0, 3)


# ---- 2. - 4. vertex normals ------------------------------------------------------------------------------------------------------
def test_verts_normals_forward_within_four_times_the_references_own_error(case):
    import pytorch3d_amd as p3d

    vg, fg = _on_gpu(case)
    n = p3d.verts_normals(vg, fg).cpu()
    err = float((n.double() - case["truth_n"]).abs().max())
    # the reference's float32 formulation on the CPU, this input: 2.0e-07 (printed by the fixture; recomputed at every run)
    gate = 4 * case["ref_err_n"]
    print(f"vertex normals against the float64 restatement: {err:.2e}, gate {gate:.2e} = 4 x {case['ref_err_n']:.2e}")
    assert err <= gate
    assert float(n[case["eps"]].abs().max()) == 0.0, "the eps group's sums are exactly zero in any order"
    apex = 162 + 63
    assert int((case["faces"] == apex).sum()) == 200 and abs(float(n[apex].norm()) - 1.0) < 1e-6


def test_verts_normals_backward_within_four_times_the_references_own_error(case):
    import pytorch3d_amd as p3d

    vg, fg = _on_gpu(case)
    v = vg.clone().requires_grad_(True)
    p3d.verts_normals(v, fg).backward(case["grad"].to(vg.device))
    got = v.grad.cpu().double()
    assert bool(torch.isfinite(got).all())
    # the reference's float32 autograd on the CPU, this input, relative to the group's largest true gradient:
    # regular vertices 3.6e-07, eps group 5.1e-08 (printed by the fixture; recomputed at every run)
    bad = []
    for name, group in (("regular", ~case["eps"]), ("eps", case["eps"])):
        err = float((got - case["truth_g"])[group].abs().max()) / case["scale_" + name]
        gate = 4 * case["ref_err_g_" + name]
        print(f"vertex-normal gradient, {name} vertices ({int(group.sum())}): {err:.2e} of the largest ({case['scale_' + name]:.2e}), gate "
              f"{gate:.2e} = 4 x {case['ref_err_g_' + name]:.2e}")
        if not err <= gate:
            bad.append((name, err, gate))
    assert not bad, bad
    assert case["scale_eps"] > 1e5 * case["scale_regular"]


def test_verts_normals_repeat_their_bits(case):
    """Two calls, two streams, a fresh and a pre-dirtied workspace, the strict flag on and off: one repetition of each."""
    from pytorch3d_amd import mesh_normals

    vg, fg = _on_gpu(case)
    d = vg.device
    g = case["grad"].to(d)
    V, F = vg.shape[0], fg.shape[0]
    inc = mesh_normals.vert_incidence(fg, V)

    def both(face_raw=None, face_rows=None):
        n, s = mesh_normals.verts_normals_forward(vg, fg, inc[0], inc[1], face_raw=face_raw)
        return n, s, mesh_normals.verts_normals_backward(g, vg, fg, s, inc[0], inc[1], face_rows=face_rows)

    first = both()
    torch.cuda.synchronize()
    runs = {"a second call": both()}
    side = torch.cuda.Stream(device=d)
    with torch.cuda.stream(side):
        runs["another stream"] = both()
    side.synchronize()
    runs["a pre-dirtied workspace"] = both(torch.full((F * 3,), float("nan"), device=d), torch.full((F * 9,), -3e30, device=d))
    with _flag(True):
        inc_strict = mesh_normals.vert_incidence(fg, V)
        assert torch.equal(inc_strict[0], inc[0]) and torch.equal(inc_strict[1], inc[1])
        runs["the strict flag"] = both()
    torch.cuda.synchronize()
    for name, run in runs.items():
        for what, a, b in zip(("normals", "sums", "grad_verts"), first, run):
            assert torch.equal(a, b), f"{what} differ with {name}"
    # the list against the definition, on the device
    off, cor = C.brute_incidence(case["faces"], V)
    assert inc[0].tolist() == off and inc[1].tolist() == cor


def test_verts_normals_trivial_sizes():
    import pytorch3d_amd as p3d

    d = _dev()
    # F = 1 (and a vertex without a face)
    v = torch.tensor([[0.0, 0, 0], [2, 0, 0], [0, 3, 0], [1, 1, 1]], device=d, requires_grad=True)
    f = torch.tensor([[0, 1, 2]], device=d)
    n = p3d.verts_normals(v, f)
    assert n.tolist() == [[0.0, 0.0, 1.0]] * 3 + [[0.0, 0.0, 0.0]]
    n.backward(torch.tensor([[1.0, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], device=d))
    _, want = C.autograd_truth(v.detach().cpu(), f.cpu(), torch.tensor([[1.0, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]]))
    assert torch.allclose(v.grad.cpu().double(), want, atol=1e-6)
    # an id out of range: its face is NaN, so are the sums of the face's other vertices and every gradient they reach -- never a
    # finite g / 1e-6 from the clamped branch
    vb = v.detach().clone().requires_grad_(True)
    nb = p3d.verts_normals(vb, torch.tensor([[0, 1, 2], [0, 1, 7]], device=d))
    assert bool(torch.isnan(nb[:2]).all()) and nb[2].tolist() == [0.0, 0.0, 1.0] and nb[3].tolist() == [0.0, 0.0, 0.0]
    nb.backward(torch.ones_like(nb))
    assert bool(torch.isnan(vb.grad[:3]).all()) and vb.grad[3].tolist() == [0.0, 0.0, 0.0]
    # F = 0: every vertex is without a face; V = 0: nothing
    e_f = torch.zeros((0, 3), dtype=torch.int64, device=d)
    v0 = v.detach().clone().requires_grad_(True)
    n0 = p3d.verts_normals(v0, e_f)
    assert n0.shape == (4, 3) and float(n0.abs().max()) == 0.0
    n0.backward(torch.ones_like(n0))
    assert float(v0.grad.abs().max()) == 0.0
    assert p3d.verts_normals(torch.zeros((0, 3), device=d), e_f).shape == (0, 3)
    # what is not float32 on the GPU raises
    with pytest.raises(RuntimeError):
        p3d.verts_normals(v.detach().double(), f)
    with pytest.raises(RuntimeError):
        p3d.verts_normals(v.detach().cpu(), f.cpu())


# ---- 5. the shim -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim_report():
    if not os.path.isdir(os.path.join(STAGE, "pytorch3d", "renderer")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_mesh_normals_case.py")], capture_output=True, text=True,
                         timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    print(json.dumps(rec))
    return rec


def test_patched_meshes_compute_their_vertex_normals_with_the_fused_node(shim_report):
    r = shim_report
    assert r["fused_calls"] == 1 and r["calls_when_cached"] == 0
    assert r["patched_vs_reference_method"] <= 4 * r["reference_cpu_error"]
    assert r["patched_vs_truth"] <= 4 * r["reference_cpu_error"]


def test_offset_verts_hands_the_incidence_list_on(shim_report):
    r = shim_report
    assert r["offset_fused_calls"] == 1 and r["offset_reuses_list"]
    assert r["offset_vs_truth"] <= 4 * r["offset_reference_cpu_error"]


def test_a_mesh_on_the_cpu_takes_the_references_method_and_uninstall_restores_it(shim_report):
    r = shim_report
    assert r["cpu_fallback_calls"] == 1 and r["cpu_fused_calls"] == 0 and r["cpu_equals_reference_formula"]
    assert r["restored"]


def test_soft_phong_render_gradient_through_the_fused_vertex_normals(shim_report):
    r = shim_report["render"]
    assert r["fused_calls"] >= 1 and r["fused_calls_when_restored"] == 0 and r["finite"] and r["largest"] > 0
    # the package's gradient gate (tests/_util.assert_face_grads_vs_truth: rtol 5e-3), here of the largest entry
    assert r["max_diff"] <= 5e-3 * r["largest"], r


# ---- 6. the reference's own test module ------------------------------------------------------------------------------------------
def _reference_module(out_dir, tag, *flags):
    out = os.path.join(str(out_dir), f"ref_suite_face_areas_normals_{tag}.json")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ref_face_areas_normals_case.py"), "--out", out, *flags],
                         capture_output=True, text=True, timeout=240)
    print(res.stdout[-2000:])
    assert res.returncode == 0, res.stderr[-3000:]
    with open(out) as f:
        report = json.load(f)
    cases = report["test_face_areas_normals"]
    assert "__import__" not in cases, cases
    return {tid.rsplit(".", 1)[-1]: r for tid, r in cases.items()}, report["__calls__"]["hip"]


def test_the_references_own_face_areas_normals_tests_reach_the_hip_kernels(tmp_path):
    """tests/test_face_areas_normals.py of the reference, unmodified: no case that passes on the torch formulation (the dispatch of
    _aux_ops switched off: what ran before the kernels) may fail on the kernels.  Outcomes per case: DESIGN.md 8.10."""
    if not os.path.isdir(os.path.join(STAGE, "pytorch3d", "renderer")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    before, _ = _reference_module(tmp_path, "torch", "--torch-formulation")
    after, calls = _reference_module(tmp_path, "hip")
    print({name: (before[name]["outcome"], after.get(name, {}).get("outcome")) for name in before})
    assert set(after) == set(before) and len(after) >= 4
    behind = [(name, after[name]["msg"][-400:]) for name in before if before[name]["outcome"] == "pass" and after[name]["outcome"] != "pass"]
    assert not behind, behind
    for name in ("test_face_areas_normals_cpu", "test_nonfloats_cpu"):  # the reference's CPU kernels on both sides
        assert after[name]["outcome"] == "pass", after[name]
    assert calls.get("face_areas_normals_forward", 0) > 0 and calls.get("face_areas_normals_backward", 0) > 0, calls
