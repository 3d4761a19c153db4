"""iterative_closest_point / corresponding_points_alignment without a GPU: the torch formulation (the reference's chain restated over
this package's knn_points) through the gates of tests/points_alignment_case.py in float32, three deliberately wrong variants refused
by the same gates, the C ABI's argument checks (no launch), and the unmodified reference's functions through the shim on CPU tensors."""
import importlib
import json
import os
import re
import subprocess
import sys
import warnings

import pytest
import torch

import points_alignment_case as C
from pytorch3d_amd import _C, _lib, build, shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PA = importlib.import_module("pytorch3d_amd.points_alignment")
ENTRIES = ("p3di_icp_workspace_bytes", "p3di_icp_match", "p3di_icp_iteration", "p3di_points_alignment")


def test_fixture_holds_the_reference_figures_and_no_gate_is_zero_by_accident():
    z = C.fixture()
    for kind, cases, names in (("align", C.ALIGN_CASES, C.ALIGN_QUANTITIES), ("icp", C.ICP_CASES, C.ICP_QUANTITIES)):
        for case in cases:
            C.check_inputs(kind, case)
            assert z[C.key(kind, case, "err32")].shape == (len(names),)
        for family in sorted({c[0] for c in cases}):
            g = C.gates(kind, family)
            print(kind, family, {q: "%.3g" % v for q, v in g.items()})
            assert 0 < g["R"] < 1e-4 and 0 < g["T"] < 1e-3  # float32 figures, and a family's largest: never a single case's 0
            assert len([c for c in cases if c[0] == family]) >= 2
    for case in C.ICP_CASES:
        its = int(z[C.key("icp", case, "iterations")])
        assert z[C.key("icp", case, "idx")].shape[0] == its and 1 <= its <= 100
        assert bool(z[C.key("icp", case, "converged")]) != (case[1] in C.UNCONVERGED)
    first = z[C.key("icp", ("icp_rigid", "200x300", 0), "first")].tolist()
    assert len(set(first)) >= 2, first  # b = 3 with clouds that converge at different iterations


@pytest.mark.parametrize("case", C.ALIGN_CASES, ids=C.case_id)
def test_alignment_formulation_passes_the_reference_gates(case):
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        before = PA.CALLS["chain"]
        out = C.run_align(PA.corresponding_points_alignment, case)
    assert PA.CALLS["chain"] == before + 1 and isinstance(out, PA.SimilarityTransform)
    C.check("align", case, C.align_values(out), "chain")
    assert len([w for w in seen if "Excessively low rank" in str(w.message)]) == (1 if case[1] in ("exact", "zero") else 0)
    # float64: the truth itself, far inside every gate
    err = C.errors(C.align_values(C.run_align(PA.corresponding_points_alignment_torch, case, dtype=torch.float64)), C.truth("align", case))
    assert max(err.values()) <= 1e-9, err


@pytest.mark.parametrize("case", C.ICP_CASES, ids=C.case_id)
def test_icp_formulation_passes_the_reference_gates(case):
    z = C.fixture()
    record = []
    sol = C.run_icp(PA.iterative_closest_point_torch, case, _record=record)
    its = int(z[C.key("icp", case, "iterations")])
    assert len(sol.t_history) == its == len(record) and sol.converged == bool(z[C.key("icp", case, "converged")])
    C.check("icp", case, C.icp_values(sol), "chain")
    assert torch.equal(torch.stack(record), z[C.key("icp", case, "idx")].long())  # the float64 run's neighbours, every iteration
    if isinstance(sol.Xt, C.Clouds):
        assert sol.Xt.num_points_per_cloud().tolist() == C.icp_inputs(case)["lengths1"].tolist()


# ---- wrong variants ---------------------------------------------------------------------------------------------------------------
def variant_alignment(X, Y, w, estimate_scale, allow_reflection, wrong=None, eps=1e-9):
    """corresponding_points_alignment on full float32 tensors with weights w (None: ones), written out; `wrong` breaks one step."""
    b, n, _ = X.shape
    w = torch.ones(b, n) if w is None else w
    total = w.sum(1).clamp(eps)
    Xmu = (X * w[..., None]).sum(1) / total[:, None]
    Ymu = (Y * w[..., None]).sum(1) / total[:, None]
    if wrong == "uncentred":  # one pass: sum w^2 x y^T - the means' product
        w2 = (w * w)[..., None]
        XY = torch.bmm((X * w2).transpose(2, 1), Y)
        sx, sy, sw2 = (X * w2).sum(1), (Y * w2).sum(1), w2.sum(1)
        XY = XY - Xmu[:, :, None] * sy[:, None, :] - sx[:, :, None] * Ymu[:, None, :] + sw2[:, :, None] * Xmu[:, :, None] * Ymu[:, None, :]
        Xc = (X - Xmu[:, None]) * w[..., None]
    else:
        power = w if wrong == "w_not_squared" else w * w
        Xc, Yc = X - Xmu[:, None], Y - Ymu[:, None]
        XY = torch.bmm((Xc * power[..., None]).transpose(2, 1), Yc)
        Xc = Xc * w[..., None]
    XY = XY / total[:, None, None]
    U, S, Vh = torch.linalg.svd(XY)
    E = torch.eye(3)[None].repeat(b, 1, 1)
    if not allow_reflection and wrong != "no_det":
        E[:, 2, 2] = torch.det(torch.bmm(U, Vh))
    R = torch.bmm(torch.bmm(U, E), Vh)
    s = torch.ones(b)
    if estimate_scale:
        s = (torch.diagonal(E, dim1=1, dim2=2) * S).sum(1) / ((Xc * Xc).sum((1, 2)) / total).clamp(eps)
    T = Ymu - s[:, None] * torch.bmm(Xmu[:, None], R)[:, 0]
    return {"R": R, "T": T, "s": s}


WRONG = {"uncentred": ("offset", "plain", 0), "no_det": ("reflect", "fix", 0), "w_not_squared": ("weights", "rand", 0)}


@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_wrong_variants_are_refused_by_the_same_gate(wrong):
    case = WRONG[wrong]
    d = C.align_inputs(case)
    args = (d["X"], d["Y"], d["weights"], d["kwargs"]["estimate_scale"], d["kwargs"]["allow_reflection"])
    assert not C.refused("align", case, variant_alignment(*args)), "the restatement itself misses the gate"
    bad = variant_alignment(*args, wrong=wrong)
    print(wrong, C.errors(bad, C.truth("align", case)), C.gates("align", case[0]))
    assert C.refused("align", case, bad)
    for other in (c for c in C.ALIGN_CASES if c[0] == "rigid"):  # the same code passes where the step does not matter
        o = C.align_inputs(other)
        if wrong != "uncentred":
            assert not C.refused("align", other, variant_alignment(o["X"], o["Y"], None, False, False, wrong=wrong))


# ---- the reference's checks, defaults and corner cases ------------------------------------------------------------------------------
def test_checks_defaults_and_corner_cases_follow_the_reference():
    import inspect

    sig = inspect.signature(PA.iterative_closest_point)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[2:]] == [
        ("init_transform", None), ("max_iterations", 100), ("relative_rmse_thr", 1e-6), ("estimate_scale", False),
        ("allow_reflection", False), ("verbose", False)]
    sig = inspect.signature(PA.corresponding_points_alignment)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[2:]] == [
        ("weights", None), ("estimate_scale", False), ("allow_reflection", False), ("eps", 1e-9)]
    assert PA.ICPSolution._fields == ("converged", "rmse", "Xt", "RTs", "t_history") and PA.SimilarityTransform._fields == ("R", "T", "s")
    gen = torch.Generator().manual_seed(5)
    X, Y = torch.randn(2, 20, 3, generator=gen), torch.randn(2, 30, 3, generator=gen)
    with pytest.raises(ValueError, match="number of batches and data dimensions"):
        PA.iterative_closest_point(X, Y[:1])
    with pytest.raises(ValueError, match="should be either Pointclouds objects or tensors"):
        PA.iterative_closest_point([X], Y)
    with pytest.raises(ValueError, match="number of batches, points and dimensions"):
        PA.corresponding_points_alignment(X, Y)
    with pytest.raises(ValueError, match="weights should have the same first two dimensions as X"):
        PA.corresponding_points_alignment(X, X, weights=torch.ones(2, 19))
    with pytest.raises(ValueError, match="number of weights should equal"):
        PA.corresponding_points_alignment(X, X, weights=[torch.ones(20), torch.ones(19)])
    with pytest.raises(ValueError, match="The initial transformation init_transform has to be"):
        PA.iterative_closest_point(X, Y, init_transform=(torch.eye(3)[None].repeat(2, 1, 1), torch.zeros(2, 3)))
    lists = PA.corresponding_points_alignment(X, X * 2 + 1, weights=[torch.ones(20), torch.ones(20)], estimate_scale=True)
    assert float((lists.s - 2).abs().max()) <= 1e-5 and float((lists.T - 1).abs().max()) <= 1e-5
    none = PA.iterative_closest_point(X, Y, max_iterations=0)
    assert none.converged is False and none.rmse is None and none.t_history == [] and torch.equal(none.Xt, X)
    assert torch.equal(none.RTs.R, torch.eye(3).expand(2, 3, 3)) and not bool(none.RTs.T.any()) and bool((none.RTs.s == 1).all())
    with pytest.warns(UserWarning, match="The size of one of the point clouds is <= dim\\+1"):
        few = PA.corresponding_points_alignment(X[:, :3], X[:, :3])
    assert few.R.shape == (2, 3, 3)
    moved = PA.apply_similarity_transform(X, lists.R, lists.T, lists.s)
    assert float((moved - (X * 2 + 1)).abs().max()) <= 1e-4
    leaf = X.clone().requires_grad_(True)
    out = PA.corresponding_points_alignment(leaf, X * 2 + 1, estimate_scale=True)  # autograd through the chain
    (out.R.sum() + out.T.sum() + out.s.sum()).backward()
    assert bool(torch.isfinite(leaf.grad).all())
    assert not PA.kernel_path(X, Y) and not PA.kernel_path(X.double(), Y.double())  # CPU tensors: the chain
    import pytorch3d_amd as p3d

    assert p3d.iterative_closest_point is PA.iterative_closest_point and p3d.SimilarityTransform is PA.SimilarityTransform
    assert p3d.corresponding_points_alignment is PA.corresponding_points_alignment and p3d.ICPSolution is PA.ICPSolution


def test_c_abi_argument_checks():
    import ctypes

    header = open(_lib.EXTENSION_HEADER_PATH).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header) and name in _lib.EXTENSION_SYMBOLS and name not in _lib.EXPORTED_SYMBOLS
    for const in ("ICP_MAX_SPLIT", "ALIGN_ESTIMATE_SCALE", "ALIGN_ALLOW_REFLECTION"):
        assert const in _lib.EXTENSION_CONSTANTS and getattr(_lib, const) == _lib.EXTENSION_CONSTANTS[const] > 0
    assert "points_alignment.hip" in build.SOURCES
    assert ("pytorch3d.ops.points_alignment", ("pytorch3d.ops",), shim._points_alignment) in shim._FUNCTION_PATCHES
    assert _C.points_alignment_fits(64, 1024, 1024) and not _C.points_alignment_fits(0, 5, 5) and not _C.points_alignment_fits(1, 0, 5)
    assert not _C.points_alignment_fits(1, 2 ** 31, 5) and not _C.points_alignment_fits(2 ** 20, 2 ** 20, 5)
    lib = _lib.load()
    need = lib.p3di_icp_workspace_bytes(3, 200)
    blocks = 3 * 4
    assert need >= 4 * (blocks * (7 + 10 + 1) + 3 * 8) and lib.p3di_icp_workspace_bytes(-1, 5) == 0 and lib.p3di_icp_workspace_bytes(3, 0) == 0
    assert lib.p3di_icp_workspace_bytes(1, 2 ** 31) == 0 and lib.p3di_icp_workspace_bytes(2 ** 20, 2 ** 20) == 0
    buf = torch.zeros(1 << 16, dtype=torch.int64)
    p = buf.data_ptr()
    thr, eps = ctypes.c_float(1e-6), ctypes.c_float(1e-9)
    assert lib.p3di_icp_match(None, None, None, None, None, None, None, 0, 5, 5, 0, None, None, 0, None) == _lib.OK  # no launch
    assert lib.p3di_icp_match(None, None, None, None, None, None, None, 3, 0, 5, 0, None, None, 0, None) == _lib.OK
    for N, P1, P2, split in ((-1, 5, 5, 0), (3, -1, 5, 0), (3, 5, -1, 0), (3, 5, 2 ** 31, 0), (3, 5, 5, 3), (3, 5, 5, 16), (3, 5, 5, -1)):
        assert lib.p3di_icp_match(p, p, None, None, None, None, None, N, P1, P2, split, p, p, need, None) == _lib.ERR_INVALID_ARG
        assert lib.p3di_icp_iteration(p, p, None, None, None, None, None, None, None, N, P1, P2, split, 0, thr, p, p, p, p, p, p, p, p, need,
                                      None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_icp_match(None, p, None, None, None, None, None, 3, 200, 5, 0, p, p, need, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_icp_match(p, None, None, None, None, None, None, 3, 200, 5, 0, p, p, need, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_icp_match(p, p, None, None, None, None, None, 3, 200, 5, 0, None, p, need, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_icp_match(p, p, None, None, p, None, p, 3, 200, 5, 0, p, p, need, None) == _lib.ERR_INVALID_ARG  # R and s without T
    assert lib.p3di_icp_match(p, p, None, None, None, None, None, 3, 200, 5, 0, p, p, need - 1, None) == _lib.ERR_WORKSPACE
    assert lib.p3di_icp_match(p, p, None, None, None, None, None, 3, 200, 5, 0, p, None, need, None) == _lib.ERR_WORKSPACE

    def iteration(**kw):
        a = dict(X=p, Y=p, R_in=None, T_in=None, s_in=None, N=3, P1=200, P2=5, flags=0, R_out=p, T_out=p, s_out=p, idx=p, Xt=p, rmse=p,
                 status=p, ws=p, nbytes=need)
        a.update(kw)
        return lib.p3di_icp_iteration(a["X"], a["Y"], None, None, None, a["R_in"], a["T_in"], a["s_in"], None, a["N"], a["P1"], a["P2"], 0,
                                      a["flags"], thr, a["R_out"], a["T_out"], a["s_out"], a["idx"], a["Xt"], a["rmse"], a["status"], a["ws"],
                                      a["nbytes"], None)

    for missing in ("X", "Y", "R_out", "T_out", "s_out", "idx", "Xt", "rmse", "status"):
        assert iteration(**{missing: None}) == _lib.ERR_INVALID_ARG, missing
    assert iteration(flags=4) == _lib.ERR_INVALID_ARG and iteration(R_in=p) == _lib.ERR_INVALID_ARG
    assert iteration(N=0) == _lib.ERR_INVALID_ARG and iteration(P1=0) == _lib.ERR_INVALID_ARG  # nothing to align: the caller answers
    assert iteration(nbytes=need - 1) == _lib.ERR_WORKSPACE and iteration(ws=None) == _lib.ERR_WORKSPACE

    def alignment(**kw):
        a = dict(X=p, Y=p, N=3, P=200, flags=3, R=p, T=p, s=p, status=p, ws=p, nbytes=need)
        a.update(kw)
        return lib.p3di_points_alignment(a["X"], a["Y"], None, None, a["N"], a["P"], a["flags"], eps, a["R"], a["T"], a["s"], a["status"],
                                         a["ws"], a["nbytes"], None)

    for missing in ("X", "Y", "R", "T", "s", "status"):
        assert alignment(**{missing: None}) == _lib.ERR_INVALID_ARG, missing
    for kw in ({"N": -1}, {"N": 0}, {"P": 0}, {"P": 2 ** 31}, {"flags": 8}):
        assert alignment(**kw) == _lib.ERR_INVALID_ARG, kw
    assert alignment(nbytes=need - 1) == _lib.ERR_WORKSPACE and alignment(ws=None) == _lib.ERR_WORKSPACE
    with pytest.raises(RuntimeError, match="must be a CUDA/HIP tensor"):
        _C.icp_match(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))


def test_the_shim_serves_the_reference_functions_and_rebinds_them():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    if not os.path.isdir(os.path.join(stage, "pytorch3d", "ops")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_points_alignment_case.py"), "cpu"], capture_output=True, text=True,
                         timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    assert rec["unpatched_is_the_reference"] and rec["calls_before_patch"] == 0 and rec["patched_everywhere"]
    assert rec["icp_equal"] and rec["icp_types"] and rec["align_equal"] and rec["pointclouds_updated"] and rec["restored"]
    # CPU tensors: the restated chain, counted as fallbacks
    assert rec["fused_calls"] == {"iterative_closest_point": 0, "corresponding_points_alignment": 0}
    assert rec["fallback_calls"] == {"iterative_closest_point": 2, "corresponding_points_alignment": 1}
