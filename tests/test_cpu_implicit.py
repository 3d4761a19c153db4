"""sample_pdf and the raymarchers without a GPU: the library's host loop against the reference's compiled operator bit for bit, the
torch formulations through the raymarch gates, deliberately wrong variants refused by the same gates, errors and shapes of the public
functions, the shim module.  Cases, inputs and gates: tests/implicit_case.py; fixture: tests/golden/implicit_ref.npz."""
import os
import re
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import implicit_case as C  # noqa: E402

import pytorch3d_amd as A  # noqa: E402
from pytorch3d_amd import _C, _lib, implicit, shim  # noqa: E402

PDF_CASES, RAY_CASES = C.pdf_cases(), C.ray_cases()


def _host(case):
    bins, weights, u, eps = C.pdf_inputs(case)
    out = u.clone()
    version = out._version
    assert implicit.sample_pdf_op(bins, weights, out, eps) is None
    assert out._version > version  # in place, and autograd knows
    return out


@pytest.mark.parametrize("case", PDF_CASES, ids=[c[0] for c in PDF_CASES])
def test_host_loop_equals_the_reference_operator_bit_for_bit(case):
    assert C.same_bits(_host(case).numpy(), C.fixture()["pdf/" + case[0]])


def test_fixture_holds_every_case_and_the_cases_hold_every_size():
    fix = C.fixture()
    assert {k[4:] for k in fix if k.startswith("pdf/")} == {c[0] for c in PDF_CASES}
    grid = [c for c in PDF_CASES if c[1] == "grid" and c[3] <= 65]
    assert {c[2] for c in grid} == set(C.PDF_B) and {c[3] for c in grid} == set(C.PDF_BINS) and {c[4] for c in grid} == set(C.PDF_S)
    assert {(c[3], c[4]) for c in grid if c[2] == 3} == {(n, s) for n in C.PDF_BINS for s in C.PDF_S}
    assert {c[3] for c in grid if c[2] == 257} == set(C.PDF_BINS) and {c[4] for c in grid if c[2] == 257} == set(C.PDF_S)
    for c in RAY_CASES:
        assert C.key(c[0], "features") in fix and (C.key(c[0], "weights") in fix) == c[6]
    assert {(c[2], c[4]) for c in RAY_CASES} >= {(P, s) for P in C.RAY_P for s in (1, 2, 5, P, P + 3)}
    assert {c[3] for c in RAY_CASES} == {1, 3, 4, 7} and {c[5] for c in RAY_CASES} == set(C.KINDS) | {"over"}
    assert {int(np.prod(c[1])) for c in RAY_CASES} >= {1, 5, 64, 65, 257} and {c[1] for c in RAY_CASES} >= {(2, 3, 4), ()}
    assert str(fix["broken_f32"]) == ""  # the reference's float32 run is finite on every case: all of them went into E_ref
    assert all(0.0 < C.e_ref(q) < 1e-5 for q in C.QUANTITIES)


def test_the_long_row_is_the_first_of_the_workspace_form():
    lib = _lib.load()
    assert ((C.LONG_BINS - 1) | 1) <= _lib.SAMPLE_PDF_LDS_FLOATS < (C.LONG_BINS | 1)
    assert lib.p3di_sample_pdf_workspace_bytes(2, C.LONG_BINS - 1) == 0 and lib.p3di_sample_pdf_workspace_bytes(2, C.LONG_BINS) >= 2 * C.LONG_BINS * 4
    assert any(c[3] == C.LONG_BINS and c[2] == 2 and c[4] == 5 for c in PDF_CASES)


def test_public_sample_pdf_det_and_uniforms():
    for case in PDF_CASES:
        if case[2] > 8 or case[3] > 65 or case[1] in ("nan", "dyadic"):  # (eps = 0 with a zero weight: the reference's check raises, below)
            continue
        bins, weights, u, eps = C.pdf_inputs(case)
        want = C.fixture()["pdf/" + case[0]]
        if case[5]:
            got = A.sample_pdf(bins, weights, case[4], det=True, eps=eps)
        else:
            keep = u.clone()
            got = A.sample_pdf(bins, weights, case[4], eps=eps, uniforms=u)
            assert torch.equal(u, keep)  # the uniforms are an input
        assert C.same_bits(got.numpy(), want), case[0]
    # leading shapes: (2, 4, n + 1) bins are 8 rows
    case = next(c for c in PDF_CASES if c[0] == "special-det")
    bins, weights, u, eps = C.pdf_inputs(case)
    got = A.sample_pdf(bins.reshape(2, 4, -1), weights.reshape(2, 4, -1), case[4], det=True, eps=eps)
    assert got.shape == (2, 4, case[4]) and C.same_bits(got.reshape(8, -1).numpy(), C.fixture()["pdf/special-det"])
    torch.manual_seed(0)
    drawn = A.sample_pdf(bins, weights, 7)
    assert drawn.shape == (8, 7) and bool(((drawn >= bins[:, :1]) & (drawn <= bins[:, -1:])).all())


def test_sample_pdf_errors():
    bins, weights = torch.linspace(0, 1, 5).expand(2, 5), torch.ones(2, 4)
    with pytest.raises(NotImplementedError, match="sample_pdf differentiability"):
        A.sample_pdf(bins, weights.clone().requires_grad_(True), 3)
    with pytest.raises(ValueError, match="Negative weights provided"):
        A.sample_pdf(bins, -weights, 3)
    with pytest.raises(ValueError, match="Negative weights provided"):  # weights.min() <= -eps, as the reference has it
        A.sample_pdf(bins, weights * torch.tensor([0.0, 1, 1, 1]), 3, eps=0.0)
    with pytest.raises(ValueError, match="Inconsistent shapes of bins and weights"):
        A.sample_pdf(bins, torch.ones(2, 5), 3)
    with pytest.raises(ValueError, match="uniforms must be float32 of shape"):
        A.sample_pdf(bins, weights, 3, uniforms=torch.rand(2, 4))
    with pytest.raises(ValueError, match="not both"):
        A.sample_pdf(bins, weights, 3, det=True, uniforms=torch.rand(2, 3))
    with pytest.raises(RuntimeError, match="must be float32"):
        implicit.sample_pdf_op(bins.double(), weights.double(), torch.rand(2, 3), 1e-5)
    with pytest.raises(RuntimeError, match="outputs must be contiguous"):
        implicit.sample_pdf_op(bins, weights, torch.rand(3, 2).t(), 1e-5)
    with pytest.raises(RuntimeError, match="expected"):
        implicit.sample_pdf_op(bins, weights, torch.rand(3, 3), 1e-5)
    with pytest.raises(TypeError):
        implicit.sample_pdf_op(bins, weights, None, 1e-5)
    empty = torch.rand(2, 0)
    implicit.sample_pdf_op(bins, weights, empty, 1e-5)  # S == 0: nothing to do


def test_c_abi_argument_checks_and_lists():
    lib, f = _lib.load(), torch.zeros(8)
    header = open(_lib.EXTENSION_HEADER_PATH).read()
    for name in ("p3di_sample_pdf", "p3di_sample_pdf_workspace_bytes", "p3di_sample_pdf_host", "p3di_ea_raymarch_forward",
                 "p3di_ea_raymarch_backward", "p3di_ea_raymarch_backward_workspace_bytes"):
        assert re.search(r"\b%s\(" % name, header) and name in _lib.EXTENSION_SYMBOLS and name not in _lib.EXPORTED_SYMBOLS
    p = f.data_ptr()
    assert lib.p3di_sample_pdf_host(p, p, p, 0, 3, 2, 1e-5) == _lib.OK and lib.p3di_sample_pdf_host(p, p, p, 2, 3, 0, 1e-5) == _lib.OK
    assert lib.p3di_sample_pdf(None, None, None, 0, 3, 2, 1e-5, None, 0, None) == _lib.OK  # no launch: runs without a GPU
    assert lib.p3di_sample_pdf(None, None, None, 2, 3, 0, 1e-5, None, 0, None) == _lib.OK
    for B, n, S in ((1, 0, 1), (-1, 3, 1), (1, 3, -1)):
        assert lib.p3di_sample_pdf_host(p, p, p, B, n, S, 1e-5) == _lib.ERR_INVALID_ARG
        assert lib.p3di_sample_pdf(p, p, p, B, n, S, 1e-5, None, 0, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_sample_pdf_host(None, p, p, 1, 1, 1, 1e-5) == _lib.ERR_INVALID_ARG
    assert lib.p3di_sample_pdf(p, None, p, 1, 1, 1, 1e-5, None, 0, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_sample_pdf(p, p, p, 1, C.LONG_BINS, 1, 1e-5, p, 16, None) == _lib.ERR_WORKSPACE
    assert lib.p3di_ea_raymarch_forward(None, None, 0, 4, 3, 1, 1.0, None, None, None) == _lib.OK
    for N, P, Cc, s in ((1, 0, 3, 1), (1, 4, 3, 0), (-1, 4, 3, 1), (1, 4, -1, 1)):
        assert lib.p3di_ea_raymarch_forward(p, p, N, P, Cc, s, 1.0, p, None, None) == _lib.ERR_INVALID_ARG
        assert lib.p3di_ea_raymarch_backward(p, p, p, None, N, P, Cc, s, 1.0, p, p, None, 0, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_ea_raymarch_forward(p, None, 1, 4, 3, 1, 1.0, p, None, None) == _lib.ERR_INVALID_ARG
    assert lib.p3di_ea_raymarch_backward_workspace_bytes(7, 64) == 0 and lib.p3di_ea_raymarch_backward_workspace_bytes(7, 65) >= 7 * 2 * 3 * 4
    assert lib.p3di_ea_raymarch_backward(p, p, p, None, 1, 65, 1, 1, 1.0, p, p, p, 8, None) == _lib.ERR_WORKSPACE
    from pytorch3d_amd import build

    assert "implicit.hip" in build.SOURCES and "sample_pdf_sample.h" in build.HEADERS and "implicit_abi.h" in build.HEADERS
    assert _C.IMPLICIT_EXPORTS == ("sample_pdf",) and len(_C.HOT_PATH_EXPORTS) == 20 and "sample_pdf" not in _C.HOT_PATH_EXPORTS
    assert shim.EXPORTS["sample_pdf"] == ("implicit", "sample_pdf_op")


# ---- raymarching ------------------------------------------------------------------------------------------------------------------
def test_torch_formulations_pass_the_gates():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert C.ray_failures(RAY_CASES, implicit.ea_raymarch_torch) == []
        assert C.ray_failures(RAY_CASES, A.ea_raymarch) == []  # CPU tensors: the public function takes the formulation


def test_absorption_only_and_float64():
    for case in RAY_CASES[::7]:
        d = C.ray_inputs(case)[0]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = A.absorption_only_raymarch(d.double())
        truth = C.fixture()[C.key(case[0], "opacities")]
        assert got.shape == d.shape[:-2] + (1,) and got.dtype == torch.float64
        assert np.abs(got.numpy() - truth).max() <= 1e-14


def test_density_bounds_warning_is_kept():
    case = next(c for c in RAY_CASES if c[5] == "over")
    d, f = C.ray_inputs(case)[:2]
    with pytest.warns(UserWarning, match="outside of valid"):
        A.ea_raymarch(d, f)
    with pytest.warns(UserWarning, match="outside of valid"):
        A.absorption_only_raymarch(d)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        A.ea_raymarch(d.clamp(0, 1), f)


class _DivisionCumprod(torch.autograd.Function):
    """cumprod whose backward divides by the input: g_x_j = sum_{k >= j} g_k c_k / x_j -- not finite where x_j is 0 (a density of 1)."""

    @staticmethod
    def forward(ctx, x):
        c = torch.cumprod(x, -1)
        ctx.save_for_backward(x, c)
        return c

    @staticmethod
    def backward(ctx, g):
        x, c = ctx.saved_tensors
        return torch.flip(torch.cumsum(torch.flip(g * c, (-1,)), -1), (-1,)) / x


def _variant(shift_by=0, opacity_from_shifted=False, division=False):
    def fn(rays_densities, rays_features, eps, s, return_weights):
        d = rays_densities[..., 0]
        x = (1.0 + eps) - d
        cp = _DivisionCumprod.apply(x) if division else torch.cumprod(x, -1)
        t = s + shift_by
        a = torch.cat([torch.ones_like(cp[..., :t]), cp[..., :-t]], -1)
        w = d * a
        feats = (w[..., None] * rays_features).sum(-2)
        opac = 1.0 - (a[..., -1:] if opacity_from_shifted else torch.prod(1.0 - d, -1, keepdim=True))
        out = torch.cat((feats, opac), -1)
        return (out, w) if return_weights else out

    return fn


def test_wrong_raymarchers_are_refused_by_the_gates():
    quiet = [c for c in RAY_CASES if c[5] != "over"]
    assert C.ray_failures(quiet, _variant()) == []  # the harness itself: the right chain passes
    off_by_one = C.ray_failures(quiet, _variant(shift_by=1))
    assert {q for _, q, _, _ in off_by_one} >= {"features", "weights", "grad_densities", "grad_features"}
    shifted_opacity = C.ray_failures(quiet, _variant(opacity_from_shifted=True))
    assert shifted_opacity and {q for _, q, _, _ in shifted_opacity} <= {"opacities", "grad_densities"}
    division = C.ray_failures(quiet, _variant(division=True))
    assert division and all(C.ray_inputs(next(c for c in quiet if c[0] == cid))[0].eq(1).any() for cid, _, _, _ in division)
    assert all(err == float("inf") and q == "grad_densities" for _, q, err, _ in division)
    with_ones = {c[0] for c in quiet if c[5] in ("one1", "one2", "all1") and c[4] < c[2]}  # (s >= P: the product reaches no weight)
    assert with_ones <= {cid for cid, _, _, _ in division}


def test_wrong_samplers_are_refused_bit_for_bit():
    small = [c for c in PDF_CASES if c[2] <= 8 and c[3] <= 65]
    refused = {"upper_bound": [], "total_from_eps": []}
    for case in small:
        bins, weights, u, eps = C.pdf_inputs(case)
        want = C.fixture()["pdf/" + case[0]]
        assert C.same_bits(C.pdf_numpy(bins, weights, u, eps), want), case[0]  # the restatement itself is right
        for name in refused:
            if not C.same_bits(C.pdf_numpy(bins, weights, u, eps, **{name: True}), want):
                refused[name].append(case[0])
    assert "dyadic-eps0" in refused["upper_bound"]  # u' equal to a partial sum: the tie rule
    assert refused["total_from_eps"] and "dyadic-eps0" not in refused["total_from_eps"]  # (eps = 0: the same sums)


def test_raymarch_errors_and_shapes():
    d, f = torch.rand(2, 3, 5, 1), torch.rand(2, 3, 5, 4)
    out, w = A.ea_raymarch(d, f, return_weights=True)
    assert out.shape == (2, 3, 5) and w.shape == (2, 3, 5) and A.ea_raymarch(d[0, 0], f[0, 0]).shape == (5,)
    assert A.absorption_only_raymarch(d).shape == (2, 3, 1)
    with pytest.raises(ValueError, match="rays_densities has to be an instance of torch.Tensor"):
        A.ea_raymarch(None, f)
    with pytest.raises(ValueError, match="rays_features has to be an instance of torch.Tensor"):
        A.ea_raymarch(d, None)
    with pytest.raises(ValueError, match="last dimension of rays_densities has to be one"):
        A.ea_raymarch(d[..., 0], f)
    with pytest.raises(ValueError, match="first to previous to last dimensions of rays_features"):
        A.ea_raymarch(d, f[:, :2])
    with pytest.raises(ValueError, match="at least one dimension"):
        A.absorption_only_raymarch(torch.tensor(0.5))
    assert not implicit.kernel_path(d, f) and not implicit.kernel_path(d.double(), f.double())  # CPU, float64: the formulation


# ---- the shim module --------------------------------------------------------------------------------------------------------------
def test_shim_module_serves_sample_pdf_and_keeps_the_pinned_stubs():
    mod = shim.make_module()
    case = next(c for c in PDF_CASES if c[0] == "special-rand")
    bins, weights, u, eps = C.pdf_inputs(case)
    out = u.clone()
    assert mod.sample_pdf(bins, weights, out, eps) is None
    assert C.same_bits(out.numpy(), C.fixture()["pdf/special-rand"])
    for name in ("knn_points_idx", "knn_points_backward", "point_face_array_dist_forward", "point_face_array_dist_backward",
                 "point_edge_array_dist_forward", "point_edge_array_dist_backward"):
        with pytest.raises(NotImplementedError, match="outside the rasterization hot path"):
            getattr(mod, name)()
