"""knn_points / knn_gather / chamfer_distance without a GPU: the package's torch formulation against the reference's recorded results
(tests/golden/chamfer_ref.npz, made by tests/golden/make_golden_chamfer.py from the reference's own code), the validation, the shim's
stub and the C ABI's declarations.

Tolerances.  The fixture's queries keep a relative gap of >= 1e-5 between consecutive distances, more than 8 x the (D + 2) 2^-24
rounding of one float32 distance, so idx must match bit for bit and dists within 2e-6 relative.  Losses: a sum of n float32 terms
in two different orders differs by at most ~n 2^-24 of the sum of the absolute terms; the cases have n <= 200 points per cloud and 3
clouds, so 1e-4 relative to the largest value leaves a factor 2 and more.  Gradients: the same reasoning per entry (each is a sum of
at most a few dozen terms, scaled like the loss).
"""
import os
import re

import pytest
import torch

import _util as U
import chamfer_case as C

import pytorch3d_amd as p3d
from pytorch3d_amd import knn as knn_mod


def _knn_params():
    return [(name, K, norm) for name, *_r, Ks, norms in C.KNN_CASES for K in Ks for norm in norms]


@pytest.mark.parametrize("name,K,norm", _knn_params())
def test_torch_formulation_matches_the_reference_neighbours(name, K, norm):
    z = C.fixture()
    _, N, P1, P2, D, l1, l2, _, _ = next(c for c in C.KNN_CASES if c[0] == name)
    p1, p2 = z[C.knn_key(name, "p1")], z[C.knn_key(name, "p2")]
    assert not knn_mod.kernel_path(p1, p2, K)
    got = p3d.knn_points(p1, p2, C.lengths_tensor(l1), C.lengths_tensor(l2), norm=norm, K=K)
    want_idx, want_d = z[C.knn_key(name, "idx", K, norm)], z[C.knn_key(name, "dists", K, norm)]
    assert got.knn is None and got.idx.dtype == torch.int64 and got.dists.dtype == torch.float32
    assert torch.equal(got.idx, want_idx)
    assert float(((got.dists - want_d).abs() - 2e-6 * want_d.abs()).max()) <= 0.0
    valid = C.valid_mask(l1, l2, N, P1, P2, K)
    assert not got.idx[~valid].any() and not got.dists[~valid].any()


def test_chunked_formulation_equals_the_unchunked_one(monkeypatch):
    z = C.fixture()
    p1, p2 = z[C.knn_key("pad", "p1")], z[C.knn_key("pad", "p2")]
    l1, l2 = C.lengths_tensor([70, 1, 33]), C.lengths_tensor([130, 64, 5])
    whole = knn_mod.torch_knn_forward(p1, p2, l1, l2, 2, 8)
    monkeypatch.setattr(knn_mod, "CHUNK_ELEMENTS", 3 * 130 * 7)  # 7 rows at a time: 70 is a multiple, the last chunk is full
    parts = knn_mod.torch_knn_forward(p1, p2, l1, l2, 2, 8)
    monkeypatch.setattr(knn_mod, "CHUNK_ELEMENTS", 3 * 130 * 9)  # 9 rows: a short last chunk
    parts9 = knn_mod.torch_knn_forward(p1, p2, l1, l2, 2, 8)
    for a, b, c in zip(whole, parts, parts9):
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("norm", [2, 1])
def test_exact_ties_go_to_the_smaller_index(norm):
    p1, p2 = C.tie_clouds()
    want_idx, want_d = C.brute64(p1, p2, None, None, 6, norm)
    assert (want_d[..., 0] == want_d[..., 1]).all()  # every query has an exact tie in front
    got = p3d.knn_points(p1, p2, norm=norm, K=6)
    assert torch.equal(got.idx, want_idx)
    assert torch.equal(got.dists.double(), want_d)  # halves of small integers: exact in float32


@pytest.mark.parametrize("name,K,norm", [("pad", 8, 2), ("pad", 3, 1), ("d5", 32, 2), ("empty", 3, 2)])
def test_explicit_backward_matches_float64_autograd(name, K, norm):
    z = C.fixture()
    _, N, P1, P2, D, l1, l2, _, _ = next(c for c in C.KNN_CASES if c[0] == name)
    p1 = z[C.knn_key(name, "p1")].clone().requires_grad_(True)
    p2 = z[C.knn_key(name, "p2")].clone().requires_grad_(True)
    got = p3d.knn_points(p1, p2, C.lengths_tensor(l1), C.lengths_tensor(l2), norm=norm, K=K)
    g = torch.randn(got.dists.shape, generator=torch.Generator().manual_seed(11))
    gp1, gp2 = torch.autograd.grad((got.dists * g).sum(), (p1, p2))
    t1, t2 = C.knn_grad_truth(p1, p2, l1, l2, got.idx, norm, g)
    # a row of grad_p1 sums K terms, a row of grad_p2 at most P1 K: float32 against float64, relative to the largest entry
    for a, t in ((gp1, t1), (gp2, t2)):
        assert float((a.double() - t).abs().max()) <= 1e-5 * max(1.0, float(t.abs().max()))
    valid = C.valid_mask(l1, l2, N, P1, P2, K)
    assert not gp1[~valid.any(2)].any()  # rows past lengths1 (and clouds without p2 points) get nothing


def test_knn_gather_and_return_nn():
    z = C.fixture()
    p1, p2 = z[C.knn_key("pad", "p1")], z[C.knn_key("pad", "p2")]
    l1, l2 = C.lengths_tensor([70, 1, 33]), C.lengths_tensor([130, 64, 5])
    got = p3d.knn_points(p1, p2, l1, l2, K=8, return_nn=True)
    assert got.knn.shape == (3, 70, 8, 3)
    assert torch.equal(got.knn, p3d.knn_gather(p2, got.idx, l2))
    assert torch.equal(got.knn[0, 5, 2], p2[0, got.idx[0, 5, 2]])
    assert not got.knn[2, :, 5:].any()  # slots past lengths2 = 5
    with pytest.raises(ValueError, match="same batch dimension"):
        p3d.knn_gather(p2[:2], got.idx, l2)


@pytest.mark.parametrize("name", [c[0] for c in C.CHAMFER_CASES])
def test_chamfer_torch_formulation_matches_the_reference(name):
    z = C.fixture()
    x, y, args, kw = C.chamfer_inputs(name)
    result = p3d.chamfer_distance(*args, **kw)
    outs = C.flatten(result)
    assert (result[1] is not None) == bool(z[C.cham_key(name, "has_normals")])
    for i, t in enumerate(outs):
        want = z[C.cham_key(name, "out%d" % i)]
        assert t.shape == want.shape, (i, t.shape, want.shape)
        assert float((t.detach() - want).abs().max()) <= 1e-4 * max(1e-3, float(want.abs().max())), i
    assert C.cham_key(name, "out%d" % len(outs)) not in z
    gx, gy = torch.autograd.grad(C.scalarise(result), (x, y), allow_unused=True)
    for got, key in ((gx, "grad_x"), (gy, "grad_y")):
        want = z[C.cham_key(name, key)]
        got = torch.zeros_like(want) if got is None else got
        assert float((got - want).abs().max()) <= 1e-4 * max(1e-3, float(want.abs().max())), key


def test_exceptions_match_the_reference():
    x, y = torch.rand(2, 5, 3), torch.rand(2, 7, 3)
    cd = p3d.chamfer_distance
    with pytest.raises(ValueError, match="batch_reduction must be one of"):
        cd(x, y, batch_reduction="max")
    with pytest.raises(ValueError, match="point_reduction must be one of"):
        cd(x, y, point_reduction="median")
    with pytest.raises(ValueError, match="Batch reduction must be None if point_reduction is None"):
        cd(x, y, point_reduction=None)
    with pytest.raises(ValueError, match="Support for 1 or 2 norm."):
        cd(x, y, norm=3)
    with pytest.raises(ValueError, match="Normals must be None if point_reduction is"):
        cd(x, y, x_normals=x, y_normals=y, point_reduction="max")
    with pytest.raises(ValueError, match=r"Expected points to be of shape \(N, P, D\)"):
        cd(x[0], y)
    with pytest.raises(ValueError, match=r"Expected lengths to be of shape \(N,\)"):
        cd(x, y, x_lengths=torch.tensor([5]))
    with pytest.raises(ValueError, match="A length value was too long"):
        cd(x, y, x_lengths=torch.tensor([5, 6]))
    with pytest.raises(ValueError, match="Expected normals to be of shape"):
        cd(x, y, x_normals=x[0], y_normals=y)
    with pytest.raises(ValueError, match="The input pointclouds should be either"):
        cd([x], y)
    with pytest.raises(ValueError, match="y does not have the correct shape."):
        cd(x, torch.rand(2, 7, 2))
    with pytest.raises(ValueError, match="y does not have the correct shape."):
        cd(x, torch.rand(3, 7, 3))
    with pytest.raises(ValueError, match=r"weights must be of shape \(N,\)."):
        cd(x, y, weights=torch.ones(3))
    with pytest.raises(ValueError, match="weights cannot be negative."):
        cd(x, y, weights=torch.tensor([1.0, -1.0]))
    with pytest.raises(ValueError, match="same batch dimension"):
        p3d.knn_points(x, y[:1])
    with pytest.raises(ValueError, match="same point dimension"):
        p3d.knn_points(x, torch.rand(2, 7, 2))
    with pytest.raises(ValueError, match="Support for 1 or 2 norm."):
        p3d.knn_points(x, y, norm=0)
    # `version` is accepted and ignored; the result is sorted whatever return_sorted says
    a = p3d.knn_points(x, y, K=3, version=2, return_sorted=False)
    b = p3d.knn_points(x, y, K=3)
    assert torch.equal(a.idx, b.idx) and (a.dists[..., 1:] >= a.dists[..., :-1]).all()


def test_operator_wrappers_refuse_cpu_tensors_and_the_shim_keeps_its_stub():
    from pytorch3d_amd import _C, shim

    x, y = torch.rand(1, 4, 3), torch.rand(1, 4, 3)
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        _C.knn_points_idx(x, y, None, None, 2, 1, -1)
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        _C.knn_points_backward(x, y, None, None, torch.zeros(1, 4, 1, dtype=torch.int64), 2, torch.zeros(1, 4, 1))
    assert "knn_points_idx" not in _C.HOT_PATH_EXPORTS and "knn_points_backward" not in _C.HOT_PATH_EXPORTS
    mod = shim.make_module()
    for name in ("knn_points_idx", "knn_points_backward"):
        with pytest.raises(NotImplementedError):
            getattr(mod, name)(None)


def test_header_declares_the_entries_and_the_library_sizes_workspaces_on_the_host():
    from pytorch3d_amd import _lib

    src = open(os.path.join(U.ROOT, "include", "p3d_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = ("p3d_knn_points_forward", "p3d_chamfer_forward_workspace_bytes", "p3d_chamfer_forward", "p3d_knn_points_backward",
             "p3d_knn_points_ordered_backward_workspace_bytes", "p3d_knn_points_ordered_backward")
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.EXPORTED_SYMBOLS
    assert re.search(r"#define P3D_ABI_VERSION 3\b", src)
    assert int(re.search(r"#define P3D_KNN_TILE (\d+)", src).group(1)) == C.TILE == _lib.KNN_TILE
    assert int(re.search(r"#define P3D_KNN_MAX_K (\d+)", src).group(1)) == _lib.KNN_MAX_K == 32
    lib = _lib.load()
    assert lib.p3d_abi_version() == 3
    assert lib.p3d_chamfer_forward_workspace_bytes(3, 130) == 3 * 3 * 4  # one float per wave of 64 queries
    assert lib.p3d_chamfer_forward_workspace_bytes(0, 130) == 0
    assert 0 < lib.p3d_knn_points_ordered_backward_workspace_bytes(100) <= lib.p3d_knn_points_ordered_backward_workspace_bytes(1000)
    # arguments are checked before anything is launched: no device needed for these answers
    assert lib.p3d_knn_points_forward(None, None, None, None, 1, 4, 4, 5, 1, 2, None, None, None) == -6   # D = 5: unsupported
    assert lib.p3d_knn_points_forward(None, None, None, None, 1, 4, 4, 3, 33, 2, None, None, None) == -6  # K = 33: unsupported
    assert lib.p3d_knn_points_forward(None, None, None, None, 1, 4, 4, 3, 1, 3, None, None, None) == -1   # norm 3
    assert lib.p3d_knn_points_forward(None, None, None, None, 1, 4, 4, 3, 1, 2, None, None, None) == -1   # null pointers
    assert lib.p3d_knn_points_forward(None, None, None, None, 0, 4, 4, 3, 1, 2, None, None, None) == 0    # nothing to do
