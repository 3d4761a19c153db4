"""estimate_pointcloud_normals / estimate_pointcloud_local_coord_frames / point_covariances without a GPU: the package's torch
formulation through the gates of tests/point_frames_case.py against the reference's recorded float64 run
(tests/golden/point_frames_ref.npz, made by tests/golden/make_golden_point_frames.py from the reference's own code; every tolerance
is MARGIN x the reference's own float32 figure, recorded there), the SAME gates on deliberately wrong variants (each must be
refused), the arguments, the paths the kernel does not take, the autograd gradient against autograd through the reference's code,
and the boundary (symbols, constants, exports, the shim's rebinding)."""
import importlib
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import point_frames_case as C  # noqa: E402
import pytorch3d_amd as p3d  # noqa: E402
from pytorch3d_amd.knn import knn_gather, torch_knn_forward  # noqa: E402

PN = importlib.import_module("pytorch3d_amd.points_normals")

CASES = C.all_cases()


def run(case, **variant):
    """Packed (cov, curv, frames, idx) of a case through the formulation, or through a deliberately wrong variant of it."""
    pts, lengths = C.inputs(case)
    K = case[1]
    if not variant:
        curv, frames = p3d.estimate_pointcloud_local_coord_frames(C.Clouds(pts, lengths), neighborhood_size=K)
        cov, idx = p3d.point_covariances(PN.recentre(pts, lengths), lengths, K, return_idx=True)
    else:
        curv, frames, cov, idx = wrong(pts, lengths, K, **variant)
    return tuple(C.pack(t, lengths) for t in (cov, curv, frames, idx))


def wrong(pts, lengths, K, recentre=True, eigh=False, tie_high=False, flip_le=False, swap=False):
    """The contract with one thing changed, from the formulation's own pieces."""
    x = PN.recentre(pts, lengths) if recentre else pts
    if tie_high:  # equal distances to the HIGHER index: the mirrored cloud's order, mapped back
        P = x.shape[1]
        live = C.live_mask(lengths, P)
        rev = torch.zeros_like(x)
        for n, length in enumerate(lengths.tolist()):
            rev[n, :length] = x[n, :length].flip(0)
        idx, _ = torch_knn_forward(rev, rev, lengths, lengths, 2, K)
        idx = (lengths[:, None, None] - 1 - idx)
        for n, length in enumerate(lengths.tolist()):
            idx[n, :length] = idx[n, :length].flip(0)
        idx = idx.masked_fill(~live[..., None], 0)
    else:
        idx, _ = torch_knn_forward(x, x, lengths, lengths, 2, K)
    nbrs = knn_gather(x, idx, lengths)
    cov = PN._covariances(nbrs)
    curv, frames = torch.linalg.eigh(cov) if eigh else PN.symeig3x3(cov)
    if swap:
        frames = frames[..., [2, 1, 0]]
    cols = []
    for c in (0, 2):
        v = frames[:, :, :, c]
        n_pos = (((nbrs - x[:, :, None]) * v[:, :, None]).sum(3) > 0).float().sum(2, keepdim=True)
        flip = (n_pos <= 0.5 * K) if flip_le else (n_pos < 0.5 * K)
        cols.append(torch.where(flip, -v, v))
    frames = torch.stack((cols[0], torch.linalg.cross(cols[0], cols[1], dim=2), cols[1]), dim=3)
    return curv, frames, cov, idx


@pytest.mark.parametrize("case", CASES, ids=C.case_id)
def test_formulation_passes_every_gate(case):
    pts, lengths = C.inputs(case)
    cov, curv, frames, idx = run(case)
    C.check(case, cov, curv, frames, idx)
    full_idx = p3d.point_covariances(PN.recentre(pts, lengths), lengths, case[1], return_idx=True)[1]
    C.check_idx_order(full_idx, PN.recentre(pts, lengths), lengths, case[1])


def test_padded_rows_are_zero_and_the_variant_builder_is_the_formulation():
    case = ("plane", 5)
    pts, lengths = C.inputs(case)
    curv, frames = p3d.estimate_pointcloud_local_coord_frames(C.Clouds(pts, lengths), neighborhood_size=5)
    cov = p3d.point_covariances(PN.recentre(pts, lengths), lengths, 5)
    dead = ~C.live_mask(lengths, pts.shape[1])
    assert dead.any() and not curv[dead].any() and not frames[dead].any() and not cov[dead].any()
    got = wrong(pts, lengths, 5)  # nothing changed: the same bits on the live rows
    for a, b in zip((curv, frames, cov), got[:3]):
        assert torch.equal(C.pack(a, lengths), C.pack(b, lengths))


@pytest.mark.parametrize("case, variant, gate", [
    (("small", 8), {"eigh": True}, "curv error"),            # a true eigen-decomposition in the blend region
    (("small", 50), {"eigh": True}, "curv error"),
    (("sphere", 50), {"recentre": False}, "cov error"),      # the missing global recentring, 3700 radii from the origin
    (("sphere", 4), {"flip_le": True}, "signs of column"),   # a flip at <= : n_pos = K / 2 turns round
    (("plane", 16), {"flip_le": True}, "signs of column"),
    (("blob", 32), {"swap": True}, "vec error"),             # columns 0 and 2 swapped
], ids=lambda v: v if isinstance(v, str) else ("-".join(map(str, v)) if isinstance(v, tuple) else "+".join(v)))
def test_the_gates_refuse_wrong_variants(case, variant, gate):
    cov, curv, frames, idx = run(case, **variant)
    with pytest.raises(AssertionError, match=gate):
        C.check(case, cov, curv, frames, idx)


@pytest.mark.parametrize("K", [3, 9, 50])
def test_the_order_gate_refuses_ties_to_the_higher_index(K):
    case = ("lattice", K)
    pts, lengths = C.inputs(case)
    x = PN.recentre(pts, lengths)
    idx = wrong(pts, lengths, K, tie_high=True)[3]
    own, _ = torch_knn_forward(x, x, lengths, lengths, 2, K)
    d = ((x[:, :, None] - knn_gather(x, idx, lengths)) ** 2).sum(3)
    assert bool((d[:, :, 1:] >= d[:, :, :-1]).all())  # a valid nearest-neighbour answer, only the ties differ
    with pytest.raises(AssertionError, match="order"):
        C.check_idx_order(idx, x, lengths, K)
    C.check_idx_order(own, x, lengths, K)


def test_argument_errors_and_inputs():
    pts = torch.rand(2, 30, 3)
    with pytest.raises(ValueError, match=r"shape \(minibatch, N, 3\)"):
        p3d.estimate_pointcloud_normals(torch.rand(2, 30, 2), 5)
    with pytest.raises(ValueError, match="neighborhood_size argument"):
        p3d.estimate_pointcloud_normals(pts, 30)
    with pytest.raises(ValueError, match="neighborhood_size argument"):
        p3d.estimate_pointcloud_local_coord_frames(C.Clouds(pts, torch.tensor([30, 5])), 5)
    with pytest.raises(ValueError, match="Pointclouds objects or tensors"):
        p3d.estimate_pointcloud_normals([pts], 5)
    with pytest.raises(ValueError):
        p3d.point_covariances(pts, None, 0)
    # defaults and return shapes of the reference; a tensor is a batch of full clouds
    big = torch.rand(1, 60, 3)
    normals = p3d.estimate_pointcloud_normals(big)
    curv, frames = p3d.estimate_pointcloud_local_coord_frames(big)
    assert normals.shape == (1, 60, 3) and curv.shape == (1, 60, 3) and frames.shape == (1, 60, 3, 3)
    assert torch.equal(normals, frames[:, :, :, 0])
    again = p3d.estimate_pointcloud_local_coord_frames(C.Clouds(big, torch.tensor([60])), 50, True, use_symeig_workaround=True)
    assert torch.equal(again[0], curv) and torch.equal(again[1], frames)
    raw = p3d.estimate_pointcloud_local_coord_frames(big, 50, False)[1]
    assert torch.equal(raw[:, :, :, 0].abs(), frames[:, :, :, 0].abs())  # disambiguation only turns vectors round
    skipped = p3d.estimate_pointcloud_local_coord_frames(big, 50, check_lengths=False)
    assert torch.equal(skipped[1], frames)


def test_paths_the_kernel_does_not_take():
    pts = torch.rand(1, 120, 3, generator=torch.Generator().manual_seed(3))
    assert not PN.kernel_path(pts, 8)  # a CPU tensor
    # K > 64: float32 against the same formulation in float64
    c32, f32 = p3d.estimate_pointcloud_local_coord_frames(pts, 70)
    c64, f64 = p3d.estimate_pointcloud_local_coord_frames(pts.double(), 70)
    assert c64.dtype == torch.float64 and float((c32 - c64).abs().max()) <= 1e-5 * float(c64.max())
    assert float((1 - (f32[..., 0].double() * f64[..., 0]).sum(-1)).abs().max()) < 1e-4
    # use_symeig_workaround=False is torch.linalg.eigh of the covariances
    c, f = p3d.estimate_pointcloud_local_coord_frames(pts, 8, False, use_symeig_workaround=False)
    want = torch.linalg.eigh(p3d.point_covariances(PN.recentre(pts, torch.tensor([120])), None, 8))
    assert torch.equal(c, want[0]) and torch.equal(f, want[1])


def test_gradient_equals_autograd_through_the_reference():
    want = C.fixture()["grad/expected"]
    got = C.grad_of(p3d.estimate_pointcloud_local_coord_frames)
    assert bool(torch.isfinite(got).all())
    worst, scale = float((got - want).abs().max()), float(want.abs().max())
    print("gradient: largest difference %.3g, largest entry %.3g" % (worst, scale))
    assert worst <= 1e-4 * scale


def test_boundary_symbols_constants_and_exports():
    from pytorch3d_amd import _C, _lib

    assert "p3d_point_frames_workgroups" in _lib.EXPORTED_SYMBOLS and _lib.FRAMES_ROWS_PER_GROUP == 64
    assert "p3d_point_frames" in _lib.EXPORTED_SYMBOLS and _lib.FRAMES_MAX_K == 64 and _lib.KNN_MAX_K == 32
    header = open(os.path.join(ROOT, "include", "p3d_amd.h")).read()
    assert "#define P3D_FRAMES_MAX_K 64" in header and "#define P3D_FRAMES_DISAMBIGUATE 1u" in header
    build = importlib.import_module("pytorch3d_amd.build")
    assert "point_frames.hip" in build.SOURCES and "knn_queue.h" in build.HEADERS
    for name in ("estimate_pointcloud_normals", "estimate_pointcloud_local_coord_frames", "point_covariances"):
        assert getattr(p3d, name) is getattr(PN, name)
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        _C.point_frames(torch.rand(1, 10, 3), None, 3)
    source = open(os.path.join(ROOT, "pytorch3d_amd", "points_normals.py")).read() + open(
        os.path.join(ROOT, "pytorch3d_amd", "csrc", "point_frames.hip")).read()
    assert "deterministic_algorithms" not in source and "atomic" not in source.replace("No atomics", "").replace("no atomics", "")
