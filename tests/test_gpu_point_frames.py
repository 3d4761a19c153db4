"""estimate_pointcloud_normals / estimate_pointcloud_local_coord_frames / point_covariances on the GPU (csrc/point_frames.hip)
through the gates of tests/point_frames_case.py against the reference's recorded float64 run (tests/golden/point_frames_ref.npz):
every tolerance is MARGIN x the reference's own float32 figure recorded there, the neighbour lists are bit-equal to
pytorch3d_amd.knn.torch_knn_forward on the recentred points.  Then the boundary flavours, reproducibility, a dense cloud that
keeps every row of the 64-entry queue live in every lane, the dispatch, the padded rows, a launch of several tiles and workgroups
per cloud, and the unmodified reference's Pointclouds.estimate_normals through the shim."""
import importlib
import json
import os
import subprocess
import sys

import pytest
import torch

import point_frames_case as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PN = importlib.import_module("pytorch3d_amd.points_normals")


def _dev():
    return torch.device("cuda:0")


def _kernel(pts, lengths, K, disambiguate=True):
    """(curv, frames, cov, idx, recentred points) of the kernel on a ragged batch, all on the GPU."""
    from pytorch3d_amd import _C

    x = PN.recentre(pts.to(_dev()), lengths.to(_dev()))
    assert PN.kernel_path(x, K)
    return _C.point_frames(x, lengths.to(_dev()), K, disambiguate, frames=True, cov=True, idx=True) + (x,)


@pytest.mark.parametrize("case", C.all_cases(), ids=C.case_id)
def test_kernel_passes_every_gate(case):
    import pytorch3d_amd as p3d

    pts, lengths = C.inputs(case)
    K = case[1]
    curv, frames, cov, idx, x = _kernel(pts, lengths, K)
    C.check(case, *(C.pack(t, lengths) for t in (cov, curv, frames, idx)))
    C.check_idx_order(idx, x, lengths, K)
    # the public functions are this launch
    got = p3d.estimate_pointcloud_local_coord_frames(C.Clouds(pts.to(_dev()), lengths.to(_dev())), neighborhood_size=K)
    assert torch.equal(got[0], curv) and torch.equal(got[1], frames)
    assert torch.equal(p3d.point_covariances(x, lengths.to(_dev()), K), cov)
    # padded rows are zero in every output
    dead = ~C.live_mask(lengths, pts.shape[1]).to(_dev())
    assert dead.any() and not any(bool(t[dead].any()) for t in (curv, frames, cov, idx))
    # without disambiguation: the same vectors up to sign, column 1 untouched by the cross product
    raw = p3d.estimate_pointcloud_local_coord_frames(C.Clouds(pts.to(_dev()), lengths.to(_dev())), K, False)
    assert torch.equal(raw[0], curv) and torch.equal(raw[1][..., 0].abs(), frames[..., 0].abs())
    assert torch.equal(raw[1][..., 2].abs(), frames[..., 2].abs())


def test_ctypes_and_pybind_flavours_are_bit_equal():
    from pytorch3d_amd import _C, build_bind

    pyb = build_bind.load()  # a flavour that does not build or import FAILS here: point_frames is new code in bind.cpp
    for case in (("blob", 64), ("lattice", 9), ("plane", 2)):
        pts, lengths = C.inputs(case)
        x, ln = PN.recentre(pts.to(_dev()), lengths.to(_dev())), lengths.to(_dev())
        for args in ((True, True, True, True), (False, True, False, False), (True, False, True, True)):
            a, b = _C.point_frames(x, ln, case[1], *args), pyb.point_frames(x, ln, case[1], *args)
            assert all((s is None and t is None) or torch.equal(s, t) for s, t in zip(a, b)), (case, args)
    full = torch.rand(2, 70, 3, device=_dev())
    a, b = _C.point_frames(full, None, 5), pyb.point_frames(full, None, 5, True, True, False, False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and b[2] is None and b[3] is None


def test_two_runs_and_a_side_stream_give_the_same_bits():
    pts, lengths = C.inputs(("sphere", 50))
    first = _kernel(pts, lengths, 50)[:4]
    second = _kernel(pts, lengths, 50)[:4]
    side = torch.cuda.Stream(_dev())
    side.wait_stream(torch.cuda.current_stream(_dev()))
    with torch.cuda.stream(side):
        third = _kernel(pts, lengths, 50)[:4]
    side.synchronize()
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("K", [64, 33])
def test_every_row_of_the_queue_live_in_all_lanes_dense(K):
    """Points on a ray at DESCENDING distance from every query of the last wave: seen from the 64 queries, which sit beyond the
    ray's near end, every candidate is nearer than all before it, so each insert shifts the whole queue of every lane -- all KQ = 64
    rows of registers carry live entries in all 64 lanes, and the first K - 1 of them are shifted out again and again."""
    P = 64 * 5
    t = torch.arange(P, dtype=torch.float32)
    pts = torch.stack([(P - t) * 0.5, 0.001 * (t % 7), 0.002 * (t % 5)], 1)[None].contiguous()  # x descends along the index
    lengths = torch.tensor([P])
    x = pts.to(_dev())  # taken as given: the order, not the centre, is the point
    from pytorch3d_amd import _C

    curv, frames, cov, idx = _C.point_frames(x, lengths.to(_dev()), K, True, frames=True, cov=True, idx=True)
    tail = idx[0, P - 64:]  # the last wave: its nearest K are the LAST K points scanned, itself included
    assert bool((tail.min(1).values >= P - 64 - K).all())
    C.check_idx_order(idx, x, lengths, K)
    # the covariances are the formulation's float32 operations in its order (the curvatures of these near-lines sit where acos
    # amplifies the last bit of its argument: they are gated on the fixture's cases, not here)
    want = PN.torch_point_frames(pts, lengths, K)[2]
    assert float((cov.cpu() - want).abs().max()) <= 1e-5 * float(want.abs().max()) and bool(torch.isfinite(curv).all())


def test_dispatch_takes_the_formulation_where_the_kernel_does_not_apply():
    import pytorch3d_amd as p3d

    pts = torch.rand(1, 150, 3, generator=torch.Generator().manual_seed(4)).to(_dev())
    assert PN.kernel_path(pts, 64) and PN.kernel_path(pts, 1)
    assert not PN.kernel_path(pts.double(), 8) and not PN.kernel_path(pts, 65) and not PN.kernel_path(pts, 8, False)
    assert not PN.kernel_path(pts.clone().requires_grad_(True), 8) and not PN.kernel_path(pts.cpu(), 8)
    fused = p3d.estimate_pointcloud_local_coord_frames(pts, 8)

    def worst(c):  # the curvatures against the kernel's, relative to the row's trace
        return float(((c.float() - fused[0]).abs().amax(-1) / fused[0].sum(-1)).max())

    # float64: the same function, so only float32 rounding separates the two -- at K >= 8 the fixture's cases put that at 1e-7
    # to 1e-5 of the trace (the lattice: 8e-5); eigh is ANOTHER function where the blend acts, only its route is checked
    for kwargs, K, arg in (({}, 8, pts.double()), ({}, 65, pts), ({"use_symeig_workaround": False}, 8, pts)):
        c, f = p3d.estimate_pointcloud_local_coord_frames(arg, K, **kwargs)
        assert c.is_cuda and c.dtype == arg.dtype and bool(torch.isfinite(f).all())
        if arg.dtype == torch.float64:
            assert worst(c) <= 1e-4, worst(c)
    leaf = pts.clone().requires_grad_(True)
    c, f = p3d.estimate_pointcloud_local_coord_frames(leaf, 8)
    (c.sum() + f[..., 0].sum()).backward()
    assert bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().sum()) > 0
    assert worst(c.detach()) <= 1e-4, worst(c.detach())  # the float32 formulation: torch's device kernels round differently


def test_long_launch_many_tiles_and_workgroups():
    """The kernel has no loop over the grid: p3d_point_frames launches p3d_point_frames_workgroups(N, P) = N * ceil(P /
    P3D_FRAMES_ROWS_PER_GROUP) workgroups, each owning its rows -- asserted from the library's own answer, which is what the launch
    uses.  What a long launch adds is the tile loop and the block index: P just past 8 tiles of P3D_KNN_TILE points, 65 workgroups
    per cloud, two clouds of different lengths, a small K."""
    from pytorch3d_amd import _C, _lib

    P, K = 8 * _lib.KNN_TILE + 37, 5
    lib = _lib.load()
    rows = _lib.FRAMES_ROWS_PER_GROUP
    assert lib.p3d_point_frames_workgroups(2, P) == 2 * ((P + rows - 1) // rows) == 130  # every row has a workgroup: one pass
    assert lib.p3d_point_frames_workgroups(1, rows) == 1 and lib.p3d_point_frames_workgroups(1, rows + 1) == 2
    assert lib.p3d_point_frames_workgroups(3, 2 ** 31 - 1) == 3 * 2 ** 25 and lib.p3d_point_frames_workgroups(2 ** 7, 2 ** 31 - 1) == -1
    assert P > 8 * _lib.KNN_TILE  # a ninth tile is staged
    gen = torch.Generator().manual_seed(21)
    pts = torch.rand(2, P, 3, generator=gen)
    lengths = torch.tensor([P, 3 * _lib.KNN_TILE + 1])
    pts[1, int(lengths[1]):] = 0
    x = PN.recentre(pts.to(_dev()), lengths.to(_dev()))
    curv, frames, cov, idx = _C.point_frames(x, lengths.to(_dev()), K, True, frames=True, cov=True, idx=True)
    C.check_idx_order(idx, x, lengths, K)
    # the formulation on the CPU from the same recentred points: the covariances are the same float32 operations in the same order;
    # the curvatures then differ by the two libraries' acos / cos / exp only (a few ulp of an angle, times 2 p <= 2 x the trace)
    want = PN.torch_point_frames(x.cpu(), lengths, K)
    live = C.live_mask(lengths, P)
    trace = want[2].diagonal(dim1=-2, dim2=-1).sum(-1)[live]
    assert float(((cov.cpu() - want[2]).abs().amax((2, 3))[live] / trace).max()) <= 1e-6
    assert float(((curv.cpu() - want[0]).abs().amax(2)[live] / trace).max()) <= 1e-5
    dead = ~live.to(_dev())
    assert not any(bool(t[dead].any()) for t in (curv, frames, cov, idx))


def test_reference_estimate_normals_through_the_shim():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_point_frames_case.py"), "cuda:0"], capture_output=True, text=True,
                         timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    print(json.dumps(rec))
    assert rec["unpatched_is_the_reference"] and rec["calls_before_patch"] == 0 and rec["patched_everywhere"]
    assert rec["estimate_normals_equal"] and rec["estimate_normals_nonzero"]
    assert rec["fused_calls"] == {"estimate_pointcloud_normals": 1, "estimate_pointcloud_local_coord_frames": 0}
    assert rec["fallback_calls"] == {"estimate_pointcloud_normals": 0, "estimate_pointcloud_local_coord_frames": 0}
    assert rec["float64_counted_as_fallback"] == 1 and rec["restored"]
