"""The launch plan of the point forward (include/p3d_amd.h: p3d_rasterize_points_ex): which launches one call of
_C.rasterize_points / _C.rasterize_points_composite makes, by the names and counts p3d_profile_* records.

Every path: plain, CUDA tie order and composite; naive and binned; K = 10 (register queues when naive, the tile-sorted kernel with its
compositor epilogue when binned) and K = 32 (the sorted kernel either way, the compositor as a pass); binned with the worst-case
workspace and with a short one (SHORT_WORKSPACE 'always', a first guess of one list entry: the host adds the stand-by launches, the
device decides which of them write).  The table was recorded before the three point forwards of the C ABI were folded into one host
function, and the file uses only what both sides of that change have: it pins that the fold kept every launch of every path.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZE, BIN_SIZE, MAX_PER_BIN, RADIUS = (64, 64), 16, 1000, 0.05

# (mode, binning, K) -> {launch scope: launches in one call}, as recorded on the parent of the fold.  The tile-sorted kernel (binned,
# K = 10) forms the image itself, unless the lists may not fit: then the stand-by's pass runs behind it, gated on the device.
_BINNING = {"bin_count": 1, "bin_scan_small": 1, "bin_fill": 1}
PLAN = {
    ("plain", "naive", 10): dict(points_naive=1),
    ("plain", "naive", 32): dict(points_naive=1),
    ("plain", "binned", 10): dict(_BINNING, points_fine=1),
    ("plain", "binned", 32): dict(_BINNING, points_fine=1),
    ("plain", "short", 10): dict(_BINNING, points_fine=1, points_naive=1),
    ("plain", "short", 32): dict(_BINNING, points_fine=1, points_naive=1),
    ("tie", "naive", 10): dict(points_cuda_order=1, points_naive=1),
    ("tie", "naive", 32): dict(points_cuda_order=1, points_naive=1),
    ("tie", "binned", 10): dict(_BINNING, points_cuda_order=1, points_fine=1),
    ("tie", "binned", 32): dict(_BINNING, points_cuda_order=1, points_fine=1),
    ("tie", "short", 10): dict(_BINNING, points_cuda_order=2, points_fine=1, points_naive=1),
    ("tie", "short", 32): dict(_BINNING, points_cuda_order=2, points_fine=1, points_naive=1),
    ("composite", "naive", 10): dict(points_composite=1, points_naive=1),
    ("composite", "naive", 32): dict(points_composite=1, points_naive=1),
    ("composite", "binned", 10): dict(_BINNING, points_fine=1),
    ("composite", "binned", 32): dict(_BINNING, points_composite=1, points_fine=1),
    ("composite", "short", 10): dict(_BINNING, points_composite=1, points_fine=1, points_naive=1),
    ("composite", "short", 32): dict(_BINNING, points_composite=1, points_fine=1, points_naive=1),
}


def _cloud(d):
    gen = torch.Generator().manual_seed(11)
    pts = torch.rand(3000, 3, generator=gen) * 2 - 1
    pts[:, 2] = pts[:, 2] + 1.5
    first = torch.tensor([0, 1200], dtype=torch.int64)
    count = torch.tensor([1200, 1800], dtype=torch.int64)
    feats = torch.rand(3000, 3, generator=gen)
    return pts.to(d), first.to(d), count.to(d), torch.full((3000,), RADIUS).to(d), feats.to(d)


def observe(mode, binning, K):
    """{launch scope: launches} of one call."""
    from pytorch3d_amd import _C, _lib

    pts, first, count, radius, feats = _cloud(torch.device("cuda:0"))
    lib = _lib.load()
    saved = (_C.SHORT_WORKSPACE, _C.SHORT_WORKSPACE_FIRST_GUESS, _C.CUDA_TIE_ORDER)
    _C.SHORT_WORKSPACE = "always" if binning == "short" else "never"
    _C.SHORT_WORKSPACE_FIRST_GUESS = 1
    _C.CUDA_TIE_ORDER = mode == "tie"
    _C._NEEDS.clear()
    bins = (0, 0) if binning == "naive" else (BIN_SIZE, MAX_PER_BIN)
    try:
        torch.cuda.synchronize()
        lib.p3d_profile_reset()
        lib.p3d_profile_enable(1)
        if mode == "composite":
            _C.rasterize_points_composite(pts, first, count, SIZE, radius, feats, _C.inv_r2_of(RADIUS), K, *bins)
        else:
            _C.rasterize_points(pts, first, count, SIZE, radius, K, *bins)
        torch.cuda.synchronize()
        lib.p3d_profile_enable(0)
        return {name: n for name, (n, _) in _lib.profile_snapshot().items()}
    finally:
        lib.p3d_profile_enable(0)
        lib.p3d_profile_reset()
        _C.SHORT_WORKSPACE, _C.SHORT_WORKSPACE_FIRST_GUESS, _C.CUDA_TIE_ORDER = saved
        _C._NEEDS.clear()


@pytest.mark.parametrize("mode,binning,K", list(PLAN))
def test_point_forward_launch_plan(mode, binning, K):
    assert observe(mode, binning, K) == PLAN[(mode, binning, K)]
