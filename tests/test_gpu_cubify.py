"""cubify on the GPU: csrc/cubify.hip against the reference's recorded results (tests/golden/cubify_ref.npz), the nested-loop
restatement of tests/cubify_case.py and, for shapes too large for loops, the torch formulation run on the CPU.  Every comparison is
torch.equal (cubify_case.misses).  The scan cases are sized from the header's P3D_CUBIFY_* constants and assert that they reach the
path they are named for.  A scan block holds items of ONE mesh (mesh n owns blocks [n * bpm, (n + 1) * bpm)), and the launches are
never capped, so there is no grid-stride round to reach: the second round that exists is the carry kernel's, over more blocks than
P3D_CUBIFY_CARRY_BLOCK."""
import importlib
import itertools
import json
import os
import subprocess
import sys
import warnings

import pytest
import torch

import cubify_case as C

import pytorch3d_amd as p3d
from pytorch3d_amd import _lib

M = importlib.import_module("pytorch3d_amd.cubify")  # (the package re-exports the FUNCTION cubify over the sub-module)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
ITEMS, LANES, CARRY = _lib.CUBIFY_ITEMS, _lib.CUBIFY_BLOCK, _lib.CUBIFY_CARRY_BLOCK


def _kernels(voxels, thresh, feats=None, align="topleft"):
    """The three lists from the kernels; asserts that the kernels ran."""
    assert M.kernel_path(voxels, feats, None, align)
    before = dict(M.CALLS)
    packed = p3d.cubify_packed(voxels, thresh, feats, align)
    assert M.CALLS["fused"] == before["fused"] + 1 and M.CALLS["formulation"] == before["formulation"]
    assert packed[0].device == voxels.device and packed[1].dtype == torch.int64 and packed[0].dtype == torch.float32
    return C.lists_of(packed)


def _formulation_on_cpu(voxels, thresh, feats=None, align="topleft"):
    return C.lists_of(M.cubify_packed_torch(voxels.cpu(), thresh, None if feats is None else feats.cpu(), align))


def _blocks(shape):
    """(scan blocks over the voxels, scan blocks over the lattice points) of a batch."""
    N, D, H, W = shape
    return N * -(-(D * H * W) // ITEMS), N * -(-((D + 1) * (H + 1) * (W + 1)) // ITEMS)


def _random(shape, density, seed):
    return C.random_voxels(shape, density, torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("name", C.cases())
def test_fixture_cases_on_the_kernels(name):
    voxels, thresh, feats, align = C.inputs(name, DEV)
    assert C.misses(_kernels(voxels, thresh, feats, align), C.expected(name), name) == []


@pytest.mark.parametrize("shape,density", [((5, 3, 3, 3), 0.5), ((3, 5, 7, 9), 0.4), ((4, 2, 2, 2), 0.6)],
                         ids=["5x3x3x3", "3x5x7x9", "4x2x2x2"])
def test_small_meshes_and_sizes_that_are_no_multiple_of_a_wave(shape, density):
    """Meshes far smaller than a scan block (27 voxels, 64 lattice points: each in a block of its own, most lanes idle, ranks restart
    per mesh) and voxel / lattice counts that are no multiple of 64 or of the workgroup."""
    N, D, H, W = shape
    m, l = D * H * W, (D + 1) * (H + 1) * (W + 1)
    assert m < ITEMS and l < ITEMS and _blocks(shape) == (N, N)
    if shape[1:] == (5, 7, 9):
        assert m % 64 and l % 64 and m > LANES and l > LANES and m % LANES and l % LANES  # more than one round, a ragged last one
    voxels, thresh = _random(shape, density, 7)
    got = _kernels(voxels.to(DEV), thresh)
    want = C.restate(voxels, thresh)
    assert C.misses(got, want) == [] and C.misses(got, _formulation_on_cpu(voxels, thresh)) == []
    assert all(int(f.min()) == 0 for f in got[1] if f.numel())  # ranks start at 0 in every mesh


@pytest.mark.parametrize("align", C.ALIGNS)
def test_one_mesh_over_several_scan_blocks(align):
    shape = (2, 16, 16, 16)
    assert _blocks(shape) == (2 * 4, 2 * 5) and 17 ** 3 % ITEMS  # a mesh spans 4 / 5 blocks, the last one ragged; carries inside a mesh
    voxels, thresh = _random(shape, 0.45, 11)
    feats = torch.rand((2, 2, 16, 16, 16), generator=torch.Generator().manual_seed(12))
    assert C.misses(_kernels(voxels.to(DEV), thresh, feats.to(DEV), align), _formulation_on_cpu(voxels, thresh, feats, align)) == []


@pytest.mark.parametrize("shape,density", [((1024 + 70, 2, 2, 3), 0.5), ((600, 8, 8, 17), 0.2)], ids=["1094x2x2x3", "600x8x8x17"])
def test_second_round_of_the_carry_scan(shape, density):
    """More scan blocks than the carry kernel's lanes: its second round, with a running total carried over.  The smallest grid that
    gets there is many tiny meshes (a block each); the second case has meshes of two blocks each across the round's border.  Some
    meshes are empty, at the border too."""
    nb_f, nb_v = _blocks(shape)
    assert nb_f > CARRY and nb_v > CARRY and nb_f < 2 * CARRY + CARRY // 2
    if shape[0] == 600:
        assert nb_f == 2 * shape[0] and nb_v == 2 * shape[0]
    voxels, thresh = _random(shape, density, 13)
    voxels[::7] = 0.0
    voxels[CARRY // (nb_f // shape[0]) - 1:CARRY // (nb_f // shape[0]) + 1] = 0.0  # the meshes on either side of the round's border
    voxels[-1] = 0.0
    got = _kernels(voxels.to(DEV), thresh)
    assert C.misses(got, _formulation_on_cpu(voxels, thresh)) == []  # (the reference side: the torch formulation on the CPU)
    assert sum(f.shape[0] for f in got[1]) > 0 and got[1][0].shape == (0, 3) and got[1][-1].shape == (0, 3)


@pytest.mark.parametrize("dims", list(itertools.permutations((2, 3, 4))), ids=lambda d: "x".join(map(str, d)))
def test_axis_order(dims):
    voxels, thresh = _random((2,) + dims, 0.5, 17 + dims[0] * 10 + dims[1])
    feats = torch.rand((2, 2) + dims, generator=torch.Generator().manual_seed(3))
    for align in C.ALIGNS:
        assert C.misses(_kernels(voxels.to(DEV), thresh, feats.to(DEV), align), C.restate(voxels, thresh, feats, align), align) == []


@pytest.mark.parametrize("K", [1, 3, 4, 7])
def test_strided_voxels_and_feats(K):
    gen = torch.Generator().manual_seed(19 + K)
    wide = torch.rand((2, 3, 4, 3, 5), generator=gen).to(DEV)  # (N, C, D, H, W): a channel slice, as the voxel head gives
    feats = torch.rand((2, 4, 3, 5, K + 2), generator=gen).to(DEV).permute(0, 4, 1, 2, 3)[:, 1:K + 1]  # K innermost in memory, sliced
    voxels = wide[:, 1]
    assert not voxels.is_contiguous() and not feats.is_contiguous() and feats.shape[1] == K
    want = C.restate(voxels.contiguous(), 0.4, feats.contiguous(), "center")
    assert C.misses(_kernels(voxels, 0.4, feats, "center"), want) == []
    permuted = torch.rand((2, 3, 5, 4), generator=gen).to(DEV).permute(0, 3, 1, 2)  # (N, D, H, W) with D innermost in memory
    assert permuted.stride()[1] == 1
    assert C.misses(_kernels(permuted, 0.5, None, "corner"), C.restate(permuted.contiguous(), 0.5, None, "corner")) == []
    stepped = torch.rand((2, 4, 6, 8), generator=gen).to(DEV)[:, ::2, 1::2, ::3]
    assert C.misses(_kernels(stepped, 0.5), C.restate(stepped.contiguous(), 0.5)) == []


def test_threshold_rounding_nan_and_inf():
    at = torch.full((1, 2, 2, 2), 0.7, dtype=torch.float32, device=DEV)  # float32(0.7) < 0.7, and `ge` rounds the threshold: occupied
    assert int(p3d.cubify_packed(at, 0.7)[3].sum()) == 48
    assert int(p3d.cubify_packed(torch.nextafter(at, torch.zeros_like(at)), 0.7)[3].sum()) == 0
    odd = torch.tensor([float("nan"), float("inf"), float("-inf"), 1.0, 0.0, float("nan"), 2.0, float("inf")], device=DEV).view(1, 2, 2, 2)
    for thresh in (0.5, float("inf"), float("-inf")):
        assert C.misses(_kernels(odd, thresh), C.restate(odd, thresh), str(thresh)) == []
    assert p3d.cubify_packed(odd, float("nan"))[0].shape == (0,)  # nothing is >= NaN


def test_empties():
    none = _kernels(torch.zeros((3, 2, 3, 2), device=DEV), 0.5)
    assert [(t.shape, t.dtype) for t in none[0] + none[1]] == [((0,), torch.float32)] * 3 + [((0,), torch.int64)] * 3
    voxels, thresh = _random((5, 3, 2, 4), 0.6, 23)
    voxels[0::2] = 0.0  # empty meshes first, in the middle and last
    got = _kernels(voxels.to(DEV), thresh)
    assert C.misses(got, C.restate(voxels, thresh)) == []
    assert [tuple(t.shape) for t in got[0][0::2] + got[1][0::2]] == [(0, 3)] * 6
    assert all(int(f.min()) == 0 and int(f.max()) == v.shape[0] - 1 for v, f in zip(got[0][1::2], got[1][1::2]))
    zero = p3d.cubify(torch.zeros((0, 3, 3, 3), device=DEV), 0.5)
    assert len(zero) == 0 and zero.verts_list() == []


def test_same_bits_on_a_second_run_and_a_side_stream():
    voxels, thresh = _random((3, 9, 10, 11), 0.5, 29)
    voxels = voxels.to(DEV)
    feats = torch.rand((3, 3, 9, 10, 11), device=DEV)
    first = _kernels(voxels, thresh, feats, "center")
    assert C.misses(_kernels(voxels, thresh, feats, "center"), [[t.cpu() for t in l] for l in first]) == []
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        again = _kernels(voxels, thresh, feats, "center")
    side.synchronize()
    assert C.misses(again, [[t.cpu() for t in l] for l in first]) == []


def test_exactly_one_host_sync(monkeypatch):
    voxels, thresh = _random((4, 6, 7, 8), 0.5, 31)
    voxels = voxels.to(DEV)
    p3d.cubify_packed(voxels, thresh)  # (the library is loaded, the coordinate tables of this shape are on the device)
    reads = []
    for name in ("cpu", "item", "tolist", "numpy"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *args, _orig=orig, _name=name, **kwargs):
            if self.is_cuda:
                reads.append(_name)
            return _orig(self, *args, **kwargs)

        monkeypatch.setattr(torch.Tensor, name, counted)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            verts, faces, nv, nf, _ = p3d.cubify_packed(voxels, thresh)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in caught if "synchroniz" in str(w.message)]
    assert reads == ["cpu"] and len(syncs) == 1, (reads, [str(w.message) for w in caught])
    assert nv.is_cuda and nf.is_cuda and verts.shape[0] == int(nv.sum())


def test_public_function_device_argument_and_views():
    voxels, thresh, feats, align = C.inputs("feats_center", DEV)
    assert M.kernel_path(voxels, feats, "cuda:0", align) and M.kernel_path(voxels, feats, torch.device("cuda"), align)
    assert not M.kernel_path(voxels, feats, "cpu", align) and not M.kernel_path(voxels.double(), feats, None, align)
    assert not M.kernel_path(voxels, feats.double(), None, align) and M.kernel_path(voxels, feats.double(), None, "corner")
    meshes = p3d.cubify(voxels, thresh, feats=feats, device=DEV, align=align)
    assert C.misses((meshes.verts_list(), meshes.faces_list(), meshes.textures), C.expected("feats_center")) == []
    v = meshes.verts_list()
    assert v[1].data_ptr() == v[0].data_ptr() + v[0].numel() * 4  # split views of one packed tensor
    before = M.CALLS["formulation"]
    host = p3d.cubify(voxels, thresh, feats=feats, device="cpu", align=align)  # another device than the voxels': the formulation
    assert M.CALLS["formulation"] == before + 1 and host.verts_list()[0].device.type == "cpu"
    assert C.misses((host.verts_list(), host.faces_list(), host.textures), C.expected("feats_center")) == []
    assert C.misses(C.lists_of(p3d.cubify_packed(voxels.double(), thresh)), C.restate(voxels.double(), thresh)) == []  # float64 on the GPU


def test_the_shim_on_the_gpu():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    if not os.path.isdir(os.path.join(stage, "pytorch3d", "ops")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_cubify_case.py"), "cuda:0"], capture_output=True, text=True,
                         timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    print(json.dumps(rec))
    assert rec["plain_leaves_cubify_alone"] and rec["plain_misses"] == [] and rec["calls_before_patch"] == 0
    assert rec["patched"] and rec["device_misses"] == [] and rec["host_misses"] == [] and rec["float64_misses"] == []
    assert rec["device_calls"] == [rec["cases"], 0] and rec["host_and_float64_calls"] == [0, 3]
    assert rec["feeds"][0][:2] == [2, rec["feeds"][0][1]] and rec["feeds"][0][2] == 4 and rec["feeds"][1] == [2, 50, 3] and rec["feeds"][2]
    assert rec["restored"]
