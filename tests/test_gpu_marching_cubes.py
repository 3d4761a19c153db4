"""csrc/marching_cubes.hip on the GPU: every fixture case against the restatement's device form (tests/marching_cubes_case.py, itself
tied to the reference's records in tests/test_cpu_marching_cubes.py), the packed form against the lists, the same bits on a second run
and on another stream, and shapes sized from the header's launch constants -- each asserting that it reaches its path -- against
marching_cubes_torch run on the CPU (pinned to the restatement in the CPU file).  Exact comparisons throughout, except the fixture's
local coordinates: 4 x the reference's own float32 rounding of the case."""
import importlib
import json
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import marching_cubes_case as C  # noqa: E402

import pytorch3d_amd as A  # noqa: E402
from pytorch3d_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
M = importlib.import_module("pytorch3d_amd.marching_cubes")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK, ITEMS, CARRY = _lib.MARCHING_CUBES_BLOCK, _lib.MARCHING_CUBES_ITEMS, _lib.MARCHING_CUBES_CARRY_BLOCK


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _fused(fn, *args):
    """fn(*args), asserting that the kernels ran and nothing else."""
    before = dict(M.CALLS)
    out = fn(*args)
    assert M.CALLS["fused"] == before["fused"] + 1 and M.CALLS["formulation"] == before["formulation"] and M.CALLS["host"] == before["host"]
    return out


def test_every_fixture_case_on_the_kernels(dev):
    assert C.failures(lambda v, i, l: _fused(A.marching_cubes, v, i, l), "device", device=dev) == []
    for name in C.cases():  # and tied to the reference's own records like the restatement
        vol, iso = C.inputs(name, dev)
        lists = _fused(A.marching_cubes, vol, iso, False)
        assert C.tie_misses(name, ([v.cpu() if torch.is_tensor(v) else v for v in lists[0]], [f.cpu() if torch.is_tensor(f) else f for f in lists[1]])) == []
    assert all(not C.inputs(n, dev)[0].is_contiguous() for n in C.STRIDED)


def test_packed_equals_the_lists_and_the_operator_gives_ascending_ids(dev):
    for name in ("rand579", "mixed_empty", "isonone"):
        vol, iso = C.inputs(name, dev)
        verts, faces, nv, nf = _fused(A.marching_cubes_packed, vol, iso, True)
        assert nv.device == vol.device and nv.dtype == torch.int64 and faces.dtype == torch.int64
        assert C.misses(C.to_lists(verts, faces, nv.tolist(), nf.tolist()), _fused(A.marching_cubes, vol, iso, True), name) == []
    vol, iso = C.inputs("rand579", dev)
    for n in range(vol.shape[0]):
        verts, faces, ids = _fused(M.marching_cubes_op, vol[n], iso)
        want = C.restate_device_one(vol[n].cpu().numpy(), iso)
        assert torch.equal(verts.cpu(), want[0]) and torch.equal(faces.cpu(), want[1]) and torch.equal(ids.cpu(), want[2])
        assert bool((ids[1:] > ids[:-1]).all())  # the reference wrapper's torch.unique is the identity on these


def test_same_bits_on_a_second_run_and_on_another_stream(dev):
    vol = torch.randn((3, 9, 10, 11), generator=torch.Generator().manual_seed(5)).to(dev)
    first = A.marching_cubes_packed(vol, 0.0)
    again = A.marching_cubes_packed(vol, 0.0)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        other = A.marching_cubes_packed(vol, 0.0)
    stream.synchronize()
    for a, b, c in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, c)


SHAPES = {  # name -> (shape, what it must reach)
    "many_tiny": ((CARRY + 6, 3, 3, 3), "more scan blocks than the carry kernel is wide: its second round; ranks restart per volume"),
    "long_row": ((2, 3, 3, 67), "a row of W - 1 = 66 cubes, longer than a wave"),
    "odd_lattice": ((3, 5, 7, 11), "385 lattice points: no multiple of 64 or of the workgroup"),
    "rounds": ((1, 9, 10, 11), "more than one round inside a scan block"),
    "two_blocks": ((2, 13, 14, 15), "two scan blocks per volume: carries inside a volume, and its second block starts mid-row"),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_sized_from_the_launch_constants(dev, name):
    shape = SHAPES[name][0]
    N, L = shape[0], shape[1] * shape[2] * shape[3]
    blocks = N * -(-L // ITEMS)
    assert {"many_tiny": blocks > CARRY and L < BLOCK, "long_row": shape[3] - 1 > 64, "odd_lattice": L % 64 and L % BLOCK and L < ITEMS,
            "rounds": BLOCK < L <= ITEMS, "two_blocks": ITEMS < L <= 2 * ITEMS and ITEMS % shape[3]}[name]
    vol = torch.randn(shape, generator=torch.Generator().manual_seed(11))  # half inside: nearly every cube emits
    for iso, local in ((0.0, False), (None, True)):
        want = A.marching_cubes_torch(vol, iso, local)
        got = _fused(A.marching_cubes_packed, vol.to(dev), iso, local)
        assert int(want[3].min()) > 0
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and torch.equal(a.cpu(), b)


def test_sizes_beyond_int32_take_the_formulation(dev):
    one = torch.zeros((1,), device=dev)
    assert not M.kernel_path(one.expand(1, 1024, 1024, 1024)) and M.kernel_path(one.expand(8, 128, 128, 128))


def test_the_unmodified_reference_function_through_the_shim(dev):
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    if not os.path.isdir(os.path.join(stage, "pytorch3d", "ops")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_marching_cubes_case.py"), "cuda:0"], capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    assert rec["plain_is_the_reference_function"] and rec["plain_misses"] == [] and rec["calls_before_patch"] == 0
    assert rec["patched"] and rec["patched_misses"] == [] and rec["patched_calls"] == [2 * rec["cases"], 0]
    assert rec["restored"] and rec["restored_misses"] == []
    assert rec["feeds"] == [[2, 50, 3], True]
