"""GraphConv / gather_scatter on the GPU: csrc/graph_conv.hip against the torch formulation of the same list order BIT FOR BIT on
every width rung and wave packing, and against the reference's recorded results (tests/golden/mesh_refine_ref.npz) through the gates
of tests/mesh_refine_case.py; views, empty shapes, the grid-stride second pass, autograd, run-to-run and stream-to-stream bits, and
the unmodified reference GraphConv through the shim."""
import importlib
import json
import os
import subprocess
import sys

import pytest
import torch

import mesh_refine_case as C

import pytorch3d_amd as p3d
from pytorch3d_amd import _C, _lib

G = importlib.import_module("pytorch3d_amd.graph_conv")  # (the package re-exports the FUNCTION graph_conv over the sub-module)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")

WIDTHS = (1, 3, 4, 5, 8, 63, 64, 65, 256, 257, 260)
SIZES = (1, 2, 63, 64, 65, 257)


def _bits(a, b):
    """Equal as bit patterns (torch.equal would let -0.0 pass for +0.0)."""
    return a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


@pytest.mark.parametrize("D", WIDTHS)
def test_kernel_equals_the_formulation_bit_for_bit(D):
    gen = torch.Generator().manual_seed(1000 + D)
    for V in SIZES:
        edges = C.graph(V, gen)  # E ~ 3 V with duplicates, self loops and isolated vertices; a hub of 700 from V = 63
        x, base = torch.randn((V, D), generator=gen), torch.randn((V, D), generator=gen)
        for directed in (True, False):
            topo = p3d.graph_topology(edges, V, directed)
            if V >= 63:
                off = topo.fwd_offsets.tolist()
                assert max(b - a for a, b in zip(off, off[1:])) >= C.HUB // 2
            dtopo = topo.to(DEV)
            for backward in (False, True):
                off, ent = topo.table(backward)
                doff, dent = dtopo.table(backward)
                assert _bits(_C.neighbor_sum(x.to(DEV), doff, dent), G.neighbor_sum_torch(x, off, ent)), (V, D, directed, backward)
                assert _bits(_C.neighbor_sum(x.to(DEV), doff, dent, base.to(DEV)), G.neighbor_sum_torch(x, off, ent, base)), (V, D, directed)


@pytest.mark.parametrize("name", C.gs_cases())
def test_gather_scatter_forward_and_backward_through_the_gates(name):
    got = C.run_gs(name, p3d.gather_scatter, DEV)
    assert got["out"].device == DEV and C.gate(name, got, show=print) == []
    want = C.run_gs(name, p3d.gather_scatter)
    assert _bits(got["out"], want["out"]) and _bits(got["gin"], want["gin"])


@pytest.mark.parametrize("name", C.gc_cases())
def test_graph_conv_forward_and_backward_through_the_gates(name):
    got = C.run_gc(name, p3d.graph_conv, DEV)
    assert C.gate(name, got, show=print) == []


@pytest.mark.parametrize("D", [4, 5, 64, 260])
def test_views_are_read_in_place_and_their_neighbours_do_not_leak(D):
    gen = torch.Generator().manual_seed(77 + D)
    V = 65
    edges = C.graph(V, gen)
    topo = p3d.graph_topology(edges, V)
    x, base = torch.randn((V, D), generator=gen), torch.randn((V, D), generator=gen)
    big = torch.full((V, D + 7), float("nan"))
    big[:, 1:1 + D] = x
    wide = torch.full((V, 2 * D + 4), float("nan"))
    wide[:, 4:4 + D] = base
    dbig, dwide = big.to(DEV), wide.to(DEV)
    rows, sbase = dbig[:, 1:1 + D], dwide[:, 4:4 + D]   # a misaligned start with stride > D; a strided base
    assert not rows.is_contiguous() and rows.data_ptr() % 16 != 0 and not sbase.is_contiguous()
    off, ent = topo.to(DEV).table()
    want = G.neighbor_sum_torch(x, *topo.table(), base)
    got = _C.neighbor_sum(rows, off, ent, sbase)
    assert _bits(got, want) and torch.isfinite(got).all()
    # the aligned strided view takes the float4 path where D allows it: the same bits
    assert _bits(_C.neighbor_sum(x.to(DEV), off, ent, sbase), want)
    # through autograd on the view
    leaf = dbig.clone().requires_grad_(True)
    out = p3d.gather_scatter(leaf[:, 1:1 + D], edges.to(DEV))
    out.backward(torch.ones_like(out))
    assert _bits(out, G.neighbor_sum_torch(x, *topo.table()))
    assert _bits(leaf.grad[:, 1:1 + D], G.neighbor_sum_torch(torch.ones(V, D), *topo.table(True)))
    assert (leaf.grad[:, 0] == 0).all() and (leaf.grad[:, 1 + D:] == 0).all()


def test_empty_shapes():
    none = torch.zeros((0, 2), dtype=torch.int64, device=DEV)
    one = torch.tensor([[0, 1]], device=DEV)
    x = torch.randn(4, 3, device=DEV)
    assert p3d.gather_scatter(x, none).tolist() == [[0.0] * 3] * 4            # E = 0: zeros, written by the kernel
    assert p3d.gather_scatter(torch.ones(0, 3, device=DEV), none).shape == (0, 3)  # V = 0
    assert p3d.gather_scatter(torch.ones(4, 0, device=DEV), one).shape == (4, 0)   # D = 0
    topo = p3d.graph_topology(none, 4)
    assert _bits(_C.neighbor_sum(x, *topo.table(), x), x)                     # E = 0 with a base: the base
    w, b = torch.ones(2, 3, device=DEV), torch.zeros(2, device=DEV)
    assert p3d.graph_conv(torch.ones(0, 3, device=DEV), one, w, b, w, b).shape == (0, 2)
    with pytest.raises(ValueError, match="same device"):
        p3d.graph_conv(x, one.cpu(), w, b, w, b)


def test_grid_stride_second_pass():
    rows_per_group = _lib.NEIGHBOR_SUM_GROUP_LANES  # D = 1: one lane per row
    V = _lib.NEIGHBOR_SUM_MAX_GROUPS * rows_per_group + 1500
    assert V > _lib.NEIGHBOR_SUM_MAX_GROUPS * rows_per_group  # the last vertices are served by a workgroup's second round
    gen = torch.Generator().manual_seed(5)
    ends = torch.cat([torch.randint(0, 1000, (3000,), generator=gen), torch.randint(V - 1000, V, (3000,), generator=gen)])
    edges = torch.stack([ends, ends[torch.randperm(6000, generator=gen)]], 1)  # only the first and last thousand vertices
    x = torch.randn((V, 1), generator=gen)
    topo = p3d.graph_topology(edges, V)
    got = _C.neighbor_sum(x.to(DEV), *topo.to(DEV).table())
    want = G.neighbor_sum_torch(x, *topo.table())
    assert _bits(got, want) and want[-1000:].abs().sum() > 0 and want[:1000].abs().sum() > 0


def test_same_bits_on_three_runs_and_a_side_stream():
    name = "gs_random_und_V257_D5"
    x, edges, directed, grad = C.inputs(name)
    x, edges = torch.cat([x] * 13, 1).to(DEV), edges.to(DEV)  # D = 65
    runs = [p3d.gather_scatter(x, edges, directed) for _ in range(3)]
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        runs.append(p3d.gather_scatter(x, edges, directed))
    side.synchronize()
    assert all(_bits(runs[0], r) for r in runs[1:])


def test_the_table_of_a_gpu_edge_tensor_is_cached_and_checked():
    G.clear_topology_cache()
    edges = torch.tensor([[0, 1], [1, 2]], device=DEV)
    x = torch.randn(3, 4, device=DEV)
    before = dict(G.CACHE_STATS)
    p3d.gather_scatter(x, edges)
    p3d.gather_scatter(x, edges)
    assert G.CACHE_STATS["misses"] == before["misses"] + 1 and G.CACHE_STATS["hits"] == before["hits"] + 1
    with pytest.raises(ValueError, match=r"outside \[0, 3\)"):
        p3d.gather_scatter(x, torch.tensor([[0, 3]], device=DEV))


def test_reference_graph_conv_through_the_shim():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    if not os.path.isdir(os.path.join(stage, "pytorch3d", "ops")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_mesh_refine_case.py"), "cuda:0"], capture_output=True,
                         text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    print(json.dumps(rec))
    assert rec["unpatched_is_the_reference"] and rec["calls_before_patch"] == 0
    assert rec["plain_misses"] == []                       # the UNMODIFIED GraphConv on the GPU, forward and backward, all gc cases
    assert rec["plain_gather_scatter_misses"] == []
    assert rec["patched"] and rec["patched_misses"] == []
    assert rec["stage_misses"] == [] and rec["stage_fallback_calls"] == 0 and rec["stage_fused_calls"]["GraphConv.forward"] == 3
    assert rec["restored"]
