"""GraphConv / gather_scatter neighbour sums without a GPU: the torch formulation of the kernel's list order through the gates of
tests/mesh_refine_case.py (the reference's gather_scatter_python and GraphConv on the CPU, tests/golden/mesh_refine_ref.npz), the
table builder, the table cache, the ABI declarations, the shim module, and deliberately wrong variants that the gates must refuse."""
import gc
import importlib
import os
import re

import numpy as np
import pytest
import torch

import mesh_refine_case as C

import pytorch3d_amd as p3d
from pytorch3d_amd import _C, _lib, build

G = importlib.import_module("pytorch3d_amd.graph_conv")  # (the package re-exports the FUNCTION graph_conv over the sub-module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1


@pytest.mark.parametrize("name", C.gs_cases())
def test_gather_scatter_formulation_through_the_gates(name):
    lines = []
    bad = C.gate(name, C.run_gs(name, p3d.gather_scatter), show=lines.append)
    print("\n".join(lines))
    assert bad == []


@pytest.mark.parametrize("name", C.gc_cases())
def test_graph_conv_formulation_through_the_gates(name):
    lines = []
    bad = C.gate(name, C.run_gc(name, p3d.graph_conv), show=lines.append)
    print("\n".join(lines))
    assert bad == []


def test_a_topology_object_serves_in_place_of_the_edges():
    name = "gs_random_und_V65_D8"
    x, edges, directed, _ = C.inputs(name)
    topo = p3d.graph_topology(edges, 65, directed)
    assert topo.fwd_offsets is topo.bwd_offsets and topo.fwd_entries is topo.bwd_entries  # undirected: one table
    assert torch.equal(p3d.gather_scatter(x, topo), p3d.gather_scatter(x, edges, directed))
    with pytest.raises(ValueError, match="built for 65 vertices"):
        p3d.gather_scatter(x[:10], topo)


def _rows(topo, backward=False):
    off, ent = topo.table(backward)
    return [ent[off[v]:off[v + 1]].tolist() for v in range(topo.V)]


def test_builder_order_multiplicity_and_isolated_vertices():
    #              0       1       2 (dup) 3 (loop) 4
    edges = [(0, 1), (2, 0), (0, 1), (3, 3), (1, 2)]
    for dtype in (torch.int32, torch.int64):
        e = torch.tensor(edges, dtype=dtype)
        und = p3d.graph_topology(e, 6)
        # by edge index; in edge (a, b) the contribution to a comes first; the loop counts twice; 4 and 5 are isolated
        assert _rows(und) == [[1, 2, 1], [0, 0, 2], [0, 1], [3, 3], [], []]
        assert und.fwd_offsets.dtype == torch.int32 and und.fwd_entries.dtype == torch.int32 and und.E == 5 and not und.directed
        d = p3d.graph_topology(e, 6, directed=True)
        assert _rows(d) == [[1, 1], [2], [0], [3], [], []]          # v <- e[1] of the edges with e[0] == v; the loop once
        assert _rows(d, backward=True) == [[2], [0, 0], [1], [3], [], []]


def test_builder_empty_shapes_and_range_check():
    none = torch.zeros((0, 2), dtype=torch.int64)
    t = p3d.graph_topology(none, 4)
    assert t.fwd_offsets.tolist() == [0] * 5 and t.fwd_entries.numel() == 0
    t0 = p3d.graph_topology(none, 0, directed=True)
    assert t0.fwd_offsets.tolist() == [0] and t0.bwd_offsets.tolist() == [0]
    assert p3d.gather_scatter(torch.ones(4, 3), none).tolist() == [[0.0] * 3] * 4
    assert p3d.gather_scatter(torch.ones(0, 3), none).shape == (0, 3)
    assert p3d.gather_scatter(torch.ones(4, 0), torch.tensor([[0, 1]])).shape == (4, 0)
    for bad in ([[0, 4]], [[-1, 0]]):
        with pytest.raises(ValueError, match=r"outside \[0, 4\)"):
            p3d.graph_topology(torch.tensor(bad), 4)
        t = p3d.graph_topology(torch.tensor(bad + [[1, 2]]), 4, check=False)  # no sync; the bad edge contributes nothing readable
        out = G.neighbor_sum_torch(torch.arange(4.0)[:, None], *t.table())
        assert out[1].item() == 2.0 and out[2].item() == 1.0 and out[3].item() == 0.0
    with pytest.raises(ValueError, match="shape"):
        p3d.graph_topology(torch.zeros((3, 3), dtype=torch.int64), 4)
    with pytest.raises(ValueError, match="type"):
        p3d.graph_topology(torch.zeros((3, 2)), 4)


def test_argument_checks_carry_the_reference_messages():
    x, e = torch.ones(4, 3), torch.tensor([[0, 1]])
    for args, msg in (((torch.ones(4), e), "input can only have 2 dimensions."), ((x, e[0]), "edges can only have 2 dimensions."),
                      ((x, torch.zeros((2, 3), dtype=torch.int64)), r"edges must be of shape \(num_edges, 2\)."),
                      ((x.double(), e), "input has to be of type torch.float32."), ((x, e.int()), "edges has to be of type torch.int64.")):
        with pytest.raises(ValueError, match=msg):
            p3d.gather_scatter(*args)
    w, b = torch.ones(2, 3), torch.zeros(2)
    empty = p3d.graph_conv(torch.ones(0, 3, requires_grad=True), e, w, b, w, b)
    assert empty.shape == (0, 2) and empty.requires_grad  # the reference's empty-graph line


def test_float64_takes_the_formulation_in_the_same_order():
    x, edges, directed, _ = C.inputs("gs_random_und_V65_D8")
    topo = p3d.graph_topology(edges, 65)
    out64 = G.neighbor_sum_torch(x.double(), *topo.table())
    assert out64.dtype == torch.float64
    assert (out64 - C.fixture()["gs_random_und_V65_D8/out64"]).abs().max() < 1e-12


def test_a_broken_table_is_skipped_or_clamped():
    rows = torch.tensor([[1.0], [10.0], [100.0]])
    # entries -1, V and INT32_MAX are skipped
    off = torch.tensor([0, 3, 5, 7], dtype=torch.int32)
    ent = torch.tensor([-1, 1, 3, INT32_MAX, 2, 0, 0], dtype=torch.int32)
    assert G.neighbor_sum_torch(rows, off, ent).flatten().tolist() == [10.0, 100.0, 2.0]
    # offsets below 0 and past the list are clamped; a row that ends before it begins is empty
    off = torch.tensor([-5, 2, 1, 99], dtype=torch.int32)
    ent = torch.tensor([0, 1, 2], dtype=torch.int32)
    assert G.neighbor_sum_torch(rows, off, ent).flatten().tolist() == [11.0, 0.0, 110.0]
    base = torch.tensor([[0.5], [0.5], [0.5]])
    assert G.neighbor_sum_torch(rows, off, ent, base).flatten().tolist() == [11.5, 0.5, 110.5]


@pytest.mark.parametrize("directed", [True, False])
def test_adjoint_identity_is_exact_on_lattice_inputs(directed):
    gen = torch.Generator().manual_seed(3)
    edges = C.graph(65, gen)
    topo = p3d.graph_topology(edges, 65, directed)
    x, y = C.features((65, 7), "lattice", gen), C.features((65, 7), "lattice", gen)
    lhs = (G.neighbor_sum_torch(x, *topo.table(False)) * y).sum()
    rhs = (x * G.neighbor_sum_torch(y, *topo.table(True))).sum()
    assert lhs.item() == rhs.item() and lhs.item() != 0


def test_the_cache_recalls_objects_never_addresses():
    G.clear_topology_cache()
    stats = G.CACHE_STATS
    edges = torch.tensor([[0, 1], [1, 2]])
    h, m = stats["hits"], stats["misses"]
    t = p3d.topology_of_edges(edges, 3)
    assert p3d.topology_of_edges(edges, 3) is t and (stats["hits"], stats["misses"]) == (h + 1, m + 1)   # the same tensor hits
    assert p3d.topology_of_edges(edges, 3, directed=True) is not t and p3d.topology_of_edges(edges, 4) is not t
    edges[1, 1] = 0                                                      # an in-place write (_version) misses
    t2 = p3d.topology_of_edges(edges, 3)
    assert t2 is not t and _rows(t2) == [[1, 1], [0, 0], []]
    # a NEW tensor at a recycled address misses: two tensors, one after the other, over the same buffer (same data_ptr, same
    # _version of 0, same shape) -- what an allocator does when it hands a freed block out again
    G.clear_topology_cache()
    buf = np.array([[0, 1], [1, 2], [2, 3], [3, 0]], dtype=np.int64)
    a = torch.from_numpy(buf)
    ptr, ta = a.data_ptr(), p3d.topology_of_edges(a, 4)
    del a
    gc.collect()
    buf[:] = [[0, 2], [2, 1], [1, 3], [3, 0]]
    b = torch.from_numpy(buf)
    assert b.data_ptr() == ptr and b._version == 0
    tb = p3d.topology_of_edges(b, 4)
    assert tb is not ta and _rows(tb) == [[2, 3], [2, 3], [0, 1], [1, 0]]
    # bounded
    keep = [torch.tensor([[0, i % 3]]) for i in range(3 * G._CACHE_SIZE)]
    for e in keep:
        p3d.topology_of_edges(e, 3)
    assert len(G._cache) == G._CACHE_SIZE


def test_header_sources_and_exports():
    header = open(os.path.join(ROOT, "include", "p3d_amd.h")).read()
    assert re.search(r"\bp3d_neighbor_sum\(", header) and "p3d_neighbor_sum" in _lib._SIGNATURES
    assert int(re.search(r"#define P3D_ABI_VERSION (\d+)", header).group(1)) == 3 == _lib.ABI_VERSION
    assert int(re.search(r"#define P3D_NEIGHBOR_SUM_MAX_GROUPS (\d+)", header).group(1)) == _lib.NEIGHBOR_SUM_MAX_GROUPS
    assert "graph_conv.hip" in build.SOURCES
    assert _C.GRAPH_EXPORTS == ("gather_scatter",) and not set(_C.GRAPH_EXPORTS) & set(_C.HOT_PATH_EXPORTS)
    assert len(_C.HOT_PATH_EXPORTS) == 20
    lib = _lib.load()
    assert lib.p3d_abi_version() == 3
    assert lib.p3d_neighbor_sum(None, 0, 0, None, 0, None, None, -1, 0, 4, None, 4, None) == -1  # a negative size
    assert lib.p3d_neighbor_sum(None, 0, 0, None, 0, None, None, 0, 0, 4, None, 4, None) == 0    # V == 0: nothing to do
    assert lib.p3d_neighbor_sum(None, 0, 0, None, 0, None, None, 5, 0, 0, None, 0, None) == 0    # D == 0: nothing to do
    assert lib.p3d_neighbor_sum(None, 0, 0, None, 0, None, None, 5, 0, 4, None, 4, None) == -1   # no output


def test_shim_module_serves_the_wrapper():
    from pytorch3d_amd import shim

    mod = shim.make_module()
    assert mod.gather_scatter is G.gather_scatter_op
    with pytest.raises(NotImplementedError):
        mod.knn_points_idx()
    x, edges, directed, grad = C.inputs("gs_lattice_dir_V65_D8")
    z = C.fixture()
    assert torch.equal(mod.gather_scatter(x, edges, True, False), z["gs_lattice_dir_V65_D8/out"].float())
    assert torch.equal(mod.gather_scatter(grad, edges, True, True), z["gs_lattice_dir_V65_D8/gin"].float())


# ---- deliberately wrong variants: the gates must refuse every one ------------------------------------------------------------------
def _sum_with(table_of):
    """A gather_scatter whose table comes from table_of(edges, V, directed, backward) -> (offsets, entries)."""
    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, edges, directed):
            ctx.args = (edges, directed)
            return G.neighbor_sum_torch(x, *table_of(edges, x.shape[0], directed, False))

        @staticmethod
        def backward(ctx, grad):
            edges, directed = ctx.args
            return G.neighbor_sum_torch(grad, *table_of(edges, grad.shape[0], directed, True)), None, None

    return Fn.apply


def _right(edges, V, directed, backward):
    return p3d.graph_topology(edges, V, directed).table(backward)


def _undirected_as_directed(edges, V, directed, backward):
    return p3d.graph_topology(edges, V, True).table(backward)


def _deduplicated(edges, V, directed, backward):
    return p3d.graph_topology(torch.unique(edges, dim=0), V, directed).table(backward)


def _loop_once(edges, V, directed, backward):
    loops = edges[:, 0] == edges[:, 1]
    off, ent = p3d.graph_topology(edges[~loops], V, directed).table(backward)
    off1, ent1 = p3d.graph_topology(edges[loops], V, True).table(backward)
    # (the order inside a row does not matter for a refusal: the lattice sums are exact)
    rows = [ent[off[v]:off[v + 1]].tolist() + ent1[off1[v]:off1[v + 1]].tolist() for v in range(V)]
    offsets = torch.tensor([0] + [len(r) for r in rows]).cumsum(0).int()
    return offsets, torch.tensor([e for r in rows for e in r], dtype=torch.int32)


def _backward_not_transposed(edges, V, directed, backward):
    return p3d.graph_topology(edges, V, directed).table(False)


@pytest.mark.parametrize("wrong, cases", [
    (_undirected_as_directed, ["gs_lattice_und_V65_D8", "gs_random_und_V65_D8"]),
    (_deduplicated, ["gs_lattice_und_V65_D8", "gs_lattice_dir_V257_D5", "gs_random_dir_V257_D5"]),
    (_loop_once, ["gs_lattice_und_V65_D8", "gs_random_und_V257_D5"]),
    (_backward_not_transposed, ["gs_lattice_dir_V65_D8", "gs_random_dir_V65_D8"]),
])
def test_the_gates_refuse_wrong_neighbour_sums(wrong, cases):
    for name in cases:
        assert C.gate(name, C.run_gs(name, _sum_with(_right))) == []
        assert C.gate(name, C.run_gs(name, _sum_with(wrong))) != [], (wrong.__name__, name)


def test_the_gates_refuse_a_layer_that_forgets_a_branch():
    def no_w0(verts, edges, w0, b0, w1, b1, directed):
        return p3d.gather_scatter(torch.nn.functional.linear(verts, w1, b1), edges, directed)

    def bias_after_the_sum(verts, edges, w0, b0, w1, b1, directed):
        return torch.nn.functional.linear(verts, w0, b0) + p3d.gather_scatter(torch.nn.functional.linear(verts, w1), edges, directed) + b1

    for name in ("gc_lattice_und_V65_5to8", "gc_random_dir_V257_8to4"):
        assert C.gate(name, C.run_gc(name, no_w0)) != [] and C.gate(name, C.run_gc(name, bias_after_the_sum)) != []


# ---- vert_align -----------------------------------------------------------------------------------------------------------------------
VA = importlib.import_module("pytorch3d_amd.vert_align")  # (the package re-exports the FUNCTION vert_align over the sub-module)


def _contract(name, **wrong):
    feats, verts, grad_out, modes = C.va_inputs(name)
    return C.contract_vert_align(feats, verts, grad_out, *modes, **wrong)


@pytest.mark.parametrize("name", C.va_cases())
def test_vert_align_chain_and_contract_through_the_gates(name):
    lines = []
    assert VA.CALLS["fused"] == 0
    bad = C.gate(name, C.run_va(name, p3d.vert_align), show=lines.append)       # CPU tensors: the reference's chain restated
    bad += C.gate(name, _contract(name), show=lines.append)                      # the float32 contract the kernels implement
    print("\n".join(lines))
    assert bad == []


def test_the_gates_refuse_wrong_samplers():
    for interp, pad, ac in C.VA_MODES:
        for kind in ("lattice", "random"):
            name = "va_%s_%s_%s_%s" % (kind, interp, pad, "ac" if ac else "nc")
            assert C.gate(name, _contract(name, swap_align=True)) != [], name
            if interp == "nearest":
                assert C.gate(name, _contract(name, half_up=True)) != [] or kind == "random", name  # (random: no coordinate on a half)
            if interp == "bilinear" and pad == "border":
                assert C.gate(name, _contract(name, border_grad=False)) != [], name
    assert C.gate("va_lattice_nearest_zeros_ac", _contract("va_lattice_nearest_zeros_ac", half_up=True)) != []
    assert C.gate("va_lattice_nearest_border_nc", _contract("va_lattice_nearest_border_nc", half_up=True)) != []


def test_nearest_rounds_half_to_even():
    feat = torch.arange(5.0).reshape(1, 1, 1, 5)  # align_corners: source x = (c + 1) * 2
    verts = torch.tensor([[[-0.75, 0, 0], [-0.25, 0, 0], [0.25, 0, 0], [0.75, 0, 0]]])  # sources 0.5, 1.5, 2.5, 3.5
    want = [0.0, 2.0, 2.0, 4.0]
    assert p3d.vert_align(feat, verts, interp_mode="nearest").flatten().tolist() == want
    got = C.contract_vert_align([feat], verts, torch.ones(1, 4, 1), "nearest", "zeros", True)
    assert got["out"].flatten().tolist() == want and got["gverts"].abs().sum() == 0


def test_contract_on_non_finite_coordinates():
    feat = torch.arange(45.0).reshape(1, 1, 5, 9) + 1
    nan, inf = float("nan"), float("inf")
    verts = torch.tensor([[[nan, 0, 0], [inf, 0, 0], [-inf, 0, 0], [1e30, 0, 0], [0, nan, 0], [0.25, 0.5, 0]]])
    go = torch.ones(1, 6, 1)
    for interp in ("bilinear", "nearest"):
        z = C.contract_vert_align([feat], verts, go, interp, "zeros", True)
        assert z["out"].flatten()[:5].tolist() == [0.0] * 5 and z["out"].flatten()[5] == 33.0   # zero rows; the neighbour untouched
        assert z["gverts"][0, :5].abs().sum() == 0 and z["gf0"].sum() == 1.0
        b = C.contract_vert_align([feat], verts, go, interp, "border", True)
        ref = p3d.vert_align(feat, verts, interp_mode=interp, padding_mode="border")           # NaN -> 0: the reference's CPU answer
        assert torch.equal(b["out"], ref) and b["out"].flatten().tolist() == [19.0, 27.0, 19.0, 27.0, 5.0, 33.0]


class _FakeMeshes:
    def __init__(self, padded, sizes):
        self.padded, self.sizes = padded, sizes

    def verts_padded(self):
        return self.padded

    def verts_padded_to_packed_idx(self):
        V = self.padded.shape[1]
        return torch.cat([torch.arange(s) + i * V for i, s in enumerate(self.sizes)]).to(self.padded.device)


class _FakeClouds:
    def __init__(self, padded):
        self.padded = padded

    def points_padded(self):
        return self.padded


def test_vert_align_arguments_and_objects_on_the_cpu():
    gen = torch.Generator().manual_seed(1)
    feat, verts = torch.randn(2, 3, 5, 9, generator=gen), torch.rand(2, 7, 3, generator=gen) * 2 - 1
    want = p3d.vert_align(feat, verts)
    assert want.shape == (2, 7, 3)
    meshes = _FakeMeshes(verts, [7, 4])
    packed = p3d.vert_align(feat, meshes, return_packed=True)
    assert packed.shape == (11, 3) and torch.equal(packed, torch.cat([want[0], want[1, :4]]))
    assert torch.equal(p3d.vert_align(feat, _FakeClouds(verts), return_packed=True), want.reshape(14, 3))
    assert torch.equal(p3d.vert_align([feat, feat[:, :1]], verts), torch.cat([want, want[..., :1]], 2))
    assert p3d.vert_align(feat, verts, padding_mode="reflection").shape == (2, 7, 3)
    for args, msg in (((feat, verts[0]), "verts tensor should be 3 dimensional"), ((feat[0], verts), r"feats must have shape \(N, C, H, W\)"),
                      ((feat[:1], verts), "inconsistent batch dimension"), ((feat, object()), "verts must be a tensor or have a")):
        with pytest.raises(ValueError, match=msg):
            p3d.vert_align(*args)
    assert not VA.kernel_path(feat, verts) and not VA.kernel_path(feat, object())


def test_vert_align_header_and_sources():
    header = open(os.path.join(ROOT, "include", "p3d_amd.h")).read()
    for name in ("p3d_vert_align_forward", "p3d_vert_align_backward", "p3d_vert_align_keys", "p3d_vert_align_ordered_backward",
                 "p3d_vert_align_workspace_bytes"):
        assert re.search(r"\b%s\(" % name, header) and name in _lib._SIGNATURES
    for macro, value in (("NEAREST", _lib.VERT_ALIGN_NEAREST), ("BORDER", _lib.VERT_ALIGN_BORDER), ("CORNERS", _lib.VERT_ALIGN_CORNERS)):
        assert int(re.search(r"#define P3D_VERT_ALIGN_%s (\d+)u" % macro, header).group(1)) == value
    assert "vert_align.hip" in build.SOURCES and "graph_conv.hip" in build.SOURCES
    lib = _lib.load()
    assert lib.p3d_vert_align_workspace_bytes(0, 4) == 0 and lib.p3d_vert_align_workspace_bytes(100, 5) > 0
    # N * H * W >= 2^31 cannot be keyed by an int32: refused before anything is read
    assert lib.p3d_vert_align_keys(2, 2 ** 15, 2 ** 15, None, 0, 0, 0, 0, None, 0, 0, None, None) == -6
    assert lib.p3d_vert_align_keys(1, 4, 4, None, 0, 0, 0, 0, None, 0, 8, None, None) == -1       # an unknown flag
    assert lib.p3d_vert_align_forward(None, 1, 0, 4, 4, 0, 0, 0, 0, None, 0, 0, 0, 0, None, 0, 0, None, 0, None) == 0  # nothing to do
