"""GraphConv and gather_scatter: per-vertex sums of neighbour rows on csrc/graph_conv.hip, forward and backward.

    graph_topology(edges, num_verts, directed=False, check=True) -> GraphTopology      the inverted index, built once per edge list
    topology_of_edges(edges, num_verts, directed=False)          -> GraphTopology      the same through a small cache
    gather_scatter(input, edges_or_topology, directed=False)     -> (V, D)             pytorch3d/ops/graph_conv.py: gather_scatter
    graph_conv(verts, edges_or_topology, w0, b0, w1, b1, directed=False) -> (V, Dout)  GraphConv.forward: w0 x + sum_nbrs w1 x
    gather_scatter_op(input, edges, directed, backward)          -> (V, D)             pytorch3d._C.gather_scatter of the shim

The reference's device kernel adds with one float atomic per (edge, channel) into a zero-filled output, so its bits depend on the
order the hardware serves the atomics.  Here every vertex owns the LIST of the rows it sums (a CSR table: offsets (V + 1), entries),
and one lane adds them in list order:

    out[v] = (base[v] or +0.0) + (((+0.0 + x[e_0]) + x[e_1]) + ...)

List order.  Entries of a row are ordered by edge index (a stable sort); in an undirected edge (a, b) the contribution to a
precedes the one to b.  Multiplicity follows scatter_add: duplicate edges count with their multiplicity, an undirected self loop
(v, v) contributes x[v] twice, a directed one once.  Directed: `fwd` holds for vertex v the e[1] of every edge with e[0] == v (the
reference's direction), `bwd` the transpose.  Undirected: one table holds both directions of every edge and is its own transpose,
order included, so it serves forward and backward.

float32 GPU tensors take the kernel (no atomics, no zero fill, no workspace; the same bits on every run, stream and launch shape).
CPU tensors, float64 and anything else take `neighbor_sum_torch`: the rows padded to the largest degree and added column by column,
the same list order, so kernel and formulation are equal bit for bit on any input.
"""
import weakref

import torch
import torch.nn.functional as F

from . import _C


class GraphTopology:
    """int32 CSR tables on the edges' device.  fwd_offsets (V + 1,), fwd_entries; bwd_offsets, bwd_entries (the same tensors when
    undirected).  V, E, directed."""

    def __init__(self, V, E, directed, fwd, bwd):
        self.V, self.E, self.directed = V, E, directed
        self.fwd_offsets, self.fwd_entries = fwd
        self.bwd_offsets, self.bwd_entries = bwd

    @property
    def device(self):
        return self.fwd_offsets.device

    def table(self, backward=False):
        return (self.bwd_offsets, self.bwd_entries) if backward else (self.fwd_offsets, self.fwd_entries)

    def to(self, device):
        device = torch.device(device)
        if device == self.device:
            return self
        fwd = (self.fwd_offsets.to(device), self.fwd_entries.to(device))
        bwd = fwd if self.bwd_offsets is self.fwd_offsets else (self.bwd_offsets.to(device), self.bwd_entries.to(device))
        return GraphTopology(self.V, self.E, self.directed, fwd, bwd)


def _csr(dest, src, V):
    """Rows of `src` grouped by `dest`, each row in the order of the arguments (stable sort)."""
    order = torch.sort(dest, stable=True).indices
    offsets = torch.searchsorted(dest[order].contiguous(), torch.arange(V + 1, device=dest.device, dtype=dest.dtype))
    return offsets.to(torch.int32).contiguous(), src[order].to(torch.int32).contiguous()


def graph_topology(edges, num_verts, directed=False, check=True):
    """edges (E, 2) int32 / int64 vertex ids, num_verts = V.  Plain torch on the device of the edges.  check=True costs one host sync
    and raises when an index is outside [0, V) (where the reference's GPU kernel would read out of bounds); check=False skips it --
    such edges then contribute nothing."""
    if not torch.is_tensor(edges) or edges.dim() != 2 or edges.shape[1] != 2:
        raise ValueError("edges must be of shape (num_edges, 2).")
    if edges.dtype not in (torch.int32, torch.int64):
        raise ValueError("edges has to be of type torch.int64 or torch.int32.")
    V, E = int(num_verts), int(edges.shape[0])
    if V < 0:
        raise ValueError("num_verts must not be negative")
    if 2 * E >= 2 ** 31 or V >= 2 ** 31 - 1:
        raise ValueError("graph_topology: 2 E and V must fit an int32")
    edges = edges.detach().to(torch.int64)
    if check and E > 0:
        lo, hi = torch.stack([edges.min(), edges.max()]).tolist()  # the one host sync
        if lo < 0 or hi >= V:
            raise ValueError("edges hold vertex indices outside [0, %d): min %d, max %d" % (V, lo, hi))
    if directed:
        fwd = _csr(edges[:, 0], edges[:, 1], V)
        bwd = _csr(edges[:, 1], edges[:, 0], V)
    else:
        # sample 2 e: to a from b; sample 2 e + 1: to b from a
        fwd = bwd = _csr(edges.reshape(-1), edges.flip(1).reshape(-1), V)
    return GraphTopology(V, E, bool(directed), fwd, bwd)


_CACHE_SIZE = 8
_cache = []  # [weakref of the edges tensor, _version, V, directed, topology], most recent last
CACHE_STATS = {"hits": 0, "misses": 0}


def topology_of_edges(edges, num_verts, directed=False):
    """graph_topology(edges, num_verts, directed) through a cache of the last few edge tensors.  An entry is recalled for the same
    tensor OBJECT (held through a weak reference, so never for a new tensor at a recycled address) with the same _version (an in-place
    write misses), V and directed.  Meshes.edges_packed() hands back the same tensor on every call: a fitting loop builds once."""
    V, directed = int(num_verts), bool(directed)
    _cache[:] = [c for c in _cache if c[0]() is not None]
    for i, c in enumerate(_cache):
        if c[0]() is edges and c[1] == edges._version and c[2] == V and c[3] == directed:
            CACHE_STATS["hits"] += 1
            _cache.append(_cache.pop(i))
            return c[4]
    CACHE_STATS["misses"] += 1
    topo = graph_topology(edges, V, directed)
    _cache[:] = [c for c in _cache if c[0]() is not edges or c[2] != V or c[3] != directed]  # a stale _version of this tensor
    _cache.append([weakref.ref(edges), edges._version, V, directed, topo])
    del _cache[:-_CACHE_SIZE]
    return topo


def clear_topology_cache():
    del _cache[:]


def neighbor_sum_torch(rows, offsets, entries, base=None):
    """The contract of p3d_neighbor_sum (include/p3d_amd.h) in torch, any float dtype and device: the rows padded to the largest
    degree and added column by column, which is the list order.  Offsets are clamped to [0, n_entries], entries outside [0, n_rows)
    skipped.  One host sync (the largest degree)."""
    n_rows, D = rows.shape
    V, n = offsets.numel() - 1, entries.numel()
    acc = rows.new_zeros((V, D))
    if V > 0 and D > 0 and n > 0 and n_rows > 0:
        begin = offsets[:-1].to(torch.int64).clamp(min=0)
        end = offsets[1:].to(torch.int64).clamp(max=n)
        ent = entries.to(torch.int64)
        for j in range(int((end - begin).max().clamp(min=0))):
            live = torch.nonzero(begin + j < end).squeeze(1)  # vertices whose list has a j-th entry
            e = ent[(begin + j)[live]]
            ok = (e >= 0) & (e < n_rows)
            live, e = live[ok], e[ok]
            acc[live] = acc[live] + rows[e]
    return acc if base is None else base + acc


def kernel_path(input, topology=None):
    """Whether a neighbour sum of `input` runs csrc/graph_conv.hip's kernel (else: the torch formulation of the same list order)."""
    return torch.is_tensor(input) and input.is_cuda and input.dtype == torch.float32 and input.dim() == 2 and \
        (topology is None or topology.device == input.device)


def _sum(rows, topology, backward, base=None):
    offsets, entries = topology.table(backward)
    if kernel_path(rows, topology) and (base is None or kernel_path(base, topology)):
        return _C.neighbor_sum(rows, offsets, entries, base)
    if offsets.device != rows.device:
        offsets, entries = topology.to(rows.device).table(backward)
    return neighbor_sum_torch(rows, offsets, entries, base)


class _NeighborSum(torch.autograd.Function):
    """out = (base or 0) + neighbour sums of input; backward: grad through to base, the transposed table's sums to input."""

    @staticmethod
    def forward(ctx, input, base, topology):
        ctx.topology = topology
        return _sum(input.detach(), topology, False, None if base is None else base.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        grad_input = _sum(grad, ctx.topology, True) if ctx.needs_input_grad[0] else None
        return grad_input, (grad if ctx.needs_input_grad[1] else None), None


def _topology(edges_or_topology, num_verts, directed):
    if isinstance(edges_or_topology, GraphTopology):
        t = edges_or_topology
        if t.V != num_verts:
            raise ValueError("the topology was built for %d vertices, the input has %d" % (t.V, num_verts))
        return t
    return topology_of_edges(edges_or_topology, num_verts, directed)


def _check_input(input):
    if not (input.dim() == 2):
        raise ValueError("input can only have 2 dimensions.")


def _check_edges(edges):
    if not (edges.dim() == 2):
        raise ValueError("edges can only have 2 dimensions.")
    if not (edges.shape[1] == 2):
        raise ValueError("edges must be of shape (num_edges, 2).")


def gather_scatter(input, edges_or_topology, directed: bool = False):
    """pytorch3d.ops.graph_conv.gather_scatter: out[v] = the sum of input over v's neighbours (directed: over e[1] of the edges
    with e[0] == v).  One autograd node; its backward is the same kernel on the transposed table.  edges (E, 2) int64 with the
    reference's checks and messages, or a GraphTopology (then `directed` is the topology's)."""
    _check_input(input)
    if not isinstance(edges_or_topology, GraphTopology):
        _check_edges(edges_or_topology)
    if not (input.dtype == torch.float32):
        raise ValueError("input has to be of type torch.float32.")
    if not isinstance(edges_or_topology, GraphTopology) and not (edges_or_topology.dtype == torch.int64):
        raise ValueError("edges has to be of type torch.int64.")
    return _NeighborSum.apply(input, None, _topology(edges_or_topology, input.shape[0], directed))


def graph_conv(verts, edges_or_topology, w0, b0, w1, b1, directed: bool = False):
    """GraphConv.forward (pytorch3d/ops/graph_conv.py:52-85): w0 x + b0 + sum over neighbours of (w1 x + b1).  The two F.linear calls
    are the reference's (the GEMMs' bits stay equal); ONE node then writes w0x + the neighbour sums of w1x -- no zero fill, no
    separate add -- and its backward passes grad through to the w0 branch and runs one neighbour-sum launch for the w1 branch."""
    edges = edges_or_topology
    if not isinstance(edges, GraphTopology) and verts.is_cuda != edges.is_cuda:
        raise ValueError("verts and edges tensors must be on the same device.")
    if verts.shape[0] == 0:
        # empty graph.
        return verts.new_zeros((0, w0.shape[0])) * verts.sum()
    _check_input(verts)
    if not isinstance(edges, GraphTopology):
        _check_edges(edges)
    verts_w0 = F.linear(verts, w0, b0)  # (V, output_dim)
    verts_w1 = F.linear(verts, w1, b1)  # (V, output_dim)
    return _NeighborSum.apply(verts_w1, verts_w0, _topology(edges, verts.shape[0], directed))


def gather_scatter_op(input, edges, directed, backward):
    """`pytorch3d._C.gather_scatter` (gather_scatter/gather_scatter.h: GatherScatter(input, edges, directed, backward)) of the shim
    module: the table comes from the cache, or is built; backward=True sums over the transposed table."""
    if not (torch.is_tensor(input) and torch.is_tensor(edges)):
        raise TypeError("gather_scatter: input and edges must be tensors")
    if input.dim() != 2:
        raise ValueError("gather_scatter: input must have shape (V, D), got %s" % (tuple(input.shape),))
    if input.device != edges.device:
        raise ValueError("gather_scatter: input is on %s and edges on %s" % (input.device, edges.device))
    with torch.no_grad():
        return _sum(input, topology_of_edges(edges, input.shape[0], bool(directed)), bool(backward))
