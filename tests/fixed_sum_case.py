"""The fixed-tree sum of the loss kernels (csrc/fixed_sum.h), restated in numpy float32 from that header's comment, and the seeded
inputs of the tests that pin it bit for bit (tests/test_gpu_loss_kernel_edges.py, section E).  Nothing here calls the package.

  level 1  a wave owns 64 consecutive terms (a term past the end is +0): six rounds of t[0::2] + t[1::2] -> one partial;
  level 2  a segment (a cloud, a batch element) owns `per_segment` consecutive partials: lane t of 256 adds the partials
           t, t + 256, ... ascending, starting from +0, then eight such rounds over the 256 lanes.
An xor butterfly and the pairwise rounds give the same bits: float32 addition is commutative, so after round r every lane of a
group of 2^r holds the pairwise sum of that group.
"""
import numpy as np
import torch

WAVE = 64
BLOCK = 256


def _rounds(x, n):
    for _ in range(n):
        x = x[..., 0::2] + x[..., 1::2]
    return x


def _padded(x, multiple):
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    out = np.zeros(-(-max(x.size, 1) // multiple) * multiple, dtype=np.float32)
    out[:x.size] = x
    return out


def wave_partials(terms):
    """Level 1: (ceil(n / 64),) float32, one partial per 64 terms."""
    return _rounds(_padded(terms, WAVE).reshape(-1, WAVE), 6).reshape(-1)


def segment_sum(partials):
    """Level 2 over one segment's partials: a float32 scalar."""
    rows = _padded(partials, BLOCK).reshape(-1, BLOCK)
    acc = np.zeros(BLOCK, dtype=np.float32)
    for row in rows:  # lane t: acc += partials[t + 256 k], k ascending
        acc = acc + row
    return _rounds(acc, 8).reshape(())


def tree_sum(terms, per_segment):
    """The sum of a segment's terms when the launch gives every segment `per_segment` partials (those past the terms are +0)."""
    p = wave_partials(terms)
    assert p.size <= max(per_segment, 1)
    out = np.zeros(max(per_segment, 1), dtype=np.float32)
    out[:p.size] = p
    return segment_sum(out)


def chain_sum(terms):
    """The same terms added left to right in float32: what the tree must NOT equal on inputs that tell the two apart."""
    t = np.asarray(terms, dtype=np.float32).reshape(-1)
    return np.add.accumulate(t, dtype=np.float32)[-1] if t.size else np.float32(0.0)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


# ---- inputs: coordinates over three orders of magnitude, so that the order of the additions shows in the last bits ----------------------------
def _spread(n, gen):
    return torch.randn(n, 3, generator=gen) * 10.0 ** (torch.rand(n, 1, generator=gen) * 3.0 - 1.5)


CHAMFER_P2 = 100
CHAMFER_SEED = 1  # chosen on the CPU: with the float32 torch distances the tree and the chain differ wherever TELLS_APART says so
# lengths of the two clouds: 3 partials with idle lanes next to a one-point cloud; 258 / 257 partials, the chain's second step in both
CHAMFER_LENGTHS = {"small": (130, 1), "second_step": (16500, 16385)}
CHAMFER_TELLS_APART = {"small": (True, False), "second_step": (True, True)}  # one term has one order


def chamfer_clouds(name, seed=CHAMFER_SEED):
    """(p1 (2, max length, 3), p2 (2, 100, 3), lengths1) -- every cloud of p2 is full."""
    lengths = CHAMFER_LENGTHS[name]
    gen = torch.Generator().manual_seed(seed)
    p1 = torch.stack([_spread(max(lengths), gen) for _ in lengths])
    p2 = torch.stack([_spread(CHAMFER_P2, gen) for _ in lengths])
    return p1, p2, torch.tensor(lengths, dtype=torch.int64)


EDGES_PER_ELEMENT = 70
POINT_EDGE_SEED = 1
POINT_EDGE_WEIGHTS = (0.75, 1.5)
# points per element: 257 partials per element, all but two of the second element's from padding blocks; an element without a point
POINT_EDGE_COUNTS = {"second_step": (16448, 65), "empty_element": (0, 130)}
POINT_EDGE_TELLS_APART = {"second_step": (True, True), "empty_element": (False, True)}


def point_edge_case(name, seed=POINT_EDGE_SEED):
    """(points (P, 3) packed, first index of each element's points, segments (140, 2, 3) packed, their first indices, weights (2,),
    the largest point count)."""
    counts = POINT_EDGE_COUNTS[name]
    gen = torch.Generator().manual_seed(seed)
    points = torch.cat([_spread(c, gen) for c in counts], 0)
    segms = torch.cat([torch.stack([_spread(EDGES_PER_ELEMENT, gen), _spread(EDGES_PER_ELEMENT, gen)], 1) for _ in counts], 0)
    pfirst = torch.tensor([0, counts[0]], dtype=torch.int64)
    sfirst = torch.tensor([0, EDGES_PER_ELEMENT], dtype=torch.int64)
    return points.contiguous(), pfirst, segms.contiguous(), sfirst, torch.tensor(POINT_EDGE_WEIGHTS), max(counts)
