"""box3d_overlap: the exact intersection volume and IoU of oriented 3D boxes on csrc/box3d.hip.

    box3d_overlap(boxes1, boxes2, eps=1e-4) -> (vol (N, M), iou (N, M))                      pytorch3d/ops/iou_box3d.py

Same name, defaults, checks, messages and return values as the reference.  boxes1 (N, 8, 3), boxes2 (M, 8, 3): the eight corners of
each box in the reference's order,

        (4) +---------+. (5)
            | ` .     |  ` .
            | (0) +---+-----+ (1)
            |     |   |     |
        (7) +-----+---+. (6)|
            ` .   |     ` . |
            (3) ` +---------+ (2)

e.g. the unit cube [0,0,0], [1,0,0], [1,1,0], [0,1,0], [0,0,1], [1,0,1], [1,1,1], [0,1,1].  Every pair is computed by the contract of
the reference's compiled CPU operator (include/p3d_amd.h): triangles clipped by planes, coplanar duplicates removed, the volume
summed about the polyhedron's centre; iou = vol / (vol1 + vol2 - vol).  float32 GPU tensors take the kernels (one wave per pair, no
list cap: a pair that outgrows the on-chip lists is redone in a second launch), float32 CPU tensors the library's host loop on the
same geometry functions.  Other dtypes are refused.

The two input checks (the four corners of every face coplanar within eps, every triangle's area at least eps) are evaluated for both
arguments together and cost ONE host sync (the reference: four).  There is no backward, as in the reference: the autograd node raises
ValueError("box3d_overlap backward is not supported").
"""
import torch

from . import _C

# the reference's Python face lists (pytorch3d/ops/iou_box3d.py: _box_planes, _box_triangles); the fifth quad is ordered differently
# from the compiled operator's and decides which three corners span the plane of the coplanarity check
_CHECK_QUADS = ((0, 1, 2, 3), (3, 2, 6, 7), (0, 1, 5, 4), (0, 3, 7, 4), (1, 2, 6, 5), (4, 5, 6, 7))
_CHECK_TRIS = ((0, 1, 2), (0, 3, 2), (4, 5, 6), (4, 6, 7), (1, 5, 6), (1, 6, 2), (0, 4, 7), (0, 7, 3), (3, 2, 6), (3, 6, 7), (0, 1, 5), (0, 4, 5))


def kernel_path(boxes1, boxes2):
    """Whether box3d_overlap(boxes1, boxes2) runs csrc/box3d.hip's kernels (else: the library's host loop, or an error)."""
    return all(torch.is_tensor(b) and b.is_cuda and b.dtype == torch.float32 and b.dim() == 3 and tuple(b.shape[1:]) == (8, 3)
               for b in (boxes1, boxes2))


def iou_box3d_op(boxes1, boxes2):
    """`pytorch3d._C.iou_box3d` of the shim module: (vol, iou) for float32 boxes (N, 8, 3), (M, 8, 3) on one device."""
    if not (torch.is_tensor(boxes1) and torch.is_tensor(boxes2)):
        raise TypeError("iou_box3d: boxes1 and boxes2 must be tensors")
    for name, b in (("boxes1", boxes1), ("boxes2", boxes2)):
        if b.dim() != 3 or tuple(b.shape[1:]) != (8, 3):
            raise ValueError("iou_box3d: %s must have shape (B, 8, 3), got %s" % (name, tuple(b.shape)))
    if boxes1.device != boxes2.device:
        raise ValueError("iou_box3d: boxes1 is on %s and boxes2 on %s" % (boxes1.device, boxes2.device))
    if boxes1.dtype != boxes2.dtype:
        raise ValueError("iou_box3d: boxes1 is %s and boxes2 %s" % (boxes1.dtype, boxes2.dtype))
    if boxes1.dtype != torch.float32:
        raise ValueError("iou_box3d: the operator takes float32 boxes, got %s" % (boxes1.dtype,))
    with torch.no_grad():
        return _C.iou_box3d(boxes1, boxes2) if boxes1.is_cuda else _C.iou_box3d_host(boxes1, boxes2)


def _failed_checks(boxes, eps):
    """(2,) bool: (a face whose fourth corner leaves the plane of the first three by eps or more, a triangle of area below eps)."""
    quads = torch.tensor(_CHECK_QUADS, dtype=torch.int64, device=boxes.device)
    tris = torch.tensor(_CHECK_TRIS, dtype=torch.int64, device=boxes.device)
    q = boxes[:, quads]  # (B, 6, 4, 3)
    e0 = torch.nn.functional.normalize(q[:, :, 1] - q[:, :, 0], dim=-1)
    e1 = torch.nn.functional.normalize(q[:, :, 2] - q[:, :, 0], dim=-1)
    normal = torch.nn.functional.normalize(torch.cross(e0, e1, dim=-1), dim=-1)
    off_plane = ((q[:, :, 3] - q[:, :, 0]) * normal).sum(-1).abs()
    t = boxes[:, tris]  # (B, 12, 3, 3)
    areas = torch.cross(t[:, :, 1] - t[:, :, 0], t[:, :, 2] - t[:, :, 0], dim=-1).norm(dim=-1) / 2
    return torch.stack([~(off_plane < eps).all(), (areas < eps).any()])


class _Box3dOverlap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, boxes1, boxes2):
        return iou_box3d_op(boxes1, boxes2)

    @staticmethod
    def backward(ctx, grad_vol, grad_iou):
        raise ValueError("box3d_overlap backward is not supported")


def box3d_overlap(boxes1, boxes2, eps: float = 1e-4):
    """See the module docstring."""
    if not all((8, 3) == tuple(box.shape[1:]) for box in (boxes1, boxes2)):
        raise ValueError("Each box in the batch must be of shape (8, 3)")
    with torch.no_grad():
        failed = torch.stack([_failed_checks(boxes1, eps), _failed_checks(boxes2.to(boxes1.device), eps)]).any(0).tolist()  # the one host sync
    if failed[0]:
        raise ValueError("Plane vertices are not coplanar")
    if failed[1]:
        raise ValueError("Planes have zero areas")
    return _Box3dOverlap.apply(boxes1, boxes2)
