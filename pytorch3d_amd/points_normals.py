"""Normals, curvatures and local coordinate frames of padded point clouds on the HIP kernel of csrc/point_frames.hip.

    estimate_pointcloud_normals(pointclouds, neighborhood_size=50, disambiguate_directions=True, *, use_symeig_workaround=True)
    estimate_pointcloud_local_coord_frames(pointclouds, neighborhood_size=50, disambiguate_directions=True, *,
                                           use_symeig_workaround=True)                          pytorch3d/ops/points_normals.py
    point_covariances(points, lengths, K, return_idx=False)                      pytorch3d/ops/utils.py get_point_covariances, fused

Same names, argument order, defaults, ValueErrors and return shapes as the reference: normals (N, P, 3); curvatures (N, P, 3)
ascending and frames (N, P, 3, 3) with the principal directions in the COLUMNS, column 0 the normal.  `pointclouds` is a tensor
(N, P, 3) or an object with points_padded() and num_points_per_cloud().  Per point: the K = neighborhood_size points of its cloud
with the smallest (dist, j) -- itself included, ties to the lower index, the order of pytorch3d_amd.knn -- on the cloud recentred
as the reference does, `points - points.sum(1) / num_points` (the sum in float64: recentre below); the mean of the neighbours and then the mean of their centred
outer products, float32, summed ascending by (dist, j); the reference's symeig3x3 (its regularised closed form, NOT a true
eigen-decomposition where the off-diagonal energy of a covariance is about 1e-6 or below: DESIGN.md 8.17); and the reference's sign
votes for column 0 and column 2, column 1 = column 0 x column 2.  Rows past a cloud's length are zeros (the reference leaves a
function of index 0 there).

The `num_points <= neighborhood_size` check reads the lengths on the host, as the reference's does; `check_lengths=False` skips
it (and the wait) for a caller who knows the clouds are large enough.

float32 GPU clouds with K <= 64, use_symeig_workaround=True and no gradient asked for take the kernel: nothing of size K per point
is materialised.  Everything else -- CPU tensors, float64, K > 64, use_symeig_workaround=False (torch.linalg.eigh), inputs that
require grad -- takes the torch formulation below: the same contract in the same operation order on pytorch3d_amd.knn's
torch_knn_forward, differentiable by plain autograd as the reference is.  There is no backward kernel: normals are estimated on
fixed targets, and the reference's gradient is only that of its regularised formula.
"""
import math

import torch

from . import _C, _lib
from .knn import knn_gather, torch_knn_forward

EPS = float(torch.finfo(torch.float32).eps)  # symeig3x3's eps, whatever the dtype


def kernel_path(points, K, use_symeig_workaround=True):
    """Whether the estimate for `points` (N, P, 3) with K neighbours runs csrc/point_frames.hip (else: the torch formulation)."""
    return (torch.is_tensor(points) and points.is_cuda and points.dtype == torch.float32 and points.dim() == 3 and points.shape[2] == 3
            and 1 <= int(K) <= _lib.FRAMES_MAX_K and bool(use_symeig_workaround) and not points.requires_grad)


def _clouds(pointclouds):
    """(points_padded, num_points): convert_pointclouds_to_tensor of the reference's ops/utils.py."""
    if hasattr(pointclouds, "points_padded") and hasattr(pointclouds, "num_points_per_cloud"):
        return pointclouds.points_padded(), pointclouds.num_points_per_cloud()
    if torch.is_tensor(pointclouds):
        return pointclouds, pointclouds.shape[1] * torch.ones(pointclouds.shape[0], device=pointclouds.device, dtype=torch.int64)
    raise ValueError("The inputs X, Y should be either Pointclouds objects or tensors.")


def recentre(points_padded, num_points):
    """The reference's `undo global mean for stability`: points - points.sum(1) / num_points, with the sum taken in float64 and the
    mean rounded ONCE to the points' dtype.  The subtraction rounds the small coordinates of a cloud (up to eps / 2 of the mean's
    size each), so the mean's last bits decide every distance and covariance after it; a float32 sum has other last bits on every
    device and reduction order, the correctly rounded mean is the same number everywhere."""
    pcl_mean = (points_padded.double().sum(1) / num_points[:, None]).to(points_padded.dtype)
    return points_padded - pcl_mean[:, None, :]


def _live(num_points, P):
    return torch.arange(P, device=num_points.device)[None, :] < num_points[:, None]


# ---- the torch formulation -------------------------------------------------------------------------------------------------------
def _neighbours(points, lengths, K):
    """(idx (N, P, K), neighbours (N, P, K, 3)): the (dist, j) order of pytorch3d_amd.knn; the gather carries the gradient."""
    with torch.no_grad():
        idx, _ = torch_knn_forward(points, points, lengths, lengths, 2, K)
    return idx, knn_gather(points, idx, lengths)


def _covariances(nbrs):
    """(N, P, K, 3) -> (N, P, 3, 3): the mean first, then the mean of the centred outer products, each summed ascending in k."""
    K = nbrs.shape[2]
    total = nbrs[:, :, 0]
    for k in range(1, K):
        total = total + nbrs[:, :, k]
    diff = nbrs - (total / K)[:, :, None]
    outer = diff.unsqueeze(4) * diff.unsqueeze(3)
    cov = outer[:, :, 0]
    for k in range(1, K):
        cov = cov + outer[:, :, k]
    return cov / K


def _sign_nz(x):
    return 2.0 * (x > 0.0).to(x.dtype) - 1.0


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _pick(cond, a, b):
    return tuple(torch.where(cond, x, y) for x, y in zip(a, b))


def _sumsq(t):
    s = t[0] * t[0]
    for x in t[1:]:
        s = s + x * x
    return s


def _unit(t):
    """torch.nn.functional.normalize on components."""
    n = torch.sqrt(_sumsq(t)).clamp_min(1e-12)
    return tuple(x / n for x in t)


def _eigenvector_set(a, alpha0, alpha1):
    """_construct_eigenvecs of symeig3x3.py on the components a[r][c]: (ev0, ev1, ev2), each a 3-tuple of tensors."""
    c = [[a[r][k] - alpha0 if r == k else a[r][k] for k in range(3)] for r in range(3)]
    r01, r12, r02 = _cross(c[0], c[1]), _cross(c[1], c[2]), _cross(c[0], c[2])
    reg = tuple(EPS * _sign_nz(x) for x in r01)
    r01, r12, r02 = (tuple(x + g for x, g in zip(r, reg)) for r in (r01, r12, r02))
    n01, n12, n02 = _sumsq(r01), _sumsq(r12), _sumsq(r02)
    best, nb = r01, n01
    take = (n12 > nb).detach()
    best, nb = _pick(take, r12, best), torch.where(take, n12, nb)
    take = (n02 > nb).detach()
    best, nb = _pick(take, r02, best), torch.where(take, n02, nb)
    root = torch.sqrt(nb)
    w = tuple(x / root for x in best)
    # _get_uv
    ax, ay, az = (x.abs() for x in w)
    axis1 = (ay < ax).detach()
    am = torch.where(axis1, ay, ax)
    axis2 = (az < am).detach()
    zero = torch.zeros_like(w[0])
    t = _pick(axis2, (-w[1], w[0], zero), _pick(axis1, (-w[2], zero, w[0]), (zero, -w[2], w[1])))
    u = _unit(t)
    v = _cross(w, u)
    # _get_ev1
    c = [[a[r][k] - alpha1 if r == k else a[r][k] for k in range(3)] for r in range(3)]
    cols = [tuple(c[r][k] for r in range(3)) for k in range(3)]
    tu, tv = tuple(_dot(u, col) for col in cols), tuple(_dot(v, col) for col in cols)
    m00, m01, m10, m11 = _dot(tu, u), _dot(tu, v), _dot(tv, u), _dot(tv, v)
    acute = _sign_nz(m00 * m10 + m01 * m11).detach()
    rs0, rs1 = m00 + acute * m10, m01 + acute * m11
    reg = EPS * _sign_nz(rs0)
    rs0, rs1 = rs0 + reg, rs1 + reg
    t0, t1 = _unit((rs1, -rs0))
    ev1 = tuple(uu * t0 + vv * t1 for uu, vv in zip(u, v))
    return w, ev1, _cross(w, ev1)


def symeig3x3(cov):
    """The reference's symeig3x3(cov, eigenvectors=True) on (..., 3, 3), component by component in the kernel's operation order:
    (eigenvalues (..., 3) ascending, eigenvectors (..., 3, 3) in the columns)."""
    a = [[cov[..., r, c] for c in range(3)] for r in range(3)]
    q = ((a[0][0] + a[1][1]) + a[2][2]) / 3.0
    # the reference's (sum of all squares - sum of the diagonal's) / 2 without its cancellation: the same number, and that
    # difference was the largest single source of float32 error in the curvatures
    p1 = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2]
    d = [a[k][k] - q for k in range(3)]
    p2 = (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + 2.0 * p1.clamp(EPS)
    p = torch.sqrt(p2 / 6.0)
    b = [[(d[r] if r == c else a[r][c]) / p for c in range(3)] for r in range(3)]
    det = (b[0][0] * (b[1][1] * b[2][2] - b[1][2] * b[2][1]) - b[0][1] * (b[1][0] * b[2][2] - b[1][2] * b[2][0])
           + b[0][2] * (b[1][0] * b[2][1] - b[1][1] * b[2][0]))
    r_ = (det / 2.0).clamp(-1.0 + EPS, 1.0 - EPS)
    phi = torch.acos(r_) / 3.0
    eig1 = q + 2 * p * torch.cos(phi)
    eig2 = q + 2 * p * torch.cos(phi + 2 * math.pi / 3)
    eig3 = 3 * q - eig1 - eig2
    blend = torch.exp(-torch.square(p1 / (6 * EPS))).detach()
    s, _ = torch.sort(torch.stack((a[0][0], a[1][1], a[2][2]), dim=-1), dim=-1)
    vals = [blend * s[..., k] + (1.0 - blend) * e for k, e in enumerate((eig2, eig3, eig1))]
    low = (vals[1] - vals[0] > vals[2] - vals[1]).detach()
    lo, hi = _eigenvector_set(a, vals[0], vals[1]), _eigenvector_set(a, vals[2], vals[1])
    cols = (_pick(low, lo[0], hi[2]), _pick(low, lo[1], hi[1]), _pick(low, lo[2], hi[0]))
    vecs = torch.stack([torch.stack([cols[c][r] for c in range(3)], dim=-1) for r in range(3)], dim=-2)
    return torch.stack(vals, dim=-1), vecs


def _disambiguate(points, nbrs, vecs):
    """_disambiguate_vector_directions: vecs (N, P, 3) turned round where fewer than half of the neighbours lie in front."""
    K = nbrs.shape[2]
    df = nbrs - points[:, :, None]
    proj = vecs[:, :, None, 0] * df[..., 0] + vecs[:, :, None, 1] * df[..., 1] + vecs[:, :, None, 2] * df[..., 2]
    n_pos = (proj > 0).to(points.dtype).sum(2, keepdim=True)
    flip = (n_pos < (0.5 * K)).to(points.dtype)
    return (1.0 - 2.0 * flip) * vecs


def torch_point_frames(points, lengths, K, disambiguate_directions=True, use_symeig_workaround=True):
    """(curvatures, frames, cov, idx) of the module docstring's contract on the points as given, any device and float dtype."""
    N, P, _ = points.shape
    idx, nbrs = _neighbours(points, lengths, K)
    cov = _covariances(nbrs)
    curv, frames = symeig3x3(cov) if use_symeig_workaround else torch.linalg.eigh(cov)
    if disambiguate_directions:
        n = _disambiguate(points, nbrs, frames[:, :, :, 0])
        z = _disambiguate(points, nbrs, frames[:, :, :, 2])
        frames = torch.stack((n, torch.cross(n, z, dim=2), z), dim=3)
    if lengths is not None:
        dead = ~_live(lengths.to(points.device), P)
        curv, frames = curv.masked_fill(dead[..., None], 0.0), frames.masked_fill(dead[..., None, None], 0.0)
        cov = cov.masked_fill(dead[..., None, None], 0.0)
    return curv, frames, cov, idx


# ---- the public functions ----------------------------------------------------------------------------------------------------------
def point_covariances(points, lengths, K, return_idx=False):
    """get_point_covariances without its (N, P, K, 3) neighbours: the covariances (N, P, 3, 3) of the K nearest neighbours of every
    point of `points` (N, P, 3) AS GIVEN (no recentring), rows past lengths (N,) -- None: full clouds -- zero; with return_idx also
    the neighbours' indices (N, P, K) int64."""
    K = int(K)
    if K < 1:
        raise ValueError("K must be at least 1.")
    if points.dim() != 3 or points.shape[2] != 3:
        raise ValueError("points has to be of shape (minibatch, N, 3)")
    if lengths is not None:
        lengths = lengths.to(device=points.device, dtype=torch.int64)
    if kernel_path(points, K):
        _, _, cov, idx = _C.point_frames(points, lengths, K, False, frames=False, cov=True, idx=return_idx)
    else:
        points = points.contiguous()
        idx, nbrs = _neighbours(points, lengths, K)
        cov = _covariances(nbrs)
        if lengths is not None:
            cov = cov.masked_fill(~_live(lengths, points.shape[1])[..., None, None], 0.0)
    return (cov, idx) if return_idx else cov


def estimate_pointcloud_local_coord_frames(pointclouds, neighborhood_size: int = 50, disambiguate_directions: bool = True, *,
                                           use_symeig_workaround: bool = True, check_lengths: bool = True):
    """See the module docstring: (curvatures (N, P, 3), local_coord_frames (N, P, 3, 3))."""
    points_padded, num_points = _clouds(pointclouds)
    ba, N, dim = points_padded.shape
    if dim != 3:
        raise ValueError("The pointclouds argument has to be of shape (minibatch, N, 3)")
    if check_lengths and (num_points <= neighborhood_size).any():
        raise ValueError("The neighborhood_size argument has to be" + " >= size of each of the point clouds.")
    K = int(neighborhood_size)
    num_points = num_points.to(points_padded.device)
    points_centered = recentre(points_padded, num_points)
    lengths = None if torch.is_tensor(pointclouds) else num_points.to(torch.int64)
    if kernel_path(points_centered, K, use_symeig_workaround):
        curvatures, frames, _, _ = _C.point_frames(points_centered, lengths, K, bool(disambiguate_directions))
    else:
        curvatures, frames, _, _ = torch_point_frames(points_centered.contiguous(), lengths, K, bool(disambiguate_directions),
                                                      bool(use_symeig_workaround))
    return curvatures, frames


def estimate_pointcloud_normals(pointclouds, neighborhood_size: int = 50, disambiguate_directions: bool = True, *,
                                use_symeig_workaround: bool = True, check_lengths: bool = True):
    """See the module docstring: normals (N, P, 3), the first vector of each local coordinate frame."""
    _, frames = estimate_pointcloud_local_coord_frames(pointclouds, neighborhood_size=neighborhood_size,
                                                       disambiguate_directions=disambiguate_directions,
                                                       use_symeig_workaround=use_symeig_workaround, check_lengths=check_lengths)
    return frames[:, :, :, 0]
