"""HardDepthShader / SoftDepthShader restated in closed form, forward and backward, without autograd (the yardstick of
tests/test_gpu_depth_blend.py; tests/test_cpu_depth_blend.py ties it to the reference's recorded behaviour).

Per pixel, slots k = 0..K-1 in their stored order, z_K := zfar:

    p_k = pix_to_face_k >= 0 ? 1 / (1 + exp(d_k / sigma)) : 0        c_k = p_0 + .. + p_k        C_k = min(c_k, 1), C_{-1} = 0
    w_k = C_k - C_{k-1}                                              depth = sum_k w_k z_k + (1 - C_{K-1}) zfar
    grad_z_k = g w_k
    grad_d_j = m_j g (-p_j (1 - p_j) / sigma) sum_{k >= j} (z_k - z_{k+1}) [c_k <= 1]

`dtype` is the precision everything is evaluated in (float64 for gating).
"""
import torch


def _probabilities(pix_to_face, dists, sigma, dtype):
    m = pix_to_face >= 0
    x = -dists.to(dtype) / sigma
    p = torch.where(m, 1.0 / (1.0 + torch.exp(-x)), torch.zeros((), dtype=dtype, device=dists.device))
    return m, p


def soft_depth_restated(pix_to_face, zbuf, dists, sigma, zfar, dtype=torch.float64):
    """-> depth (N,H,W,1)"""
    _, p = _probabilities(pix_to_face, dists, sigma, dtype)
    C = torch.cumsum(p, dim=-1).clamp(max=1.0)
    w = C - torch.cat([torch.zeros_like(C[..., :1]), C[..., :-1]], dim=-1)
    return ((w * zbuf.to(dtype)).sum(-1) + (1.0 - C[..., -1]) * float(zfar)).unsqueeze(-1)


def soft_depth_restated_backward(pix_to_face, zbuf, dists, sigma, zfar, grad_depth, dtype=torch.float64):
    """-> (grad_zbuf, grad_dists), both (N,H,W,K)"""
    m, p = _probabilities(pix_to_face, dists, sigma, dtype)
    z = zbuf.to(dtype)
    g = grad_depth.to(dtype).reshape(pix_to_face.shape[:3] + (1,))
    c = torch.cumsum(p, dim=-1)
    C = c.clamp(max=1.0)
    w = C - torch.cat([torch.zeros_like(C[..., :1]), C[..., :-1]], dim=-1)
    znext = torch.cat([z[..., 1:], torch.full_like(z[..., :1], float(zfar))], dim=-1)
    t = (z - znext) * (c <= 1.0).to(dtype)
    s = torch.flip(torch.cumsum(torch.flip(t, dims=[-1]), dim=-1), dims=[-1])
    grad_d = g * s * (-p * (1.0 - p) / sigma) * m.to(dtype)
    return g * w, grad_d


def soft_depth_fragile(pix_to_face, dists, sigma, tol=1e-6):
    """(N,H,W) bool: pixels where the [c_k <= 1] decision may legitimately differ between float32 and float64 -- the float64
    running sum is within `tol` of 1 at some slot k while a slot j <= k still has a derivative p_j (1 - p_j) > tol."""
    _, p = _probabilities(pix_to_face, dists, sigma, torch.float64)
    c = torch.cumsum(p, dim=-1)
    live = torch.cummax((p * (1.0 - p) > tol).to(torch.int8), dim=-1).values > 0
    return (((c - 1.0).abs() <= tol) & live).any(-1)


def hard_depth_restated(pix_to_face, zbuf, zfar):
    """-> depth (N,H,W,1): copies, no arithmetic"""
    z0 = zbuf[..., :1]
    return torch.where(pix_to_face[..., :1] >= 0, z0, torch.full_like(z0, float(zfar)))


def hard_depth_restated_backward(pix_to_face, grad_depth):
    """-> grad_zbuf (N,H,W,K)"""
    g = torch.zeros(pix_to_face.shape, dtype=grad_depth.dtype, device=grad_depth.device)
    g[..., :1] = torch.where(pix_to_face[..., :1] >= 0, grad_depth.reshape(pix_to_face.shape[:3] + (1,)), torch.zeros_like(g[..., :1]))
    return g


def output_bound(K, zfar, zbuf):
    """|depth32 - depth64| <= 2 (K + 1) 2^-23 Z, Z = max(zfar, |zbuf|.max()): two ulps of sigmoid error and one rounding of the
    running sum per slot, each times a depth difference of at most Z, plus K + 1 roundings of the weighted sum."""
    Z = max(abs(float(zfar)), float(zbuf.abs().max()) if zbuf.numel() else 0.0)
    return 2.0 * (K + 1) * 2.0 ** -23 * Z


def grad_close(g, r):
    """The project's gate for blend gradients (tests/test_gpu_blending.py)."""
    r = r.to(g.dtype)
    return torch.allclose(g, r, atol=1e-4 * max(1.0, float(r.abs().max()) if r.numel() else 0.0), rtol=1e-3)


def depth_inputs(gen, N, H, W, K, sigma, pattern="prefix", faces=50):
    """Seeded fragments (pix_to_face i64, zbuf f32, dists f32), all (N,H,W,K), on the CPU.
    "prefix": per pixel a uniform number 0..K of valid leading slots, zbuf ascending in 0.8-3.8; dists of 35 % of the slots
    uniform in (-1e-2, 0) (interior: probability exactly 1 in float32 at sigma <= 3e-4), of the others uniform in
    (-3 sigma, 6 sigma); empty slots hold -1 in all three tensors, as the rasterizer leaves them.
    "full": the same with every slot valid.  "holes": randint(-1, faces) per slot and unsorted zbuf."""
    shape = (N, H, W, K)
    z = torch.rand(shape, generator=gen) * 3.0 + 0.8
    interior = torch.rand(shape, generator=gen) < 0.35
    d_in = -torch.rand(shape, generator=gen) * 1e-2
    d_edge = (torch.rand(shape, generator=gen) * 9.0 - 3.0) * sigma
    d = torch.where(interior, d_in, d_edge)
    face = torch.randint(0, faces, shape, generator=gen)
    if pattern == "holes":
        p2f = torch.randint(-1, faces, shape, generator=gen)
    else:
        z = torch.sort(z, dim=-1).values
        n_valid = torch.randint(0, K + 1, (N, H, W, 1), generator=gen) if pattern == "prefix" else torch.full((N, H, W, 1), K)
        p2f = torch.where(torch.arange(K).view(1, 1, 1, K) < n_valid, face, torch.full_like(face, -1))
    empty = p2f < 0
    z = torch.where(empty, torch.full_like(z, -1.0), z)
    d = torch.where(empty, torch.full_like(d, -1.0), d)
    return p2f.contiguous(), z.contiguous(), d.contiguous()


def pixel_classes(pix_to_face, dists, sigma):
    """Fractions of pixels that are (empty, unsaturated: the probabilities sum to less than 1, saturated by slot 0,
    saturated at a later slot), on the float32 running sum."""
    _, p = _probabilities(pix_to_face, dists, sigma, torch.float32)
    c = torch.cumsum(p, dim=-1)
    empty = (pix_to_face < 0).all(-1)
    unsat = ~empty & (c[..., -1] < 1.0)
    first = ~empty & (c[..., 0] >= 1.0)
    later = ~empty & ~unsat & ~first
    n = float(empty.numel())
    return tuple(float(x.sum()) / n for x in (empty, unsat, first, later))
