"""A restatement of SplatterBlender's blend (pytorch3d/renderer/splatter_blend.py, after the camera call) for the tests:
the continuous part (splat weights, sums, normalisation, compositing) in float64, the occlusion classification in the
inputs' float32 (it is a chain of comparisons; float64 differences could order near-ties differently than the reference).
Written per direction with shifted views instead of the reference's (N,H,W,K,9,5) tensors.  Differentiable in colors and
coords (torch autograd)."""
import math

import torch
import torch.nn.functional as F


def _shift(t, dh, dw):
    """out[:, h, w] = t[:, h + dh, w + dw], zero outside the image; t (N, H, W, ...)."""
    N, H, W = t.shape[:3]
    pad = [0, 0] * (t.dim() - 3) + [1, 1, 1, 1]
    p = F.pad(t, pad)
    return p[:, 1 + dh:1 + dh + H, 1 + dw:1 + dw + W]


def splatter_blend_restated(colors, coords, mask, sigma, background, one_convention=False):
    """colors, coords (N,H,W,K,3) float32, mask (N,H,W,K) bool, background (3) -> RGBA (N,H,W,4) float64.
    one_convention=True delivers each splat from the neighbour its occlusion test looked at -- the "clean" pairing the
    reference does NOT use; the tests show that the fixtures tell the two apart."""
    N, H, W, K, _ = colors.shape
    fg = ~mask
    rgb = torch.where(fg[..., None], colors.double(), torch.zeros((), dtype=torch.float64))
    xy = coords[..., :2].double()
    z32 = torch.where(mask, torch.ones((), dtype=coords.dtype), coords[..., 2].detach())
    two_s2 = 2.0 * sigma * sigma
    norm = 1.05 / sum(math.exp(-((d // 3 - 1) ** 2 + (d % 3 - 1) ** 2) / two_s2) for d in range(9))
    frac = torch.floor(xy.detach()) - xy + 0.5  # d/dxy = -1
    layer = torch.arange(K)
    C = [torch.zeros(N, H, W, 4, dtype=torch.float64) for _ in range(3)]
    for d in range(9):
        dr, dc = d // 3 - 1, d % 3 - 1
        # occlusion: q against its unfold neighbour (h + dr, w + dc), depth 0 outside
        p = _shift(z32, dr, dc)
        qtop_to_p, id_qp = (p - z32[..., :1]).abs().min(-1)
        ptop_to_q, id_pq = (p[..., :1] - z32).abs().min(-1)
        occ = torch.where(ptop_to_q < qtop_to_p, -id_pq, id_qp)[..., None]  # (N,H,W,1)
        # the splat in direction d, weighted with offset (dr, dc) on (x, y), lands on q from the source (h + dc, w + dr)
        u = frac[..., 0] + dr
        v = frac[..., 1] + dc
        wgt = fg.double() * norm * torch.exp(-(u * u + v * v) / two_s2)  # (N,H,W,K) at the source
        rgba = torch.cat([rgb * wgt[..., None], wgt[..., None]], -1)  # (N,H,W,K,4)
        rgba = _shift(rgba, dr, dc) if one_convention else _shift(rgba, dc, dr)
        for b, sel in enumerate((occ > layer, occ == layer, occ < layer)):
            C[b] = C[b] + (rgba * sel[..., None].double()).sum(3)
    out = torch.cat([torch.as_tensor(background, dtype=torch.float64).reshape(3), torch.zeros(1, dtype=torch.float64)])
    out = out.expand(N, H, W, 4)
    for b in (2, 1, 0):
        nb = C[b] / torch.maximum(C[b][..., 3:4], torch.ones((), dtype=torch.float64))
        out = nb + (1.0 - nb[..., 3:4]) * out
    return out
