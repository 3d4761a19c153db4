"""GPU parity of the blending row: sigmoid_alpha_blend (`pytorch3d._C` operator) and the
fused softmax_rgb_blend, against the reference-generated fixture (tests/golden/blend_ref.npz: the reference's
C++ CPU kernels and its Python function + autograd), the oracle on random inputs, and -- at the bench
workload's full size -- a dense torch re-derivation of blending.py:147-244 with torch autograd.
Tolerances: outputs 1e-5 (north_star), gradients rtol 1e-3.

Per capacity, per branch (ties, faces beyond zfar, saturated sigmoids, empty pixels, equal planes), the second grid-stride round, the
argument and alignment checks of the C entries, all against a float64 chain through a per-class gate: tests/test_gpu_blend_edges.py.
"""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

import _util as U
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
Frag = namedtuple("Frag", "pix_to_face zbuf dists")


def _load():
    g = np.load(os.path.join(U.GOLDEN, "blend_ref.npz"))
    return {k: (torch.from_numpy(g[k]) if g[k].ndim else g[k].item()) for k in g.files}


def test_sigmoid_alpha_blend_vs_reference_cpu_kernels():
    from pytorch3d_amd import _C

    g = _load()
    d = torch.device("cuda:0")
    a = _C.sigmoid_alpha_blend(g["dists"].to(d), g["pix_to_face"].to(d), g["sigma"])
    assert torch.allclose(a.cpu(), g["sig_alphas"], atol=1e-6, rtol=0)
    gd = _C.sigmoid_alpha_blend_backward(g["sig_grad_alphas"].to(d), g["sig_alphas"].to(d), g["dists"].to(d),
                                         g["pix_to_face"].to(d), g["sigma"])
    ref = g["sig_grad_dists"]
    assert torch.allclose(gd.cpu(), ref, atol=1e-6 * ref.abs().max().item(), rtol=1e-5)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_softmax_rgb_blend_vs_reference_python(tag):
    import pytorch3d_amd as p3d

    g = _load()
    d = torch.device("cuda:0")
    k = lambda n: g[f"sm_{tag}_{n}"]
    colors = g["colors"].to(d).requires_grad_(True)
    dists = g["dists"].to(d).requires_grad_(True)
    zbuf = g["zbuf"].to(d).requires_grad_(True)
    zn = k("znear").to(d) if isinstance(k("znear"), torch.Tensor) else float(k("znear"))
    zf = k("zfar").to(d) if isinstance(k("zfar"), torch.Tensor) else float(k("zfar"))
    bp = p3d.BlendParams(sigma=k("sigma"), gamma=k("gamma"), background_color=tuple(k("bg").tolist()))
    img = p3d.softmax_rgb_blend(colors, Frag(g["pix_to_face"].to(d), zbuf, dists), bp, znear=zn, zfar=zf)
    assert torch.allclose(img.cpu(), k("out"), atol=1e-5, rtol=1e-5)
    img.backward(k("grad_out").to(d))
    for got, name in ((colors.grad, "grad_colors"), (dists.grad, "grad_dists"), (zbuf.grad, "grad_zbuf")):
        ref = k(name)
        assert torch.allclose(got.cpu(), ref, atol=1e-4 * max(1.0, ref.abs().max().item()), rtol=1e-3), name


# 17 / 24 / 32: the <32> instantiations (round 5: softmax_blend_bwd_kernel<32> is one of the two kernels of the library that hold
# registers in AGPRs -- pytorch3d_amd/build.py: AGPR_KERNELS_TESTED points here); `dense`: every slot of every pixel holds a face,
# i.e. every register row of the kernels is live (the round-4 miscompile showed only on inputs that fill the queues)
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 8, 10, 16, 17, 24, 32, 33, 40, 150])
def test_blend_kernels_vs_oracle_all_capacities(K, dense):
    import pytorch3d_amd as p3d
    from pytorch3d_amd import _C

    d = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(K)
    N, H, W = 2, 13, 11
    p2f = torch.randint(0 if dense else -1, 30, (N, H, W, K), generator=gen)
    dists = (torch.rand(N, H, W, K, generator=gen) - 0.4) * 5e-4
    zbuf = torch.rand(N, H, W, K, generator=gen) * 3 + 0.8
    colors = torch.rand(N, H, W, K, 3, generator=gen)
    sigma, gamma, bg = 2e-4, 1e-3, (0.2, 0.4, 0.6)
    a = _C.sigmoid_alpha_blend(dists.to(d), p2f.to(d), sigma)
    assert torch.allclose(a.cpu(), orc.sigmoid_alpha_blend(dists, p2f, sigma), atol=1e-6, rtol=0)
    ga = torch.randn(N, H, W, generator=gen)
    gd = _C.sigmoid_alpha_blend_backward(ga.to(d), a, dists.to(d), p2f.to(d), sigma)
    ref = orc.sigmoid_alpha_blend_backward(ga, a.cpu(), dists, p2f, sigma)
    assert torch.allclose(gd.cpu(), ref, atol=1e-6 * max(1.0, ref.abs().max().item()), rtol=1e-5)

    cg, dg, zg = (t.to(d).requires_grad_(True) for t in (colors, dists, zbuf))
    img = p3d.softmax_rgb_blend(cg, Frag(p2f.to(d), zg, dg), p3d.BlendParams(sigma, gamma, bg), znear=0.5, zfar=10.0)
    ref = orc.softmax_rgb_blend(colors, p2f, dists, zbuf, sigma, gamma, bg, znear=0.5, zfar=10.0)
    assert torch.allclose(img.cpu(), ref, atol=1e-5, rtol=1e-5)
    go = torch.randn(N, H, W, 4, generator=gen)
    img.backward(go.to(d))
    rc, rd, rz = orc.softmax_rgb_blend_backward(go, colors, p2f, dists, zbuf, sigma, gamma, bg, znear=0.5, zfar=10.0)
    for got, r in ((cg.grad, rc), (dg.grad, rd), (zg.grad, rz)):
        assert torch.allclose(got.cpu(), r, atol=1e-4 * max(1.0, r.abs().max().item()), rtol=1e-3)


def test_blend_empty_and_background_only():
    import pytorch3d_amd as p3d
    from pytorch3d_amd import _C

    d = torch.device("cuda:0")
    p2f = torch.full((1, 4, 4, 3), -1, dtype=torch.int64, device=d)
    z = torch.full((1, 4, 4, 3), -1.0, device=d)
    c = torch.rand(1, 4, 4, 3, 3, device=d)
    img = p3d.softmax_rgb_blend(c, Frag(p2f, z, z), p3d.BlendParams(background_color=(0.1, 0.2, 0.3)))
    assert torch.allclose(img[..., :3], torch.tensor([0.1, 0.2, 0.3], device=d).expand(1, 4, 4, 3), atol=1e-6)
    assert (img[..., 3] == 0).all()
    assert (_C.sigmoid_alpha_blend(z, p2f, 1e-4) == 0).all()
    e = _C.sigmoid_alpha_blend(z[:0], p2f[:0], 1e-4)
    assert e.shape == (0, 4, 4)


def test_softmax_rgb_blend_at_bench_size_vs_dense_torch():
    """N=8, 512x512, K=8 fragments of the bench generator: the fused kernels against blending.py:147-244 restated
    with torch ops on the GPU (+ torch autograd)."""
    import math

    import pytorch3d_amd as p3d

    d = torch.device("cuda:0")
    verts, faces = U.hetero_batch(8, seed=5)
    m = p3d.PackedMeshes([v.to(d) for v in verts], [f.to(d) for f in faces])
    blur = math.log(1.0 / 1e-4 - 1.0) * 1e-4
    p2f, zbuf, bary, dists = p3d.rasterize_meshes(m, image_size=512, blur_radius=blur, faces_per_pixel=8,
                                                  perspective_correct=True, clip_barycentric_coords=True)
    gen = torch.Generator().manual_seed(0)
    colors = torch.rand(8, 512, 512, 8, 3, generator=gen).to(d)
    sigma, bg = 1e-4, (1.0, 0.5, 0.25)
    gamma = 1e-4

    def dense(colors, dists, zbuf):
        eps = 1e-10
        mask = p2f >= 0
        prob = torch.sigmoid(-dists / sigma) * mask
        alpha = torch.prod(1.0 - prob, dim=-1)
        z_inv = (100.0 - zbuf) / (100.0 - 1.0) * mask
        z_inv_max = torch.max(z_inv, dim=-1).values[..., None].clamp(min=eps)
        wn = prob * torch.exp((z_inv - z_inv_max) / gamma)
        delta = torch.exp((eps - z_inv_max) / gamma).clamp(min=eps)
        denom = wn.sum(dim=-1)[..., None] + delta
        rgb = ((wn[..., None] * colors).sum(dim=-2) + delta * torch.tensor(bg, device=d)) / denom
        return torch.cat([rgb, (1.0 - alpha)[..., None]], -1)

    # alpha does not involve the depth softmax: tight (the reference's own test checks alpha only, atol 1e-7 on
    # tiny inputs, tests/test_blending.py:132).  RGB: the exponent (z_inv - z_inv_max) / gamma amplifies the ONE-ulp
    # difference between torch-GPU's "multiply by the reciprocal of a Python scalar" (BinaryDivTrueKernel.cu) and a
    # true division by 1 / gamma: at gamma = 1e-4 the reference itself is only defined to ~1e-3 (its CPU and GPU
    # paths differ by that much), at gamma = 1e-2 to ~1e-5.  We follow the true-division (CPU / double) evaluation.
    for gm, rgb_tol in ((1e-4, 2e-3), (1e-2, 2e-5)):
        gamma = gm
        c1, d1, z1 = (t.detach().clone().requires_grad_(True) for t in (colors, dists, zbuf))
        c2, d2, z2 = (t.detach().clone().requires_grad_(True) for t in (colors, dists, zbuf))
        img = p3d.softmax_rgb_blend(c1, Frag(p2f, z1, d1), p3d.BlendParams(sigma, gamma, bg))
        ref = dense(c2, d2, z2)
        assert torch.allclose(img[..., 3], ref[..., 3], atol=1e-6, rtol=0)
        assert (img[..., :3] - ref[..., :3]).abs().max().item() <= rgb_tol, (img - ref).abs().max().item()
        go = torch.randn(img.shape, generator=gen).to(d)
        img.backward(go)
        ref.backward(go)
        for name, a, b in (("colors", c1.grad, c2.grad), ("dists", d1.grad, d2.grad), ("zbuf", z1.grad, z2.grad)):
            scale = max(1.0, b.abs().max().item())
            err = (a - b).abs().max().item() / scale
            assert err <= 50 * rgb_tol, (name, gm, err)
