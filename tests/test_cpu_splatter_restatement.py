"""CPU side of the fused splatter (pytorch3d_amd/splatter.py):

  * the float64 restatement that tests/test_gpu_splatter.py judges the kernel by (tests/splatter_restatement.py) equals the
    reference's SplatterBlender on CPU -- on the committed fixture (tests/golden/splatter_ref.npz, every machine) and live
    on fresh random inputs (where the reference checkout exists); the "one convention for both direction indexings"
    variant does NOT, on every fixture case;
  * shim.patch_reference_python() installs the SplatterPhongShader.forward patch, uninstall_python_patches() removes it,
    and on CPU tensors the patched forward falls back to the reference's own result (subprocess: the shim replaces
    sys.modules entries).
"""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import _util as U
from splatter_restatement import splatter_blend_restated

REFERENCE = os.environ.get("P3D_REFERENCE_ROOT", "/root/reference")
HAVE_REFERENCE = os.path.isdir(os.path.join(REFERENCE, "pytorch3d", "renderer"))
TAGS = ["k1_holes", "k3_ties", "k3_asym", "k8_holes", "k8_ties", "k8_asym"]


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_equals_the_reference_fixture(tag):
    g = np.load(os.path.join(U.GOLDEN, "splatter_ref.npz"))
    t = lambda k: torch.from_numpy(g[f"{tag}_{k}"])  # noqa: E731
    c = t("colors").clone().requires_grad_(True)
    x = t("coords").clone().requires_grad_(True)
    sigma = float(g[f"{tag}_sigma"])
    img = splatter_blend_restated(c, x, t("mask"), sigma, t("background"))
    (img * t("grad_out").double()).sum().backward()
    assert float((img.detach().float() - t("image")).abs().max()) <= 2e-6
    for ours, ref in ((c.grad, t("grad_colors")), (x.grad, t("grad_coords"))):
        assert float((ours.float() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    clean = splatter_blend_restated(t("colors"), t("coords"), t("mask"), sigma, t("background"), one_convention=True)
    assert float((clean.float() - t("image")).abs().max()) > 1e-2, "the fixture does not tell the two direction pairings apart"


SCRIPT = textwrap.dedent("""
    import sys, warnings
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    import torch
    import pytorch3d_amd.shim as shim
    shim.install(%r)
    from pytorch3d.renderer import BlendParams, FoVPerspectiveCameras, Materials, PointLights, TexturesVertex
    from pytorch3d.renderer.mesh import shader as shader_mod
    from pytorch3d.renderer.mesh.rasterizer import Fragments
    from pytorch3d.renderer.splatter_blend import SplatterBlender
    from pytorch3d.structures import Meshes
    from splatter_restatement import splatter_blend_restated

    # live: the restatement against the reference's SplatterBlender on random inputs (identity screen transform)
    class Ident:
        def transform_points_screen(self, p, image_size=None, with_xyflip=True):
            return p.clone()
    gen = torch.Generator().manual_seed(7)
    for (N, H, W, K, sigma) in ((2, 11, 6, 5, 0.5), (1, 2, 3, 2, 0.4), (1, 1, 1, 1, 0.5)):
        hh = torch.arange(H, dtype=torch.float32).view(1, H, 1, 1)
        ww = torch.arange(W, dtype=torch.float32).view(1, 1, W, 1)
        x = ww + 0.5 + (torch.rand(N, H, W, K, generator=gen) - 0.5) * 0.98
        y = hh + 0.5 + (torch.rand(N, H, W, K, generator=gen) - 0.5) * 0.98
        z = torch.sort(torch.rand(N, H, W, K, generator=gen) * 4 + 1, -1).values
        coords = torch.stack([x, y, z], -1)
        colors = torch.rand(N, H, W, K, 3, generator=gen)
        mask = torch.rand(N, H, W, K, generator=gen) < 0.2
        go = torch.randn(N, H, W, 4, generator=gen)
        c1, x1 = colors.clone().requires_grad_(True), coords.clone().requires_grad_(True)
        ref = SplatterBlender((N, H, W, K), "cpu")(c1, x1, Ident(), mask, BlendParams(sigma=sigma, background_color=(0.3, 0.2, 0.1)))
        (ref * go).sum().backward()
        c2, x2 = colors.clone().requires_grad_(True), coords.clone().requires_grad_(True)
        ours = splatter_blend_restated(c2, x2, mask, sigma, (0.3, 0.2, 0.1))
        (ours * go.double()).sum().backward()
        assert float((ours.detach().float() - ref.detach()).abs().max()) <= 2e-6
        for a, b in ((c2.grad, c1.grad), (x2.grad, x1.grad)):
            assert float((a.float() - b).abs().max()) <= 1e-5 * max(float(b.abs().max()), 1e-6)

    # the patch: installed, counted, falls back on CPU tensors to the reference's own result, removed again
    orig = shader_mod.SplatterPhongShader.forward
    verts = torch.tensor([[-0.6, -0.6, 0.0], [0.6, -0.6, 0.0], [0.0, 0.7, 0.0], [0.0, 0.0, 0.4]])
    faces = torch.tensor([[0, 1, 2], [0, 1, 3]])
    meshes = Meshes(verts=[verts], faces=[faces], textures=TexturesVertex(verts_features=[torch.rand(4, 3, generator=gen)]))
    H = W = 6
    p2f = torch.randint(-1, 2, (1, H, W, 2), generator=gen)
    bary = torch.rand(1, H, W, 2, 3, generator=gen)
    bary = bary / bary.sum(-1, keepdim=True)
    frags = Fragments(pix_to_face=p2f, zbuf=torch.rand(1, H, W, 2, generator=gen) + 2, bary_coords=bary,
                      dists=torch.zeros(1, H, W, 2))
    cams = FoVPerspectiveCameras(T=torch.tensor([[0.0, 0.0, 3.0]]))
    kw = dict(cameras=cams, lights=PointLights(), materials=Materials(), blend_params=BlendParams(sigma=0.5))

    def render():
        return shader_mod.SplatterPhongShader(**kw)(frags, meshes)

    want = render()
    shim.patch_reference_python()
    assert shader_mod.SplatterPhongShader.forward is not orig
    assert getattr(shader_mod.SplatterPhongShader.forward, "__wrapped__", None) is orig
    shim.PATCH_CALLS.clear()
    got = render()
    assert shim.PATCH_CALLS["SplatterPhongShader.forward"] == [0, 1], shim.PATCH_CALLS
    assert torch.equal(got, want)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        shader_mod.SplatterPhongShader(**dict(kw, blend_params=BlendParams(sigma=0.3)))(frags, meshes)
    assert any("sigma=0.3" in str(x.message) for x in w)
    shim.uninstall_python_patches()
    assert shader_mod.SplatterPhongShader.forward is orig
    print("OK")
""")


@pytest.mark.skipif(not HAVE_REFERENCE, reason="reference checkout not present (GPU box)")
def test_reference_splatter_live_and_shader_patch_install_fallback_uninstall():
    script = SCRIPT % (U.ROOT, os.path.join(U.ROOT, "tests"), REFERENCE)
    res = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300, cwd=U.ROOT)
    assert res.returncode == 0 and "OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
