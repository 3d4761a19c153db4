"""HardDepthShader / SoftDepthShader on the fused kernels (pytorch3d_amd/blending.py: hard_depth_blend, soft_depth_blend;
csrc/blend.hip).

  * kernel vs the reference's two shader classes on CPU (tests/golden/depth_ref.npz, make_golden_depth.py);
  * kernel vs the float64 restatement (tests/depth_restatement.py) over every compiled capacity, rows that are not a
    multiple of 16 bytes and the generic form, three slot patterns each; saturated sigmoids; one launch at a size users run;
  * bit-identical runs, strided views, one gradient only, empty batch, K above the limit;
  * the unmodified reference MeshRenderer with either depth shader through shim.install(patch_python=True).

Gates.  Output of the soft shader: |depth - depth64| <= 2 (K + 1) 2^-23 max(zfar, |zbuf|.max()) (depth_restatement.output_bound:
two ulps of sigmoid error and one rounding of the running sum per slot, each times a depth difference, plus the K + 1 roundings
of the weighted sum); twice that against the fixture, whose float32 values carry the same error.  Gradients: the gate of
tests/test_gpu_blending.py, allclose(atol=1e-4 max(1, |ref|.max()), rtol=1e-3).  The hard shader copies values: torch.equal.
"""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _util as U
import depth_restatement as dr

pytestmark = pytest.mark.gpu

ROOT = U.ROOT
STAGE = os.path.join(ROOT, "oracle", "_ref", "reference_py")
DEV = torch.device("cuda:0")


def _frags(p2f, zbuf, dists):
    return SimpleNamespace(pix_to_face=p2f, zbuf=zbuf, dists=dists)


def _run_soft(p2f, zbuf, dists, sigma, zfar, grad_out):
    """-> (depth, grad_zbuf, grad_dists) on the GPU"""
    from pytorch3d_amd import BlendParams, soft_depth_blend

    z = zbuf.to(DEV).detach().clone().requires_grad_(True)
    d = dists.to(DEV).detach().clone().requires_grad_(True)
    img = soft_depth_blend(_frags(p2f.to(DEV), z, d), BlendParams(sigma=sigma), zfar=zfar)
    img.backward(grad_out.to(DEV))
    torch.cuda.synchronize()
    return img.detach(), z.grad, d.grad


def _run_hard(p2f, zbuf, zfar, grad_out):
    from pytorch3d_amd import hard_depth_blend

    z = zbuf.to(DEV).detach().clone().requires_grad_(True)
    img = hard_depth_blend(_frags(p2f.to(DEV), z, None), zfar=zfar)
    img.backward(grad_out.to(DEV))
    torch.cuda.synchronize()
    return img.detach(), z.grad


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_kernels_vs_reference_fixture(tag):
    g = np.load(os.path.join(U.GOLDEN, "depth_ref.npz"))
    t = lambda k: torch.from_numpy(np.asarray(g[f"{tag}_{k}"]))  # noqa: E731
    p2f, zbuf, dists, sigma, zfar = t("pix_to_face"), t("zbuf"), t("dists"), float(t("sigma")), float(t("zfar"))
    zfar_arg = torch.tensor([zfar], device=DEV) if tag == "b" else zfar  # b: cameras.zfar of FoVPerspectiveCameras, a (1,) tensor
    img, gz, gd = _run_soft(p2f, zbuf, dists, sigma, zfar_arg, t("grad_out"))
    assert img.shape == p2f.shape[:3] + (1,) and img.dtype == torch.float32
    err = float((img.cpu().double() - t("soft_depth").double()).abs().max())
    bound = 2.0 * dr.output_bound(p2f.shape[3], zfar, zbuf)
    print(tag, "soft output vs fixture", err, "gate", bound)
    assert err <= bound
    assert dr.grad_close(gz.cpu(), t("soft_grad_zbuf")) and dr.grad_close(gd.cpu(), t("soft_grad_dists"))
    himg, hgz = _run_hard(p2f, zbuf, zfar_arg, t("grad_out"))
    assert himg.shape == p2f.shape[:3] + (1,)
    assert torch.equal(himg.cpu(), t("hard_depth")) and torch.equal(hgz.cpu(), t("hard_grad_zbuf"))


@pytest.mark.parametrize("pattern", ["prefix", "holes", "full"])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8, 10, 16, 17, 24, 32, 33, 40, 64, 150])
def test_kernels_vs_float64_restatement(K, pattern):
    sigma, zfar = 1e-4, 100.0
    gen = torch.Generator().manual_seed(1000 * K + len(pattern))
    p2f, zbuf, dists = dr.depth_inputs(gen, 2, 13, 11, K, sigma, pattern)
    grad_out = torch.randn(2, 13, 11, 1, generator=gen)
    img, gz, gd = _run_soft(p2f, zbuf, dists, sigma, zfar, grad_out)
    want = dr.soft_depth_restated(p2f, zbuf, dists, sigma, zfar)
    wz, wd = dr.soft_depth_restated_backward(p2f, zbuf, dists, sigma, zfar, grad_out)
    err = float((img.cpu().double() - want).abs().max())
    print(K, pattern, "soft output error", err, "bound", dr.output_bound(K, zfar, zbuf))
    assert err <= dr.output_bound(K, zfar, zbuf)
    assert dr.grad_close(gz.cpu().double(), wz), "grad_zbuf"
    assert dr.grad_close(gd.cpu().double(), wd), "grad_dists"
    himg, hgz = _run_hard(p2f, zbuf, zfar, grad_out)
    assert torch.equal(himg.cpu(), dr.hard_depth_restated(p2f, zbuf, zfar))
    assert torch.equal(hgz.cpu(), dr.hard_depth_restated_backward(p2f, grad_out))


@pytest.mark.parametrize("K", [4, 5, 40])
@pytest.mark.parametrize("dist", [-2e-2, 2e-2])
def test_saturated_sigmoids(dist, K):
    """-dists / sigma = +-200: a probability of exactly 1, respectively an exponential that overflows, in float32."""
    sigma, zfar = 1e-4, 100.0
    gen = torch.Generator().manual_seed(77 + K)
    p2f, zbuf, _ = dr.depth_inputs(gen, 2, 13, 11, K, sigma, "prefix")
    dists = torch.full(p2f.shape, dist)
    grad_out = torch.randn(2, 13, 11, 1, generator=gen)
    img, gz, gd = _run_soft(p2f, zbuf, dists, sigma, zfar, grad_out)
    for t in (img, gz, gd):
        assert bool(torch.isfinite(t).all())
    want = dr.soft_depth_restated(p2f, zbuf, dists, sigma, zfar)
    covered = p2f[..., :1] >= 0
    assert torch.equal(want.float(), torch.where(covered, zbuf[..., :1], torch.full_like(want, zfar).float()) if dist < 0
                       else torch.full_like(want, zfar).float())
    assert float((img.cpu().double() - want).abs().max()) <= dr.output_bound(K, zfar, zbuf)
    assert float(gd.abs().max()) <= 1e-20
    wz, _ = dr.soft_depth_restated_backward(p2f, zbuf, dists, sigma, zfar, grad_out)
    assert dr.grad_close(gz.cpu().double(), wz)


def test_one_launch_at_a_size_users_run():
    """N = 16, 512 x 512, K = 8; the float64 restatement evaluated on the GPU is the yardstick.  The [c_k <= 1] decision may
    legitimately differ where the running sum is within rounding of 1 while a slot up to k still has a live derivative
    (depth_restatement.soft_depth_fragile): such pixels are left out of the grad_dists comparison only, and may not exceed
    1e-5 of the pixels (2 and 0 of 1 048 576 for two seeds of this recipe on CPU)."""
    sigma, zfar, K = 1e-4, 100.0, 8
    gen = torch.Generator().manual_seed(512)
    p2f, zbuf, dists = (t.to(DEV) for t in dr.depth_inputs(gen, 16, 512, 512, K, sigma, "prefix"))
    grad_out = torch.randn(16, 512, 512, 1, generator=gen).to(DEV)
    img, gz, gd = _run_soft(p2f, zbuf, dists, sigma, zfar, grad_out)
    want = dr.soft_depth_restated(p2f, zbuf, dists, sigma, zfar)
    err = float((img.double() - want).abs().max())
    print("soft output error", err, "bound", dr.output_bound(K, zfar, zbuf))
    assert err <= dr.output_bound(K, zfar, zbuf)
    wz, wd = dr.soft_depth_restated_backward(p2f, zbuf, dists, sigma, zfar, grad_out)
    assert dr.grad_close(gz.double(), wz), "grad_zbuf"
    fragile = dr.soft_depth_fragile(p2f, dists, sigma)
    share = float(fragile.double().mean())
    print("fragile pixels", int(fragile.sum()), "of", fragile.numel())
    assert share <= 1e-5
    keep = ~fragile
    assert dr.grad_close(gd.double()[keep], wd[keep]), "grad_dists"
    himg, hgz = _run_hard(p2f, zbuf, zfar, grad_out)
    assert torch.equal(himg, dr.hard_depth_restated(p2f, zbuf, zfar))
    assert torch.equal(hgz, dr.hard_depth_restated_backward(p2f, grad_out))


@pytest.mark.parametrize("K", [8, 5, 40])
def test_two_runs_are_bit_identical(K):
    gen = torch.Generator().manual_seed(5)
    p2f, zbuf, dists = dr.depth_inputs(gen, 2, 64, 48, K, 1e-4, "prefix")
    grad_out = torch.randn(2, 64, 48, 1, generator=gen)
    a = _run_soft(p2f, zbuf, dists, 1e-4, 100.0, grad_out) + _run_hard(p2f, zbuf, 100.0, grad_out)
    b = _run_soft(p2f, zbuf, dists, 1e-4, 100.0, grad_out) + _run_hard(p2f, zbuf, 100.0, grad_out)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_strided_views_and_single_gradients():
    from pytorch3d_amd import BlendParams, hard_depth_blend, soft_depth_blend

    sigma, zfar, K = 1e-4, 100.0, 4
    gen = torch.Generator().manual_seed(9)
    big = [t.to(DEV) for t in dr.depth_inputs(gen, 2, 24, 20, 2 * K, sigma, "holes")]
    grad_out = torch.randn(2, 24, 20, 1, generator=gen)
    views = [t[..., 1:1 + K] for t in big]
    assert not any(v.is_contiguous() for v in views)
    p2f, zbuf, dists = (v.contiguous() for v in views)
    want = _run_soft(p2f, zbuf, dists, sigma, zfar, grad_out)
    hwant = _run_hard(p2f, zbuf, zfar, grad_out)
    z = views[1].detach().requires_grad_(True)
    d = views[2].detach().requires_grad_(True)
    assert not z.is_contiguous() and not d.is_contiguous()
    img = soft_depth_blend(_frags(views[0], z, d), BlendParams(sigma=sigma), zfar=zfar)
    img.backward(grad_out.to(DEV))
    assert torch.equal(img.detach(), want[0]) and torch.equal(z.grad, want[1]) and torch.equal(d.grad, want[2])
    z2 = views[1].detach().requires_grad_(True)
    himg = hard_depth_blend(_frags(views[0], z2, None), zfar=zfar)
    himg.backward(grad_out.to(DEV))
    assert torch.equal(himg.detach(), hwant[0]) and torch.equal(z2.grad, hwant[1])
    # one gradient only: the other one is None, the wanted one unchanged
    for want_z in (True, False):
        z = zbuf.detach().clone().requires_grad_(want_z)
        d = dists.detach().clone().requires_grad_(not want_z)
        img = soft_depth_blend(_frags(p2f, z, d), BlendParams(sigma=sigma), zfar=zfar)
        img.backward(grad_out.to(DEV))
        assert torch.equal(img.detach(), want[0])
        if want_z:
            assert d.grad is None and torch.equal(z.grad, want[1])
        else:
            assert z.grad is None and torch.equal(d.grad, want[2])


def test_empty_batch_bad_k_and_bad_zfar():
    from pytorch3d_amd import BlendParams, hard_depth_blend, soft_depth_blend

    bp = BlendParams(sigma=1e-4)
    e = _frags(torch.zeros(0, 6, 5, 3, dtype=torch.int64, device=DEV), torch.zeros(0, 6, 5, 3, device=DEV, requires_grad=True),
               torch.zeros(0, 6, 5, 3, device=DEV, requires_grad=True))
    for img in (soft_depth_blend(e, bp), hard_depth_blend(e)):
        assert img.shape == (0, 6, 5, 1) and img.dtype == torch.float32 and img.is_cuda
        img.sum().backward()
    gen = torch.Generator().manual_seed(2)
    f = _frags(*(t.to(DEV) for t in dr.depth_inputs(gen, 1, 3, 3, 151, 1e-4, "full")))
    with pytest.raises((ValueError, RuntimeError)):
        soft_depth_blend(f, bp)
    with pytest.raises((ValueError, RuntimeError)):
        hard_depth_blend(f)
    f = _frags(*(t.to(DEV) for t in dr.depth_inputs(gen, 2, 3, 3, 4, 1e-4, "full")))
    for bad in (torch.tensor([50.0, 60.0], device=DEV), torch.tensor([50.0], device=DEV, requires_grad=True), "far"):
        with pytest.raises(ValueError):
            soft_depth_blend(f, bp, zfar=bad)
        with pytest.raises(ValueError):
            hard_depth_blend(f, zfar=bad)
    with pytest.raises(ValueError):
        soft_depth_blend(_frags(f.pix_to_face, f.zbuf, None), bp)
    with pytest.raises(RuntimeError, match="float32"):
        soft_depth_blend(_frags(f.pix_to_face, f.zbuf.double(), f.dists), bp)


def test_reference_mesh_renderer_with_depth_shaders_through_the_shim():
    if not os.path.isdir(os.path.join(STAGE, "pytorch3d", "renderer")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference checkout exists)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_depth_render_case.py")], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    j = json.loads([line for line in res.stdout.splitlines() if line.startswith("{")][-1])
    if "skipped" in j:
        pytest.skip(j["skipped"])
    print(json.dumps(j))
    for name in ("SoftDepthShader", "HardDepthShader"):
        rec = j[name]
        assert rec["calls"][name + ".forward"] == [1, 0], rec["calls"]
        assert rec["shape"] == [2, 48, 48, 1]
        assert 0.1 < rec["covered"] < 0.9
        assert rec["grad_finite"] and rec["grad_max"] > 0.0
    assert j["SoftDepthShader"]["error"] <= j["SoftDepthShader"]["bound"]
    assert j["SoftDepthShader"]["soft_pixels"] > 0.0  # the blur does blend depths somewhere: not the hard image
    assert j["HardDepthShader"]["equal"]
