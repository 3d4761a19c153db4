"""CPU suite for the depth shaders' fused path (pytorch3d_amd/blending.py: hard_depth_blend, soft_depth_blend; csrc/blend.hip).

  * the four C entries are declared in the header and bound, the two functions exist and refuse CPU tensors;
  * tests/golden/depth_ref.npz (the reference's HardDepthShader / SoftDepthShader on CPU, make_golden_depth.py) against the
    float64 restatement (tests/depth_restatement.py), output and gradient gates: ties the yardstick of the GPU tests to the
    reference's recorded behaviour;
  * where the reference checkout is present: the patched shader forwards on CPU fragments fall back to the originals, raise
    what they raise, and are restored by uninstall_python_patches().
"""
import os
import re
import subprocess
import sys
import textwrap
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _util as U
import depth_restatement as dr

REFERENCE = os.environ.get("P3D_REFERENCE_ROOT", "/root/reference")
ROOT = U.ROOT
ENTRIES = ("p3d_soft_depth_blend_forward", "p3d_soft_depth_blend_backward", "p3d_hard_depth_blend_forward",
           "p3d_hard_depth_blend_backward")
TAGS = ("a", "b", "c", "d")


def test_entries_are_declared_and_bound_and_cpu_tensors_refused():
    import pytorch3d_amd as p3d
    from pytorch3d_amd import _lib

    header = open(os.path.join(ROOT, "include", "p3d_amd.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+3\b", header) and _lib.ABI_VERSION == 3
    gen = torch.Generator().manual_seed(0)
    p2f, zbuf, dists = dr.depth_inputs(gen, 1, 4, 3, 2, 1e-4)
    frags = SimpleNamespace(pix_to_face=p2f, zbuf=zbuf, dists=dists)
    with pytest.raises(RuntimeError, match="GPU path only"):
        p3d.hard_depth_blend(frags, zfar=10.0)
    with pytest.raises(RuntimeError, match="GPU path only"):
        p3d.soft_depth_blend(frags, p3d.BlendParams(sigma=1e-4), zfar=10.0)
    with pytest.raises(ValueError, match="requires Fragments.dists"):
        p3d.soft_depth_blend(SimpleNamespace(pix_to_face=p2f, zbuf=zbuf, dists=None), p3d.BlendParams(sigma=1e-4))


def _case(tag):
    g = np.load(os.path.join(U.GOLDEN, "depth_ref.npz"))
    t = {k[len(tag) + 1:]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith(tag + "_")}
    t["sigma"], t["zfar"] = float(t["sigma"]), float(t["zfar"])
    return t


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_agrees_with_the_float64_restatement(tag):
    t = _case(tag)
    p2f, zbuf, dists, sigma, zfar, g = t["pix_to_face"], t["zbuf"], t["dists"], t["sigma"], t["zfar"], t["grad_out"]
    K = p2f.shape[3]
    assert t["soft_depth"].shape == p2f.shape[:3] + (1,) and t["soft_depth"].dtype == torch.float32
    want = dr.soft_depth_restated(p2f, zbuf, dists, sigma, zfar)
    err = float((t["soft_depth"].double() - want).abs().max())
    bound = dr.output_bound(K, zfar, zbuf)
    print(tag, "soft output error", err, "bound", bound)
    assert err <= bound
    gz, gd = dr.soft_depth_restated_backward(p2f, zbuf, dists, sigma, zfar, g)
    assert dr.grad_close(t["soft_grad_zbuf"].double(), gz)
    assert dr.grad_close(t["soft_grad_dists"].double(), gd)
    assert torch.equal(t["hard_depth"], dr.hard_depth_restated(p2f, zbuf, zfar))
    assert torch.equal(t["hard_grad_zbuf"], dr.hard_depth_restated_backward(p2f, g))


def test_fixture_pins_every_branch():
    for tag in ("a", "b"):
        t = _case(tag)
        assert min(dr.pixel_classes(t["pix_to_face"], t["dists"], t["sigma"])) >= 0.05, tag
    d = _case("d")
    valid = d["pix_to_face"] >= 0
    assert bool((~valid[..., :-1] & valid[..., 1:]).any())  # a hole in front of a face
    assert bool((d["zbuf"][..., 1:] < d["zbuf"][..., :-1]).any())  # unsorted depths


SCRIPT = textwrap.dedent("""
    import sys
    sys.path.insert(0, %r)
    sys.path.insert(0, %r + "/tests")
    import torch
    import run_reference_suite as rrs
    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim
    shim.install(%r)
    from pytorch3d.renderer import BlendParams, FoVPerspectiveCameras
    from pytorch3d.renderer.mesh.rasterizer import Fragments
    from pytorch3d.renderer.mesh.shader import HardDepthShader, SoftDepthShader
    import depth_restatement as dr

    originals = {HardDepthShader: HardDepthShader.forward, SoftDepthShader: SoftDepthShader.forward}
    shim.install(patch_python=True)
    for cls, orig in originals.items():
        assert cls.forward is not orig and cls.forward.__wrapped__ is orig

    gen = torch.Generator().manual_seed(3)
    N, H, W, K = 2, 6, 5, 4
    p2f, zbuf, dists = dr.depth_inputs(gen, N, H, W, K, 1e-4)
    frags = Fragments(pix_to_face=p2f, zbuf=zbuf, bary_coords=torch.zeros(N, H, W, K, 3), dists=dists)
    one = FoVPerspectiveCameras(zfar=40.0)
    two = FoVPerspectiveCameras(zfar=torch.tensor([40.0, 60.0]))
    assert tuple(two.zfar.shape) == (2,)
    shim.PATCH_CALLS.clear()
    for cls in (HardDepthShader, SoftDepthShader):
        shader = cls(cameras=one, blend_params=BlendParams(sigma=1e-4))
        got = shader(frags, None)
        want = originals[cls](shader, frags, None)
        assert got.shape == (N, H, W, 1) and torch.equal(got, want), cls.__name__
        assert shim.PATCH_CALLS[cls.__name__ + ".forward"] == [0, 1], shim.PATCH_CALLS
        # a per-image zfar: the reference's own exception, through the patch as without it
        raised = []
        for call in (lambda s: s(frags, None, cameras=two), lambda s: originals[cls](s, frags, None, cameras=two)):
            try:
                call(shader)
                raised.append(None)
            except Exception as e:
                raised.append(type(e))
        assert raised[0] is not None and raised[0] is raised[1], (cls.__name__, raised)
        # no cameras anywhere: the reference's ValueError
        try:
            cls()(frags, None)
            raise AssertionError("no exception without cameras")
        except ValueError as e:
            assert "Cameras must be specified" in str(e)
    shim.uninstall_python_patches()
    for cls, orig in originals.items():
        assert cls.forward is orig
    print("ok")
""")


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "pytorch3d", "renderer")),
                    reason="reference checkout not present (GPU box)")
def test_patched_depth_shaders_fall_back_on_cpu_and_are_restored():
    res = subprocess.run([sys.executable, "-c", SCRIPT % (ROOT, ROOT, REFERENCE)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stdout[-2000:] + res.stderr[-4000:]
