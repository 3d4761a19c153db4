"""Golden fixture for HardDepthShader / SoftDepthShader, generated FROM THE REFERENCE (build container only).

    python tests/golden/make_golden_depth.py   ->  tests/golden/depth_ref.npz

The reference's two shader classes (pytorch3d/renderer/mesh/shader.py:377-445) called on CPU on seeded fragments
(tests/depth_restatement.py: depth_inputs), plus torch autograd of a seeded upstream gradient to zbuf and dists:

    a  N = 2, 9 x 7, K = 5, sigma 1e-4, zfar = 100.0 by keyword
    b  N = 1, 12 x 10, K = 8, sigma 3e-4, zfar from FoVPerspectiveCameras(zfar=50): a (1,) tensor
    c  N = 2, 9 x 7, K = 1, sigma 1e-4, zfar = 100.0 by keyword
    d  N = 2, 9 x 7, K = 5, sigma 1e-4, zfar = 30.0 by keyword, random holes and unsorted zbuf

The generator asserts that empty pixels, pixels whose probabilities sum to less than 1, pixels saturated by slot 0 and
pixels saturated at a later slot each make up at least 5 % of case a and of case b (SEED was picked so): every branch of
the kernels is pinned by the fixture.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [  # tag, N, H, W, K, sigma, zfar (None: the cameras'), pattern
    ("a", 2, 9, 7, 5, 1e-4, 100.0, "prefix"),
    ("b", 1, 12, 10, 8, 3e-4, None, "prefix"),
    ("c", 2, 9, 7, 1, 1e-4, 100.0, "prefix"),
    ("d", 2, 9, 7, 5, 1e-4, 30.0, "holes"),
]
CAMERA_ZFAR = 50.0
SEED = 2024


def draw(seed):
    import depth_restatement as dr

    gen = torch.Generator().manual_seed(seed)
    inputs = {}
    for tag, N, H, W, K, sigma, _, pattern in CASES:
        inputs[tag] = dr.depth_inputs(gen, N, H, W, K, sigma, pattern)
        inputs[tag + "_grad_out"] = torch.randn(N, H, W, 1, generator=gen)
    return inputs


def main():
    import depth_restatement as dr
    import make_golden as mg

    mg.bind_reference()
    from pytorch3d.renderer import BlendParams, FoVPerspectiveCameras
    from pytorch3d.renderer.mesh.rasterizer import Fragments
    from pytorch3d.renderer.mesh.shader import HardDepthShader, SoftDepthShader

    inputs = draw(SEED)
    out = {}
    for tag, N, H, W, K, sigma, zfar, pattern in CASES:
        p2f, zbuf, dists = inputs[tag]
        g = inputs[tag + "_grad_out"]
        classes = dr.pixel_classes(p2f, dists, sigma)
        print(tag, "empty / unsaturated / saturated by slot 0 / saturated later:", ["%.2f" % c for c in classes])
        if tag in ("a", "b"):
            assert min(classes) >= 0.05, (tag, classes)
        cameras = FoVPerspectiveCameras(zfar=CAMERA_ZFAR)
        kwargs = {} if zfar is None else {"zfar": zfar}
        rec = {"pix_to_face": p2f, "zbuf": zbuf, "dists": dists, "sigma": sigma, "zfar": CAMERA_ZFAR if zfar is None else zfar,
               "grad_out": g}
        for name, shader in (("soft", SoftDepthShader(cameras=cameras, blend_params=BlendParams(sigma=sigma))),
                             ("hard", HardDepthShader(cameras=cameras))):
            z = zbuf.clone().requires_grad_(True)
            d = dists.clone().requires_grad_(True)
            bary = torch.zeros(N, H, W, K, 3)
            img = shader(Fragments(pix_to_face=p2f, zbuf=z, bary_coords=bary, dists=d), None, **kwargs)
            assert img.shape == (N, H, W, 1) and img.dtype == torch.float32
            (img * g).sum().backward()
            rec[name + "_depth"] = img
            rec[name + "_grad_zbuf"] = z.grad
            if name == "soft":
                rec[name + "_grad_dists"] = d.grad
            else:
                assert d.grad is None
        out.update({f"{tag}_{k}": v for k, v in rec.items()})
    mg.save("depth_ref", **out)


if __name__ == "__main__":
    main()
