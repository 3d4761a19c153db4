"""Golden fixture for SplatterPhongShader's blend, generated FROM THE REFERENCE (build container only).

    python tests/golden/make_golden_splatter.py   ->  tests/golden/splatter_ref.npz

Blend cases: the reference's SplatterBlender (pytorch3d/renderer/splatter_blend.py) on CPU with an identity screen
transform (the camera call is out of the kernel's scope), forward + torch autograd of a random grad_out to the colours
and screen coordinates.  N = 2, H x W = 9 x 7, K in {1, 3, 8}: background holes and one all-background image, exact depth
ties, a depth layout that only changes along h (the reference pairs the splat of neighbour (dh, dw) with the occlusion
test of neighbour (dw, dh); this layout tells the pairings apart), sigma 0.5 and 0.35, non-white backgrounds.

Render case: the reference's MeshRenderer(MeshRasterizer, SplatterPhongShader) on CPU (its C++ CPU rasterizer + Python
shading / splatter) with FoVPerspectiveCameras, PointLights and TexturesVertex, plus the gradients of a random loss to
the vertices and vertex colours.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 9, 7


class _ScreenIdentity:
    """A camera whose screen transform is the identity: SplatterBlender then blends the given screen coordinates."""

    def transform_points_screen(self, points, image_size=None, with_xyflip=True):
        return points.clone()


def blend_inputs(gen, K, kind):
    N = 2
    hh = torch.arange(H, dtype=torch.float32).view(1, H, 1, 1)
    ww = torch.arange(W, dtype=torch.float32).view(1, 1, W, 1)
    # screen x, y near the pixel centres (x along w, y along h as with_xyflip=False gives them), kept 1e-2 away from integers
    x = (ww + 0.5 + (torch.rand(N, H, W, K, generator=gen) - 0.5) * 0.96).expand(N, H, W, K)
    y = (hh + 0.5 + (torch.rand(N, H, W, K, generator=gen) - 0.5) * 0.96).expand(N, H, W, K)
    z = torch.sort(torch.rand(N, H, W, K, generator=gen) * 3 + 0.5, dim=-1).values
    mask = torch.rand(N, H, W, K, generator=gen) < 0.15
    if kind == "holes":
        mask[1] = True  # one all-background image
        mask[0, 2:4, 1:3] = True  # a hole
    elif kind == "ties":
        z[:, 3, :, 0] = 1.25  # a row of equal top layers
        z[:, :, 4, :] = z[:, :, 3, :]  # a column equal to its neighbour
        if K > 1:
            z[:, 5, 5, 1] = z[:, 5, 5, 0]  # equal layers inside a pixel
        mask[:, 6] = False
    elif kind == "asym":
        k = torch.arange(K, dtype=torch.float32).view(1, 1, 1, K)
        z = (1.0 + 0.3 * hh + 0.3 * k).expand(N, H, W, K).clone()  # changes along h only: (dh, 0) != (0, dh)
        mask[:] = False
        mask[:, 7:, :, K - 1] = True
    coords = torch.stack([x, y, z], -1).contiguous()
    colors = torch.rand(N, H, W, K, 3, generator=gen)
    return colors, coords, mask


CASES = [  # tag, K, kind, sigma, background
    ("k1_holes", 1, "holes", 0.5, (0.2, 0.3, 0.4)),
    ("k3_ties", 3, "ties", 0.5, (1.0, 1.0, 1.0)),
    ("k3_asym", 3, "asym", 0.5, (0.1, 0.6, 0.9)),
    ("k8_holes", 8, "holes", 0.35, (0.7, 0.2, 0.1)),
    ("k8_ties", 8, "ties", 0.5, (0.0, 0.0, 0.0)),
    ("k8_asym", 8, "asym", 0.35, (0.3, 0.3, 0.9)),
]


def blend_cases(out, gen):
    from pytorch3d.renderer import BlendParams
    from pytorch3d.renderer.splatter_blend import SplatterBlender

    for tag, K, kind, sigma, bg in CASES:
        colors, coords, mask = blend_inputs(gen, K, kind)
        c = colors.clone().requires_grad_(True)
        x = coords.clone().requires_grad_(True)
        blender = SplatterBlender((2, H, W, K), "cpu")
        img = blender(c, x, _ScreenIdentity(), mask, BlendParams(sigma=sigma, background_color=bg))
        g = torch.randn(img.shape, generator=gen)
        (img * g).sum().backward()
        out.update({f"{tag}_colors": colors, f"{tag}_coords": coords, f"{tag}_mask": mask, f"{tag}_sigma": sigma,
                    f"{tag}_background": torch.tensor(bg), f"{tag}_image": img, f"{tag}_grad_out": g,
                    f"{tag}_grad_colors": c.grad, f"{tag}_grad_coords": x.grad})


def render_case(out, gen):
    import _util as U
    from pytorch3d.renderer import (BlendParams, FoVPerspectiveCameras, Materials, MeshRasterizer, MeshRenderer, PointLights,
                                    RasterizationSettings, SplatterPhongShader, TexturesVertex, look_at_view_transform)
    from pytorch3d.structures import Meshes

    v0, f0 = U.ico_sphere(2)
    v1, f1 = U.torus(0.35, 0.9, 10, 14)
    verts_l = [v0.clone().requires_grad_(True), (v1 * 0.9).clone().requires_grad_(True)]
    faces_l = [f0, f1]
    cols_l = [torch.rand(v.shape[0], 3, generator=gen).requires_grad_(True) for v in verts_l]
    meshes = Meshes(verts=verts_l, faces=faces_l, textures=TexturesVertex(verts_features=cols_l))
    elev, azim = torch.tensor([10.0, 35.0]), torch.tensor([20.0, -50.0])
    R, T = look_at_view_transform(dist=2.7, elev=elev, azim=azim)
    cameras = FoVPerspectiveCameras(R=R, T=T, znear=1.0, zfar=100.0)
    settings = RasterizationSettings(image_size=40, blur_radius=0.0, faces_per_pixel=4, bin_size=0)
    lights = PointLights(location=((1.5, 2.0, -2.0), (-2.0, 1.0, -1.5)), ambient_color=((0.4, 0.4, 0.4),),
                         diffuse_color=((0.5, 0.4, 0.6),), specular_color=((0.3, 0.3, 0.3),))
    materials = Materials(shininess=24.0)
    blend = BlendParams(sigma=0.5, background_color=(0.2, 0.3, 0.4))
    renderer = MeshRenderer(MeshRasterizer(cameras=cameras, raster_settings=settings),
                            SplatterPhongShader(cameras=cameras, lights=lights, materials=materials, blend_params=blend))
    img = renderer(meshes)
    g = torch.randn(img.shape, generator=gen)
    (img * g).sum().backward()
    out.update({"render_image": img, "render_grad_image": g, "render_verts": meshes.verts_packed(),
                "render_faces": meshes.faces_packed(), "render_verts_colors": torch.cat(cols_l),
                "render_num_verts": torch.tensor([v.shape[0] for v in verts_l]),
                "render_num_faces": torch.tensor([f.shape[0] for f in faces_l]), "render_elev": elev, "render_azim": azim,
                "render_grad_verts": torch.cat([v.grad for v in verts_l]),
                "render_grad_verts_colors": torch.cat([c.grad for c in cols_l])})


def main():
    import make_golden as mg

    mg.bind_reference()
    gen = torch.Generator().manual_seed(2024)
    out = {}
    blend_cases(out, gen)
    render_case(out, gen)
    mg.save("splatter_ref", **out)


if __name__ == "__main__":
    main()
