#!/usr/bin/env python
"""The UNMODIFIED reference's VolumeRenderer through pytorch3d_amd.shim on the GPU, in a process of its own (the shim replaces
sys.modules entries).  Prints one JSON line; tests/test_gpu_volume_sampler.py reads it.

* plain install() leaves VolumeSampler.forward alone; patch_python=True patches it;
* VolumeRenderer(NDCMultinomialRaysampler (8 x 8 rays, 20 points), EmissionAbsorptionRaymarcher) over a 6 x 7 x 8 Volumes with a
  non-zero translation and voxel size whose densities, features and translation require grad, forward and backward, patched and
  with the reference's methods restored (the sampler's and the raymarcher's): fused calls counted, images and gradients compared.
  Gates: the images within 4 E_ref max|images| with the smaller of the sampler's and the marcher's E_ref of the features; a volume
  gradient is the sampler's backward of the marcher's, so its gate is the sum of the two, 4 (E_sampler + E_marcher) max|gradient|;
  the translation's gradient comes through grad_origins, gated alike;
* under torch.use_deterministic_algorithms(True) the patched renderer takes the ordered backward and gives the same bits twice;
* a CPU call and a `reflection` call are fallbacks; uninstall_python_patches() restores the method."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VS = "VolumeSampler.forward"


def _reference_root():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    return next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage)
                 if c and os.path.isdir(os.path.join(c, "pytorch3d", "renderer", "implicit"))), None)


def report(ref_root):
    import torch

    import implicit_case as IC
    import run_reference_suite as rrs
    import volume_sampler_case as C

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim
    from pytorch3d_amd import _C

    d = torch.device("cuda:0")
    out = {}
    shim.install(ref_root)
    from pytorch3d.renderer.implicit import raymarching
    from pytorch3d.renderer.implicit import renderer as ref_renderer

    out["not_patched_by_plain_install"] = not getattr(ref_renderer.VolumeSampler.forward, "__p3d_amd__", False)
    shim.install(ref_root, patch_python=True)
    from pytorch3d.renderer import FoVPerspectiveCameras, NDCMultinomialRaysampler, VolumeRenderer, look_at_view_transform
    from pytorch3d.renderer.implicit.utils import RayBundle
    from pytorch3d.structures import Volumes

    vs_cls, ea_cls = ref_renderer.VolumeSampler, raymarching.EmissionAbsorptionRaymarcher
    patched_vs, patched_ea = vs_cls.forward, ea_cls.forward
    out["patched"] = bool(getattr(patched_vs, "__p3d_amd__", False)) and patched_vs.__wrapped__ is not patched_vs

    def calls():
        return list(shim.PATCH_CALLS.get(VS, [0, 0]))

    gen = torch.Generator().manual_seed(17)
    D, H, W = C.WORLD_GRID
    params = [torch.rand((2, 1, D, H, W), generator=gen), torch.rand((2, 3, D, H, W), generator=gen), torch.tensor([C.WORLD_TRANSLATION] * 2)]
    R, T = look_at_view_transform(dist=3.0, elev=(10.0, 40.0), azim=(20.0, 200.0))
    cameras = FoVPerspectiveCameras(R=R, T=T, device=d)
    renderer = VolumeRenderer(raysampler=NDCMultinomialRaysampler(image_width=8, image_height=8, n_pts_per_ray=20, min_depth=1.5, max_depth=4.5),
                              raymarcher=ea_cls())
    target = torch.rand(2, 8, 8, 4, generator=gen).to(d)

    def run():
        dens, feats, trans = (p.clone().to(d).requires_grad_(True) for p in params)
        volumes = Volumes(densities=dens, features=feats, voxel_size=C.WORLD_VOXEL_SIZE[0], volume_translation=trans)
        images, _ = renderer(cameras=cameras, volumes=volumes)
        loss = ((images - target) ** 2).mean()
        gd, gf, gt = torch.autograd.grad(loss, (dens, feats, trans))
        torch.cuda.synchronize()
        return images.detach().cpu().double(), gd.cpu().double(), gf.cpu().double(), gt.cpu().double()

    before = calls()
    img_p, gd_p, gf_p, gt_p = run()
    after = calls()
    vs_cls.forward, ea_cls.forward = patched_vs.__wrapped__, patched_ea.__wrapped__
    try:
        img_o, gd_o, gf_o, gt_o = run()
    finally:
        vs_cls.forward, ea_cls.forward = patched_vs, patched_ea
    e_img = min(C.e_ref("rays_features"), IC.e_ref("features"))
    marcher = IC.e_ref("grad_densities") + IC.e_ref("grad_features")
    out["renderer"] = {
        "fused_calls": after[0] - before[0], "fallback_calls": after[1] - before[1], "fused_calls_when_restored": calls()[0] - after[0],
        "finite": bool(all(torch.isfinite(t).all() for t in (img_p, gd_p, gf_p, gt_p))),
        "images_difference": float((img_p - img_o).abs().max()), "images_gate": C.GATE_FACTOR * e_img * float(img_o.abs().max()),
        "grad_volumes_difference": max(float((gd_p - gd_o).abs().max()) / float(gd_o.abs().max()), float((gf_p - gf_o).abs().max()) / float(gf_o.abs().max())),
        "grad_volumes_gate": C.GATE_FACTOR * (min(C.e_ref("grad_densities"), C.e_ref("grad_features")) + marcher),
        "grad_volumes_max": min(float(gd_o.abs().max()), float(gf_o.abs().max())),
        "grad_pose_difference": float((gt_p - gt_o).abs().max()), "grad_pose_max": float(gt_o.abs().max()),
        "grad_pose_gate": C.GATE_FACTOR * (C.e_ref("grad_origins") + marcher) * float(gt_o.abs().max())}

    # ---- the strict deterministic flag: the ordered backward, the same bits twice ----------------------------------------------------
    before, ordered_before = calls(), _C.VOLUME_SAMPLE_CALLS["ordered"]
    torch.use_deterministic_algorithms(True)
    try:
        a = run()
        mid = calls()
        b = run()
        out["deterministic"] = {"fused_calls": mid[0] - before[0], "ordered_calls": (_C.VOLUME_SAMPLE_CALLS["ordered"] - ordered_before) // 2,
                                "same_bits": bool(all(torch.equal(x, y) for x, y in zip(a, b)))}
    except RuntimeError as e:
        out["deterministic"] = {"fused_calls": 0, "ordered_calls": 0, "same_bits": False, "error": str(e)[:300]}
    finally:
        torch.use_deterministic_algorithms(False)

    # ---- a CPU call and a reflection call are fallbacks -------------------------------------------------------------------------------
    def sampler_call(device, padding_mode):
        before = calls()
        volumes = Volumes(densities=params[0].to(device), features=params[1].to(device), voxel_size=0.4)
        o = torch.rand(2, 5, 3, generator=gen).to(device) - 0.5
        rd, rf = vs_cls(volumes, padding_mode=padding_mode)(RayBundle(o, torch.nn.functional.normalize(o + 0.3, dim=-1), torch.rand(2, 5, 6, generator=gen).to(device), None))
        assert rd.shape == (2, 5, 6, 1) and rf.shape == (2, 5, 6, 3)
        after = calls()
        return {"fused": after[0] - before[0], "fallback": after[1] - before[1]}

    out["cpu_call"] = sampler_call("cpu", "zeros")
    out["reflection_call"] = sampler_call(d, "reflection")

    shim.uninstall_python_patches()
    out["restored"] = vs_cls.forward is patched_vs.__wrapped__
    print(json.dumps(out))


def main():
    ref_root = _reference_root()
    if ref_root is None:
        print(json.dumps({"skipped": "the reference's Python package is not on this machine"}))
        return
    report(ref_root)


if __name__ == "__main__":
    main()
