#!/usr/bin/env python
"""The UNMODIFIED reference's pytorch3d.renderer.implicit through pytorch3d_amd.shim on the GPU, in a process of its own (the shim
replaces sys.modules entries).  Prints one JSON line; tests/test_gpu_implicit.py reads it.

* plain install(): the reference's sample_pdf (its Python function over `_C.sample_pdf`) on GPU and on CPU tensors, against the fixture;
* patch_python=True: ImplicitRenderer(MonteCarloRaysampler, EmissionAbsorptionRaymarcher) with a tiny seeded volumetric function,
  forward and backward, patched and with the originals restored: fused calls counted, images and parameter gradients compared.
  The gate of the images is the raymarch gate of the features, 4 E_ref max|images|; a parameter gradient is a linear map of
  (grad_densities, grad_features), so its gate is 4 (E_ref[grad_densities] + E_ref[grad_features]) max|gradient|;
* a CPU call is a fallback; the bounds warning is kept; uninstall_python_patches() restores the two methods."""
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

EA, AO = "EmissionAbsorptionRaymarcher.forward", "AbsorptionOnlyRaymarcher.forward"


def _reference_root():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    return next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage)
                 if c and os.path.isdir(os.path.join(c, "pytorch3d", "renderer", "implicit"))), None)


def report(ref_root):
    import torch

    import implicit_case as C
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    d = torch.device("cuda:0")
    out = {}

    # ---- install() alone: the reference's own sample_pdf -------------------------------------------------------------------------
    shim.install(ref_root)
    from pytorch3d.renderer.implicit.sample_pdf import sample_pdf

    case = next(c for c in C.pdf_cases() if c[0] == "special-det")
    bins, weights, _, eps = C.pdf_inputs(case)
    want = C.fixture()["pdf/special-det"]
    on_gpu = sample_pdf(bins.to(d), weights.to(d), case[4], det=True, eps=eps)
    on_cpu = sample_pdf(bins, weights, case[4], det=True, eps=eps)
    out["install_alone"] = {"gpu_bit_equal": on_gpu.is_cuda and C.same_bits(on_gpu.cpu().numpy(), want), "cpu_bit_equal": C.same_bits(on_cpu.numpy(), want),
                            "gpu_equals_cpu": bool(torch.equal(on_gpu.cpu(), on_cpu))}

    # ---- patch_python=True -------------------------------------------------------------------------------------------------------
    shim.install(ref_root, patch_python=True)
    from pytorch3d.renderer import FoVPerspectiveCameras, ImplicitRenderer, MonteCarloRaysampler, look_at_view_transform
    from pytorch3d.renderer.implicit import raymarching
    from pytorch3d.renderer.implicit.utils import ray_bundle_to_ray_points

    ea_cls, ao_cls = raymarching.EmissionAbsorptionRaymarcher, raymarching.AbsorptionOnlyRaymarcher
    patched = (ea_cls.forward, ao_cls.forward)
    out["patched"] = {"ea": bool(getattr(ea_cls.forward, "__p3d_amd__", False)), "ao": bool(getattr(ao_cls.forward, "__p3d_amd__", False))}

    def calls():
        return {n: list(shim.PATCH_CALLS.get(n, [0, 0])) for n in (EA, AO)}

    gen = torch.Generator().manual_seed(11)
    params = [torch.tensor([0.1, -0.2, 0.05]), torch.tensor(1.5), 0.5 * torch.randn(3, 3, generator=gen)]
    R, T = look_at_view_transform(dist=3.0, elev=(10.0, 40.0), azim=(20.0, 200.0))
    cameras = FoVPerspectiveCameras(R=R, T=T, device=d)
    renderer = ImplicitRenderer(raysampler=MonteCarloRaysampler(-1.0, 1.0, -1.0, 1.0, n_rays_per_image=96, n_pts_per_ray=48, min_depth=1.5, max_depth=4.5),
                                raymarcher=ea_cls())
    target = torch.rand(2, 96, 4, generator=gen).to(d)

    def run():
        centre, sharp, mix = (p.clone().to(d).requires_grad_(True) for p in params)

        def volume(ray_bundle, **kwargs):
            x = ray_bundle_to_ray_points(ray_bundle)
            density = 1.0 - torch.exp(-torch.nn.functional.softplus(sharp) * torch.exp(-((x - centre) ** 2).sum(-1, keepdim=True)))
            return density, torch.sigmoid(x @ mix)

        torch.manual_seed(3)  # the Monte Carlo rays: the same draws on both sides
        images, _ = renderer(cameras=cameras, volumetric_function=volume)
        loss = ((images - target.reshape(images.shape)) ** 2).mean()
        grads = torch.autograd.grad(loss, (centre, sharp, mix))
        torch.cuda.synchronize()
        return images.detach().cpu().double(), torch.cat([g.reshape(-1) for g in grads]).cpu().double()

    before = calls()
    img_p, grad_p = run()
    after = calls()
    ea_cls.forward, ao_cls.forward = patched[0].__wrapped__, patched[1].__wrapped__
    try:
        img_o, grad_o = run()
    finally:
        ea_cls.forward, ao_cls.forward = patched
    out["renderer"] = {"fused_calls": after[EA][0] - before[EA][0], "fallback_calls": after[EA][1] - before[EA][1],
                       "fused_calls_when_restored": calls()[EA][0] - after[EA][0],
                       "finite": bool(torch.isfinite(img_p).all() and torch.isfinite(grad_p).all()),
                       "images_difference": float((img_p - img_o).abs().max()), "images_gate": C.GATE_FACTOR * C.e_ref("features") * float(img_o.abs().max()),
                       "grad_params_difference": float((grad_p - grad_o).abs().max()),
                       "grad_params_gate": C.GATE_FACTOR * (C.e_ref("grad_densities") + C.e_ref("grad_features")) * float(grad_o.abs().max())}

    # ---- a CPU call is a fallback; the warning stays -------------------------------------------------------------------------------
    before = calls()
    dens, feats = torch.rand(4, 6, 1), torch.rand(4, 6, 3)
    ea_cls()(dens, feats)
    ao_cls()(dens)
    after = calls()
    out["cpu_call"] = {"fused": sum(after[n][0] - before[n][0] for n in (EA, AO)), "fallback": sum(after[n][1] - before[n][1] for n in (EA, AO))}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        ea_cls()((1.5 * dens).to(d), feats.to(d))
    out["warning_kept"] = any("outside of valid" in str(w.message) for w in caught)

    shim.uninstall_python_patches()
    out["restored"] = ea_cls.forward is patched[0].__wrapped__ and ao_cls.forward is patched[1].__wrapped__
    print(json.dumps(out))


def main():
    ref_root = _reference_root()
    if ref_root is None:
        print(json.dumps({"skipped": "the reference's Python package is not on this machine"}))
        return
    report(ref_root)


if __name__ == "__main__":
    main()
