#!/usr/bin/env python
"""The UNMODIFIED reference's HarmonicEmbedding and ray samplers through pytorch3d_amd.shim on the GPU, in a process of its own (the
shim replaces sys.modules entries).  Prints one JSON line; tests/test_gpu_harmonic.py reads it.

* plain install() leaves HarmonicEmbedding.forward and _jiggle_within_stratas alone; patch_python=True patches both;
* HarmonicEmbedding(10) and HarmonicEmbedding(4, append_input=False) of the reference on GPU tensors: one fused call each, no
  fallback, output and x.grad within gate 2 (the small-log pool of tests/harmonic_case.py: x in [-1, 1], logspace) of the float64
  restatement -- the reference's own forward on a `.double()` copy of the module;
* NDCMultinomialRaysampler and MonteCarloRaysampler with stratified_sampling=True: `lengths` bit-equal to the unpatched run under
  the same seed, one fused call each; without stratification `lengths` is still a stride-0 view;
* a CPU call and a float64 call of either are fallbacks; uninstall_python_patches() restores both, and a plain install() afterwards
  patches neither."""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HE, JG = "HarmonicEmbedding.forward", "_jiggle_within_stratas"


def _reference_root():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    return next((c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage)
                 if c and os.path.isdir(os.path.join(c, "pytorch3d", "renderer", "implicit"))), None)


def report(ref_root):
    import torch

    import harmonic_case as C
    import run_reference_suite as rrs

    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    d = torch.device("cuda:0")
    out = {}
    shim.install(ref_root)
    from pytorch3d.renderer.implicit import harmonic_embedding as ref_he
    from pytorch3d.renderer.implicit import raysampling as ref_rs

    own_forward, own_jiggle = ref_he.HarmonicEmbedding.forward, ref_rs._jiggle_within_stratas
    out["not_patched_by_plain_install"] = not getattr(own_forward, "__p3d_amd__", False) and not getattr(own_jiggle, "__p3d_amd__", False)
    shim.install(ref_root, patch_python=True)
    from pytorch3d.renderer import FoVPerspectiveCameras, MonteCarloRaysampler, NDCMultinomialRaysampler, look_at_view_transform

    patched_forward, patched_jiggle = ref_he.HarmonicEmbedding.forward, ref_rs._jiggle_within_stratas
    out["patched"] = (bool(getattr(patched_forward, "__p3d_amd__", False)) and patched_forward.__wrapped__ is own_forward
                      and bool(getattr(patched_jiggle, "__p3d_amd__", False)) and patched_jiggle.__wrapped__ is own_jiggle)

    def calls(name):
        return list(shim.PATCH_CALLS.get(name, [0, 0]))

    def delta(name, before):
        after = calls(name)
        return {"fused": after[0] - before[0], "fallback": after[1] - before[1]}

    # ---- the embedding ------------------------------------------------------------------------------------------------------------------
    gen = torch.Generator().manual_seed(C.SEED + 901)
    pool = C.case_by_id("small-d3-n10-r5-a1")  # x in [-1, 1], logspace: the pool whose E_ref gates these two modules
    for name, module in (("embedding_10", ref_he.HarmonicEmbedding(10)), ("embedding_4_no_append", ref_he.HarmonicEmbedding(4, append_input=False))):
        x = (2 * torch.rand((64, 16, 3), generator=gen) - 1).to(d).requires_grad_(True)
        module = module.to(d)
        g = torch.randn((64, 16, module.get_output_dim(3)), generator=gen).to(d)
        before = calls(HE)
        got = module(x)
        (gx,) = torch.autograd.grad(got, x, g)
        counted = delta(HE, before)
        xd = x.detach().double().requires_grad_(True)
        truth = own_forward(copy.deepcopy(module).double(), xd)
        (tgx,) = torch.autograd.grad(truth, xd, g.double())
        out[name] = {"fused_calls": counted["fused"], "fallback_calls": counted["fallback"],
                     "out_difference": float((got.double() - truth).abs().max()),
                     "out_gate": C.GATE_FACTOR * C.e_ref(pool, "out") * float(truth.abs().max()),
                     "grad_difference": float((gx.double() - tgx).abs().max()), "grad_max": float(tgx.abs().max()),
                     "grad_gate": C.GATE_FACTOR * C.e_ref(pool, "grad_x") * float(tgx.abs().max())}
    module = ref_he.HarmonicEmbedding(6)
    before = calls(HE)
    module(torch.rand(5, 3))
    out["cpu_embedding"] = delta(HE, before)
    before = calls(HE)
    copy.deepcopy(module).double().to(d)(torch.rand(5, 3, dtype=torch.float64, device=d))
    out["float64_embedding"] = delta(HE, before)

    # ---- the stratified depths of two ray samplers ----------------------------------------------------------------------------------------
    R, T = look_at_view_transform(dist=3.0, elev=(10.0, 40.0), azim=(20.0, 200.0))
    cameras = FoVPerspectiveCameras(R=R, T=T, device=d)
    samplers = {"ndc_multinomial": NDCMultinomialRaysampler(image_width=9, image_height=7, n_pts_per_ray=20, min_depth=0.5, max_depth=4.0,
                                                            stratified_sampling=True),
                "monte_carlo": MonteCarloRaysampler(-1.0, 1.0, -1.0, 1.0, 33, 65, 0.5, 4.0, stratified_sampling=True)}
    for name, sampler in samplers.items():
        before = calls(JG)
        torch.manual_seed(31)
        ours = sampler(cameras).lengths
        counted = delta(JG, before)
        ref_rs._jiggle_within_stratas = own_jiggle
        try:
            torch.manual_seed(31)
            theirs = sampler(cameras).lengths
            plain = sampler(cameras, stratified_sampling=False).lengths
        finally:
            ref_rs._jiggle_within_stratas = patched_jiggle
        out[name] = {"same_bits": bool(torch.equal(ours, theirs)) and ours.shape == theirs.shape, "fused_calls": counted["fused"],
                     "fallback_calls": counted["fallback"], "jiggled": not bool(torch.equal(ours, plain))}
    plain = samplers["ndc_multinomial"](cameras, stratified_sampling=False).lengths  # patched: nothing of it is touched
    out["lengths_without_stratification_stride"] = max(plain.stride()[:-1])
    centers = torch.linspace(0.5, 4.0, 8)[None].expand(3, 8)
    before = calls(JG)
    ref_rs._jiggle_within_stratas(centers)
    out["cpu_depths"] = delta(JG, before)
    before = calls(JG)
    ref_rs._jiggle_within_stratas(centers.double().to(d))
    out["float64_depths"] = delta(JG, before)

    shim.uninstall_python_patches()
    out["restored"] = ref_he.HarmonicEmbedding.forward is own_forward and ref_rs._jiggle_within_stratas is own_jiggle
    shim.install(ref_root)
    out["plain_install_after_restore_patches_neither"] = (ref_he.HarmonicEmbedding.forward is own_forward
                                                          and ref_rs._jiggle_within_stratas is own_jiggle)
    print(json.dumps(out))


def main():
    ref_root = _reference_root()
    if ref_root is None:
        print(json.dumps({"skipped": "the reference's Python package is not on this machine"}))
        return
    report(ref_root)


if __name__ == "__main__":
    main()
