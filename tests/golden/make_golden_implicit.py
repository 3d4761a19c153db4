"""Golden fixture for sample_pdf and the raymarchers, generated FROM THE REFERENCE (build container only).

    python tests/golden/make_golden_implicit.py   ->  tests/golden/implicit_ref.npz

The generator compiles the reference's csrc/sample_pdf/sample_pdf_cpu.cpp with a binding of a few lines (BINDING below, the
generator's own) through torch.utils.cpp_extension.load into a build directory OUTSIDE the repository, and loads the reference's
pytorch3d/renderer/implicit/raymarching.py (pure torch) by path.  It records, for the cases of tests/implicit_case.py,
* pdf/<case>: the samples the compiled operator writes over the case's uniforms;
* <case>/features, opacities, grad_densities, grad_features (and weights where the case returns them): the float64 outputs and
  autograd gradients of the reference's EmissionAbsorptionRaymarcher, the truth.  The weights are the reference's own expression,
  rays_densities * _shifted_cumprod((1 + eps) - rays_densities, shift), with the case's gradient into them added to the loss;
* E_ref/<quantity>: the largest error of the reference's float32 CPU run against the truth over all cases, relative to the case's
  largest |truth|;
* broken_f32: the ids of the cases whose float32 reference run is not finite (left out of E_ref), joined by newlines.
Nothing of pytorch3d_amd is in the loop; the inputs are redrawn from seeds by the tests, so the file holds outputs only.

Asserted here: where a quantity's truth is all zeros (a ray of one point of density 0) the float32 run gives exact zeros too; the case
at 1.5 raises the reference's bounds warning and no other case does; the AbsorptionOnlyRaymarcher's opacity equals the last channel.
"""
import importlib.util
import os
import sys
import tempfile
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

REFERENCE = os.environ.get("P3D_REFERENCE_ROOT", "/root/reference")

BINDING = """
#include <torch/extension.h>
void SamplePdfCpu(const torch::Tensor& bins, const torch::Tensor& weights, const torch::Tensor& outputs, float eps);
PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) { m.def("sample_pdf", &SamplePdfCpu); }
"""


def reference_sample_pdf():
    from torch.utils.cpp_extension import load

    build_dir = os.path.join(tempfile.gettempdir(), "p3d_ref_sample_pdf")
    os.makedirs(build_dir, exist_ok=True)
    binding = os.path.join(build_dir, "binding.cpp")
    with open(binding, "w") as f:
        f.write(BINDING)
    csrc = os.path.join(REFERENCE, "pytorch3d", "csrc")
    # (-ffp-contract=off: the operator's expressions as written, the contract include/p3d_amd.h states; x86-64 has no FMA without -march)
    return load(name="p3d_ref_sample_pdf", sources=[os.path.join(csrc, "sample_pdf", "sample_pdf_cpu.cpp"), binding],
                extra_include_paths=[csrc], build_directory=build_dir, extra_cflags=["-O2", "-ffp-contract=off"], verbose=False).sample_pdf


def reference_raymarching():
    spec = importlib.util.spec_from_file_location("p3d_ref_raymarching", os.path.join(REFERENCE, "pytorch3d", "renderer", "implicit", "raymarching.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import implicit_case as C

    out = {}
    op = reference_sample_pdf()
    for case in C.pdf_cases():
        bins, weights, u, eps = C.pdf_inputs(case)
        samples = u.clone()
        op(bins, weights, samples, eps)
        out["pdf/" + case[0]] = samples.numpy()
        if case[2] <= 8 and case[3] <= 65:  # the numpy restatement the CPU tests derive their wrong variants from agrees with the operator
            assert C.same_bits(C.pdf_numpy(bins, weights, u, eps), samples.numpy()), case[0]
    print("sample_pdf:", len(C.pdf_cases()), "cases")

    ref = reference_raymarching()

    def reference_fn(d, f, eps, s, rw):
        res = ref.EmissionAbsorptionRaymarcher(surface_thickness=s)(d, f, eps=eps)
        if not rw:
            return res
        return res, d[..., 0] * ref._shifted_cumprod((1.0 + eps) - d[..., 0], shift=s)

    worst, broken = {q: 0.0 for q in C.QUANTITIES}, []
    for case in C.ray_cases():
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            truth = C.run_ray(reference_fn, case, dtype=torch.float64)
            f32 = C.run_ray(reference_fn, case, dtype=torch.float32)
        assert bool(caught) == (case[5] == "over"), (case[0], [str(w.message) for w in caught])
        d = C.ray_inputs(case)[0]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ao = ref.AbsorptionOnlyRaymarcher()(d.double()).numpy()
        assert np.array_equal(ao, truth["opacities"]), case[0]
        fine = all(np.isfinite(v).all() for v in f32.values() if v is not None)
        if not fine:
            broken.append(case[0])
        for q in C.QUANTITIES:
            if truth[q] is None:
                continue
            scale = float(np.abs(truth[q]).max())
            assert np.isfinite(truth[q]).all(), (case[0], q)
            out[C.key(case[0], q)] = truth[q]
            if fine and scale == 0.0:  # (a ray of one point of density 0: exact zeros, which the gate 4 E_ref * 0 then asks for)
                assert not f32[q].any(), (case[0], q)
            elif fine:
                worst[q] = max(worst[q], float(np.abs(f32[q] - truth[q]).max()) / scale)
    for q in C.QUANTITIES:
        out["E_ref/" + q] = np.float64(worst[q])
        print("E_ref %-15s %.3e" % (q, worst[q]))
    out["broken_f32"] = np.array("\n".join(broken))
    print("raymarching:", len(C.ray_cases()), "cases;", "float32 reference run not finite on:", broken or "none")
    np.savez_compressed(C.FIXTURE, **out)
    print("wrote", C.FIXTURE, os.path.getsize(C.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
