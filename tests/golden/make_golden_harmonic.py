"""Golden fixture for HarmonicEmbedding and the stratified ray depths, recorded FROM THE REFERENCE on the CPU (build container only).

    python tests/golden/make_golden_harmonic.py   ->  tests/golden/harmonic_ref.npz

Loads the reference's pytorch3d/renderer/implicit/harmonic_embedding.py (pure torch) by path, and takes the one function
`_jiggle_within_stratas` out of its raysampling.py by name (the module itself imports the cameras; the function needs torch alone).
Imports only torch and numpy; nothing of pytorch3d_amd computes anything here.  The inputs are redrawn from seeds by the tests
(tests/harmonic_case.py), so the file holds outputs only:
* <case>/out, grad_x, grad_cov: the TRUTH -- the reference module after `.double()` (its float32 buffers keep their values) on the
  case's float32 inputs in float64, with float64 autograd of the case's seeded gradient into the output;
* E_ref/<pool>/<quantity>: the largest error of the reference's own float32 CPU run against that truth, relative to the case's
  max |truth|, over the cases of one pool (argument class x logspace);
* E_sin, E_exp: the largest error of the reference's float32 CPU output against the argument-exact truth of the case file (sin in
  float64 of the float32 argument; with diag_cov times exp in float64 of the float32 exponent), over all cases without / with diag_cov;
* <special case>/nonfinite_<quantity>: the positions that are not finite in the truth (they are left out of every pool);
* <depth case>/uniforms, depths: the reference's _jiggle_within_stratas on the case's centres and the draw it made (captured by
  seeding: torch.rand_like of a float32 CPU tensor of the same shape under the same seed); for the edge cases the function runs with
  `rand_like` answering the case's uniforms (exactly 0, and the largest float32 below 1).
Asserted here: every pool holds at least 6 cases and no pool is zero; the reference's float32 run has the truth's non-finite slots;
the module's _frequencies equal the case file's bit for bit; the underflow case's factors are exactly 0 somewhere and 1-ish elsewhere.
"""
import ast
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

REFERENCE = os.environ.get("P3D_REFERENCE_ROOT") or os.path.join(ROOT, "oracle", "_ref", "reference_py")  # the staged copy
IMPLICIT = os.path.join(REFERENCE, "pytorch3d", "renderer", "implicit")


def reference_harmonic_embedding():
    spec = importlib.util.spec_from_file_location("p3d_ref_harmonic_embedding", os.path.join(IMPLICIT, "harmonic_embedding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HarmonicEmbedding


def reference_jiggle(torch_module=torch):
    """The reference's _jiggle_within_stratas, compiled from its own source with `torch_module` as its `torch`."""
    path = os.path.join(IMPLICIT, "raysampling.py")
    tree = ast.parse(open(path).read(), path)
    fn = next(node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == "_jiggle_within_stratas")
    space = {"torch": torch_module}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), space)
    return space["_jiggle_within_stratas"]


def main():
    import harmonic_case as C

    Ref = reference_harmonic_embedding()
    out, pools, members = {}, {}, {}
    e_arg = {"sin": 0.0, "exp": 0.0}
    for case in C.cases():
        inp = C.inputs(case)
        module = Ref(case.n, case.omega, case.logspace, case.append)
        if case.freqs == "hand":
            module._frequencies = inp[2].clone()
        assert torch.equal(module._frequencies, inp[2]), case.id

        def make(mod):
            return lambda x, f, cov, append: mod(x, diag_cov=cov)

        f32 = C.run(make(module), case, inp=inp)
        truth = C.run(make(module.double()), case, inp=C.inputs(case, dtype=torch.float64))
        assert module._zero_half_pi.dtype == torch.float64 and float(module._zero_half_pi[1]) == float(C.HALF_PI32)
        which = "exp" if case.cov else "sin"
        e_arg[which] = max(e_arg[which], C.argument_error(case, f32["out"], inp))
        if case.cov == "top":
            e = np.exp(np.float32(-0.5) * (inp[1].numpy()[..., None] * (inp[2].numpy() ** 2)))
            assert (e == 0).any() and e.max() > 0.99, case.id
        for q in C.QUANTITIES:
            if truth[q] is None:
                continue
            out[C.key(case.id, q)] = truth[q]
            finite = np.isfinite(truth[q])
            assert np.array_equal(np.isfinite(f32[q]), finite), (case.id, q)
            if case.special:
                out[C.key(case.id, "nonfinite_" + q)] = ~finite
                assert (~finite).any()
                continue
            assert finite.all(), (case.id, q)
            if truth[q].size == 0:
                continue
            scale = float(np.abs(truth[q]).max())
            assert scale > 0, (case.id, q)
            k = (C.pool(case), q)
            pools[k] = max(pools.get(k, 0.0), float(np.abs(f32[q] - truth[q]).max()) / scale)
        if not case.special and np.prod(case.lead, dtype=np.int64) > 0:
            members[C.pool(case)] = members.get(C.pool(case), 0) + 1
    for name, count in sorted(members.items()):
        assert count >= 6, (name, count)
        print("pool %-12s %2d cases" % (name, count))
    for (name, q), e in sorted(pools.items()):
        assert e > 0, (name, q)
        out[f"E_ref/{name}/{q}"] = np.float64(e)
        print("E_ref %-12s %-9s %.3e" % (name, q, e))
    for which, e in e_arg.items():
        assert e > 0
        out["E_" + which] = np.float64(e)
        print("E_%s %.3e" % (which, e))

    jiggle = reference_jiggle()
    for case in C.depth_cases():
        centers = C.depth_centers(case)
        before = centers.clone()
        if case.edge:
            u = C.edge_uniforms(case)
            proxy = types.SimpleNamespace(Tensor=torch.Tensor, cat=torch.cat, rand_like=lambda t, u=u: u.clone())
            depths = reference_jiggle(proxy)(centers)
        else:
            torch.manual_seed(C.depth_seed(case))
            depths = jiggle(centers)
            torch.manual_seed(C.depth_seed(case))
            u = torch.rand_like(torch.empty((case.rows, case.n)))
        assert torch.equal(centers, before) and depths.shape == centers.shape and depths.dtype == torch.float32
        lo = torch.cat((centers[..., :1], 0.5 * (centers[..., 1:] + centers[..., :-1])), -1)
        hi = torch.cat((0.5 * (centers[..., 1:] + centers[..., :-1]), centers[..., -1:]), -1)
        assert torch.equal(depths, lo + (hi - lo) * u), case.id  # the draw was captured
        out[C.key(case.id, "uniforms")], out[C.key(case.id, "depths")] = u.numpy(), depths.numpy()
    np.savez_compressed(C.FIXTURE, **out)
    print("wrote", C.FIXTURE, os.path.getsize(C.FIXTURE), "bytes;", len(C.cases()), "+", len(C.depth_cases()), "cases")
    assert os.path.getsize(C.FIXTURE) < 2 ** 19


if __name__ == "__main__":
    main()
