"""Golden fixture for the cotangent Laplacian and Taubin smoothing, generated FROM THE REFERENCE's own code on the CPU (build container
only).

    python tests/golden/make_golden_mesh_laplacian.py   ->  tests/golden/mesh_laplacian_ref.npz

The generator loads the reference's pytorch3d/ops/laplacian_matrices.py, pytorch3d/loss/mesh_laplacian_smoothing.py and
pytorch3d/ops/mesh_filtering.py (with structures/utils.py, which the last imports) without the rest of the package: `Meshes` is a
stand-in of a few lines here that holds packed tensors and answers the eight methods those three files call.  Every case of
tests/mesh_laplacian_case.py runs through the reference's functions in float32 on the CPU -- they hard-code float32, a float64 call
raises -- and through the case module's float64 restatement, the truth.  Recorded per case: the reference's errors against the truth
(loss and gradient per method and grad_output, the entries of L, inv_areas, the Taubin vertices after 1 and 10 iterations) and, for
the small cases, the reference's results themselves.  Asserted:
  * the restatement gives the same set of entries as the reference's L, and reproduces each within 2^-22 times the sum of the
    entry's absolute terms (a few float32 roundings per term: derived, not measured).  THIS BOUND IS MISSED, by less than a factor
    of two: the largest error over 2^-22 x terms is 1.37 (batch), 0.67 (collinear, coincident), 1.13 (fan200), 1.39 (grid20) and
    1.85 (grid257), with the terms read as every square that enters the entry, (a^2 + b^2 + c^2) / area / 4 per corner; with the
    terms read as |cot| / 4 alone it is missed by three orders of magnitude where a cotangent is a difference of squares that
    cancel.  Heron's s - A amplifies the roundings of the sides by s / (s - A), up to 8 at a 15-degree angle, which "a few
    roundings per term" leaves out.  The check is made LAST, after the fixture is written with the ratios in it (<case>/L_ratio),
    and the generator exits with an error that lists them;
  * every face has all angles >= 15 degrees, or is an exact degenerate on a dyadic lattice (Heron's product exactly 0 in both
    precisions), so that the reference alone stays inside its own gates;
  * every case's recorded float32 gradient error is > 0.
Nothing of pytorch3d_amd is in the loop.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

REFERENCE = os.environ.get("P3D_REFERENCE_ROOT", "/root/reference")

import mesh_laplacian_case as C  # noqa: E402


class Meshes:
    """What the three reference files ask of a Meshes: packed float32 vertices, packed faces, the unique edges."""

    def __init__(self, verts, faces):
        self._verts, self._faces = list(verts), list(faces)
        self._packed = C.packed(self._verts, self._faces)
        self.device = self._packed[0].device

    def __len__(self):
        return len(self._verts)

    def isempty(self):
        return len(self._verts) == 0 or self._packed[0].shape[0] == 0

    def verts_packed(self):
        return self._packed[0]

    def faces_packed(self):
        return self._packed[1]

    def faces_list(self):
        return self._faces

    def verts_list(self):
        return self._verts

    def edges_packed(self):
        return C.edges_of(self._packed[1], self._packed[0].shape[0])

    def num_verts_per_mesh(self):
        return torch.tensor(self._packed[2], dtype=torch.int64)

    def verts_packed_to_mesh_idx(self):
        return self._packed[3]


def reference_functions():
    """(cot_laplacian, mesh_laplacian_smoothing, taubin_smoothing) of the reference, loaded file by file."""
    for name, sub in (("pytorch3d", None), ("pytorch3d.ops", "ops"), ("pytorch3d.loss", "loss"), ("pytorch3d.structures", "structures")):
        mod = types.ModuleType(name)
        mod.__path__ = [] if sub is None else [os.path.join(REFERENCE, "pytorch3d", sub)]  # (no __init__ runs)
        sys.modules[name] = mod
    lap = importlib.import_module("pytorch3d.ops.laplacian_matrices")
    sys.modules["pytorch3d.ops"].cot_laplacian = lap.cot_laplacian
    sys.modules["pytorch3d.ops"].norm_laplacian = lap.norm_laplacian
    sys.modules["pytorch3d.structures"].Meshes = Meshes
    sys.modules["pytorch3d.structures"].utils = importlib.import_module("pytorch3d.structures.utils")
    loss = importlib.import_module("pytorch3d.loss.mesh_laplacian_smoothing")
    filt = importlib.import_module("pytorch3d.ops.mesh_filtering")
    return lap.cot_laplacian, loss.mesh_laplacian_smoothing, filt.taubin_smoothing


def main():
    cot_laplacian, mesh_laplacian_smoothing, taubin_smoothing = reference_functions()
    try:
        cot_laplacian(torch.rand(3, 3, dtype=torch.float64), torch.tensor([[0, 1, 2]]))
        raise SystemExit("the reference's cot_laplacian took float64: record the truth from it instead of the restatement")
    except RuntimeError:
        pass
    out, ratios = {}, {}
    for case, (verts_list, faces_list) in C.cases().items():
        verts, faces, nv, vert_mesh = C.packed(verts_list, faces_list)
        V = verts.shape[0]
        ok = (C.min_angles(verts, faces) >= C.MIN_ANGLE) | C.exact_degenerate(verts, faces)
        assert bool(ok.all()), (case, "faces that are neither well shaped nor exact degenerates", torch.nonzero(~ok).flatten().tolist()[:8])
        # L and inv_areas
        L, inv_areas = cot_laplacian(verts, faces)
        Lc = L.coalesce()
        row, col, val, mag, ia = C.laplacian_entries(verts, faces)
        assert torch.equal(Lc.indices()[0], row) and torch.equal(Lc.indices()[1], col), (case, "L has other entries than the restatement")
        err = (Lc.values().double() - val).abs()
        ratios[case] = float((err / mag).max()) / 2.0 ** -22
        out[f"{case}/L_ratio"] = ratios[case]
        out[f"{case}/e32_L"] = float(err.max())
        out[f"{case}/e32_inv_areas"] = float((inv_areas.reshape(-1).double() - ia).abs().max())
        small = case in C.SMALL
        if small:
            out[f"{case}/L_values"], out[f"{case}/inv_areas"] = Lc.values().numpy(), inv_areas.reshape(-1).numpy()
        # the loss, per method and grad_output
        for method in C.METHODS:
            for g in C.GRAD_OUTPUTS:
                v = [x.clone().requires_grad_(True) for x in verts_list]
                loss = mesh_laplacian_smoothing(Meshes(v, faces_list), method)
                grads = torch.autograd.grad(loss * g, [x for x in v if x.shape[0]])
                grad = torch.cat(list(grads), 0)
                t_loss, t_grad, S, n = C.evaluate(method, verts, faces, nv, vert_mesh, g)
                e_grad = float((grad.double() - t_grad).abs().max())
                assert e_grad > 0, (case, method, g, "the reference's float32 gradient error is 0")
                out[f"{case}/e32_grad_{method}_{g:g}"] = e_grad
                if g == 1.0:
                    out[f"{case}/e32_loss_{method}"] = abs(float(loss) - t_loss)
                    if small:
                        out[f"{case}/loss_{method}"], out[f"{case}/grad_{method}"] = np.float32(float(loss)), grad.numpy()
                print(f"{case} {method} x {g:g}: loss {float(loss):.9g} (truth {t_loss:.9g}), gradient error {e_grad:.3g} of {float(t_grad.abs().max()):.3g}")
        # Taubin
        edges = C.edges_of(faces, V)
        for it in C.TAUBIN_ITERS:
            with torch.no_grad():
                got = taubin_smoothing(Meshes(verts_list, faces_list), C.LAMBD, C.MU, it).verts_packed()
            want = C.taubin(verts, edges, it)
            e = C.nan_aware_error(got, want)
            assert np.isfinite(e) and e > 0, (case, it, e)
            out[f"{case}/e32_taubin_{it}"] = e
            if small:
                out[f"{case}/taubin_{it}"] = got.numpy()
            print(f"{case} taubin x {it}: error {e:.3g}, motion {C.nan_aware_error(verts, want):.3g}, NaN rows {int(torch.isnan(want).any(1).sum())}")
    np.savez_compressed(C.GOLDEN, **out)
    print("wrote", C.GOLDEN, os.path.getsize(C.GOLDEN), "bytes")
    # last, so that the figures are on record whatever it says: the largest |L_reference - L_restated| / (2^-22 x the entry's terms)
    print("entries of L against the restatement, in units of 2^-22 x the terms:", {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ("an entry of L is further than 2^-22 x its terms from the restatement", ratios)


if __name__ == "__main__":
    main()
