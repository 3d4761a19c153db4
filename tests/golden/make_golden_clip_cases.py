"""Golden fixture of the clipping cases, recorded FROM THE REFERENCE's own clip.py on the CPU (build container only).

    python tests/golden/make_golden_clip_cases.py   ->  tests/golden/clip_cases_ref.npz

Imports the unmodified reference package as make_golden_clip.py does (make_golden.bind_reference: its Python with pytorch3d._C bound
to its own CPU kernels).  Nothing of pytorch3d_amd computes anything here; the inputs are redrawn from seeds by the tests
(tests/clip_case.py, which also says what the file holds and why only some rows of the large quantities).
* TRUTH: the reference's clip_faces and convert_clipped_rasterization_to_original_faces in float64 -- inputs cast to double and
  torch.set_default_dtype(torch.float64) around each call, because their internal torch.zeros take the default dtype.
* E_ref/<quantity>: the same calls in float32 against that truth, over every row of every case.
* A mesh with first[n] == F (an empty mesh at the end) makes the reference index out of range; it is run without those meshes and
  (F_clipped, 0) is recorded for them -- what dst[F] = F_clipped gives.
Asserted here: float32 and float64 give the same index tables on every case; every gated truth is finite; a row whose truth is zero
is zero in float32; the onplane cases are exact (float32 == float64 bit for bit, gradients included); the case file's restatement in
float64 equals the truth to 1e-12 of each row's scale on ALL rows (the tests can re-check only the rows held).
"""
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))


@contextlib.contextmanager
def default_dtype(dtype):
    before = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(before)


def main():
    import clip_case as C
    import make_golden as mg

    mg.bind_reference()
    torch.set_num_threads(1)  # the reference's float32 sums in one order, so that E_ref is the same number on every run
    from pytorch3d.renderer.mesh import clip as ref
    from pytorch3d.renderer.mesh.rasterize_meshes import rasterize_meshes
    from pytorch3d.structures import Meshes

    def clip_faces(fv, first, count, fr):
        F = fv.shape[0]
        n = int((first < F).sum()) if F else first.numel()
        assert bool((first[n:] == F).all()) and bool((count[n:] == 0).all())
        with default_dtype(fv.dtype):
            cf = ref.clip_faces(fv, first[:n], count[:n], fr)
        if n < first.numel() and cf.faces_clipped_to_unclipped_idx is not None:
            pad = first.numel() - n
            cf.mesh_to_face_first_idx = torch.cat([cf.mesh_to_face_first_idx, torch.full((pad,), cf.face_verts.shape[0], dtype=torch.int64)])
            cf.num_faces_per_mesh = torch.cat([cf.num_faces_per_mesh, torch.zeros(pad, dtype=torch.int64)])
        return cf

    def convert(p2f, bary, cf):
        with default_dtype(bary.dtype):
            return ref.convert_clipped_rasterization_to_original_faces(p2f, bary, cf)

    impl = C.Impl(clip_faces, convert, ref.ClipFrustum, ref.ClippedFaces)
    out, worst = {}, {q: 0.0 for q in C.BLOCK_QUANTITIES + C.SAMPLE_QUANTITIES}

    def record(case, truth, f32, mine):
        for name in C.int_quantities(case):
            assert (truth[name] is None) == (f32[name] is None) == (mine[name] is None), (case.id, name)
            if truth[name] is not None:
                assert np.array_equal(truth[name], f32[name]) and np.array_equal(truth[name], mine[name]), (case.id, name)
                out[C.key(case.id, name)] = truth[name].astype(np.int32)
        for q in C.float_quantities(case):
            if truth[q] is None:
                assert f32[q] is None and mine[q] is None, (case.id, q)
                continue
            name = q.split("/")[0]
            if q in C.SAMPLE_QUANTITIES:
                assert np.isfinite(truth[q]).all()
                scale = float(np.abs(truth[q]).max())
                worst[name] = max(worst[name], float(np.abs(f32[q] - truth[q]).max()) / scale)
                assert float(np.abs(mine[q] - truth[q]).max()) <= 1e-12 * scale, (case.id, q)
            else:
                ok = C.gated_rows(case, q, truth)
                t, a, m = truth[q][ok], f32[q][ok], mine[q][ok]
                assert np.isfinite(t).all(), (case.id, q)
                scale = C.row_scale(t)
                err = C.row_max(np.abs(a - t))
                assert not err[scale == 0.0].any(), (case.id, q)
                if (scale > 0).any():
                    worst[name] = max(worst[name], float((err[scale > 0] / scale[scale > 0]).max()))
                assert (C.row_max(np.abs(m - t)) <= 1e-12 * scale).all(), (case.id, q)
                if isinstance(case, C.Case) and case.kind == "onplane":
                    assert np.array_equal(a, t), (case.id, q)  # exact arithmetic
            out[C.key(case.id, q)] = truth[q][C.held(truth[q].shape[0])]

    for case in C.cases():
        truth = C.run_clip(impl, case, dtype=torch.float64)
        record(case, truth, C.run_clip(impl, case), C.run_clip(C.torch_impl(), case, dtype=torch.float64))
        if case.kind == "onplane":
            f32 = C.run_clip(impl, case)
            out[C.key(case.id, "f32_face_verts")] = f32["face_verts"].astype(np.float32)
            out[C.key(case.id, "f32_barycentric_conversion")] = f32["barycentric_conversion"].astype(np.float32)
    np.savez_compressed(C.FIXTURE, **out)  # the convert inputs are drawn from the tables just recorded
    C.fixture.cache_clear()
    for case in C.convert_cases():
        truth = C.run_convert(impl, case, dtype=torch.float64)
        record(case, truth, C.run_convert(impl, case), C.run_convert(C.torch_impl(), case, dtype=torch.float64))

    # ---- the pipeline scenes: the reference's rasterize_meshes on its CPU kernels, and its own residual of the invariant ---------------
    for tag, persp in C.PIPELINE.items():
        verts, faces = C.pipeline_scene(tag)
        p2f, zbuf, bary, dists = rasterize_meshes(Meshes(verts=[verts], faces=[faces]), image_size=C.PIPELINE_IMAGE, blur_radius=0.0,
                                                  faces_per_pixel=C.PIPELINE_K, bin_size=0, perspective_correct=persp,
                                                  clip_barycentric_coords=False, z_clip_value=C.PIPELINE_Z_CLIP, cull_to_frustum=True)
        xy, z, n = C.pipeline_residual(verts, faces, p2f, zbuf, bary, persp)
        assert n > 100 and xy < 1e-5 and z < 1e-5, (tag, n, xy, z)
        clipped = ref.clip_faces(verts[faces], torch.tensor([0]), torch.tensor([12]),
                                 ref.ClipFrustum(z_clip_value=C.PIPELINE_Z_CLIP, perspective_correct=persp, **C.BOX))
        assert clipped.barycentric_conversion.shape[0] == 8 * 2 + 4  # every face crosses the plane
        print("pipeline %-10s fragments %d residual xy %.3e z %.3e" % (tag, n, xy, z))
        out.update({C.key(tag, "pix_to_face"): p2f.numpy().astype(np.int32), C.key(tag, "zbuf"): zbuf.numpy(), C.key(tag, "bary"): bary.numpy(),
                    C.key(tag, "dists"): dists.numpy(), C.key(tag, "residual_xy"): np.float64(xy), C.key(tag, "residual_z"): np.float64(z)})
    for q, v in worst.items():
        out["E_ref/" + q] = np.float64(v)
        print("E_ref %-24s %.3e" % (q, v))
    np.savez_compressed(C.FIXTURE, **out)
    C.fixture.cache_clear()
    print("wrote", C.FIXTURE, os.path.getsize(C.FIXTURE), "bytes;", len(C.cases()), "clip cases,", len(C.convert_cases()), "convert cases")
    assert os.path.getsize(C.FIXTURE) < 1_000_000


if __name__ == "__main__":
    main()
