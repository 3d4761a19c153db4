"""Golden fixture for sample_points_from_meshes, generated FROM THE REFERENCE's own code on the CPU (build container only).

    python tests/golden/make_golden_sample_points.py   ->  tests/golden/sample_points_ref.npz

The reference's pytorch3d.ops.sample_points_from_meshes runs unmodified on the ragged batch of tests/sample_points_case.py.  Its two
sources of randomness are replaced for the call: `Tensor.multinomial` by the float64 inverse CDF of RECORDED uniforms u0 (the first
face whose float64 prefix sum is above u0 * total), `torch.rand` by the recorded u1, u2; and `Tensor.sqrt` is the correctly rounded
IEEE root for the call (see recorded_randomness: torch's vectorised CPU sqrt is not).  Everything else -- areas, packed_to_padded,
the gathers, the weights, line 112, the normals, TexturesVertex.sample_textures -- is the reference's code on its CPU kernels; nothing
of pytorch3d_amd is in the loop.  (The textures are sampled from the batch of the non-empty meshes alone: the reference's texture
branch does not take a batch with an empty mesh.)  The batch the reference sees is the first FOUR meshes: for the fifth, whose faces are all degenerate,
its multinomial raises (this package gives zero rows there, which the tests check on their own).  Packed face indices of the first
four meshes are the same in both batches.

The u0 are drawn, and redrawn where needed, so that u0 * total keeps a relative distance of at least 1e-5 of the total from every
table boundary.  The script verifies that distance on the float64 cumsum AND on torch's float32 cumsum, and that both pick the same
face: a float32 table within D(F) 2^-24 < 2e-6 of the exact one must then reproduce the golden indices bit for bit.
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

MARGIN = 1e-5
SEED = 17
SQRT_STATS = [0, 0]  # roots where torch's own float32 sqrt is not the correctly rounded one, roots taken


def boundary_distance(row, t):
    """min over the table's entries of |t - entry| / total, per t."""
    return np.abs(np.asarray(t, dtype=np.float64)[:, None] - np.asarray(row, dtype=np.float64)[None, :]).min(1) / float(row[-1])


def draw_uniforms(rows, N, S, gen):
    """(N, S, 3) float32; the u0 of a mesh with a table redrawn until u0 * total is MARGIN away from every boundary."""
    u = torch.rand((N, S, 3), generator=gen, dtype=torch.float32)
    for n, row in enumerate(rows):
        if row.size == 0 or not row[-1] > 0:
            continue
        for _ in range(100):
            bad = boundary_distance(row, u[n, :, 0].double().numpy() * row[-1]) < 2 * MARGIN
            if not bad.any():
                break
            u[n, torch.from_numpy(bad), 0] = torch.rand((int(bad.sum()),), generator=gen, dtype=torch.float32)
        else:
            raise AssertionError("no admissible u0 found")
    return u


@contextlib.contextmanager
def recorded_randomness(u_valid):
    """Inside: Tensor.multinomial(num_samples, replacement=True) on the (n_valid, max_F) padded areas is the float64 inverse CDF of
    u_valid[:, :, 0]; torch.rand(2, n_valid, S, ...) is u_valid[:, :, 1:]."""
    real_multinomial, real_rand, real_sqrt = torch.Tensor.multinomial, torch.rand, torch.Tensor.sqrt

    def multinomial(self, num_samples, replacement=False, **kw):
        assert replacement and tuple(self.shape[:1]) == tuple(u_valid.shape[:1]) and num_samples == u_valid.shape[1]
        cdf = torch.cumsum(self.double(), 1)
        return torch.searchsorted(cdf, u_valid[:, :, 0].double() * cdf[:, -1:], right=True)

    def rand(*size, **kw):
        assert tuple(size) == (2, u_valid.shape[0], u_valid.shape[1]), size
        return u_valid[:, :, 1:].permute(2, 0, 1).contiguous().to(kw.get("dtype") or torch.float32)

    def sqrt(self):
        # The reference's `u.sqrt()` as the IEEE operation it stands for: the float64 root rounded to float32 is the correctly rounded
        # float32 root (53 >= 2 x 24 + 2 bits).  torch's vectorised float32 sqrt on the CPU returns a neighbour of it for about one
        # input in a hundred (counted below), and a golden made with it would pin that host library's error, not the reference's
        # arithmetic.
        exact = real_sqrt(self.double()).to(self.dtype)
        SQRT_STATS[0] += int((real_sqrt(self) != exact).sum())
        SQRT_STATS[1] += self.numel()
        return exact

    torch.Tensor.multinomial, torch.rand, torch.Tensor.sqrt = multinomial, rand, sqrt
    try:
        yield
    finally:
        torch.Tensor.multinomial, torch.rand, torch.Tensor.sqrt = real_multinomial, real_rand, real_sqrt


def main():
    import make_golden as mg
    import sample_points_case as C

    mg.bind_reference()
    from pytorch3d.ops.sample_points_from_meshes import sample_points_from_meshes
    from pytorch3d.renderer.mesh.textures import TexturesVertex
    from pytorch3d.structures import Meshes

    verts_list, faces_list = C.ragged_batch()
    verts, faces, first, nf = C.pack(verts_list, faces_list)
    gen = torch.Generator().manual_seed(SEED)
    features = [torch.rand(v.shape[0], 3, generator=gen) for v in verts_list]
    rows64 = C.tables64(C.areas64(verts, faces), first, nf)
    # torch's own float32 cumsum of the float32 areas the reference computes
    fv = verts[faces]
    a32 = torch.linalg.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0]).norm(dim=1) / 2.0
    rows32 = [torch.cumsum(a32[int(a):int(a) + int(n)], 0).numpy() for a, n in zip(first.tolist(), nf.tolist())]

    ref = Meshes(verts=verts_list[:4], faces=faces_list[:4])
    valid = [n for n in range(4) if int(nf[n]) > 0]
    ref_valid = Meshes(verts=[verts_list[n] for n in valid], faces=[faces_list[n] for n in valid],
                       textures=TexturesVertex(verts_features=[features[n] for n in valid]))
    out = {"verts": verts, "faces": faces, "first_idx": first, "num_faces": nf, "features": torch.cat(features, 0),
           "texture_meshes": np.asarray(valid)}
    worst = float("inf")
    for S in C.SAMPLE_COUNTS:
        u = draw_uniforms(rows64, 5, S, gen)
        i64 = C.choose(rows64, first, u[:, :, 0].numpy())
        i32 = C.choose(rows32, first, u[:, :, 0].numpy(), dtype=np.float32)
        for n in valid:
            for rows, dt in ((rows64, np.float64), (rows32, np.float32)):
                t = (u[n, :, 0].numpy().astype(dt) * dt(rows[n][-1])).astype(np.float64)
                d = float(boundary_distance(rows[n], t).min())
                worst = min(worst, d)
                assert d >= MARGIN, (S, n, dt, d)
        assert np.array_equal(i64, i32), S
        with recorded_randomness(u[valid]):
            samples, normals = sample_points_from_meshes(ref, S, return_normals=True)
            # (the reference's texture branch views the VALID meshes' indices as (len(meshes), S, 1, 1): it needs a batch without an
            # empty mesh, so the textures come from the batch of the valid meshes alone, rows in the order of `texture_meshes`)
            s3, textures = sample_points_from_meshes(ref_valid, S, return_textures=True)
        assert torch.equal(s3, samples[valid])
        # what the reference chose, read back from its samples: the golden indices are the float64 inverse CDF it was handed
        assert np.array_equal(i64[4], np.full(S, -1)) and np.array_equal(i64[2], np.full(S, -1))
        out["uniforms_%d" % S], out["idx_%d" % S] = u, torch.from_numpy(i64[:4])
        out["samples_%d" % S], out["normals_%d" % S], out["textures_%d" % S] = samples, normals, textures
        # the reference's samples are those of the recorded indices (float64 restatement, to float32 rounding)
        want = C.samples64(verts, faces, i64[:4], C.weights64(u[:4].numpy()))
        assert np.abs(samples.double().numpy() - want).max() < 1e-6, S
    print("roots where this host's torch float32 sqrt is not correctly rounded: %d of %d" % tuple(SQRT_STATS))
    print("smallest distance of u0 * total from a table boundary, relative to the total: %.3g (margin %g)" % (worst, MARGIN))
    mg.save("sample_points_ref", **out)


if __name__ == "__main__":
    main()
