"""Golden fixture for the VolumeSampler kernels, recorded FROM THE REFERENCE's own Python on the CPU (build container only).

    python tests/golden/make_golden_volume_sampler.py   ->  tests/golden/volume_sampler_ref.npz

Imports the unmodified reference package (the staged copy under oracle/_ref/reference_py, or P3D_REFERENCE_ROOT) under plain
pytorch3d_amd.shim.install(), which leaves pytorch3d.renderer.implicit alone, as the other generators do.  Nothing of pytorch3d_amd
computes anything here; the inputs are redrawn from seeds by the tests (tests/volume_sampler_case.py), so the file holds outputs only:
* <case>/<quantity>: the TRUTH -- the reference's steps 2 and 3 (its ray_bundle_variables_to_ray_points, F.grid_sample, permute and
  view, as VolumeSampler.forward writes them) in float64 on the case's float32 local rays, with autograd gradients to both volumes
  and to local origins, directions and lengths;
* E_ref/<quantity>: the largest error of the reference's own float32 CPU VolumeSampler.forward against that truth over all cases,
  relative to the case's largest |truth|.  The module runs on a Volumes object whose world-to-local transform is the identity (a
  subclass that overrides the two transform getters: the cases ARE local rays), except for the world case, which runs on a real
  Volumes with a translation and a voxel size;
* world/matrix, world/origins_local, world/directions_local: that Volumes' world-to-local matrix and what the reference's own step 1
  makes of the world rays in float32 -- the local rays the world case starts from;
* <lattice case>/f32_densities, f32_features: F.grid_sample's float32 CPU outputs, which the kernels must equal bit for bit.
Asserted here: the condition of the case file's header on every case (no sample near a lattice plane; exact ones have the same
float32 and float64 source index); every truth is finite; the float32 run of a lattice case equals its truth exactly; where a truth is
all zeros the float32 run is too; the case file's MatrixVolumes stand-in reproduces the reference's step 1 bit for bit.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import run_reference_suite as rrs
    import volume_sampler_case as C

    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    ref_root = next(c for c in (os.environ.get("P3D_REFERENCE_ROOT"), stage) if c and os.path.isdir(os.path.join(c, "pytorch3d", "renderer")))
    rrs._stub_missing_packages()
    import pytorch3d_amd.shim as shim

    shim.install(ref_root)
    from pytorch3d.renderer.implicit import renderer as ref
    from pytorch3d.renderer.implicit.utils import RayBundle, ray_bundle_variables_to_ray_points
    from pytorch3d.structures import Volumes
    from pytorch3d.transforms import Transform3d

    assert not getattr(ref.VolumeSampler.forward, "__p3d_amd__", False)

    class LocalVolumes(Volumes):  # world == local: the cases are local rays
        def world_to_local_coords(self, points):
            return points

        def get_world_to_local_coords_transform(self):
            return Transform3d(dtype=self.densities().dtype, device=self.device)

    def truth_fn(dens, feats, o, d, l, sample_mode, padding_mode, align_corners):
        """renderer.py:360-415 on local rays (any dtype)."""
        points = ray_bundle_variables_to_ray_points(o, d, l)
        flat = points.view(points.shape[0], -1, 1, 1, 3)
        N = o.shape[0]
        dens = dens.expand(N, *dens.shape[1:])
        rd = torch.nn.functional.grid_sample(dens, flat, mode=sample_mode, padding_mode=padding_mode, align_corners=align_corners)
        rd = rd.permute(0, 2, 3, 4, 1).view(*points.shape[:-1], dens.shape[1])
        if feats is None:
            return rd, rd.split([dens.shape[1], 0], dim=-1)[1]
        feats = feats.expand(N, *feats.shape[1:])
        rf = torch.nn.functional.grid_sample(feats, flat, mode=sample_mode, padding_mode=padding_mode, align_corners=align_corners)
        return rd, rf.permute(0, 2, 3, 4, 1).view(*points.shape[:-1], feats.shape[1])

    def module_fn(dens, feats, o, d, l, sample_mode, padding_mode, align_corners):
        """The reference's module itself, float32."""
        N = o.shape[0]
        vols = LocalVolumes(densities=dens.expand(N, *dens.shape[1:]), features=None if feats is None else feats.expand(N, *feats.shape[1:]),
                            align_corners=align_corners)
        return ref.VolumeSampler(vols, sample_mode=sample_mode, padding_mode=padding_mode)(RayBundle(o, d, l, None))

    out = {}
    # ---- the world case's step 1, by the reference ---------------------------------------------------------------------------------
    wo, wd, wl = C.world_rays()
    world = C.case_by_id("world")
    D, H, W = world.grid
    real = Volumes(densities=torch.zeros((world.N, 1, D, H, W)), voxel_size=torch.tensor([C.WORLD_VOXEL_SIZE] * world.N),
                   volume_translation=torch.tensor([C.WORLD_TRANSLATION] * world.N))
    sampler = ref.VolumeSampler(real)
    local_o = real.world_to_local_coords(wo)
    local_d = sampler._get_ray_directions_transform().transform_points(wd.view(world.N, -1, 3)).view(wd.shape)
    matrix = real.get_world_to_local_coords_transform().get_matrix()
    out["world/matrix"], out["world/origins_local"], out["world/directions_local"] = matrix.numpy(), local_o.numpy(), local_d.numpy()
    stand_in = C.MatrixVolumes(None, None, matrix)
    assert torch.equal(stand_in.world_to_local_coords(wo), local_o)
    assert float(matrix[:, 3, :3].abs().min()) > 0.01  # a translation that a direction must not take

    worst = {q: 0.0 for q in C.QUANTITIES}
    for case in C.cases():
        inp = C.inputs(case, local_rays=(local_o, local_d) if case.kind == "world" else None)
        assert C.clear_of_planes(case, inp[2], inp[3], inp[4]), case.id
        truth = C.run(truth_fn, case, dtype=torch.float64, inp=inp)
        if case.kind == "world":
            vols = Volumes(densities=inp[0], features=inp[1], voxel_size=torch.tensor([C.WORLD_VOXEL_SIZE] * case.N),
                           volume_translation=torch.tensor([C.WORLD_TRANSLATION] * case.N))
            f32 = C.run(truth_fn, case, inp=inp)
            with torch.no_grad():
                rd, rf = ref.VolumeSampler(vols)(RayBundle(wo, wd, wl, None))
            assert torch.equal(rd.double(), torch.from_numpy(f32["rays_densities"])) and torch.equal(rf.double(), torch.from_numpy(f32["rays_features"]))
        else:
            f32 = C.run(module_fn, case, inp=inp)
        for q in C.QUANTITIES:
            if truth[q] is None:
                continue
            assert np.isfinite(truth[q]).all(), (case.id, q)
            out[C.key(case.id, q)] = truth[q]
            scale = float(np.abs(truth[q]).max()) if truth[q].size else 0.0
            if case.kind == "lattice":
                assert np.array_equal(f32[q], truth[q]), (case.id, q)
            if scale == 0.0:
                assert not f32[q].any(), (case.id, q)
            else:
                assert np.isfinite(f32[q]).all(), (case.id, q)
                worst[q] = max(worst[q], float(np.abs(f32[q] - truth[q]).max()) / scale)
        if case.kind == "lattice":
            with torch.no_grad():
                rd, rf = truth_fn(*inp[:5], case.mode, case.padding, case.align)
            out[C.key(case.id, "f32_densities")], out[C.key(case.id, "f32_features")] = rd.numpy(), rf.numpy()
    for q in C.QUANTITIES:
        out["E_ref/" + q] = np.float64(worst[q])
        print("E_ref %-16s %.3e" % (q, worst[q]))
    np.savez_compressed(C.FIXTURE, **out)
    print("wrote", C.FIXTURE, os.path.getsize(C.FIXTURE), "bytes;", len(C.cases()), "cases")
    assert os.path.getsize(C.FIXTURE) < 2 ** 20


if __name__ == "__main__":
    main()
