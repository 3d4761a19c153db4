"""csrc/clip.hip on the GPU, per face and per row: every case of tests/clip_case.py through the gates of the fixture (tables bit-exact,
floats within 4 E_ref of each face's or row's scale, zero rows exactly zero), the onplane cases bit for bit, clip_backward's bits
across runs and streams, strided samples, one launch beyond grid_for's cap and 1024 scan blocks, the un-clipping invariant of the
whole rasterize_meshes pipeline, and an image with every face gone.  Each test prints its worst error against its gate.
Not reached: the cap of 4 * 8192 waves in convert_bwd_kernel, which needs more than 134 million samples."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import clip_case as C  # noqa: E402

import pytorch3d_amd as p3d  # noqa: E402
from pytorch3d_amd import clip  # noqa: E402

pytestmark = pytest.mark.gpu
CASES, CONVERT = C.cases(), C.convert_cases()
DEV = "cuda:0"


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_clip_cases_through_the_gates(case):
    assert C.failures([case], C.kernel_impl(), device=DEV, verbose=True) == []
    if case.kind == "onplane":  # exact arithmetic: the reference's float32 bits, and the truth's
        fix, got, t = C.fixture(), C.run_clip(C.kernel_impl(), case, device=DEV), C.truth(case)
        assert C.same_bits(got["face_verts"], fix[C.key(case.id, "f32_face_verts")])
        assert C.same_bits(got["barycentric_conversion"], fix[C.key(case.id, "f32_barycentric_conversion")])
        for q in C.float_quantities(case):
            assert np.array_equal(got[q], t[q]), q


@pytest.mark.parametrize("case", CONVERT, ids=[c.id for c in CONVERT])
def test_convert_cases_through_the_gates(case):
    assert C.failures([case], C.kernel_impl(), device=DEV, verbose=True) == []


def test_strided_samples_are_what_contiguous_ones_are():
    def slices(p2f, bary):  # every other sample of tensors twice as long, and the first three of five columns
        wide_p = torch.full((1, 1, p2f.shape[2], 2), -1, dtype=p2f.dtype, device=p2f.device)
        wide_b = torch.zeros((1, 1, bary.shape[2], 1, 5), dtype=bary.dtype, device=bary.device)
        wide_p[..., :1], wide_b[..., :3] = p2f, bary
        assert not wide_p[..., :1].is_contiguous() and not wide_b[..., :3].is_contiguous()
        return wide_p[..., :1], wide_b[..., :3]

    for cid in ("convert-S4097-random", "convert-S257-fresh"):
        case = C.case_by_id(cid)
        got = C.run_convert(C.kernel_impl(), case, device=DEV, through=slices)
        plain = C.run_convert(C.kernel_impl(), case, device=DEV)
        assert [(q, n) for q, _, n in C.errors(case, got) if n] == []
        for q in ("pix_to_face_unclipped", "bary_unclipped", "grad_bary_clipped"):  # (grad_conversion: atomics, gated only)
            assert np.array_equal(got[q], plain[q]), (cid, q)


def test_clip_backward_has_the_same_bits_on_every_run_and_stream():
    for cid in ("seeded-persp", "scan-F2049", "branch-flat"):
        case = C.case_by_id(cid)
        first = C.run_clip(C.kernel_impl(), case, device=DEV)
        second = C.run_clip(C.kernel_impl(), case, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            third = C.run_clip(C.kernel_impl(), case, device=DEV)
        side.synchronize()
        for q in C.float_quantities(case):  # one thread per face gathers its gradients: nothing to reorder
            assert np.array_equal(first[q], second[q]) and np.array_equal(first[q], third[q]), (cid, q)


def test_one_launch_beyond_the_grid_cap_and_1024_scan_blocks():
    """F = 2 097 152 + 1500: classify, emit and backward take a second grid-stride pass (8192 workgroups of 256), the scans have more
    than 1024 blocks of 1024 rows.  Tables: all faces against the restatement's cumulative sums on the device.  Floats: the first 2048
    faces, 1024 around index 1 048 576 and the last 3548 against the float64 restatement of those faces alone (faces are independent),
    rows matched through the tables."""
    F = 2_097_152 + 1500
    assert -(-F // 256) > 8192 and -(-F // 1024) > 1024
    g = torch.Generator().manual_seed(C.SEED + 9)
    fv = torch.cat([torch.rand(F, 3, 2, generator=g) * 3 - 1.5, torch.rand(F, 3, 1, generator=g) * 2 - 0.5], -1)
    first = torch.tensor([0, F // 3, F // 2])
    count = torch.tensor([F // 3, F // 2 - F // 3, F - F // 2])
    settings = dict(z_clip_value=0.25, perspective_correct=True, **C.BOX)
    fv_d = fv.to(DEV).requires_grad_(True)
    cf = clip.clip_faces(fv_d, first.to(DEV), count.to(DEV), clip.ClipFrustum(**settings))
    with torch.no_grad():
        want = C.clip_faces_torch(fv_d.detach(), first.to(DEV), count.to(DEV), C.Frustum(**settings))
    for name in C.TABLES:
        assert torch.equal(getattr(cf, name), getattr(want, name)), name
    Fc, T = cf.face_verts.shape[0], cf.barycentric_conversion.shape[0]
    assert Fc > F and T > F // 2
    del want
    gd = torch.Generator(device=DEV).manual_seed(C.SEED + 10)
    g_fv, g_conv = torch.randn((Fc, 3, 3), generator=gd, device=DEV), torch.randn((T, 3, 3), generator=gd, device=DEV)
    ((cf.face_verts * g_fv).sum() + (cf.barycentric_conversion * g_conv).sum()).backward()

    idx = torch.cat([torch.arange(2048), 1_048_576 - 512 + torch.arange(1024), F - 3548 + torch.arange(3548)])
    leaf = fv[idx].double().requires_grad_(True)
    sub = C.clip_faces_torch(leaf, torch.tensor([0]), torch.tensor([idx.numel()]), C.Frustum(**settings))
    c2u_all, c2u_sub = cf.faces_clipped_to_unclipped_idx.cpu(), sub.faces_clipped_to_unclipped_idx
    within = torch.arange(c2u_sub.numel()) - torch.searchsorted(c2u_sub, c2u_sub)  # 0, or 1 on the second face of a case-4 pair
    rows = (torch.searchsorted(c2u_all, idx[c2u_sub]) + within).to(DEV)  # the same faces in the big launch's output
    assert torch.equal(c2u_all[rows.cpu()], idx[c2u_sub])
    has = sub.faces_clipped_to_conversion_idx >= 0
    conv_rows = cf.faces_clipped_to_conversion_idx[rows[has.to(DEV)]]
    assert bool((conv_rows >= 0).all())
    g_conv_sub = torch.zeros_like(sub.barycentric_conversion)
    g_conv_sub[sub.faces_clipped_to_conversion_idx[has]] = g_conv[conv_rows].cpu().double()
    ((sub.face_verts * g_fv[rows].cpu().double()).sum() + (sub.barycentric_conversion * g_conv_sub).sum()).backward()
    worst = {"face_verts": C.block_errors(cf.face_verts[rows].detach().cpu(), sub.face_verts.detach(), "face_verts"),
             "barycentric_conversion": C.block_errors(cf.barycentric_conversion[conv_rows].detach().cpu(),
                                                      sub.barycentric_conversion[sub.faces_clipped_to_conversion_idx[has]].detach(), "barycentric_conversion"),
             "grad_face_verts": C.block_errors(fv_d.grad[idx.to(DEV)].cpu(), leaf.grad, "grad_face_verts")}
    for q, (ratio, n) in worst.items():
        print("big launch %-24s worst error / gate %.3f%s" % (q, ratio, "  BEYOND: %d" % n if n else ""))
    assert all(n == 0 for _, n in worst.values()), worst
    assert bool(fv_d.grad[-1].any()) == bool(leaf.grad[-1].any())  # the last face was reached


@pytest.mark.parametrize("bin_size", [0, 8])
@pytest.mark.parametrize("tag", list(C.PIPELINE))
def test_unclipped_barycentrics_give_back_the_pixel_and_its_depth(tag, bin_size):
    """Every fragment of rasterize_meshes(z_clip_value=0.25) names an ORIGINAL face and barycentrics on it: applied to that face they
    give back the pixel centre (through z when perspective_correct) and the fragment's zbuf.  Gate: 4 x the residual of the reference's
    own CPU pipeline on the same scene, recorded in the fixture."""
    fix, persp = C.fixture(), C.PIPELINE[tag]
    verts, faces = C.pipeline_scene(tag)
    m = p3d.PackedMeshes([verts.to(DEV)], [faces.to(DEV)])
    p2f, zbuf, bary, dists = p3d.rasterize_meshes(m, image_size=(C.PIPELINE_IMAGE, C.PIPELINE_IMAGE), blur_radius=0.0, faces_per_pixel=C.PIPELINE_K,
                                                  bin_size=bin_size, perspective_correct=persp, clip_barycentric_coords=False,
                                                  z_clip_value=C.PIPELINE_Z_CLIP, cull_to_frustum=True)
    xy, z, n = C.pipeline_residual(verts, faces, p2f, zbuf, bary, persp)
    ref_p2f = torch.from_numpy(fix[C.key(tag, "pix_to_face")].astype(np.int64))
    gate_xy, gate_z = C.GATE_FACTOR * float(fix[C.key(tag, "residual_xy")]), C.GATE_FACTOR * float(fix[C.key(tag, "residual_z")])
    print("%s bin_size %d: %d fragments, %.1f %% of pix_to_face as the reference's; residual xy %.3e (gate %.3e) z %.3e (gate %.3e)"
          % (tag, bin_size, n, 100.0 * float((p2f.cpu() == ref_p2f).float().mean()), xy, gate_xy, z, gate_z))
    assert n >= 100 and int(p2f.max()) < 12
    assert xy <= gate_xy and z <= gate_z


def test_every_face_gone_leaves_an_empty_image():
    g = torch.Generator().manual_seed(C.SEED + 11)
    behind = torch.cat([torch.rand(9, 2, generator=g) - 0.5, -torch.rand(9, 1, generator=g)], 1)  # all behind z = 0.25
    outside = torch.cat([torch.rand(9, 2, generator=g) - 0.5, torch.rand(9, 1, generator=g) + 0.5], 1)
    outside[0::3] = 2.0 + torch.rand(3, 3, generator=g)  # vertex 0 of each face beyond right: culled by the reference's reading
    faces = torch.arange(9).view(3, 3)
    for verts in (behind, outside):
        cf = clip.clip_faces(verts[faces].to(DEV), torch.tensor([0], device=DEV), torch.tensor([3], device=DEV),
                             clip.ClipFrustum(z_clip_value=0.25, **C.BOX))
        assert cf.face_verts.shape == (0, 3, 3) and cf.faces_clipped_to_unclipped_idx.numel() == 0 and int(cf.num_faces_per_mesh.sum()) == 0
        leaf = verts.to(DEV).requires_grad_(True)
        m = p3d.PackedMeshes([leaf], [faces.to(DEV)])
        p2f, zbuf, bary, dists = p3d.rasterize_meshes(m, image_size=(16, 16), blur_radius=0.0, faces_per_pixel=2, z_clip_value=0.25, cull_to_frustum=True)
        assert p2f.shape == (1, 16, 16, 2) and bool((p2f == -1).all()) and bool((zbuf == -1).all()) and bool((bary == -1).all())
