"""The machinery of tests/test_gpu_cloud_kernel_edges.py, proved on the CPU.

  1. Every case of that file with the package's torch formulation (which CPU tensors take) in place of the kernels of
     csrc/sample_points.hip, csrc/fps_ball.hip and csrc/points_to_volumes.hip, through the SAME gate functions
     (sample_points_case, fps_ball_case, points_to_volumes_case): the generators, the asserted reach conditions -- recomputed from
     the host code's constants -- and the gates hold for a correct implementation.
  2. The gates are not vacuous: six deliberately wrong answers, each of which must be rejected.
"""
import functools
import importlib

import numpy as np
import pytest
import torch

import fps_ball_case as FB
import points_to_volumes_case as PV
import sample_points_case as SP


def _p3d():
    import pytorch3d_amd as p3d

    return p3d


def _p2v():
    return importlib.import_module("pytorch3d_amd.points_to_volumes")


def _formulation_table(verts, faces, first, nf):
    """(float32 areas (F,), cumulative table (F,)) of the torch formulation: pytorch3d_amd.sample_points.face_table, unpadded."""
    from pytorch3d_amd import sample_points as sp

    fv = verts[faces]
    a, b = fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0]
    cx, cy, cz = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    areas = (torch.sqrt(cx * cx + cy * cy + cz * cz) / 2.0).numpy()
    cdf, _ = sp.face_table(verts, faces, first, nf)
    table = np.concatenate([cdf[n, :int(c)].numpy() for n, c in enumerate(nf.tolist())] + [np.zeros(0, np.float32)])
    return areas, table.astype(np.float32)


# ---- A. sample_points backward over long runs ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long_forward():
    verts, faces, first, nf = SP.long_run_batch()
    u = SP.long_run_grads("samples")[0]
    _, _, idx, bary = _p3d().sample_points_packed(verts, faces, first, nf, SP.LONG_S, u, True)
    return verts, faces, first, nf, u, idx.numpy(), bary.numpy()


def test_the_long_run_case_reaches_what_it_is_for():
    verts, faces, first, nf, u, idx, _ = _long_forward()
    assert SP.backward_plan(3 * SP.LONG_S) == (1688, 320) and SP.backward_plan(2048 * 64) == (2048, 64)  # one step up to 131 072 samples
    assert SP.backward_plan(64 * 10000)[1] == 320  # the measured workload takes the same five steps
    reach = SP.long_run_reach(idx, nf)
    assert reach["span"] // SP.WAVE_STEP == 5
    areas, table = _formulation_table(verts, faces, first, nf)
    SP.gate_table(areas, faces, first, nf, u, idx, table)
    # the ordered form: more than 256 waves of sorted samples, and the one face of mesh 0 is a segment over more than 256 of them
    assert -(-int((idx >= 0).sum()) // 64) > 256 and int((idx == 0).sum()) // 64 > 256


@pytest.mark.parametrize("which", ["samples", "both"])
def test_formulation_passes_the_long_run_gate_and_a_lost_fourth_step_is_rejected(which):
    """Wrong answer 1: the rows without every sample of one wave's fourth step, as a flush that loses the step leaves them -- for a
    wave inside the one-face mesh, the wave whose table fills up, a wave across a mesh boundary and a wave of the 300-face mesh.  The
    gate's tolerance is dominated by the formulation's sequential index_put on the one face (printed below), and still every lost
    step is hundreds of times beyond it: no per-face check is needed on top of gate_grads."""
    verts, faces, first, nf, u, idx, w = _long_forward()
    _, gs, gn = SP.long_run_grads(which)
    x = verts.clone().requires_grad_(True)
    samples, normals, idx2, _ = _p3d().sample_points_packed(x, faces, first, nf, SP.LONG_S, u, True)
    assert np.array_equal(idx2.numpy(), idx)
    torch.autograd.backward([samples] + ([normals] if gn is not None else []), [gs] + ([gn] if gn is not None else []))
    known = SP.grads_gate(verts, faces, idx, w, gs, gn)
    err, tol = SP.gate_grads(verts, faces, idx, w, x.grad.numpy(), gs, gn, "long runs " + which, known=known)
    assert tol > 0
    f32 = SP.formulation_grads32(verts, faces, idx, w, gs, gn)
    print("formulation's error on the one face %.3g, elsewhere %.3g" % (np.abs(f32 - known[0])[:3].max(), np.abs(f32 - known[0])[3:].max()))
    reach = SP.long_run_reach(idx, nf)
    for wave in (reach["one_key"], reach["flush"], reach["straddle"][0], reach["straddle"][1] + 3):
        wrong, _ = SP.grads64(verts, faces, SP.drop_fourth_step(idx, wave), w, gs, gn)
        print("wave %d without its fourth step: error %.3g, gate %.3g" % (wave, np.abs(wrong - known[0]).max(), tol))
        with pytest.raises(AssertionError):
            SP.gate_grads(verts, faces, idx, w, wrong, gs, gn, "lost step", known=known)


# ---- B. sample_points forward with many small meshes -----------------------------------------------------------------------------------------
def test_formulation_passes_the_gate_of_many_small_meshes():
    verts, faces, first, nf = SP.many_small_meshes()
    SP.small_meshes_reach(first, nf, faces.shape[0])
    u = SP.uniforms(700, 65, 82)
    samples, normals, idx, bary = (t.numpy() for t in _p3d().sample_points_packed(verts, faces, first, nf, 65, u, True))
    areas, table = _formulation_table(verts, faces, first, nf)
    SP.gate_small_meshes(verts, faces, first, nf, u, areas, table, samples, normals, idx, bary)
    # the gate bites: a table that does not restart at the mesh after the run of empty ones, and a row written for an empty mesh
    n = 350 + 5 + int(np.argmax(nf.numpy()[355:] > 0))
    lo, hi = int(first[n]), int(first[n] + nf[n])
    carried = table.copy()
    carried[lo:hi] += table[lo - 1]
    with pytest.raises(AssertionError):
        SP.gate_small_meshes(verts, faces, first, nf, u, areas, carried, samples, normals, idx, bary)
    wrong = idx.copy()
    wrong[352] = 0
    with pytest.raises(AssertionError):
        SP.gate_small_meshes(verts, faces, first, nf, u, areas, table, samples, normals, wrong, bary)


# ---- C. fps ties on every rung -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [3, 2])
@pytest.mark.parametrize("P", FB.TIE_P)
def test_formulation_orders_the_ties_of_every_rung_and_two_wrong_tie_rules_are_rejected(P, D):
    """Wrong answers 2 and 3: the highest index among equal maxima; and a lane that keeps the later of its equal slots (i + 1024 over
    i) under an otherwise correct reduction -- that one is the right answer up to 1024 points and wrong on every rung above."""
    points, lengths, start = FB.tie_clouds(P, D)
    assert points.shape == (2, P, D) and float(points.abs().max()) <= 6 and torch.equal(points, points.round())
    assert len({tuple(p) for p in points[0, :FB.TIE_SITES].tolist()}) == FB.TIE_SITES
    want, tied = FB.fps64(points, lengths, FB.TIE_K, start)
    FB.tie_reach(P, lengths, tied, want)
    assert sorted(want[0, :FB.TIE_SITES].tolist()) == list(range(FB.TIE_SITES)) and not want[0, FB.TIE_SITES:].any()
    sel, idx = _p3d().sample_farthest_points(points, torch.tensor(lengths), FB.TIE_K, start_idxs=start)
    FB.gate_fps_ties(points, lengths, start, idx, sel, want)
    for rule, rejected in (("last", True), ("later_slot", P > 1024)):
        wrong = FB.fps64(points, lengths, FB.TIE_K, start, rule)[0]
        wrong_sel = _p3d().masked_gather(points, torch.from_numpy(wrong))
        if rejected:
            with pytest.raises(AssertionError):
                FB.gate_fps_ties(points, lengths, start, wrong, wrong_sel, want)
        else:
            FB.gate_fps_ties(points, lengths, start, wrong, wrong_sel, want)


def test_the_ladder_restated_for_the_ties_is_the_hosts():
    from pytorch3d_amd import _lib

    assert _lib.FPS_REGISTER_POINTS == 16384
    assert [FB.fps_plan(P) for P in FB.TIE_P] == [(64, 1), (128, 1), (256, 1), (512, 1), (1024, 1), (1024, 2), (1024, 4), (1024, 8),
                                                   (1024, 16), (1024, 0)]
    assert FB.fps_plan(64) == (64, 1) and FB.fps_plan(65) == (128, 1) and FB.fps_plan(1025) == (1024, 2) and FB.fps_plan(16385) == (1024, 0)


# ---- D. points_to_volumes at size and at the remaining channel counts ----------------------------------------------------------------------
def _run(case, inp):
    m = _p2v()
    return PV.run_operators(case, inp, "cpu", m.points_to_volumes_forward_op, m.points_to_volumes_backward_op)


@pytest.mark.parametrize("case", PV.generated_cases("long", "channels0", "channels2", "channels4", "channels8"), ids=PV.case_id)
def test_formulation_equals_the_restatement_on_the_generated_cases(case):
    inp = PV.inputs(case)
    got = _run(case, inp)
    PV.judge(case, inp, got, recorded=False)
    C = inp["features"].shape[2]
    assert got["features"].shape[1] == C and got["grad_points_features"].shape[2] == C
    if C == 0 and case[2] == "trilinear":  # the gradient of the locations comes from the density gradient alone, and there is one
        assert got["grad_points_3d"].abs().sum() > 0


@pytest.mark.parametrize("case", PV.generated_cases("long"), ids=PV.case_id)
def test_an_ordered_sum_that_stops_after_256_waves_is_rejected(case):
    """Wrong answer 4.  The nearest mode of "long" has 118 waves: nothing lies past wave 256 there, and its restatement is unchanged."""
    inp = PV.inputs(case)
    waves, none, position = PV.ordered_reach(case, inp)
    _, at = PV.keys64(case, inp)
    keep = position[at] < 256 * 64
    got = _run(case, inp)
    dens, feat, _, _ = PV.forward64(case, inp, keep)
    stopped = dict(got, densities=dens.float(), features=feat.float())
    if waves > 256:
        assert not bool(keep.all())
        with pytest.raises(AssertionError):
            PV.judge(case, inp, stopped, recorded=False)
    else:
        assert bool(keep.all())
        PV.judge(case, inp, stopped, recorded=False)


@pytest.mark.parametrize("mode", ["trilinear", "nearest"])
def test_bad_coordinates_are_skipped_and_a_far_point_that_wraps_into_the_grid_is_rejected(mode):
    """Wrong answer 6: the point at 1e15 added at its location modulo the grid."""
    case, inp, good, inp_good = PV.bad_coordinate_inputs(mode)
    assert int(good.sum()) == 70 and int((~good).sum()) == 21
    pts = inp["points_3d"][0, ~good]
    assert int(torch.isnan(pts).any(1).sum()) == 3 and int(torch.isinf(pts).any(1).sum()) == 6 and int((pts.abs() == 1e15).any(1).sum()) == 3
    got = _run(case, inp)
    PV.judge_bad_coordinates(case, got, good, inp_good)
    far = int(torch.nonzero((inp["points_3d"][0] == 1e15).any(1))[0])
    wrapped = dict(inp_good)
    loc = torch.tensor([1.0, 2.0, 1.0])  # a voxel of the (3, 4, 5) grid, aligned: p = 2 loc / (grid - 1) - 1, exact
    wrapped["points_3d"] = torch.cat([inp_good["points_3d"], (2 * loc / torch.tensor([4.0, 3.0, 2.0]) - 1)[None, None]], 1)
    wrapped["features"] = torch.cat([inp_good["features"], inp["features"][:, far:far + 1]], 1)
    wrapped["mask"] = torch.ones(1, 71)
    dens, feat, _, _ = PV.forward64(case, wrapped)
    assert not torch.equal(dens, PV.forward64(case, inp_good)[0])
    with pytest.raises(AssertionError):
        PV.judge_bad_coordinates(case, dict(got, densities=dens.float(), features=feat.float()), good, inp_good)


@pytest.mark.parametrize("case", PV.generated_cases("oversized"), ids=PV.case_id)
def test_a_grid_larger_than_the_tensor_is_cut_at_the_tensors_extent(case):
    """Wrong answer 5: corners bounded by the grid and not by the tensor's extent -- the formulation handed the whole buffer, which is
    the tensor such a forward believes in: a wrong value in the poison, not a write out of bounds."""
    m = _p2v()
    inp, got, buffers = PV.run_oversized(case, "cpu", m.points_to_volumes_forward_op, m.points_to_volumes_backward_op)
    PV.judge(case, inp, got, recorded=False)
    assert all(PV.poison_untouched(buf, shape) for buf, shape in buffers)
    # the restatement has samples that only the cut removes
    grid_bound = dict(inp, densities=torch.zeros(2, 1, 5, 6, 7))
    assert PV.corners64(case, grid_bound)[0].shape[0] > PV.corners64(case, inp)[0].shape[0]
    (buf_d, dens), (buf_f, feat) = PV.padded_buffers(inp)
    m.points_to_volumes_forward_op(inp["points_3d"], inp["features"], buf_d, buf_f, inp["grid_sizes"], PV.full_mask(inp),
                                   inp["point_weight"], case[3], case[2] == "trilinear")
    assert not (PV.poison_untouched(buf_d, dens.shape) and PV.poison_untouched(buf_f, feat.shape))


@pytest.mark.parametrize("mode", ["trilinear", "nearest"])
def test_a_transposed_mask_gives_the_bits_of_the_contiguous_one(mode):
    case = ("lattice", "mixed_grids", mode, True)
    inp = PV.inputs(case)
    strided = PV.transposed(inp["mask"])
    assert strided.stride() == (1, 2) and inp["mask"].stride() == (65, 1) and torch.equal(strided, inp["mask"])
    a, b = _run(case, inp), _run(case, dict(inp, mask=strided))
    assert all(torch.equal(a[k], b[k]) for k in a)
    PV.judge(case, inp, b)
