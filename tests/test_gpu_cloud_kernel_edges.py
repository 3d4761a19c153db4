"""The paths of csrc/sample_points.hip, csrc/fps_ball.hip and csrc/points_to_volumes.hip that their fixtures and first tests were too
small to reach, on the kernels, through the gates of sample_points_case, fps_ball_case and points_to_volumes_case.
tests/test_cpu_cloud_kernel_edges.py runs the same cases through the same gates on the package's torch formulation and shows that
each gate rejects a wrong answer.  Every input comes from a seeded CPU generator; where the host code's constants set a shape, the
condition that proves the path is reached is recomputed from them and asserted.

  A. sample_points backward over long runs: face_sums_kernel with several steps per wave, a slot found occupied from an earlier step,
     the flush of a full table, the span rounding and the clamp of the last wave; the ordered form over thousands of waves
     (pass2_kernel beyond its first block, one segment across more than 256 waves).
  B. sample_points forward with 700 small meshes: many heads in one wave, runs of empty meshes at the start, in the middle and at the end.
  C. fps: equal minima in the slots of one lane, in the rows of a wave, across waves and in the workspace form's loop, on every rung.
  D. points_to_volumes: 938 waves of the ordered sum, C in {0, 2, 4, 7, 8}, coordinates that are not finite or do not fit an int64, a
     grid larger than the tensor, a transposed mask.
"""
import contextlib
import functools
import importlib

import numpy as np
import pytest
import torch

import fps_ball_case as FB
import points_to_volumes_case as PV
import sample_points_case as SP

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _p3d():
    import pytorch3d_amd as p3d

    return p3d


def _p2v():
    return importlib.import_module("pytorch3d_amd.points_to_volumes")


@contextlib.contextmanager
def _flag(on):
    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])


def _profiled(fn):
    """(fn(), the names of the launches the built-in timing recorded while it ran)."""
    from pytorch3d_amd import _lib

    _lib.load().p3d_profile_reset()
    _lib.load().p3d_profile_enable(1)
    try:
        out = fn()
        ran = set(_lib.profile_snapshot())
    finally:
        _lib.load().p3d_profile_enable(0)
        _lib.load().p3d_profile_reset()
    return out, ran


def _sample(verts, faces, first, nf, S, u):
    """The forward into poisoned outputs -> (numpy samples, normals, idx, bary, table, the kernels' float32 areas)."""
    d = _dev()
    N, nan = int(nf.numel()), float("nan")
    out = (torch.full((N, S, 3), nan, device=d), torch.full((N, S, 3), nan, device=d), torch.full((N, S), -7, dtype=torch.int64, device=d),
           torch.full((N, S, 3), nan, device=d))
    table = []
    got = _p3d().sample_points_packed(verts.to(d), faces.to(d), first.to(d), nf.to(d), S, u.to(d), True, _table_out=table, _out=out)
    areas = _p3d().face_areas_normals(verts.to(d), faces.to(d))[0]  # the same arithmetic, by contract
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in got) + (table[0].cpu().numpy(), areas.cpu().numpy())


# ---- A. sample_points backward over long runs ----------------------------------------------------------------------------------------------
def _long_grad(which, ordered, stream=None):
    d = _dev()
    verts, faces, first, nf = SP.long_run_batch()
    u, gs, gn = SP.long_run_grads(which)
    ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    with ctx, _flag(ordered):
        x = verts.to(d).requires_grad_(True)
        samples, normals, idx, bary = _p3d().sample_points_packed(x, faces.to(d), first.to(d), nf.to(d), SP.LONG_S, u.to(d), gn is not None)
        torch.autograd.backward([samples] + ([normals] if gn is not None else []), [gs.to(d)] + ([gn.to(d)] if gn is not None else []))
        if stream is not None:
            stream.synchronize()
    torch.cuda.synchronize()
    return x.grad.cpu(), idx.cpu().numpy(), bary.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _long_known(which):
    """The kernels' indices and weights of the long-run case and grads_gate on them: computed once, shared by both forms."""
    verts, faces, first, nf = SP.long_run_batch()
    u, gs, gn = SP.long_run_grads(which)
    _, _, idx, bary, _, _ = _sample(verts, faces, first, nf, SP.LONG_S, u)
    return idx, bary, SP.grads_gate(verts, faces, idx, bary, gs, gn)


def test_long_run_forward_is_the_hosts_choice_and_reaches_every_path():
    verts, faces, first, nf = SP.long_run_batch()
    u = SP.long_run_grads("samples")[0]
    _, _, idx, _, table, areas = _sample(verts, faces, first, nf, SP.LONG_S, u)
    SP.gate_table(areas, faces, first, nf, u, idx, table)
    reach = SP.long_run_reach(idx, nf)
    print("long runs: span %d, %d waves; one key in wave %d, flush in wave %d, boundaries in waves %s, last wave %d" % (
        reach["span"], reach["waves"], reach["one_key"], reach["flush"], reach["straddle"], reach["last"]))
    assert reach["span"] == 320


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("which", ["samples", "both"])
def test_long_run_gradients_against_the_float64_restatement(which, ordered):
    verts, faces, first, nf = SP.long_run_batch()
    _, gs, gn = SP.long_run_grads(which)
    (got, idx, w), ran = _profiled(lambda: _long_grad(which, ordered))
    want_idx, want_w, known = _long_known(which)
    assert np.array_equal(idx, want_idx) and SP.bits_equal(w, want_w)
    SP.long_run_reach(idx, nf)  # span >= 256, a wave of one key, a wave that flushes, both boundaries inside waves, a partial last wave
    SP.gate_grads(verts, faces, idx, w, got.numpy(), gs, gn, "long runs " + which + (" ordered" if ordered else " atomic"), known=known)
    atomic = {"sample_points_face_sums", "scatter_face_grads"}
    in_order = {"sample_points_face_sums_ordered_pass1", "sample_points_face_sums_ordered_pass2", "scatter_face_grads_ordered_pass1"}
    assert (in_order <= ran and not (atomic & ran)) if ordered else (atomic <= ran and not (in_order & ran)), sorted(ran)
    if ordered:
        # pass2_kernel beyond its first block of 256 waves, and the one face of mesh 0 a segment over more than 256 waves
        num_sorted = int((idx >= 0).sum())
        assert -(-num_sorted // 64) > 256 and int((idx == 0).sum()) // 64 > 256
        again = _long_grad(which, True)[0]
        other = _long_grad(which, True, stream=torch.cuda.Stream(device=_dev()))[0]
        assert torch.equal(got, again) and torch.equal(got, other)


# ---- B. sample_points forward with many small meshes -----------------------------------------------------------------------------------------
def test_many_small_meshes_with_runs_of_empty_ones():
    verts, faces, first, nf = SP.many_small_meshes()
    SP.small_meshes_reach(first, nf, faces.shape[0])
    u = SP.uniforms(700, 65, 82)
    samples, normals, idx, bary, table, areas = _sample(verts, faces, first, nf, 65, u)
    SP.gate_small_meshes(verts, faces, first, nf, u, areas, table, samples, normals, idx, bary)


# ---- C. fps ties on every rung -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [3, 2])
@pytest.mark.parametrize("P", FB.TIE_P)
def test_fps_orders_equal_minima_on_every_rung(P, D):
    from pytorch3d_amd import _lib

    fps_mod = importlib.import_module("pytorch3d_amd.sample_farthest_points")
    assert _lib.FPS_REGISTER_POINTS == 16384
    points, lengths, start = FB.tie_clouds(P, D)
    want, tied = FB.fps64(points, lengths, FB.TIE_K, start)
    FB.tie_reach(P, lengths, tied, want)
    d = _dev()
    assert fps_mod.kernel_path(points.to(d))
    (sel, idx), ran = _profiled(lambda: _p3d().sample_farthest_points(points.to(d), torch.tensor(lengths, device=d), FB.TIE_K,
                                                                      start_idxs=start.to(d)))
    assert ("sample_farthest_points_workspace" in ran) == (FB.fps_plan(P)[1] == 0), sorted(ran)
    FB.gate_fps_ties(points, lengths, start, idx, sel, want)
    cpu_sel, cpu_idx = _p3d().sample_farthest_points(points, torch.tensor(lengths), FB.TIE_K, start_idxs=start)
    assert torch.equal(idx.cpu(), cpu_idx) and torch.equal(sel.cpu(), cpu_sel)


# ---- D. points_to_volumes at size and at the remaining channel counts ----------------------------------------------------------------------
def _calls():
    from pytorch3d_amd import _C

    return dict(_C.POINTS_TO_VOLUMES_CALLS)


def _run(case, inp, form):
    """run_operators on the kernels in the form asked for, asserted to be the form that ran."""
    m = _p2v()
    before = _calls()
    with _flag(form == "ordered"):
        got = PV.run_operators(case, inp, _dev(), m.points_to_volumes_forward_op, m.points_to_volumes_backward_op)
    after = _calls()
    assert after[form] == before[form] + 1 and sum(after.values()) == sum(before.values()) + 1
    return got


@pytest.mark.parametrize("form", ["atomic", "ordered"])
@pytest.mark.parametrize("case", PV.generated_cases("long", "channels0", "channels2", "channels4", "channels8"), ids=PV.case_id)
def test_kernels_equal_the_restatement_on_the_generated_cases(case, form):
    inp = PV.inputs(case)
    if case[1] == "long":
        waves, none, _ = PV.ordered_reach(case, inp)  # > 256 waves (trilinear), whole waves of -1 keys, a voxel cut by a wave border
        assert waves == (938 if case[2] == "trilinear" else 118)
    got = _run(case, inp, form)
    PV.judge(case, inp, got, recorded=False)
    C = inp["features"].shape[2]
    assert got["features"].shape[1] == C and got["grad_points_features"].shape[2] == C
    if C == 0 and case[2] == "trilinear":
        assert got["grad_points_3d"].abs().sum() > 0


@pytest.mark.parametrize("form", ["atomic", "ordered"])
@pytest.mark.parametrize("mode", ["trilinear", "nearest"])
def test_bad_coordinates_are_skipped_by_the_kernels(mode, form):
    case, inp, good, inp_good = PV.bad_coordinate_inputs(mode)
    PV.judge_bad_coordinates(case, _run(case, inp, form), good, inp_good)


@pytest.mark.parametrize("form", ["atomic", "ordered"])
@pytest.mark.parametrize("case", PV.generated_cases("oversized"), ids=PV.case_id)
def test_a_grid_larger_than_the_tensor_is_cut_at_the_tensors_extent(case, form):
    m = _p2v()
    before = _calls()
    with _flag(form == "ordered"):
        inp, got, buffers = PV.run_oversized(case, _dev(), m.points_to_volumes_forward_op, m.points_to_volumes_backward_op)
    assert _calls()[form] == before[form] + 1
    PV.judge(case, inp, got, recorded=False)
    assert all(PV.poison_untouched(buf, shape) for buf, shape in buffers)


@pytest.mark.parametrize("form", ["atomic", "ordered"])
@pytest.mark.parametrize("mode", ["trilinear", "nearest"])
def test_a_transposed_mask_gives_the_bits_of_the_contiguous_one(mode, form):
    case = ("lattice", "mixed_grids", mode, True)
    inp = PV.inputs(case)
    strided = PV.transposed(inp["mask"])
    assert strided.to(_dev()).stride() == (1, 2) and torch.equal(strided, inp["mask"])
    a, b = _run(case, inp, form), _run(case, dict(inp, mask=strided), form)
    assert all(torch.equal(a[k], b[k]) for k in a)
    PV.judge(case, inp, b)
