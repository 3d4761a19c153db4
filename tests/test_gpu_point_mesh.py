"""Point-mesh distances on the GPU (csrc/point_mesh.hip): the kernels against the reference's recorded results
(tests/golden/point_mesh_ref.npz) with the comparisons and tolerances of tests/test_cpu_point_mesh.py, for the four directions, in the
atomic and the ordered backward; the split over waves; determinism; the star; one larger shape against the package's own torch
formulation (which the CPU file pins to the fixture); the fused losses; the shim.
"""
import contextlib
import json
import os
import subprocess
import sys
import warnings

import pytest
import torch

import _util as U
import point_mesh_case as C

pytestmark = pytest.mark.gpu

ROOT = U.ROOT


def _dev():
    return torch.device("cuda:0")


@contextlib.contextmanager
def _flag(on):
    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])


def _op_params():
    return [(kind, name, direction) for kind in C.KINDS for name in C.OP_CASES for direction in C.DIRECTIONS[kind]]


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("kind,name,direction", _op_params())
def test_kernels_match_the_reference(kind, name, direction, ordered):
    from pytorch3d_amd import point_mesh as pm

    z = C.fixture()
    with _flag(ordered):
        got = C.run_direction(pm, z, kind, name, direction, device=_dev())
    C.check_direction(z, kind, name, direction, *got, who="kernels (%s)" % ("ordered" if ordered else "atomic"))


@pytest.mark.parametrize("kind", C.KINDS)
def test_every_split_gives_the_same_bits(kind):
    """Forced split 1, 2, 4, 8 and automatic: on the tile-boundary batch, the ragged batch and one mesh against one scan with many
    tiles per wave (the shape the split is for)."""
    from pytorch3d_amd import _C

    z = C.fixture()
    gen = torch.Generator().manual_seed(11)
    corners = 3 if kind == "tri" else 2
    shapes = [C.op_inputs(z, kind, "tiles", device=_dev()), C.op_inputs(z, kind, "ragged", device=_dev()),
              (torch.rand(700, 3, generator=gen).to(_dev()), torch.zeros(1, dtype=torch.int64, device=_dev()),
               torch.rand(1500, corners, 3, generator=gen).to(_dev()), torch.zeros(1, dtype=torch.int64, device=_dev()), 700, 1500)]
    for points, pfirst, prims, sfirst, max_p, max_s in shapes:
        for direction in C.DIRECTIONS[kind]:
            max_q = max_p if direction.startswith("point") else max_s
            first = _C.point_mesh_forward(direction, points, pfirst, prims, sfirst, max_q, split=1)
            for split in (2, 4, 8, 0):
                d, i = _C.point_mesh_forward(direction, points, pfirst, prims, sfirst, max_q, split=split)
                assert torch.equal(d, first[0]) and torch.equal(i, first[1]), (direction, split)


@pytest.mark.parametrize("kind", C.KINDS)
def test_exact_ties_go_to_the_larger_index(kind):
    from pytorch3d_amd import _C

    points, prims, twin = C.tie_case(kind)
    z1 = torch.zeros(1, dtype=torch.int64, device=_dev())
    a, b = points.to(_dev()), prims.to(_dev())
    for split in (1, 4):
        _, idxs = _C.point_mesh_forward(C.DIRECTIONS[kind][0], a, z1, b, z1, a.shape[0], split=split)
        idxs = idxs.cpu()
        assert torch.equal(twin[idxs], idxs), "the earlier copy of a duplicated primitive was returned"
        assert int((idxs >= 90).sum()) >= 10
        _, idxs = _C.point_mesh_forward(C.DIRECTIONS[kind][1], torch.cat([a, a], 0), z1, b, z1, b.shape[0], split=split)
        assert bool((idxs >= points.shape[0]).all())


def test_the_kernels_write_every_entry_and_rows_without_targets_read_nothing():
    """The batches with an empty cloud and with a mesh without faces, after NaN-filled buffers went back to the allocator (torch.empty
    hands them out again): every entry is written, a row without targets holds FLT_MAX / 0 and gets a zero gradient."""
    from pytorch3d_amd import _C

    z = C.fixture()
    for kind in C.KINDS:
        for name in ("empty_cloud", "empty_mesh"):
            points, pfirst, prims, sfirst, max_p, max_s = C.op_inputs(z, kind, name, device=_dev())
            for direction in C.DIRECTIONS[kind]:
                point_query = direction.startswith("point")
                junk = [torch.full((4096,), float("nan"), device=_dev()) for _ in range(4)]
                del junk
                d, i = _C.point_mesh_forward(direction, points, pfirst, prims, sfirst, max_p if point_query else max_s)
                want_d, want_i = z[C.key(kind, name, "dists", direction)], z[C.key(kind, name, "idxs", direction)]
                none = want_d == C.FLT_MAX
                assert bool(torch.isfinite(d).all()) and torch.equal(d.cpu()[none], want_d[none]) and bool((i.cpu()[none] == 0).all())
                assert bool((i >= 0).all())
                gp, gs = _C.point_mesh_backward(direction, points, prims, i, torch.ones_like(d), 5e-3, pfirst, sfirst)
                gq = (gp if point_query else gs).cpu()
                assert bool((gq[none] == 0).all()) and bool(torch.isfinite(gp).all()) and bool(torch.isfinite(gs).all())


def _star_grad(kind, ordered, stream=None):
    from pytorch3d_amd import point_mesh as pm

    points, prims = C.star_case(kind)
    ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    z1 = torch.zeros(1, dtype=torch.int64, device=_dev())
    with ctx, _flag(ordered):
        a, b = points.to(_dev()), prims.to(_dev()).requires_grad_(True)
        fn = pm.point_face_distance if kind == "tri" else pm.point_edge_distance
        d = fn(a, z1, b, z1, a.shape[0])
        (grad,) = torch.autograd.grad((d * C.upstream(a.shape[0]).to(_dev())).sum(), (b,))
    if stream is not None:
        stream.synchronize()
    return grad


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("kind", C.KINDS)
def test_star_scatter_within_its_bound(kind, ordered):
    """Every point is nearest to primitive 0: its gradient is a sum of 300 terms.  Each term is compared in float64 (the restatement
    on the same pairs); the sum may lose in-degree x 2^-23 x the largest term whatever the order of the additions."""
    points, prims = C.star_case(kind)
    P = points.shape[0]
    up = C.upstream(P).double()
    b = prims.double().requires_grad_(True)
    d = C.pair_dist64(points.double(), b[torch.zeros(P, dtype=torch.int64)])
    terms = torch.stack([torch.autograd.grad(d[q] * up[q], b, retain_graph=True)[0][0] for q in range(P)])  # (P, corners, 3)
    truth = terms.sum(0)
    bound = P * 2.0 ** -23 * float(terms.abs().max())
    got = _star_grad(kind, ordered).cpu().double()
    err = float((got[0] - truth).abs().max())
    print("star", kind, "ordered" if ordered else "atomic", "error %.3g" % err, "bound %.3g" % bound)
    assert err <= bound and float(got[1].abs().max()) == 0.0


def _loss_run(name, tag, stream=None, ordered=True):
    import pytorch3d_amd as p3d

    z = C.fixture()
    ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    with ctx, _flag(ordered):
        verts, faces, points = C.mesh_inputs(z, name, device=_dev())
        meshes, pcls = p3d.PackedMeshes(verts, faces), p3d.PackedPointclouds(points)
        loss = p3d.point_mesh_face_distance(meshes, pcls) if tag == "face" else p3d.point_mesh_edge_distance(meshes, pcls)
        grads = torch.autograd.grad(loss, verts + points)
    if stream is not None:
        stream.synchronize()
    return (loss.detach(),) + tuple(grads)


def test_ordered_backward_and_fused_sums_give_the_same_bits_on_two_runs_and_two_streams():
    torch.cuda.synchronize()
    for kind in C.KINDS:
        first = _star_grad(kind, True)
        torch.cuda.synchronize()
        again, other = _star_grad(kind, True), _star_grad(kind, True, torch.cuda.Stream(device=_dev()))
        torch.cuda.synchronize()
        assert torch.equal(first, again) and torch.equal(first, other), kind
    for tag in ("face", "edge"):
        first = _loss_run("ragged", tag)
        torch.cuda.synchronize()
        again, other = _loss_run("ragged", tag), _loss_run("ragged", tag, torch.cuda.Stream(device=_dev()))
        torch.cuda.synchronize()
        for a, b, c in zip(first, again, other):
            assert torch.equal(a, b) and torch.equal(a, c), tag
        # the forward has no atomic with the flag off either: the loss is the same bits
        assert torch.equal(_loss_run("ragged", tag, ordered=False)[0], first[0])
    with warnings.catch_warnings():  # with the flag off the call neither raises nor warns
        warnings.simplefilter("error")
        _star_grad("tri", False)
    torch.cuda.synchronize()


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("tag", ["face", "edge"])
@pytest.mark.parametrize("name", ["ico2", "ragged"])
def test_fused_losses_match_the_reference(name, tag, ordered):
    got = _loss_run(name, tag, ordered=ordered)
    n = (len(got) - 1) // 2
    C.check_mesh_loss(C.fixture(), name, tag, got[0], got[1:1 + n], got[1 + n:], who="fused (%s)" % ("ordered" if ordered else "atomic"))


def test_small_faces_case_gives_the_same_loss_in_both_vertex_orders():
    """The reference's test_small_faces_case and its own criterion (assertClose: rtol 1e-5, atol 1e-8)."""
    z = C.fixture()
    got = [float(_loss_run(name, "face", ordered=False)[0]) for name in ("small_faces_a", "small_faces_b")]
    for g, name in zip(got, ("small_faces_a", "small_faces_b")):
        want = float(z["mesh/%s/face_loss" % name])
        assert abs(g - want) <= 1e-5 * abs(want) + 1e-8
    assert abs(got[0] - got[1]) <= 1e-5 * abs(got[1]) + 1e-8


def test_fused_losses_never_wait_for_the_device():
    """Both losses, forward and backward, under torch's sync debug mode, on work that has run once before (the topology's edge table is
    built, with host syncs, on the first call and kept)."""
    import pytorch3d_amd as p3d

    z = C.fixture()
    verts, faces, points = C.mesh_inputs(z, "ragged", device=_dev())
    meshes, pcls = p3d.PackedMeshes(verts, faces), p3d.PackedPointclouds(points)
    g = torch.ones((), device=_dev())

    def watched(fn):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            return fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
            torch.cuda.synchronize()

    def forwards():
        return p3d.point_mesh_face_distance(meshes, pcls), p3d.point_mesh_edge_distance(meshes, pcls)

    def backwards(losses):
        return torch.autograd.grad(losses[0], verts + points, g) + torch.autograd.grad(losses[1], verts + points, g)

    backwards(forwards())  # once, unwatched
    losses = watched(forwards)
    grads = watched(lambda: backwards(losses))
    assert all(bool(torch.isfinite(t).all()) for t in grads) and float(grads[0].abs().max()) > 0
    assert losses[0].grad_fn.__class__.__name__.startswith("_PointMeshLoss")  # ONE autograd node


@pytest.mark.parametrize("kind", C.KINDS)
def test_larger_shape_matches_the_torch_formulation(kind):
    """2 x 3000 points x 2000 primitives: the kernels against the package's torch formulation on the same GPU, judged like a fixture
    case -- E from that formulation against float64, indices exact where the float64 gap is at least 16 E."""
    from pytorch3d_amd import point_mesh as pm

    gen = torch.Generator().manual_seed(23)
    corners = 3 if kind == "tri" else 2
    num_points, num_prims = [3000, 3000], [2000, 2000]
    points, prims = torch.rand(6000, 3, generator=gen), torch.rand(4000, corners, 3, generator=gen)
    pfirst, sfirst = C.first_idx(num_points).to(_dev()), C.first_idx(num_prims).to(_dev())
    for direction in C.DIRECTIONS[kind]:
        point_query = direction.startswith("point")
        a, b = points.to(_dev()).requires_grad_(True), prims.to(_dev()).requires_grad_(True)
        best64, gap = C.minima64(a.detach(), b.detach(), num_points, num_prims, point_query)  # float64 on the GPU
        want_d, want_i = pm.torch_forward(direction, a.detach(), pfirst, b.detach(), sfirst)
        up = C.upstream(want_d.shape[0]).to(_dev())
        want_gp, want_gs = pm.torch_backward(direction, a.detach(), b.detach(), want_i, up, 5e-3, pfirst, sfirst)
        E = float((want_d.double() - best64).abs().max())
        gp64, gs64 = C.grads64(a.detach(), b.detach(), want_i, up, torch.ones_like(gap, dtype=torch.bool), point_query)
        Egp, Egs = float((want_gp.double() - gp64).abs().max()), float((want_gs.double() - gs64).abs().max())
        ok = C.admitted(gap, E).cpu()
        assert float(ok.double().mean()) >= 1.0 - C.MAX_DROPPED
        d = getattr(pm, direction + "_distance")(a, pfirst, b, sfirst, 3000 if point_query else 2000)
        i = getattr(pm, direction + "_dist_forward")(a.detach(), pfirst, b.detach(), sfirst, 3000 if point_query else 2000)[1]
        gp, gs = torch.autograd.grad((d * up).sum(), (a, b))
        err = float((d.detach() - want_d).abs().max())
        egp, egs = float((gp - want_gp).abs().max()), float((gs - want_gs).abs().max())
        print("%s: dist error %.3g (4 E = %.3g), grad_points %.3g (%.3g), grad_prims %.3g (%.3g), admitted %d of %d"
              % (direction, err, 4 * E, egp, 4 * Egp, egs, 4 * Egs, int(ok.sum()), ok.numel()))
        assert torch.equal(i.cpu()[ok], want_i.cpu()[ok])
        assert err <= 4 * E and egp <= 4 * Egp and egs <= 4 * Egs


# ---- the shim ------------------------------------------------------------------------------------------------------------------------
def test_shim_serves_and_patches_the_reference_losses():
    stage = os.path.join(ROOT, "oracle", "_ref", "reference_py")
    if not os.path.isdir(os.path.join(stage, "pytorch3d", "loss")):
        pytest.skip("oracle/_ref/reference_py is not staged (run __graft_entry__.build() where the reference exists)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shim_point_mesh_case.py")], capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    if "skipped" in rec:
        pytest.skip(rec["skipped"])
    z = C.fixture()
    assert rec["plain_is_reference"] and rec["patched_everywhere"] and rec["restored"]
    for part in ("plain", "patched", "patched_cpu"):
        for name in ("ico2", "ragged"):
            for tag in ("face", "edge"):
                r = rec[part][name][tag]
                grads = [torch.tensor(g) for g in r["grads"]]
                n = len(grads) // 2
                C.check_mesh_loss(z, name, tag, r["loss"], grads[:n], grads[n:], who="shim %s" % part)
    assert rec["fused_calls"] == {"point_mesh_face_distance": 2, "point_mesh_edge_distance": 2} and rec["fallbacks_in_fused_part"] == 0
    assert rec["cpu_fallback_calls"] == {"point_mesh_face_distance": 2, "point_mesh_edge_distance": 2} and rec["cpu_fused_calls"] == 0
