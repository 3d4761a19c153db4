"""The HIP kernels against the REFERENCE'S OWN DEVICE KERNELS on the same MI355X.

oracle/_ref/p3d_ref_hip_nofma.so = the reference's hot-path .cu files, translated by torch's hipify and compiled for
gfx950 with -ffp-contract=off (oracle/build_ref_hip.py; a checker, never part of the product).  With contraction off
the reference's device code evaluates exactly the expression trees SURVEY.md appendix A lists, so:

  * pix_to_face / point idx must be IDENTICAL and zbuf / bary / dists BIT-EQUAL between our kernels and the
    reference's -- this pins the "CUDA order" branch of the C oracle (and our kernels) to the reference's device code bit
    for bit, at small sizes, on the cow (BASELINE configs[1]) and on bench meshes at 512^2 (configs[2]);
  * the one documented deviation is the order / eviction among entries whose depths tie EXACTLY: we keep the total order
    (z, index) of the reference's CPU and Python implementations, the reference's CUDA queue evicts the first maximum
    it finds and bubble-sorts by z alone (SURVEY appendix A "Top-K").  Exact ties are common with clipped barycentrics
    (two faces seen from outside across their shared edge both clip to that edge).  So: zbuf must be bit-equal
    everywhere, and wherever the index agrees bary / dists must be bit-equal; index differences may only sit in slots
    whose depth ties with another candidate, their count is printed.

oracle/_ref/p3d_ref_hip.so (hipcc defaults: FMA contraction, like nvcc's -fmad=true) is what a user of the reference would
run: against it the north_star tolerances apply (indices equal up to tie swaps, floats within 1e-5).
"""
import math
import os

import numpy as np
import pytest
import torch

import _util as U
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SOFTRAS_BLUR = math.log(1.0 / 1e-4 - 1.0) * 1e-4


def _need(nofma):
    m = orc.ref_hip_module(nofma=nofma)
    if m is None:
        pytest.skip("oracle/_ref/p3d_ref_hip*.so not built (oracle/build_ref_hip.py, build container only)")
    return m


def _d():
    return torch.device("cuda:0")


def _both(mod, fv, first, count, nbr, size, blur, K, bin_size, M, persp=True, clip=True, cull=False):
    from pytorch3d_amd import _C

    d = _d()
    args = (fv.to(d), first.to(d), count.to(d), nbr.to(d), size, blur, K, bin_size, M, persp, clip, cull)
    ours = _C.rasterize_meshes(*args)
    theirs = mod.rasterize_meshes(*args)
    torch.cuda.synchronize()
    return [o.cpu() for o in ours], [t.cpu() for t in theirs]


def _assert_equal_up_to_exact_depth_ties(tag, ours, theirs, max_frac=2e-3):
    n_idx, bit, diffs = _cmp(tag, ours, theirs)
    assert bit[0], f"{tag}: zbuf is not bit-equal"
    assert max(diffs) == 0.0, f"{tag}: bary / dists differ where the index agrees: {diffs}"
    if n_idx:
        # a differing slot must tie in depth with a neighbouring slot of its pixel, or be the last slot (the tie partner
        # is the candidate that was evicted)
        z = ours[1]
        K = z.shape[-1]
        tie_prev = torch.zeros_like(z, dtype=torch.bool)
        tie_prev[..., 1:] = z[..., 1:] == z[..., :-1]
        tie_next = torch.zeros_like(z, dtype=torch.bool)
        tie_next[..., :-1] = z[..., :-1] == z[..., 1:]
        last = torch.zeros_like(z, dtype=torch.bool)
        last[..., K - 1] = True
        diff = ours[0] != theirs[0]
        unexplained = int((diff & ~(tie_prev | tie_next | last)).sum())
        print(f"[{tag}] {n_idx} index differences, all at exact depth ties: {unexplained == 0}")
        assert unexplained == 0
        assert n_idx <= max_frac * diff.numel()
    return n_idx


def _cmp(tag, ours, theirs):
    same = ours[0] == theirs[0]
    n_idx = int((~same).sum())
    bit = [bool(torch.equal(a, b)) for a, b in zip(ours[1:], theirs[1:])]
    diffs = []
    for a, b in zip(ours[1:], theirs[1:]):
        m = same[..., None].expand_as(a) if a.dim() == 5 else same
        diffs.append(float((a[m] - b[m]).abs().max()) if m.any() else 0.0)
    print(f"[{tag}] idx mismatches {n_idx} / {same.numel()}; zbuf/bary/dists bit-equal {bit}; max diff where idx agrees {diffs}")
    return n_idx, bit, diffs


@pytest.mark.parametrize("persp,clip,cull", [(False, False, False), (True, False, False), (True, True, False), (True, True, True)])
def test_small_soups_bit_equal_to_reference_device_code(persp, clip, cull):
    mod = _need(True)
    gen = torch.Generator().manual_seed(7)
    F, N, K = 300, 3, 4
    fv = U.triangle_soup(F, gen, behind_every=11)
    first, count = U.split_counts(F, N)
    nbr = torch.full((F,), -1, dtype=torch.int64)
    for size, blur, bs in (((64, 64), 0.0, 0), ((64, 64), 0.01, 16), ((48, 80), 0.003, 0), ((80, 48), 0.003, 8)):
        ours, theirs = _both(mod, fv, first, count, nbr, size, blur, K, bs, 400 if bs else 0, persp, clip, cull)
        _assert_equal_up_to_exact_depth_ties(f"soup {size} blur {blur} bin {bs}", ours, theirs)


@pytest.fixture
def cuda_tie_order():
    from pytorch3d_amd import _C

    saved = _C.CUDA_TIE_ORDER
    _C.CUDA_TIE_ORDER = True
    yield _C
    _C.CUDA_TIE_ORDER = saved


@pytest.mark.parametrize("K", [1, 2, 3, 4, 8, 12, 20, 60])
def test_cuda_tie_order_is_the_references_device_result_where_depths_tie_exactly(cuda_tie_order, K):
    """`_C.CUDA_TIE_ORDER` (include/p3d_amd.h: P3D_RASTER_CUDA_TIE_ORDER): a soup in which every face exists three times
    (exact depth ties at every sample, at every place of the queue) and every eighth face has a clipped-face neighbour: with the
    switch on, ALL FOUR outputs equal the reference's device kernels bit for bit -- naive and binned, three flag sets; with it
    off the indices differ (the test has teeth).  270 faces: ONE 512-face chunk of the reference's coarse stage, whose bins
    are then in ascending face order -- see the next test."""
    _C = cuda_tie_order
    mod = _need(True)
    gen = torch.Generator().manual_seed(100 + K)
    base = U.triangle_soup(90, gen, behind_every=13)
    order = torch.randperm(270, generator=gen)
    fv = base.repeat(3, 1, 1)[order].contiguous()  # copies of a face at scattered indices
    F = fv.shape[0]
    nbr = torch.full((F,), -1, dtype=torch.int64)
    for a in range(0, F - 1, 8):
        nbr[a], nbr[a + 1] = a + 1, a
    first, count = U.split_counts(F, 2)
    differed = 0
    # (48, 80) with bin_size 12: internal bins that are NOT whole 8 x 8 sub-tiles -- the lane-mask words of the marks would be shared
    # between sub-tiles of neighbouring bins there, so that launch marks in place (raster_mesh.hip: words_ok)
    for (size, blur, bs), (persp, clip, cull) in zip((((40, 40), 0.01, 0), ((64, 48), 0.004, 16), ((33, 70), 0.0, 8), ((48, 80), 0.004, 12)),
                                                     ((True, True, False), (False, False, False), (True, False, True), (True, True, False))):
        _C.CUDA_TIE_ORDER = True
        ours, theirs = _both(mod, fv, first, count, nbr, size, blur, K, bs, 400 if bs else 0, persp, clip, cull)
        assert torch.equal(ours[0], theirs[0]), f"K={K} {size} bin {bs}: {int((ours[0] != theirs[0]).sum())} indices differ"
        for name, x, y in zip(("zbuf", "bary", "dists"), ours[1:], theirs[1:]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"K={K} {size} bin {bs}: {name}"
        _C.CUDA_TIE_ORDER = False
        plain, _ = _both(mod, fv, first, count, nbr, size, blur, K, bs, 400 if bs else 0, persp, clip, cull)
        differed += int((plain[0] != theirs[0]).sum())
    if K <= 8:  # (beyond: few pixels of this soup collect K hits)
        assert differed > 0, "the soup was meant to hold boundary ties"


@pytest.mark.parametrize("K", [2, 5, 8, 20])
def test_cuda_tie_order_flag_with_and_without_room_for_the_marks(K):
    """The replay finds its pixels through the lane masks the fine kernel leaves in the LAST bytes of the workspace, or -- when the
    caller's workspace has no room for them (include/p3d_amd.h: P3D_RASTER_CUDA_TIE_ORDER) -- through the marks in the
    output itself (the naive launch without a workspace): same bits either way, and the same as the binned launch on a worst-case,
    a short and an overflowing workspace, on the soup of the test above (every face three times: exact depth ties everywhere, every eighth face with a clipped neighbour)."""
    import ctypes

    from pytorch3d_amd import _C, _lib

    lib = _lib.load()
    d = _d()
    gen = torch.Generator().manual_seed(300 + K)
    base = U.triangle_soup(90, gen, behind_every=13)
    order = torch.randperm(270, generator=gen)
    fv = base.repeat(3, 1, 1)[order].contiguous().to(d)
    F = fv.shape[0]
    nbr = torch.full((F,), -1, dtype=torch.int64)
    for a in range(0, F - 1, 8):
        nbr[a], nbr[a + 1] = a + 1, a
    nbr = nbr.to(d)
    first, count = [t.to(d) for t in U.split_counts(F, 2)]
    N, H, W = 2, 72, 56
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(bin_size, M, nbytes):
        out = _C._mesh_outputs(N, H, W, K, d)
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=d) if nbytes is not None else None
        rc = lib.p3d_rasterize_meshes_ex(_C._ptr(fv), _C._ptr(first), _C._ptr(count), _C._ptr(nbr), F, N, H, W, 0.004, K, bin_size,
                                         M, 1, 1, 0, _C._ptr(out[0]), _C._ptr(out[1]), _C._ptr(out[2]), _C._ptr(out[3]), None,
                                         _lib.RASTER_CUDA_TIE_ORDER, _C._ptr(ws) if ws is not None else None, nbytes or 0, stream)
        _lib.check(rc, "rasterize_meshes_ex (CUDA tie order)")
        torch.cuda.synchronize()
        assert int((out[0] == -2).sum()) == 0, "a mark survived the replay"
        return out

    marks = N * ((H + 7) // 8) * ((W + 7) // 8) * 8 + 1024
    naive_without = run(0, 0, None)
    naive_with = run(0, 0, marks)
    worst = lib.p3d_rasterize_meshes_workspace_bytes(F, N, H, W, 16, 400)
    short = lib.p3d_rasterize_meshes_short_workspace_bytes(F, N, H, W, 16, 400, 20 * F)
    binned_with = run(16, 400, worst)
    binned_short = run(16, 400, short)  # the marks come off the end of whatever the caller gave: the lists get what is left
    binned_tiny = run(16, 400, lib.p3d_rasterize_meshes_short_workspace_bytes(F, N, H, W, 16, 400, 0))  # lists overflow: naive fallback
    for name, got in (("naive, marks in the workspace", naive_with), ("binned, worst-case workspace", binned_with),
                      ("binned, short workspace", binned_short), ("binned, lists overflow", binned_tiny)):
        assert torch.equal(got[0], naive_without[0]), f"K={K} {name}: {int((got[0] != naive_without[0]).sum())} indices differ"
        for x, y in zip(got[1:], naive_without[1:]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"K={K} {name}"
    mod = orc.ref_hip_module(nofma=True) if hasattr(orc, "ref_hip_module") else None
    if mod is not None:
        theirs = mod.rasterize_meshes(fv, first, count, nbr, (H, W), 0.004, K, 0, 0, True, True, False)
        assert torch.equal(naive_without[0], theirs[0])


def test_cuda_tie_order_on_bench_meshes_equals_the_references_naive_device_kernel(cuda_tie_order):
    """Two meshes of the bench batch (config 3 as written) at 512^2, K = 8: our binned launch with the CUDA tie order against the
    reference's NAIVE device kernel (every pixel walks its mesh's faces in ascending index, rasterize_meshes.cu:300-320) -- all
    four outputs bit-equal.  The reference's BINNED device path is not a fixed target at ties: its coarse stage appends the
    faces of each 512-face chunk to a bin at an offset taken with atomicAdd (rasterize_coarse.cu:185), so the order of a bin's
    faces across chunks, and with it which of several equally deep faces survives at the K-th place, is whatever order the
    chunks' workgroups arrived in; the count of entries in which the reference's own two paths differ is printed."""
    _C = cuda_tie_order
    mod = _need(True)
    verts, faces = U.hetero_batch(64, seed=0, torus_div=U.CONFIG3_TORUS_DIV)
    nf = [int(f.shape[0]) for f in faces]
    order = sorted(range(64), key=lambda i: nf[i])
    pick = [order[40], order[20]]
    from pytorch3d_amd import PackedMeshes

    m = PackedMeshes([verts[i] for i in pick], [faces[i] for i in pick])
    fv = m.verts_packed()[m.faces_packed()].contiguous()
    first, count = m.mesh_to_faces_packed_first_idx(), m.num_faces_per_mesh()
    F = fv.shape[0]
    nbr = torch.full((F,), -1, dtype=torch.int64)
    d = _d()
    dev = [t.to(d) for t in (fv, first, count, nbr)]
    M = int(max(10000, F / 5))
    ours = _C.rasterize_meshes(*dev, (512, 512), SOFTRAS_BLUR, 8, 32, M, True, True, False)
    naive = mod.rasterize_meshes(*dev, (512, 512), SOFTRAS_BLUR, 8, 0, 0, True, True, False)
    binned = mod.rasterize_meshes(*dev, (512, 512), SOFTRAS_BLUR, 8, 32, M, True, True, False)
    torch.cuda.synchronize()
    _C.CUDA_TIE_ORDER = False
    plain = _C.rasterize_meshes(*dev, (512, 512), SOFTRAS_BLUR, 8, 32, M, True, True, False)
    n = ours[0].numel()
    print(f"[bench meshes {[nf[i] for i in pick]} faces, 512^2, K=8] pix_to_face entries differing from the reference's naive device "
          f"kernel: ours with the (z, index) order {int((plain[0] != naive[0]).sum())}, ours with the CUDA tie order "
          f"{int((ours[0] != naive[0]).sum())}, the reference's own binned path {int((binned[0] != naive[0]).sum())} (of {n})")
    assert torch.equal(ours[0], naive[0])
    for x, y in zip(ours[1:], naive[1:]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert int((plain[0] != naive[0]).sum()) > 0  # the ties are there


@pytest.mark.parametrize("K", [1, 2, 5, 8, 10, 40, 70, 120])
def test_points_cuda_tie_order_equals_the_references_naive_device_kernel(cuda_tie_order, K):
    """rasterize_points with `_C.CUDA_TIE_ORDER`: a cloud in which every point exists three times (same position and depth,
    scattered indices) at radii that put dozens of them on a pixel -- exact depth ties at every place of the queue.  idx, zbuf and
    dists of the naive and the binned launch equal the reference's NAIVE device kernel bit for bit (its binned path orders a bin
    across 512-point chunks by atomicAdd arrival, rasterize_coarse.cu:185); without the switch the indices differ."""
    _C = cuda_tie_order
    mod = _need(True)
    d = _d()
    gen = torch.Generator().manual_seed(300 + K)
    base = torch.rand((700, 3), generator=gen) * torch.tensor([2.0, 2.0, 2.0]) - torch.tensor([1.0, 1.0, -0.1])
    base[::41, 2] = -0.3
    order = torch.randperm(2100, generator=gen)
    pts = base.repeat(3, 1)[order].contiguous().to(d)
    rad = (torch.rand((700,), generator=gen) * 0.25 + 0.05).repeat(3)[order].contiguous().to(d)
    first = torch.tensor([0, 900], dtype=torch.int64, device=d)
    count = torch.tensor([900, 1200], dtype=torch.int64, device=d)
    differed = 0
    for size, bs in (((48, 48), 0), ((64, 40), 16), ((33, 70), 8)):
        theirs = mod.rasterize_points(pts, first, count, size, rad, K, 0, 0)
        _C.CUDA_TIE_ORDER = True
        ours = _C.rasterize_points(pts, first, count, size, rad, K, bs, 3000 if bs else 0)
        assert torch.equal(ours[0], theirs[0]), f"K={K} {size} bin {bs}: {int((ours[0] != theirs[0]).sum())} indices differ"
        assert torch.equal(ours[1].view(torch.int32), theirs[1].view(torch.int32))
        assert torch.equal(ours[2].view(torch.int32), theirs[2].view(torch.int32))
        _C.CUDA_TIE_ORDER = False
        plain = _C.rasterize_points(pts, first, count, size, rad, K, bs, 3000 if bs else 0)
        differed += int((plain[0] != theirs[0]).sum())
    if 2 <= K <= 40:  # (K = 1: both procedures keep the lowest index of the nearest depth)
        assert differed > 0, "the cloud was meant to hold boundary ties"


def test_cow_and_bench_meshes_bit_equal_to_reference_device_code():
    mod = _need(True)
    g = np.load(os.path.join(U.GOLDEN, "cow_ref.npz"))
    fv = torch.from_numpy(g["verts_ndc"])[torch.from_numpy(g["faces"]).long()].contiguous()
    F = fv.shape[0]
    first = torch.zeros(1, dtype=torch.int64)
    count = torch.tensor([F], dtype=torch.int64)
    nbr = torch.full((F,), -1, dtype=torch.int64)
    ours, theirs = _both(mod, fv, first, count, nbr, (256, 256), 1e-4, 8, 16, 10000)
    _assert_equal_up_to_exact_depth_ties("cow 256^2 K=8 (configs[1])", ours, theirs)
    # configs[2]: four bench meshes incl. the largest, 512^2, K=8, SoftRas blur; bin_size 32, M large enough for 20k faces
    verts, faces = U.hetero_batch(64, seed=0, torus_div=U.CONFIG3_TORUS_DIV)
    nf = [int(f.shape[0]) for f in faces]
    order = sorted(range(64), key=lambda i: nf[i])
    pick = [order[-1], order[0], order[32], order[48]]
    from pytorch3d_amd import PackedMeshes

    m = PackedMeshes([verts[i] for i in pick], [faces[i] for i in pick])
    fv = m.verts_packed()[m.faces_packed()].contiguous()
    first, count = m.mesh_to_faces_packed_first_idx(), m.num_faces_per_mesh()
    nbr = torch.full((fv.shape[0],), -1, dtype=torch.int64)
    ours, theirs = _both(mod, fv, first, count, nbr, (512, 512), SOFTRAS_BLUR, 8, 32, 10000)
    _assert_equal_up_to_exact_depth_ties("bench meshes 512^2 K=8 (configs[2], tori unscaled)", ours, theirs)
    # backward on the same fragments: the reference's device backward vs ours
    from pytorch3d_amd import _C

    d = _d()
    gen = torch.Generator().manual_seed(231)
    gz = torch.randn(ours[1].shape, generator=gen).to(d)
    gb = torch.randn(ours[2].shape, generator=gen).to(d)
    gd = torch.randn(ours[3].shape, generator=gen).to(d)
    a = _C.rasterize_meshes_backward(fv.to(d), ours[0].to(d), gz, gb, gd, True, True)
    b = mod.rasterize_meshes_backward(fv.to(d), ours[0].to(d), gz, gb, gd, True, True)
    # gate (tests/_util.py): float64 restatement of the reference's formulas, error against the sum of the absolute
    # per-sample terms; the reference's device result is judged by the same gate and ours must agree with it where it passes
    U.assert_face_grads_vs_truth("bench meshes backward vs float64 / reference device backward", a, fv.to(d), ours[0].to(d), gz, gb, gd,
                                 True, True, reference=b.to(d))


def test_points_and_compositors_vs_reference_device_code():
    mod = _need(True)
    from pytorch3d_amd import _C

    d = _d()
    gen = torch.Generator().manual_seed(3)
    P, H, W, K, r = 200_000, 256, 256, 10, 0.02
    pts = torch.cat([torch.rand(P, 2, generator=gen) * 2 - 1, torch.rand(P, 1, generator=gen) * 2 + 0.5], 1).to(d)
    first = torch.zeros(1, dtype=torch.int64, device=d)
    count = torch.full((1,), P, dtype=torch.int64, device=d)
    radius = torch.full((P,), r, device=d)
    a = _C.rasterize_points(pts, first, count, (H, W), radius, K, 32, 100000)
    b = mod.rasterize_points(pts, first, count, (H, W), radius, K, 32, 100000)
    # the reference's point queue orders by z alone; ours by (z, idx): indices may differ only where depths tie exactly
    assert torch.equal(a[1], b[1]), "zbuf"
    same = a[0] == b[0]
    z = a[1]
    tie = torch.zeros_like(same)
    tie[..., 1:] |= z[..., 1:] == z[..., :-1]
    tie[..., :-1] |= z[..., :-1] == z[..., 1:]
    tie[..., K - 1] = True
    print(f"[points] idx differences {int((~same).sum())} / {same.numel()}, all at exact depth ties: {bool((same | tie).all())}")
    assert bool((same | tie).all()) and int((~same).sum()) < 1e-4 * same.numel()
    assert torch.equal(a[2][same], b[2][same])
    idx = a[0].long().permute(0, 3, 1, 2)
    alphas = (1 - a[2] / (r * r)).clamp(0, 1).permute(0, 3, 1, 2)
    feats = torch.rand(5, P, generator=gen).to(d)
    for name in ("accum_alphacomposite", "accum_weightedsumnorm", "accum_weightedsum"):
        o = getattr(_C, name)(feats, alphas, idx)
        t = getattr(mod, name)(feats, alphas.contiguous(), idx.contiguous())
        assert torch.allclose(o, t, atol=1e-6, rtol=1e-6), name
        go = torch.randn(o.shape, generator=gen).to(d)
        gf, ga = getattr(_C, name + "_backward")(go, feats, alphas, idx)
        tf, ta = getattr(mod, name + "_backward")(go, feats, alphas.contiguous(), idx.contiguous())
        assert torch.allclose(gf, tf, atol=1e-4, rtol=1e-4) and torch.allclose(ga, ta, atol=1e-5, rtol=1e-4), name


@pytest.mark.parametrize("K", [10, 24])
def test_config4_at_full_size_vs_reference_device_code(K):
    """K = 10 and K = 24 (round 5): `point_tile_sorted_kernel`, queues in LDS (K = 24: 48 KB per workgroup), at the same size.  BASELINE configs[3] exactly as `bench.py` times it (other_configs: 1M points xy ~ U(-1,1), z ~ U(0.5,2.5), seed 0,
    radius 0.01, 512^2, K = 10, bin_size 32, features (3, P)): rasterizer + alpha compositor, forward and
    backward, against the reference's device kernels (rasterize_points.cu:87-217, 366-462; alpha_composite.cu:24-233; the
    reference takes ~96 ms for it on this GPU).  zbuf bit-equal; idx differences only at exact depth ties; dists bit-equal where
    idx agrees; compositor within 1e-6; gradients within the reference's own tolerances (tests/test_rasterize_points.py:234
    atol 2e-6 on grad_points for unit upstreams -- here the upstreams are N(0,1) and ~80 entries meet per point: 1e-4 of the
    largest entry; tests/test_compositing.py:207 atol 1e-6 -> rtol 1e-4 on sums of ~10 terms)."""
    mod = _need(True)
    from pytorch3d_amd import _C

    d = _d()
    gen = torch.Generator().manual_seed(0)
    P, H, r, C = 1_000_000, 512, 0.01, 3
    pts = torch.cat([torch.rand(P, 2, generator=gen) * 2 - 1, torch.rand(P, 1, generator=gen) * 2 + 0.5], 1).to(d)
    feats = torch.rand(C, P, generator=gen).to(d)
    first = torch.zeros(1, dtype=torch.int64, device=d)
    count = torch.full((1,), P, dtype=torch.int64, device=d)
    radius = torch.full((P,), r, device=d)
    gz = torch.randn((1, H, H, K), generator=gen).to(d)
    gd = torch.randn((1, H, H, K), generator=gen).to(d)
    gi = torch.randn((1, C, H, H), generator=gen).to(d)
    a = _C.rasterize_points(pts, first, count, (H, H), radius, K, 32, 200000)
    b = mod.rasterize_points(pts, first, count, (H, H), radius, K, 32, 200000)
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), "zbuf is not bit-equal at 1M points"
    same = a[0] == b[0]
    z = a[1]
    tie = torch.zeros_like(same)
    tie[..., 1:] |= z[..., 1:] == z[..., :-1]
    tie[..., :-1] |= z[..., :-1] == z[..., 1:]
    tie[..., K - 1] = True
    n_idx = int((~same).sum())
    print(f"[config 4, 1M points 512^2 K={K}] idx differences {n_idx} / {same.numel()}, not at an exact depth tie: "
          f"{int((~same & ~tie).sum())}; slot fill {float((a[0] >= 0).float().mean()):.3f}")
    assert bool((same | tie).all()) and n_idx <= 1e-4 * same.numel()
    assert torch.equal(a[2].view(torch.int32)[same], b[2].view(torch.int32)[same]), "dists differ where the index agrees"
    # compositor on OUR fragments through both implementations (the permuted views the reference's Python hands over)
    alphas = (1 - a[2] / (r * r)).clamp(0, 1).permute(0, 3, 1, 2)
    pidx = a[0].long().permute(0, 3, 1, 2)
    img = _C.accum_alphacomposite(feats, alphas, pidx)
    img_ref = mod.accum_alphacomposite(feats, alphas.contiguous(), pidx.contiguous())
    assert float((img - img_ref).abs().max()) <= 1e-6
    gf, ga = _C.accum_alphacomposite_backward(gi, feats, alphas, pidx)
    gf_ref, ga_ref = mod.accum_alphacomposite_backward(gi, feats, alphas.contiguous(), pidx.contiguous())
    assert torch.allclose(ga, ga_ref, atol=1e-5, rtol=1e-4)
    assert float((gf - gf_ref).abs().max()) <= 1e-4 * float(gf_ref.abs().max())
    gp = _C.rasterize_points_backward(pts, a[0], gz, gd)
    gp_ref = mod.rasterize_points_backward(pts, a[0], gz, gd)
    assert float((gp - gp_ref).abs().max()) <= 1e-4 * float(gp_ref.abs().max())
    assert int((gp != 0).any(1).sum()) == int((gp_ref != 0).any(1).sum())


def test_against_the_default_build_of_the_reference_within_north_star_tolerances():
    """hipcc's default flags contract mul+add into FMA (as nvcc does): depths move by an ulp, ties at shared edges may
    swap.  north_star: indices equal (up to such swaps), zbuf / bary / dists within 1e-5."""
    mod = _need(False)
    verts, faces = U.hetero_batch(3, seed=5, fmin=2000, fmax=8000)
    from pytorch3d_amd import PackedMeshes

    m = PackedMeshes(verts, faces)
    fv = m.verts_packed()[m.faces_packed()].contiguous()
    first, count = m.mesh_to_faces_packed_first_idx(), m.num_faces_per_mesh()
    nbr = torch.full((fv.shape[0],), -1, dtype=torch.int64)
    ours, theirs = _both(mod, fv, first, count, nbr, (512, 512), SOFTRAS_BLUR, 8, 32, 10000)
    n_idx, _, diffs = _cmp("3 meshes 512^2 vs default (FMA) reference build", ours, theirs)
    assert n_idx <= 5e-4 * ours[0].numel()
    assert max(diffs) <= 1e-5
    assert torch.allclose(ours[1], theirs[1], atol=1e-5, rtol=0)
