"""The launches around mesh_fine and mesh_backward that the step no longer makes:

  1. a null clipped_faces_neighbor_idx is an array of -1, bit for bit, in every reader (binned, naive, generic K, the replay
     of the CUDA tie order); a clipped mesh through the mirror keeps its tensor and still matches the oracle;
  2. p3d_rasterize_meshes_verts_ex (the face gather inside the count pass of the binning) writes the bytes of
     p3d_gather_face_verts_pre + p3d_rasterize_meshes_ex: face_verts, face_pre, the four outputs, the cover and its list;
  3. the cover and its list header need no clearing by the caller (the count pass clears them), on the split kernels
     (fewer than 512 tiles) and on the list-from-the-plan path (more than 512 tiles, sides multiples of 16);
  4. the backward's grad_verts cleared by the forward: same gradient, once only, not under use_deterministic_algorithms.

Small meshes throughout: an icosphere of 20 faces, one of 1 280 and a torus of 2 100 (the latter two cross the 1 024-face
chunk of the count pass)."""
import pytest
import torch

import _util as U

pytestmark = pytest.mark.gpu

BLUR = 2e-3


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_BATCH = {}


def _batch(kind="three"):
    """(verts list, faces list) on the CPU, made once.  'three': 20 + 1 280 + 2 100 faces; 'hole': the same with an empty mesh in
    the middle; 'ten': the three, cycled to ten meshes."""
    if kind not in _BATCH:
        gen = torch.Generator().manual_seed(77)
        meshes = [U.ico_sphere(0), U.ico_sphere(3), U.torus(0.45, 1.0, 30, 35)]
        assert [int(f.shape[0]) for _, f in meshes] == [20, 1280, 2100]
        verts = [U.to_ndc(v @ U.random_rotation(gen).T, scale=s) for (v, _), s in zip(meshes, (1.0, 1.0, 0.6))]
        faces = [f for _, f in meshes]
        if kind == "ten":  # the three, cycled: 4 410 tiles at 336 x 336, beyond the single-workgroup scan of small launches
            verts, faces = [verts[i % 3] for i in range(10)], [faces[i % 3] for i in range(10)]
        if kind == "hole":
            verts = [verts[0], torch.zeros((0, 3)), verts[1], verts[2]]
            faces = [faces[0], torch.zeros((0, 3), dtype=torch.int64), faces[1], faces[2]]
        _BATCH[kind] = (verts, faces)
    return _BATCH[kind]


def _packed(verts, faces, d):
    """packed verts (V,3), packed faces (F,3) with the vertex offsets added, first, count -- all on the device."""
    vo, fs = 0, []
    for v, f in zip(verts, faces):
        fs.append(f + vo)
        vo += v.shape[0]
    count = torch.tensor([f.shape[0] for f in faces], dtype=torch.int64)
    first = torch.cumsum(count, 0) - count
    return torch.cat(verts, 0).float().contiguous().to(d), torch.cat(fs, 0).contiguous().to(d), first.to(d), count.to(d)


def _call(d, size, K, bin_size, first, count, F, face_verts=None, packed=None, nbr="tensor", tie=False, cover_fill=0, M=None,
          want_pre=True, want_zero=False):
    """One call of p3d_rasterize_meshes_ex (face_verts given) or p3d_rasterize_meshes_verts_ex (packed = (verts, faces)) with a
    cover-list buffer pre-filled with `cover_fill` bytes.  -> dict of everything the call wrote."""
    from pytorch3d_amd import _C, _lib

    lib = _lib.load()
    H, W = size
    N = int(count.shape[0])
    M = int(M if M is not None else max(F, 1))
    out = _C._mesh_outputs(N, H, W, K, d)
    for o in out:
        o.view(torch.uint8).fill_(0xA5)
    flags = _lib.RASTER_CUDA_TIE_ORDER if tie else _lib.RASTER_COVER_LIST
    words = N * ((H + 15) // 16) * ((W + 15) // 16)
    cover = None
    if not tie:
        cover = torch.full((lib.p3d_rasterize_meshes_cover_list_bytes(N, H, W),), cover_fill, dtype=torch.uint8, device=d).view(torch.int32)
    ws = _C._workspace(lib.p3d_rasterize_meshes_workspace_bytes(F, N, H, W, bin_size, M) if bin_size else
                       (N * ((H + 7) // 8) * ((W + 7) // 8) * 8 + 1024 if tie else 0), d)
    nb = torch.full((F,), -1, dtype=torch.int64, device=d) if nbr == "tensor" else None
    tail = (_C._ptr(first), _C._ptr(count), _C._ptr(nb), F, N, H, W, BLUR, K, bin_size, M if bin_size else 0, 1, 1, 0, _C._ptr(out[0]),
            _C._ptr(out[1]), _C._ptr(out[2]), _C._ptr(out[3]), _C._ptr(cover), flags, _C._ptr(ws), ws.numel(), _C._stream(d))
    res = {}
    if packed is not None:
        verts, faces = packed
        V = int(verts.shape[0])
        fv = torch.full((F, 3, 3), -7.0, device=d)  # a sentinel: what the call does not write stays visible
        pre = torch.full((F, 4), -7.0, device=d) if want_pre else None
        zero = torch.full((V, 3), -7.0, device=d) if want_zero else None
        rc = lib.p3d_rasterize_meshes_verts_ex(_C._ptr(verts), _C._ptr(faces), V, _C._ptr(fv), _C._ptr(pre), _C._ptr(zero), *tail)
        res.update(face_verts=fv, face_pre=pre, zero=zero)
    else:
        rc = lib.p3d_rasterize_meshes_ex(_C._ptr(face_verts), *tail)
    _lib.check(rc, "rasterize_meshes")
    torch.cuda.synchronize()
    res.update(out=out, words=words)
    if cover is not None:
        n = int(cover[words])
        res.update(cover=cover[:words].clone(), count=n, list=cover[words + 16:words + 16 + max(n, 0)].clone())
    return res


def _gather(verts, faces, d):
    from pytorch3d_amd import _C, _lib

    lib = _lib.load()
    V, F = int(verts.shape[0]), int(faces.shape[0])
    fv = torch.full((F, 3, 3), -7.0, device=d)
    fp = torch.full((F, 4), -7.0, device=d)
    if F:
        _lib.check(lib.p3d_gather_face_verts_pre(_C._ptr(verts), _C._ptr(faces), V, F, _C._ptr(fv), _C._ptr(fp), _C._stream(d)), "gather")
    torch.cuda.synchronize()
    return fv, fp


def _bytes_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


def _same_outputs(a, b, what):
    for name, x, y in zip(("pix_to_face", "zbuf", "bary", "dists"), a["out"], b["out"]):
        assert _bytes_equal(x, y), f"{what}: {name} differs"
    if "cover" in a and "cover" in b:
        assert torch.equal(a["cover"], b["cover"]), f"{what}: cover words differ"
        assert a["count"] == b["count"], f"{what}: list counts differ ({a['count']} vs {b['count']})"


# ---------------------------------------------------------------------------------------------------------------------
# 1. null neighbor
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["binned_k8", "naive_k8", "bins12_k5", "tie_order_binned", "tie_order_naive"])
def test_null_neighbor_equals_all_minus_one(case):
    d = _dev()
    verts, faces, first, count = _packed(*_batch(), d)
    fv, _ = _gather(verts, faces, d)
    F = int(faces.shape[0])
    size, K, bin_size, tie = {"binned_k8": ((64, 64), 8, 8, False), "naive_k8": ((64, 64), 8, 0, False),
                              "bins12_k5": ((48, 80), 5, 12, False), "tie_order_binned": ((64, 64), 8, 8, True),
                              "tie_order_naive": ((64, 64), 8, 0, True)}[case]
    a = _call(d, size, K, bin_size, first, count, F, face_verts=fv, nbr="tensor", tie=tie)
    b = _call(d, size, K, bin_size, first, count, F, face_verts=fv, nbr=None, tie=tie)
    hits = int((a["out"][0] >= 0).sum())
    print(f"[{case}] {hits} (pixel, k) hits")
    assert hits > 1000
    _same_outputs(a, b, case)
    if not tie:
        assert torch.equal(a["list"].sort().values, b["list"].sort().values)


def test_mirror_switch_and_clipped_mesh_vs_oracle():
    """The mirror hands no tensor on when nothing is clipped (and the same bits come out as with one); a mesh that IS clipped keeps
    its neighbour tensor and matches the oracle's naive rasterizer on the clipped faces."""
    import pytorch3d_amd as p3d
    from oracle import oracle as orc
    from pytorch3d_amd import _C, clip

    d = _dev()
    verts, faces = _batch()
    m = p3d.PackedMeshes([v.to(d) for v in verts], [f.to(d) for f in faces])
    kw = dict(image_size=64, blur_radius=BLUR, faces_per_pixel=8, perspective_correct=True, clip_barycentric_coords=True)
    assert _C.NULL_NEIGHBOR
    a = p3d.rasterize_meshes(m, **kw)
    _C.NULL_NEIGHBOR = False
    try:
        b = p3d.rasterize_meshes(m, **kw)
    finally:
        _C.NULL_NEIGHBOR = True
    for x, y in zip(a, b):
        assert _bytes_equal(x, y)
    # the 1 280-face sphere pushed towards the camera: the plane z = 1.2 cuts it
    v = verts[1].clone()
    v[:, 2] -= 1.4
    mc = p3d.PackedMeshes([v.to(d)], [faces[1].to(d)])
    zc = 1.2
    got = p3d.rasterize_meshes(mc, z_clip_value=zc, bin_size=8, **kw)
    fr = clip.ClipFrustum(left=-1, right=1, top=-1, bottom=1, perspective_correct=True, z_clip_value=zc, cull=False)
    cf = clip.clip_faces(mc.verts_packed()[mc.faces_packed()], mc.mesh_to_faces_packed_first_idx(), mc.num_faces_per_mesh(), frustum=fr)
    nbr = cf.clipped_faces_neighbor_idx
    assert nbr is not None and int((nbr >= 0).sum()) > 0, "the case must clip faces into pairs"
    ref = orc.rasterize_meshes_naive(cf.face_verts.cpu(), cf.mesh_to_face_first_idx.cpu(), cf.num_faces_per_mesh.cpu(), nbr.cpu(), (64, 64),
                                     BLUR, 8, True, True, False)
    p2f_u, bary_u = clip.convert_clipped_rasterization_to_original_faces(ref[0].to(d), ref[2].to(d), cf)
    assert int((got[0] >= 0).sum()) > 1000
    assert torch.equal(got[0], p2f_u), "pix_to_face of the clipped mesh differs from the oracle"
    assert torch.allclose(got[1].cpu(), ref[1], atol=1e-5, rtol=0) and torch.allclose(got[3].cpu(), ref[3], atol=1e-5, rtol=0)
    assert torch.allclose(got[2], bary_u, atol=1e-5, rtol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the fused entry
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["three", "hole", "bad_ids", "naive", "generic_k5"])
def test_fused_entry_equals_gather_plus_rasterizer(case):
    d = _dev()
    verts, faces, first, count = _packed(*_batch("hole" if case == "hole" else "three"), d)
    if case == "bad_ids":
        faces = faces.clone()
        V = int(verts.shape[0])
        faces[5, 1] -= V           # negative ids wrap once
        faces[1500, 0] -= V
        faces[7, 2] = V            # out of range: NaN corners, nothing read
        faces[2000, 1] = -V - 1
        faces[3399, 0] = 1 << 40
    F = int(faces.shape[0])
    size, K, bin_size = ((48, 80), 5, 12) if case == "generic_k5" else ((64, 64), 8, 0 if case == "naive" else 8)
    fv, fp = _gather(verts, faces, d)
    a = _call(d, size, K, bin_size, first, count, F, face_verts=fv)
    b = _call(d, size, K, bin_size, first, count, F, packed=(verts, faces), want_zero=True, cover_fill=0xFF)
    assert _bytes_equal(b["face_verts"], fv), "face_verts differs from p3d_gather_face_verts_pre"
    assert _bytes_equal(b["face_pre"], fp), "face_pre differs from p3d_gather_face_verts_pre"
    assert not bool((fv == -7.0).all(-1).all(-1).any()), "the stand-alone gather left a face unwritten"
    if case == "bad_ids":
        assert bool(torch.isnan(fv[7, 2]).all()) and bool(torch.isnan(fv[2000, 1]).all()) and bool(torch.isnan(fv[3399, 0]).all())
        assert bool(torch.isfinite(fv[5]).all()) and bool(torch.isfinite(fv[1500]).all())
    assert int((b["zero"] != 0).sum()) == 0, "zero_verts was not cleared"
    assert int((a["out"][0] >= 0).sum()) > 1000
    _same_outputs(a, b, case)
    assert torch.equal(a["list"].sort().values, b["list"].sort().values)
    # without the records and without the buffer to clear
    c = _call(d, size, K, bin_size, first, count, F, packed=(verts, faces), want_pre=False)
    assert _bytes_equal(c["face_verts"], fv)
    _same_outputs(a, c, case + " (no records)")


def test_fused_entry_with_no_faces():
    d = _dev()
    verts = torch.rand(5, 3, device=d)
    faces = torch.zeros((0, 3), dtype=torch.int64, device=d)
    first, count = torch.zeros(2, dtype=torch.int64, device=d), torch.zeros(2, dtype=torch.int64, device=d)
    for bin_size in (8, 0):
        r = _call(d, (32, 32), 4, bin_size, first, count, 0, packed=(verts, faces), want_zero=True, cover_fill=0xFF, M=10)
        assert int((r["out"][0] != -1).sum()) == 0 and int((r["out"][1] != -1).sum()) == 0
        assert int((r["zero"] != 0).sum()) == 0
        assert int(r["cover"].abs().sum()) == 0 and r["count"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. the cover needs no memset
# ---------------------------------------------------------------------------------------------------------------------
def _grads(shape, gen, d):
    return [torch.randn(s, generator=gen).to(d) for s in (shape, tuple(shape) + (3,), shape)]


@pytest.mark.parametrize("size,kind", [((64, 64), "three"), ((256, 256), "three"), ((336, 336), "ten")],
                         ids=["48_tiles", "768_tiles_list_by_plan_image_order", "4410_tiles_list_by_plan_sorted_order"])
def test_cover_and_list_need_no_clearing(size, kind):
    """48 tiles: the split kernels list a word when its first bit is set.  More than 512 tiles with sides that are multiples of
    16: the list comes from the tile plan -- 768 tiles take the single-workgroup scan (tiles walked in image order, slots by
    arank), 4 410 tiles the sorted tile order."""
    from pytorch3d_amd import _C, _lib

    d = _dev()
    lib = _lib.load()
    verts, faces, first, count = _packed(*_batch(kind), d)
    F, N, (H, W), K = int(faces.shape[0]), int(count.shape[0]), size, 8
    fv, fp = _gather(verts, faces, d)
    clean = _call(d, size, K, 16, first, count, F, face_verts=fv, cover_fill=0)
    runs = [_call(d, size, K, 16, first, count, F, face_verts=fv, cover_fill=0xFF) for _ in range(2)]
    runs.append(_call(d, size, K, 16, first, count, F, packed=(verts, faces), cover_fill=0xFF))
    for i, r in enumerate(runs):
        _same_outputs(clean, r, f"dirty buffer, run {i}")
        assert torch.equal(clean["list"].sort().values, r["list"].sort().values), f"run {i}: lists differ"
    words, lst = clean["cover"], clean["list"]
    nonzero = torch.nonzero(words).reshape(-1).to(torch.int32)
    assert nonzero.numel() > 10
    listed = set(lst.tolist())
    assert len(listed) == lst.numel(), "a word is listed twice"
    assert set(nonzero.tolist()) <= listed, "a non-empty word is missing from the list"
    by_plan = N * (H // 16) * (W // 16) > 512
    if by_plan:
        # the plan's A: tiles (= 16 x 16 bins) whose list holds a face
        bins = _C._rasterize_meshes_coarse(fv, first, count, size, BLUR, 16, min(F, 1024))  # (a cut list still says 'not empty')
        A = int((bins >= 0).any(-1).sum())
        print(f"[{size}] {nonzero.numel()} non-empty words, {lst.numel()} listed, plan A = {A}")
        assert clean["count"] == A
    else:
        assert listed == set(nonzero.tolist())
    if not by_plan or kind != "three":
        return
    # the backward through that list against the backward without a cover, in the gate of tests/test_gpu_mesh_backward_queue.py
    gen = torch.Generator().manual_seed(5)
    p2f = clean["out"][0]
    gz, gb, gd = _grads(tuple(p2f.shape), gen, d)
    buf = torch.zeros((lib.p3d_rasterize_meshes_cover_list_bytes(N, H, W) // 4,), dtype=torch.int32, device=d)
    buf[:clean["words"]] = words
    buf[clean["words"]] = clean["count"]
    buf[clean["words"] + 16:clean["words"] + 16 + lst.numel()] = lst
    cover = buf[:clean["words"]].view(N, H // 16, W // 16)
    assert _C.cover_has_list(cover, N, H, W)
    V = int(verts.shape[0])
    with_list = _C._mesh_backward(fv, faces, V, p2f, gz, gb, gd, True, True, cover, fp)
    without = _C._mesh_backward(fv, faces, V, p2f, gz, gb, gd, True, True, None, fp)
    truth = U.face_grad_truth(fv.cpu(), p2f.cpu(), gz.cpu(), gb.cpu(), gd.cpu(), True, True, faces=faces.cpu(), num_verts=V)
    for tag, got in (("with the list", with_list), ("without a cover", without)):
        U.assert_face_grads_vs_truth(f"{size} {tag}", got.cpu(), None, None, None, None, None, True, True, truth=truth)
    _, scale, sing = truth
    gated = ~sing.reshape(V, 1).expand_as(scale)
    both = ((with_list.cpu().double() - without.cpu().double()).abs() / scale)[gated]
    print(f"[{size}] list vs no cover: max |difference| / scale = {float(both.max()):.2e}")
    assert float(both.max()) <= 5e-3


# ---------------------------------------------------------------------------------------------------------------------
# 4. grad_verts cleared by the forward
# ---------------------------------------------------------------------------------------------------------------------
def _mirror(d, need_grad=True):
    import pytorch3d_amd as p3d

    verts, faces = _batch()
    vp = torch.cat(verts, 0).float().to(d).requires_grad_(need_grad)
    m = p3d.PackedMeshes([v.to(d) for v in verts], [f.to(d) for f in faces]).update_verts_packed(vp)
    out = p3d.rasterize_meshes(m, image_size=64, blur_radius=BLUR, faces_per_pixel=8, perspective_correct=True,
                               clip_barycentric_coords=True)
    return vp, m, out


def test_precleared_grad_verts():
    from pytorch3d_amd import _C

    d = _dev()
    gen = torch.Generator().manual_seed(11)
    vp, m, out = _mirror(d)
    node = out[1].grad_fn
    assert node.zeroed_grad_verts is not None and tuple(node.zeroed_grad_verts.shape) == tuple(vp.shape)
    g = _grads(tuple(out[0].shape), gen, d)
    torch.autograd.backward(list(out[1:]), g, retain_graph=True)
    first = vp.grad.clone()
    assert node.zeroed_grad_verts is None, "the buffer serves one backward"
    vp.grad = None
    torch.autograd.backward(list(out[1:]), g)
    second = vp.grad.clone()
    # the call on a buffer of its own
    faces = m.faces_packed()
    fv = vp.detach()[faces].contiguous()
    V = int(vp.shape[0])
    plain = _C._mesh_backward(fv, faces, V, out[0], g[0], g[1], g[2], True, True, None)
    truth = U.face_grad_truth(fv.cpu(), out[0].cpu(), g[0].cpu(), g[1].cpu(), g[2].cpu(), True, True, faces=faces.cpu(), num_verts=V)
    _, scale, sing = truth
    gated = ~sing.reshape(V, 1).expand_as(scale)
    for tag, got in (("first backward (cleared by the forward)", first), ("second backward (retain_graph)", second), ("own buffer", plain)):
        U.assert_face_grads_vs_truth(tag, got.cpu(), None, None, None, None, None, True, True, truth=truth)
    for tag, got in (("first vs own buffer", first), ("second vs own buffer", second)):
        dev = ((got.cpu().double() - plain.cpu().double()).abs() / scale)[gated]
        print(f"[{tag}] max |difference| / scale = {float(dev.max()):.2e}")
        assert float(dev.max()) <= 5e-3
    # a forward that needs no gradient hands nothing on
    with torch.no_grad():
        _, _, out_ng = _mirror(d)
    assert out_ng[1].grad_fn is None
    _, _, out_frozen = _mirror(d, need_grad=False)
    assert out_frozen[1].grad_fn is None


def test_precleared_grad_verts_is_not_used_when_deterministic():
    from pytorch3d_amd import _C

    d = _dev()
    gen = torch.Generator().manual_seed(12)
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        grads = []
        for fused in (True, True, False):
            _C.FUSED_GATHER = fused
            vp, m, out = _mirror(d)
            assert out[1].grad_fn.zeroed_grad_verts is None
            if not grads:
                g = _grads(tuple(out[0].shape), gen, d)
            torch.autograd.backward(list(out[1:]), g)
            grads.append(vp.grad.clone())
    finally:
        _C.FUSED_GATHER = True
        torch.use_deterministic_algorithms(was)
    assert _bytes_equal(grads[0], grads[1]), "two deterministic runs differ"
    assert _bytes_equal(grads[0], grads[2]), "the fused and the unfused path differ under use_deterministic_algorithms"
    assert float(grads[0].abs().sum()) > 0
