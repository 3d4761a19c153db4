"""The instruction diet of mesh_backward (K = 4 / 8, perspective + clip) and mesh_fine.

1. Runs (raster_mesh_bwd.hip: run_reduce in front of the packed per-sample gradient, p3d_geom.h: face_sample_bwd<PRE, true>).
   pix_to_face is written by hand: lane = slot * (64 / K) + pixel, so a face repeated along a row at one slot is a run of
   neighbouring lanes inside a group of 64 / K pixels (8 at K = 8, 16 at K = 4).  Every group of every row and slot takes one
   of the patterns below: runs of 1, 2, 3, 5, 8 (and 12, 13, 16 at K = 4), runs that start at the group's first pixel, runs
   that end at its last, runs between empty pixels, two faces alternating pixel by pixel.  Containment: the same layout with
   the samples of one ordinary face handed to a zero-area face (three collinear vertices) -- it then sits in lanes next to
   ordinary faces at the same slot -- against the layout with those samples empty: the ordinary faces' gradients are finite
   and the same within the gate.  Per-face and per-vertex output, with and without the per-face records (without them the
   kernels keep the scalar arithmetic: the control).
2. Empty slots (raster_mesh.hip: write_pixel): pixels with 0, 1, K - 1, K and more than K faces, every output bit against
   the CPU oracle, the -1 entries included; the plain kernels (more than 512 tiles) and the split kernel of a one-image launch.
3. Range masks (raster_mesh.hip: stage_chunk): faces whose box edges ARE float32 pixel-centre values or their float
   neighbours on either side, faces far larger than the image, coordinates of 1e6, a NaN vertex; partial tiles on both
   axes; naive, split and plain binned kernels, every output bit against the CPU oracle.  (The NaN faces are what this case
   first caught: at K = 4 with blur the library -- before the range index as after it -- dropped them from pixels whose queue was
   full, 8 pix_to_face entries in two of the six cases.  Their clipped barycentrics are all 0 and their depth is 0; the staging
   depth cull took the smallest vertex depth for a bound.  stage_chunk now exempts a face whose area is NaN.)"""
import math

import pytest
import torch

import _util as U
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------------
# 1. runs
# ---------------------------------------------------------------------------------------------------------------------------
# a group's pixels as run lengths; negative: that many empty pixels; "alt": two faces alternating
PATTERNS = {
    8: [[8], [1, 2, 5], [5, 3], [3, -2, 3], [-1, 2, -2, 3], [2, 3, -3], "alt", [1, 1, 2, 1, 3]],
    4: [[16], [1, 2, 3, 5, 5], [8, 8], [3, 13], [-2, 12, -2], "alt", [5, -3, 8], [1, 15], [2, -1, 13]],
}


def _big_faces(n, gen):
    """n smooth faces that each cover the whole image."""
    base = torch.tensor([[-4.0, -4.0, 1.2], [4.0, -4.0, 1.3], [0.0, 4.0, 1.25]])
    fv = base[None].repeat(n, 1, 1)
    fv[:, :, :2] += (torch.rand(n, 3, 2, generator=gen) - 0.5) * 0.8
    fv[:, :, 2] += (torch.rand(n, 1, generator=gen) - 0.5) * 0.4 + (torch.rand(n, 3, generator=gen) - 0.5) * 0.1
    return fv.float()


def _run_layout(K, size):
    """pix_to_face (1, H, W, K) over faces 0 .. 3 K - 1 (slot k draws from 3 k .. 3 k + 2) and the run lengths that occur."""
    H, W = size
    pix = 64 // K
    pats = PATTERNS[K]
    p2f = torch.full((1, H, W, K), -1, dtype=torch.int64)
    seen = set()
    for y in range(H):
        for k in range(K):
            for g in range(W // pix):
                pat = pats[(y * K + k + 3 * g) % len(pats)]
                pool = [3 * k, 3 * k + 1, 3 * k + 2]
                x = g * pix
                if pat == "alt":
                    for i in range(pix):
                        p2f[0, y, x + i, k] = pool[(i + y) % 2]
                    seen.add("alt")
                    continue
                assert sum(abs(r) for r in pat) == pix
                for r, n in enumerate(pat):
                    if n > 0:
                        p2f[0, y, x:x + n, k] = pool[(r + y) % 3]
                        seen.add((n, x == g * pix, x + n == (g + 1) * pix))
                    x += abs(n)
    return p2f, seen


def _backward(fv, p2f, gz, gb, gd, K, to_verts, with_pre):
    from pytorch3d_amd import _C, _lib

    d = _dev()
    lib = _lib.load()
    F = fv.shape[0]
    _, H, W, _ = p2f.shape
    faces = torch.arange(3 * F, dtype=torch.int64, device=d).reshape(F, 3)  # every face owns its vertices
    pre = torch.empty((F, 4), device=d)
    out = torch.full((F, 3, 3), float("nan"), device=d)
    rc = lib.p3d_rasterize_meshes_backward_ex(
        _C._ptr(fv), _C._ptr(faces) if to_verts else None, _C._ptr(pre) if with_pre else None, _C._ptr(p2f), _C._ptr(gz), _C._ptr(gb),
        _C._ptr(gd), None, F, 3 * F if to_verts else 0, 1, H, W, K, 1, 1, _lib.BWD_MAKE_FACE_PRE if with_pre else 0, _C._ptr(out), None, 0,
        _C._stream(d))
    _lib.check(rc, "rasterize_meshes_backward_ex")
    return out.cpu()


@pytest.mark.parametrize("size", [(16, 16), (32, 32)])
@pytest.mark.parametrize("K", [4, 8])
def test_runs_and_containment_of_a_zero_area_face(K, size):
    d = _dev()
    gen = torch.Generator().manual_seed(4100 + K + size[0])
    fv = _big_faces(3 * K + 1, gen)
    D = 3 * K  # the zero-area face: three collinear vertices
    fv[D] = torch.tensor([[-1.0, -1.0, 1.2], [0.25, 0.25, 1.3], [1.0, 1.0, 1.25]])
    p2f, seen = _run_layout(K, size)
    lengths = {s[0] for s in seen if s != "alt"}
    want = {1, 2, 3, 5, 8} | ({12, 13, 16} if K == 4 else set())
    assert want <= lengths and "alt" in seen, (lengths, seen)
    assert any(s != "alt" and s[1] for s in seen) and any(s != "alt" and s[2] for s in seen)  # starts at the first pixel / ends at the last
    assert any(s != "alt" and not s[1] and not s[2] for s in seen)
    gz = torch.randn(p2f.shape, generator=gen)
    gb = torch.randn(tuple(p2f.shape) + (3,), generator=gen)
    gd = torch.randn(p2f.shape, generator=gen)
    victim = 3 * 2 + 1  # an ordinary face of slot 2: its samples go to the zero-area face, or are emptied
    with_deg = torch.where(p2f == victim, torch.full_like(p2f, D), p2f)
    without = torch.where(p2f == victim, torch.full_like(p2f, -1), p2f)
    assert int((with_deg == D).sum()) > 0
    truth_runs = U.face_grad_truth(fv, p2f, gz, gb, gd, True, True)
    truth_wo = U.face_grad_truth(fv, without, gz, gb, gd, True, True)
    fv_d, gz_d, gb_d, gd_d = fv.to(d).contiguous(), gz.to(d), gb.to(d), gd.to(d)
    for to_verts in (False, True):
        for with_pre in (True, False):
            tag = f"K={K} {size} {'per vertex' if to_verts else 'per face'}, records {with_pre}"
            got = _backward(fv_d, p2f.to(d), gz_d, gb_d, gd_d, K, to_verts, with_pre)
            U.assert_face_grads_vs_truth("runs " + tag, got, fv, None, None, None, None, True, True, truth=truth_runs)
            a = _backward(fv_d, with_deg.to(d), gz_d, gb_d, gd_d, K, to_verts, with_pre)
            b = _backward(fv_d, without.to(d), gz_d, gb_d, gd_d, K, to_verts, with_pre)
            assert bool(torch.isfinite(a[:D]).all()), f"{tag}: a zero-area face's partials reached an ordinary face"
            assert float(b[D].abs().max()) == 0.0 and float(b[victim].abs().max()) == 0.0
            U.assert_face_grads_vs_truth("without the zero-area face " + tag, b, fv, None, None, None, None, True, True, truth=truth_wo)
            a_ord = a.clone()
            a_ord[D] = 0.0
            U.assert_face_grads_vs_truth("beside the zero-area face " + tag, a_ord, fv, None, None, None, None, True, True, truth=truth_wo)
            _, scale, sing = truth_wo
            gated = ~sing.reshape(-1, 1, 1).expand_as(scale)
            dev = ((a_ord.double() - b.double()).abs() / scale)[gated]
            print(f"[{tag}] with / without the zero-area face: max |difference| / scale = {float(dev.max()):.2e}")
            assert float(dev.max()) <= 5e-3


# ---------------------------------------------------------------------------------------------------------------------------
# 2. empty slots
# ---------------------------------------------------------------------------------------------------------------------------
def _bits_equal(tag, ours, ref):
    assert ours[0].dtype == torch.int64
    assert torch.equal(ours[0], ref[0]), f"{tag}: pix_to_face differs in {int((ours[0] != ref[0]).sum())} entries"
    for name, a, b in zip(("zbuf", "bary", "dists"), ours[1:], ref[1:]):
        same = torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
        assert same, f"{tag}: {name} differs in {int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum())} entries"


def _run_ours(fv, first, count, size, blur, K, bin_size, M):
    from pytorch3d_amd import _C

    d = _dev()
    nbr = torch.full((fv.shape[0],), -1, dtype=torch.int64)
    out = _C.rasterize_meshes(fv.to(d), first.to(d), count.to(d), nbr.to(d), size, blur, K, bin_size, M, True, True, False)
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def _batch_of_copies(fv, ref, N):
    """The mesh N times, one copy per image, and the oracle's one-image result repeated with the face numbers shifted."""
    F = fv.shape[0]
    first = torch.arange(N, dtype=torch.int64) * F
    count = torch.full((N,), F, dtype=torch.int64)
    shift = (torch.arange(N, dtype=torch.int64) * F).reshape(N, 1, 1, 1)
    p2f = ref[0].expand(N, -1, -1, -1)
    want = [torch.where(p2f >= 0, p2f + shift, p2f)] + [r.expand(N, *r.shape[1:]).contiguous() for r in ref[1:]]
    return fv.repeat(N, 1, 1), first, count, want


def _copies_for_plain_kernels(size):
    """Images enough for more than 512 tiles of 16 x 16 pixels: above that the plain kernels run, not the split ones."""
    tiles = math.ceil(size[0] / 16) * math.ceil(size[1] / 16)
    return 512 // tiles + 2


def _staircase(K, gen):
    """K + 3 wedges that open to the right, each starting a little further right and a little deeper: from left to right a
    pixel holds 0, 1, 2, ... K + 3 faces."""
    n = K + 3
    fv = torch.empty((n, 3, 3))
    for j in range(n):
        x = -0.8 + 1.6 * j / (n - 1) + 0.01 * float(torch.rand((), generator=gen))
        z = 1.0 + 0.1 * j
        fv[j] = torch.tensor([[x, -5.0, z], [x + 20.0, 0.3, z + 0.05], [x, 5.0, z + 0.02]])
    return fv


@pytest.mark.parametrize("size", [(24, 40), (17, 33)])
@pytest.mark.parametrize("K", [4, 8])
def test_empty_slots_bit_equal_to_the_oracle(K, size):
    gen = torch.Generator().manual_seed(4200 + K + size[1])
    fv = _staircase(K, gen)
    F = fv.shape[0]
    first, count = U.split_counts(F, 1)
    nbr = torch.full((F,), -1, dtype=torch.int64)
    blur = 2e-3
    ref = orc.rasterize_meshes_naive(fv, first, count, nbr, size, blur, K, True, True, False)
    many = orc.rasterize_meshes_naive(fv, first, count, nbr, size, blur, K + 3, True, True, False)
    held = (many[0] >= 0).sum(-1)
    for cls in (0, 1, K - 1, K):
        assert bool((held == cls).any()), f"no pixel with {cls} faces"
    assert bool((held > K).any()), "no pixel with more than K faces"
    assert bool((ref[0] == -1).any()) and bool((ref[1] == -1.0).any())
    # one image: the split kernel; the naive kernel
    _bits_equal(f"K={K} {size} one image, binned", _run_ours(fv, first, count, size, blur, K, 16, 64), ref)
    _bits_equal(f"K={K} {size} one image, naive", _run_ours(fv, first, count, size, blur, K, 0, 0), ref)
    # more than 512 tiles: the plain kernel
    N = _copies_for_plain_kernels(size)
    fvn, firstn, countn, want = _batch_of_copies(fv, ref, N)
    _bits_equal(f"K={K} {size} {N} images, binned", _run_ours(fvn, firstn, countn, size, blur, K, 16, 64), want)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. range masks
# ---------------------------------------------------------------------------------------------------------------------------
def _centres(S1, S2):
    """float32 pixel centres of an axis of S1 pixels, operation by operation as pix_to_ndc forms them (p3d_geom.h)."""
    rng = torch.tensor(2.0 * S1 / S2 if S1 > S2 else 2.0, dtype=torch.float32)
    off = rng / 2.0
    i = torch.arange(S1, dtype=torch.float32)
    return -off + (rng * i + off) / float(S1)


def _edge_faces(size, blur, gen):
    H, W = size
    cx, cy = _centres(W, H), _centres(H, W)
    sb = torch.tensor(blur, dtype=torch.float32).sqrt()
    inf = torch.tensor(float("inf"))
    faces = []
    for _ in range(48):
        i0, i1 = sorted(int(v) for v in torch.randint(0, W, (2,), generator=gen))
        j0, j1 = sorted(int(v) for v in torch.randint(0, H, (2,), generator=gen))
        # the box's low edges are x0 - sqrt(blur), its high edges x1 + sqrt(blur) in float32: chosen so that they land on the centres
        x0, x1, y0, y1 = cx[i0] + sb, cx[min(i1 + 1, W - 1)] - sb, cy[j0] + sb, cy[min(j1 + 1, H - 1)] - sb
        which = int(torch.randint(0, 3, (1,), generator=gen))
        if which == 1:  # the float neighbours: the strict comparisons fall on the other side
            x0, x1, y0, y1 = (torch.nextafter(v, s) for v, s in ((x0, inf), (x1, -inf), (y0, inf), (y1, -inf)))
        elif which == 2:
            x0, x1, y0, y1 = (torch.nextafter(v, s) for v, s in ((x0, -inf), (x1, inf), (y0, -inf), (y1, inf)))
        z = 0.6 + 1.5 * float(torch.rand((), generator=gen))
        if int(torch.randint(0, 2, (1,), generator=gen)):
            faces.append([[x0, y0, z], [x1, y0, z + 0.1], [x0, y1, z + 0.05]])
        else:
            faces.append([[x1, y1, z], [x0, y1, z + 0.1], [x1, y0, z + 0.05]])
    faces.append([[-50.0, -50.0, 1.9], [60.0, -40.0, 2.0], [0.0, 70.0, 2.1]])       # far larger than the image
    faces.append([[-1e6, -1e6, 2.4], [1e6, -1e6, 2.5], [0.0, 1e6, 2.6]])
    faces.append([[-1e6, 0.1, 2.4], [-0.2, 0.3, 2.5], [-0.3, -1e6, 2.6]])             # one box edge inside, three far outside
    faces.append([[float("nan"), -0.5, 1.0], [0.5, -0.5, 1.1], [0.0, 0.5, 1.2]])      # a NaN vertex
    faces.append([[-0.5, -0.5, 1.0], [0.5, float("nan"), 1.1], [0.0, 0.5, 1.2]])
    return torch.tensor([[[float(c) for c in v] for v in f] for f in faces], dtype=torch.float32)


@pytest.mark.parametrize("size", [(16, 16), (17, 33), (40, 24)])
@pytest.mark.parametrize("blur", [0.0, 1e-3])
@pytest.mark.parametrize("K", [4, 8])
def test_range_masks_on_pixel_centres_bit_equal_to_the_oracle(K, blur, size):
    gen = torch.Generator().manual_seed(4300 + K + size[0] + int(blur * 1e4))
    fv = _edge_faces(size, blur, gen)
    F = fv.shape[0]
    first, count = U.split_counts(F, 1)
    nbr = torch.full((F,), -1, dtype=torch.int64)
    ref = orc.rasterize_meshes_naive(fv, first, count, nbr, size, blur, K, True, True, False)
    assert int((ref[0] >= 0).sum()) > 0
    _bits_equal(f"K={K} blur={blur} {size} naive", _run_ours(fv, first, count, size, blur, K, 0, 0), ref)
    _bits_equal(f"K={K} blur={blur} {size} one image, binned", _run_ours(fv, first, count, size, blur, K, 16, 128), ref)
    N = _copies_for_plain_kernels(size)
    fvn, firstn, countn, want = _batch_of_copies(fv, ref, N)
    _bits_equal(f"K={K} blur={blur} {size} {N} images, binned", _run_ours(fvn, firstn, countn, size, blur, K, 16, 128), want)
