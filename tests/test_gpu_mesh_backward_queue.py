"""mesh_backward, K = 4 / 8: the survivor queue in front of the wave table and the table's packed 44-byte slots
(pytorch3d_amd/csrc/raster_mesh_bwd.hip, wave_table.h).

What the cases aim at, per 16 x 16 area (one wave):
  * tiny soup     hundreds of distinct faces: the 108-slot table flushes and spills several times, the queue overflows
                  into the table in the middle of the area again and again;
  * mid soup      partial areas on both axes, a queue that fills to the brim;
  * one face      every queued entry is the same face (the longest summation chain in one table step), the only table
                  step is the one that empties the queue after the last row;
  * few large     areas of a single row and of a single column: a row segment shorter than a step;
  * hand-made     pix_to_face written by hand so that no two neighbouring lanes agree: 64 survivors in every step, each
                  step goes to the table as it is; and the same with every other row empty.
Every case runs K = 4 and 8, per-face and per-vertex output, with and without the per-face records, with a cover and
without, each gated by tests/_util.py: assert_face_grads_vs_truth at its default rtol against oracle/backward_f64.py."""
import pytest
import torch

import _util as U

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _forward(fv, size, K):
    from pytorch3d_amd import _C

    d = _dev()
    F = fv.shape[0]
    first, count = U.split_counts(F, 1)
    nbr = torch.full((F,), -1, dtype=torch.int64)
    (p2f, zbuf, bary, dists), cover = _C._rasterize_meshes_covered(fv.to(d), first.to(d), count.to(d), nbr.to(d), size, 2e-3, K, 8, 2000,
                                                                    True, True, False)
    assert _C.cover_has_list(cover, 1, *size)
    return p2f, cover


def _big_faces(n, gen):
    """n smooth faces that each cover the whole image."""
    base = torch.tensor([[-4.0, -4.0, 1.2], [4.0, -4.0, 1.3], [0.0, 4.0, 1.25]])
    fv = base[None].repeat(n, 1, 1)
    fv[:, :, :2] += (torch.rand(n, 3, 2, generator=gen) - 0.5) * 0.8
    fv[:, :, 2] += (torch.rand(n, 1, generator=gen) - 0.5) * 0.4 + (torch.rand(n, 3, generator=gen) - 0.5) * 0.1
    return fv.float()


def _hand_made(K, gen, blank_odd_rows):
    fv = _big_faces(16, gen)
    H = W = 32
    p2f = torch.empty((1, H, W, K), dtype=torch.int64)
    for y in range(H):
        for x in range(W):
            # neighbouring pixels of a row sit in neighbouring lanes of a step, slot by slot: no slot repeats its left neighbour's face
            while True:
                p2f[0, y, x] = torch.randperm(16, generator=gen)[:K]
                if x == 0 or not bool((p2f[0, y, x] == p2f[0, y, x - 1]).any()):
                    break
    if blank_odd_rows:
        p2f[:, 1::2] = -1
    # the row cover of this pix_to_face, written as the forward writes it: bit r of word (n, y / 16, x / 16) <=> row y = 16 * (y / 16) + r
    # of that area holds a face; it brings no list, so the backward makes one in its workspace
    has = (p2f[..., 0] >= 0).reshape(1, H // 16, 16, W // 16, 16).any(-1)  # (1, cy, r, cx)
    cover = (has.to(torch.int32) << torch.arange(16, dtype=torch.int32)[None, None, :, None]).sum(2).to(torch.int32)
    return fv, p2f, cover


CASES = {
    "tiny_soup": lambda K, gen: (U.smooth_soup(1500, gen, size=0.12), (32, 48)),
    "mid_soup": lambda K, gen: (U.smooth_soup(300, gen, size=0.6), (40, 56)),
    "one_face": lambda K, gen: (torch.tensor([[[-3.0, -3.0, 1.2], [3.0, -3.0, 1.3], [0.0, 3.0, 1.25]]]), (24, 40)),
    "few_large": lambda K, gen: (U.smooth_soup(12, gen, size=3.0), (33, 17)),
    "hand_made": None,
    "hand_made_blank_rows": None,
}


@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("case", list(CASES))
def test_backward_queue_and_packed_table(case, K):
    from pytorch3d_amd import _C, _lib

    d = _dev()
    lib = _lib.load()
    gen = torch.Generator().manual_seed(900 + K)
    if CASES[case] is None:
        fv, p2f, cover = _hand_made(K, gen, case.endswith("blank_rows"))
        p2f, cover = p2f.to(d), cover.to(d)
        size = (32, 32)
        assert not _C.cover_has_list(cover, 1, *size)
    else:
        fv, size = CASES[case](K, gen)
        p2f, cover = _forward(fv, size, K)
    F = fv.shape[0]
    H, W = size
    per_area = [int(p2f[0, y:y + 16, x:x + 16].unique().numel()) for y in range(0, H, 16) for x in range(0, W, 16)]
    print(f"[{case} K={K}] {int((p2f >= 0).sum())} samples, distinct faces per 16 x 16 area (with -1): {per_area}")
    assert int((p2f >= 0).sum()) > 0
    gz = torch.randn(p2f.shape, generator=gen)
    gb = torch.randn(tuple(p2f.shape) + (3,), generator=gen)
    gd = torch.randn(p2f.shape, generator=gen)
    truth = U.face_grad_truth(fv, p2f.cpu(), gz, gb, gd, True, True)
    fv_d, gz_d, gb_d, gd_d = fv.to(d).contiguous(), gz.to(d), gb.to(d), gd.to(d)
    # every face owns its vertices: grad_verts (3 F, 3) IS grad_face_verts (F, 3, 3), gated by the same float64 values
    faces = torch.arange(3 * F, dtype=torch.int64, device=d).reshape(F, 3)
    pre = torch.empty((F, 4), device=d)
    has_list = _C.cover_has_list(cover, 1, *size)
    ws = _C.backward_workspace(cover, 1, H, W, d)

    def backward(to_verts, with_pre, with_cover):
        out = torch.full((F, 3, 3), float("nan"), device=d)
        flags = (_lib.BWD_MAKE_FACE_PRE if with_pre else 0) | (_lib.BWD_COVER_HAS_LIST if (with_cover and has_list) else 0)
        rc = lib.p3d_rasterize_meshes_backward_ex(
            _C._ptr(fv_d), _C._ptr(faces) if to_verts else None, _C._ptr(pre) if with_pre else None, _C._ptr(p2f), _C._ptr(gz_d), _C._ptr(gb_d),
            _C._ptr(gd_d), _C.cover_ptr(cover, 1, H, W) if with_cover else None, F, 3 * F if to_verts else 0, 1, H, W, K, 1, 1, flags,
            _C._ptr(out), _C._ptr(ws) if with_cover else None, ws.numel() if with_cover else 0, _C._stream(d))
        _lib.check(rc, "rasterize_meshes_backward_ex")
        return out.cpu()

    _, scale, sing = truth
    gated = ~sing.reshape(F, 1, 1).expand_as(scale)
    for to_verts in (False, True):
        for with_pre in (False, True):
            got = {}
            for with_cover in (True, False):
                tag = f"{case} K={K} {'per vertex' if to_verts else 'per face'}, records {with_pre}, cover {with_cover}"
                got[with_cover] = backward(to_verts, with_pre, with_cover)
                U.assert_face_grads_vs_truth(tag, got[with_cover], fv, None, None, None, None, True, True, truth=truth)
            both = ((got[True].double() - got[False].double()).abs() / scale)[gated]
            print(f"[{case} K={K} verts {to_verts} records {with_pre}] cover vs no cover: max |difference| / scale = {float(both.max()):.2e}")
            assert float(both.max()) <= 5e-3
