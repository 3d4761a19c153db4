"""The fine mesh rasterizer's walk over a tile plan (csrc/binning.h: TilePlan; csrc/raster_mesh.hip: "Which tile", "Piggyback
fill"): the tile's row requested with the plan header at the head of a workgroup, the background fill keyed by the walk position
and handed out in quarter-tiles to whichever wave is done first, the trailing barrier that is skipped after a tile's last chunk.

Every case compares all four outputs, bit for bit, with the C oracle's naive rasterizer under SoftRas blur, perspective-correct
and clipped barycentrics (as tests/test_gpu_meshes.py does).  The shapes are the smallest that reach each path:

  * more than kSplitMaxTiles = 512 tiles of 16 x 16 pixels, or the split kernels run and no plan is walked;
  * N <= 64 images with <= 4096 tiles are binned by the single-workgroup scan, which writes no tile order: the workgroups take
    the tiles in image order and the fill is keyed by the tile's rank among the active ones (cases 1-8 and 10);
  * N = 65 images of 48 x 48 (585 tiles) are binned by the general scan, which writes the tile order: the walk the bench launch
    takes (cases 11-15).

Expected values come from the oracle alone; a scene's oracle outputs are computed once and shared.
"""
import functools

import pytest
import torch

import _util as U
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

BLUR = 9.2102e-4  # SoftRas: log(1 / 1e-4 - 1) * 1e-4
M = 5000


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _sphere(level):
    v, f = U.ico_sphere(level)
    return v[f].contiguous()  # (F, 3, 3)


def _place(level, scale, cx, cy, z=2.0):
    fv = _sphere(level) * scale
    fv = fv.clone()
    fv[..., 0] += cx
    fv[..., 1] += cy
    fv[..., 2] += z
    return fv


def _pack(per_image):
    """per_image: a list (one entry per image) of lists of (level, scale, cx, cy) spheres -> fv, first, count, nbr."""
    fvs, first, count, at = [], [], [], 0
    for spheres in per_image:
        parts = [_place(*s) for s in spheres]
        n = sum(int(p.shape[0]) for p in parts)
        fvs += parts
        first.append(at)
        count.append(n)
        at += n
    fv = torch.cat(fvs, 0).contiguous() if fvs else torch.zeros((0, 3, 3))
    return fv, torch.tensor(first, dtype=torch.int64), torch.tensor(count, dtype=torch.int64), torch.full((at,), -1, dtype=torch.int64)


# ico_sphere(2): 320 faces.  Scale 0.05 on a 224-pixel image is a disc of ~11 pixels: all 320 faces in one or two tiles (lists of
# more than one chunk of 256); scale 0.3 spreads them over ~20 tiles (lists of 20..100 faces); the rest of the image is background.
SCENES = {
    "three": [[(2, 0.30, -0.35, 0.30), (2, 0.05, 0.62, -0.55)], [(2, 0.55, 0.10, -0.05)], [(2, 0.12, -0.70, -0.66)]],
    "small4": [[(2, 0.10, -0.5 + 0.3 * i, 0.4 - 0.25 * i)] for i in range(4)],
    "offscreen": [[(2, 0.3, 3.0, 0.2)], [(2, 0.2, -0.3, -4.0)], [(2, 0.4, 5.0, 5.0)]],
    "full": [[(2, 2.5, 0.0, 0.0, 4.0)], [(2, 3.0, 0.2, -0.1, 5.0)], [(2, 2.8, -0.1, 0.1, 4.5)], [(2, 2.6, 0.0, 0.0, 4.0)], [(2, 2.7, 0.1, 0.1, 4.0)]],
    "one": [[(2, 0.5, 0.1, -0.2)]],
    # 65 images of 48 x 48: two of three hold a sphere of 80 faces somewhere, every eleventh a tiny one of 320 (two chunks in one tile)
    "many": [([] if i % 3 == 2 else [(1, 0.25 + 0.05 * (i % 4), -0.5 + 0.17 * (i % 7), 0.5 - 0.2 * (i % 6))]) +
             ([(2, 0.08, 0.6, -0.6)] if i % 11 == 0 else []) for i in range(65)],
}


@functools.lru_cache(maxsize=None)
def _scene(name):
    return _pack(SCENES[name])


@functools.lru_cache(maxsize=None)
def _oracle(name, size, K):
    fv, first, count, nbr = _scene(name)
    return tuple(orc.rasterize_meshes_naive(fv, first, count, nbr, size, BLUR, K, True, True, False))


def _ours(name, size, K, bin_size=16, max_faces=M, covered=False):
    from pytorch3d_amd import _C

    d = _dev()
    fv, first, count, nbr = (t.to(d) for t in _scene(name))
    if covered:
        out, cover = _C._rasterize_meshes_covered(fv, first, count, nbr, size, BLUR, K, bin_size, max_faces, True, True, False)
    else:
        out, cover = _C.rasterize_meshes(fv, first, count, nbr, size, BLUR, K, bin_size, max_faces, True, True, False), None
    torch.cuda.synchronize()
    return out, cover


def _assert_equal(ours, ref, tag):
    assert torch.equal(ours[0].cpu(), ref[0]), f"pix_to_face differs ({tag}): {(ours[0].cpu() != ref[0]).sum().item()} elements"
    for nm, a, b in zip(("zbuf", "bary", "dists"), ours[1:], ref[1:]):
        assert torch.equal(a.cpu(), b), f"{nm} not bit-exact ({tag}): max diff {(a.cpu() - b).abs().max().item()}"


def _tiles(name, size):
    return len(SCENES[name]) * ((size[0] + 15) // 16) * ((size[1] + 15) // 16)


def _list_lengths(name, size):
    """Faces in every tile's bin list, as the coarse stage sees them (16-pixel bins): from the library's own coarse operator."""
    from pytorch3d_amd import _C

    d = _dev()
    fv, first, count, _ = (t.to(d) for t in _scene(name))
    bins = _C._rasterize_meshes_coarse(fv, first, count, size, BLUR, 16, M)
    return (bins >= 0).sum(-1).flip(1).flip(2)  # (N, BH, BW) -> cover orientation (outputs are stored flipped)


def _active_tiles(name, size):
    return _list_lengths(name, size) > 0


def _check_list_and_backward(name, size, K):
    """The list behind the cover: every non-zero cover word, no duplicates, one entry per active tile; the backward through the list
    equals the backward without a cover."""
    from pytorch3d_amd import _C

    d = _dev()
    out, cover = _ours(name, size, K, covered=True)
    _assert_equal(out, _oracle(name, size, K), f"{name} {size} K={K} covered")
    N, (H, W) = len(SCENES[name]), size
    assert _C.cover_has_list(cover, N, H, W)
    words = cover.numel()
    buf = torch.empty(0, dtype=torch.int32, device=d).set_(cover.untyped_storage(), 0, (2 * words + 16,))
    n_listed = int(buf[words])
    listed = buf[words + 16: words + 16 + n_listed].cpu().tolist()
    nonzero = torch.nonzero(cover.reshape(-1) != 0).flatten().cpu().tolist()
    assert len(set(listed)) == len(listed), "a word is listed twice"
    assert set(nonzero) <= set(listed), "a non-empty cover word is not listed"
    active = _active_tiles(name, size)
    assert n_listed == int(active.sum()), (n_listed, int(active.sum()))
    assert sorted(listed) == torch.nonzero(active.reshape(-1)).flatten().cpu().tolist()
    fv = _scene(name)[0].to(d)
    gen = torch.Generator().manual_seed(5)
    gz, gd = (torch.randn(out[1].shape, generator=gen).to(d) for _ in range(2))
    gb = torch.randn(out[2].shape, generator=gen).to(d)
    truth = _C.rasterize_meshes_backward(fv, out[0].clone(), gz, gb, gd, True, True)  # no cover: every row is read
    with_list = _C.rasterize_meshes_backward(fv, out[0], gz, gb, gd, True, True, _cover=cover)
    scale = truth.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-6)
    # the same samples in another order of float atomics: the bound of tests/test_gpu_cover.py
    assert float(((with_list - truth).abs() / scale).max()) < 5e-3


def test_case01_plan_walk_with_list_588_tiles():
    size = (224, 224)
    assert _tiles("three", size) == 588
    ref = _oracle("three", size, 8)
    per_tile = _list_lengths("three", size)
    assert int((per_tile == 0).sum()) > 0 and int(per_tile.max()) > 256 and int(((per_tile > 64) & (per_tile <= 256)).sum()) > 0, \
        "background tiles, lists of more than 64 faces and lists of more than one chunk"
    _check_list_and_backward("three", size, 8)
    _assert_equal(_ours("three", size, 8)[0], ref, "three K=8")


def test_case02_mostly_background():
    size = (192, 192)
    assert _tiles("small4", size) == 576
    active = _active_tiles("small4", size)
    a = int(active.sum())
    assert a > 0 and (576 - a + a - 1) // a >= 2, "q_bg >= 2"
    out, _ = _ours("small4", size, 8)
    _assert_equal(out, _oracle("small4", size, 8), "small4")
    # every element of a tile without a face is -1 in all four outputs (the oracle says so too; asserted on its own)
    bg = (~active).repeat_interleave(16, 1).repeat_interleave(16, 2)
    assert bool((out[0][bg] == -1).all()) and all(bool((o[bg] == -1.0).all()) for o in out[1:])


def test_case03_all_offscreen_returns_all_minus_one():
    size = (224, 224)
    assert _tiles("offscreen", size) == 588 and int(_active_tiles("offscreen", size).sum()) == 0
    out, _ = _ours("offscreen", size, 8)
    assert bool((out[0] == -1).all()) and all(bool((o == -1.0).all()) for o in out[1:])
    _assert_equal(out, _oracle("offscreen", size, 8), "offscreen")


def test_case04_no_background_tiles():
    size = (176, 176)  # 5 x 121 = 605 tiles
    assert _tiles("full", size) > 512 and bool(_active_tiles("full", size).all())
    _assert_equal(_ours("full", size, 8)[0], _oracle("full", size, 8), "full")


def test_case05_partial_tiles():
    size = (200, 232)
    assert _tiles("three", size) == 585
    _assert_equal(_ours("three", size, 8)[0], _oracle("three", size, 8), "three 200x232")
    _assert_equal(_ours("three", size, 8, covered=True)[0], _oracle("three", size, 8), "three 200x232 covered")


@pytest.mark.parametrize("K", [4, 2, 3], ids=["case06_K4_piggyback", "case07_K2_own_fill", "case08_K3_generic_epilogue"])
def test_other_queue_lengths(K):
    size = (224, 224)
    _assert_equal(_ours("three", size, K)[0], _oracle("three", size, K), f"three K={K}")


def test_case09_bins_of_several_tiles_walk_no_plan():
    size = (528, 528)  # 33 tiles a side: bins of 32 pixels, four tiles each
    _assert_equal(_ours("one", size, 8, bin_size=32)[0], _oracle("one", size, 8), "one 528x528")


def test_case10_short_workspace(monkeypatch):
    from pytorch3d_amd import _C

    monkeypatch.setattr(_C, "SHORT_WORKSPACE", "always")
    size = (224, 224)
    before = _C.WORKSPACE_STATS["short_calls"]
    out, _ = _ours("three", size, 8, max_faces=200000)
    assert _C.WORKSPACE_STATS["short_calls"] == before + 1 and _C.WORKSPACE_STATS["last_entries"] is not None
    _assert_equal(out, _oracle("three", size, 8), "three short workspace")


# ---- the walk in the plan's tile order: 65 images, the general scan

MANY = (48, 48)


def test_case11_tile_order_walk_with_list():
    assert _tiles("many", MANY) == 585
    active = _active_tiles("many", MANY)
    assert 0 < int(active.sum()) < 585
    _check_list_and_backward("many", MANY, 8)
    _assert_equal(_ours("many", MANY, 8)[0], _oracle("many", MANY, 8), "many K=8")


@pytest.mark.parametrize("K", [4, 2, 3])
def test_case12_tile_order_walk_other_queue_lengths(K):
    _assert_equal(_ours("many", MANY, K)[0], _oracle("many", MANY, K), f"many K={K}")


def test_case13_tile_order_walk_partial_tiles():
    size = (40, 56)  # 3 x 4 tiles, the last row and column partial: 780 tiles
    _assert_equal(_ours("many", size, 8)[0], _oracle("many", size, 8), "many 40x56")


def test_case14_tile_order_walk_short_workspace(monkeypatch):
    from pytorch3d_amd import _C

    monkeypatch.setattr(_C, "SHORT_WORKSPACE", "always")
    before = _C.WORKSPACE_STATS["short_calls"]
    out, _ = _ours("many", MANY, 8, max_faces=200000)
    assert _C.WORKSPACE_STATS["short_calls"] == before + 1
    _assert_equal(out, _oracle("many", MANY, 8), "many short workspace")


def test_case15_tile_order_walk_all_offscreen_and_all_covered():
    from pytorch3d_amd import _C

    d = _dev()
    for spheres, tag in (([(1, 0.3, 4.0, 4.0)], "offscreen"), ([(1, 3.0, 0.0, 0.0, 5.0)], "covered")):
        fv, first, count, nbr = _pack([spheres] * 65)
        ref = orc.rasterize_meshes_naive(fv, first, count, nbr, MANY, BLUR, 8, True, True, False)
        out = _C.rasterize_meshes(fv.to(d), first.to(d), count.to(d), nbr.to(d), MANY, BLUR, 8, 16, M, True, True, False)
        torch.cuda.synchronize()
        _assert_equal(out, ref, f"many {tag}")
        if tag == "offscreen":
            assert bool((out[0] == -1).all())
