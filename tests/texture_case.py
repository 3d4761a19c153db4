"""Inputs, references and the gate of the texture kernels (csrc/texture.hip, csrc/texture_multi.hip with uvm_sample.h, csrc/atlas.hip
with atlas_cell.h); the yardstick of tests/test_gpu_texture_edges.py.  tests/test_cpu_texture_case.py ties it to the reference's recorded
results and shows, without a GPU, that the gate is feasible for the oracle's restatement and rejects six structural mutants.

References, every one in torch on the CPU:

    chain(x, mode, dtype)        TexturesUV.sample_textures as the reference states it (renderer/mesh/textures.py:1190-1273): the
                                 barycentric interpolation of faces_verts_uvs (background to uv = (0, 0)), torch.lerp onto the grid,
                                 F.grid_sample over the permuted and expanded maps; gradients by torch autograd
    chain_multi(x, mode, dtype)  its maps_ids branch (textures.py:1274-1315): face 0's id for background samples, z = 2 id / (M - 1) - 1,
                                 the 5-D grid_sample.  chain() dispatches to it when x holds maps_ids
    kernel_order(x, mode)        oracle.sample_uv* / sample_uv_multi*: the float32 restatement in the kernels' order
    restated(x, mode, mutant)    the sampler spelt out in torch ops (source index, clamp, floor / nearbyint, corner gather), float32;
                                 exists to carry the MUTANTS, and passes the gate itself
    atlas_chain(...)             TexturesAtlas.sample_textures (textures.py:594-620) by torch indexing; the backward is the float64
                                 index_put_(accumulate=True) sum
float64 is the yardstick, float32 the reference chain's own arithmetic.  A sample with pix_to_face >= F (or, with maps_ids, a face
without an id) reads zero and has no gradient in every one of them -- the reference itself would fail to index.

Gate.  For every quantity and class:

    max |got - chain64|  <=  max(MARGIN * max |chain32 - chain64|, ulp32(max |chain64|))

and `got` is finite wherever chain64 is; a class whose float64 figures are not finite fails.  texels and grad_bary: per sample class,
over the elements of the class.  grad_face_uvs and grad_maps: per image, over the rows (faces, texels) that some sample of that image
touches; an entry that no sample of any image touches must be exactly 0.0.

Sample classes: whole pixel rows (blend_case.class_rows), the same rows in every image.

    general     a face of the `inside` block, random barycentrics: uv inside [0, 1]
    outside     a face whose u or v lies outside [0, 1] by up to 0.3; every eighth sample a face at +-5 or +-1e6: partial and empty
                footprints under zeros padding, a clamped index with multiplier 0 under border padding
    lattice     one-hot barycentrics on faces whose vertex uvs are drawn from {0, 1/16, ..., 1}: with map sides 2^a or 5 * 2^a every
                index is a short dyadic number, exact in both precisions, and lands on nearbyintf ties, on integers (weights 0 and 1),
                on the clamp equalities and on u = 0.5 (the |w| < 0.5 switch of torch.lerp)
    run         runs of 1 to 200 consecutive pixels of one slot on one face, as a rasterizer leaves them
    background  pix_to_face = -1, barycentrics -1

Conditions, asserted by inputs(): a sample is redrawn (new barycentrics), never left out, until -- outside `lattice` -- its float64 ix
and iy lie farther than TOL from every integer, in nearest mode from every half-integer, under border padding from 0 and size - 1.
Otherwise float32 and float64 could take different texels, chain32's error would be a texel difference and the gate would prove
nothing.  An axis is exempt where no rounding can change the texels: size 1 with align_corners or border padding (the index is 0), a
clamped index beyond TOL, a footprint wholly outside the map beyond TOL under zeros padding.  The map coordinate of the multi-map
branch is exact for M - 1 a power of two, which inputs() asserts.
"""
import itertools

import torch
import torch.nn.functional as TF

import _util  # noqa: F401 -- puts the repository root on sys.path (kernel_order imports the oracle)
from blend_case import class_rows
from box3d_case import MARGIN
from mesh_refine_case import ulp32

CLASSES = ("general", "outside", "lattice", "run", "background")
QUANTITIES = ("texels", "grad_bary", "grad_face_uvs", "grad_maps")
MODES = tuple(itertools.product((True, False), ("zeros", "border"), ("bilinear", "nearest")))  # (align_corners, padding, sampling)
MUTANTS = ("map_of_image_0", "background_map_grad_dropped", "lost_step", "border_keeps_multiplier", "half_away_from_zero", "iz_rounded")
TOL = 1e-4
PILE_SCALE = 16.0  # see inputs()
LOST_STEP = (1, 5)  # (image, 64-sample step) whose scatter contributions the mutant `lost_step` loses: a `general` row

# csrc/texture.hip, mirrored (tests/test_cpu_texture_case.py reads them from the source text)
UV_SLOTS, TEXEL_SLOTS, RESERVE, LANES = 128, 320, 64, 64
SPAN_SAMPLES, MAX_WAVES = 4096, 4 * 16384

# the cases of tests/test_gpu_texture_edges.py
SHAPE = (3, 24, 64, 2)  # N, H, W, K: 3072 samples per image, one workgroup, four waves of 12 steps
FACES = 300
MAP = (32, 40)
CHANNELS = (1, 2, 3, 4, 5, 8)
SMALL_MAPS = ((1, 1), (1, 8), (8, 1), (2, 2))
SMALL_SHAPE = (3, 16, 16, 1)
LATTICE_MAPS = ((8, 16), (16, 8))
MULTI = ((2, 1), (3, 3), (5, 5))  # (M, C)
SEED = 4100
# Seeds per kind of case (see case()).  texels and grad_bary are written per sample and repeat bit for bit, so whether a cell passes is
# settled by its inputs; a class is one row of pixels, and the largest of its few hundred errors against MARGIN x the largest of
# chain(float32)'s keeps a tail when most of the error sits in a few samples: grad_texels are therefore drawn from one binade
# (inputs()).  While sample_uv_bwd_kernel summed d texel / d index as four products per channel, grad_bary came to 1.15 of its bound
# on the 2 x 2 map (seed 4100, class `outside`) and to 1.04 and 1.14 on the 8 x 1 map (seed 5100, class `run`), all three at noalign,
# border, bilinear; since it takes the differences of neighbouring corners first, as ATen's vectorised CPU kernel does, the largest
# err / bound of these cases on the GPU is 0.66.  `small` keeps the seed at which that was measured.
SEEDS = {"main": SEED, "small": SEED + 1000, "lattice": SEED, "one_face": SEED, "multi": SEED}


def mode_kw(mode):
    return dict(align_corners=mode[0], padding_mode=mode[1], sampling_mode=mode[2])


def mode_id(mode):
    return f"{'align' if mode[0] else 'noalign'}-{mode[1]}-{mode[2]}"


def _ceil_div(a, b):
    return -(-a // b)


def span_of(HWK):
    """Samples per wave of sample_uv_bwd_kernel, as p3d_sample_uv_backward computes them."""
    waves = min(_ceil_div(HWK, SPAN_SAMPLES), MAX_WAVES)
    bx = _ceil_div(waves, 4)
    return _ceil_div(_ceil_div(HWK, bx * 4), LANES) * LANES


# ---- sample positions in float64 -------------------------------------------------------------------------------------------------
def _index64(coord01, size, align, flip):
    """Unclamped source index of a uv coordinate (float64): the lerp onto [-1, 1] (v flipped), then grid_sampler_unnormalize."""
    g = 1.0 - 2.0 * coord01 if flip else 2.0 * coord01 - 1.0
    return (g + 1.0) / 2.0 * (size - 1) if align else ((g + 1.0) * size - 1.0) / 2.0


def _axis_settled(x, size, align, border, nearest):
    """Per sample: can no rounding of `x` (an unclamped float64 index) change which texels it reads?"""
    if size == 1 and (align or border):
        return torch.ones_like(x, dtype=torch.bool)
    frac = x - torch.floor(x)
    ok = torch.minimum(frac, 1.0 - frac) > TOL
    if nearest:
        ok &= (frac - 0.5).abs() > TOL
    if border:
        clamped = (x < -TOL) | (x > size - 1 + TOL)
        at_edge = (x.abs() <= TOL) | ((x - (size - 1)).abs() <= TOL)
        return (ok | clamped) & ~at_edge
    return ok | (x < -1.0 - TOL) | (x > size + TOL)


def _uv64(x):
    """(P, 2) float64 uv of every sample, P = N H W K; background and faceless samples at (0, 0)."""
    f = x["pix_to_face"].reshape(-1)
    F = x["face_uvs"].shape[0]
    face = (f >= 0) & (f < F)
    fu = x["face_uvs"].double()[f.clamp(0, max(F - 1, 0))] if F else torch.zeros(f.numel(), 3, 2, dtype=torch.float64)
    uv = (x["bary"].double().reshape(-1, 3, 1) * fu).sum(1)
    return torch.where(face[:, None], uv, torch.zeros((), dtype=torch.float64))


def _valid(x):
    """(P,) samples that read anything: not pix_to_face >= F; with maps_ids, the face (face 0 for the background) has an id."""
    f = x["pix_to_face"].reshape(-1)
    ok = f < x["face_uvs"].shape[0]
    if "maps_ids" in x:
        ok &= f.clamp(min=0) < x["maps_ids"].numel()
    return ok


def _map_id(x):
    """(P,) int64 map of every sample (0 where it has none)"""
    f = x["pix_to_face"].reshape(-1).clamp(min=0)
    ids = x["maps_ids"].reshape(-1)
    if ids.numel() == 0:
        return torch.zeros_like(f)
    return torch.where(f < ids.numel(), ids[f.clamp(max=ids.numel() - 1)], torch.zeros_like(f))


def footprint(x, mode):
    """-> (keys (P, corners) int64, image (P,)): the texels inside the map that each sample reads, from its float64 position, as
    ((z) * Hm + y) * Wm + x within its image's maps; -1: corner outside, or a sample that reads nothing."""
    align, pad, samp = mode
    border, nearest = pad == "border", samp == "nearest"
    maps = x["maps"]
    multi = "maps_ids" in x
    Hm, Wm = maps.shape[-3], maps.shape[-2]
    uv = _uv64(x)
    axes = [(_index64(uv[:, 0], Wm, align, False), Wm), (_index64(uv[:, 1], Hm, align, True), Hm)]
    if multi:
        M = maps.shape[1]
        axes.append((_index64(_map_id(x).double() / (M - 1), M, align, False), M))
    else:
        axes.append((torch.zeros(uv.shape[0], dtype=torch.float64), 1))
    cands = []
    for pos, size in axes:
        if border:
            pos = pos.clamp(0, size - 1)
        base = [torch.round(pos).long()] if nearest else [torch.floor(pos).long(), torch.floor(pos).long() + 1]
        cands.append([(i, (i >= 0) & (i < size)) for i in base])
    valid = _valid(x)
    keys = []
    for (xi, xo), (yi, yo), (zi, zo) in itertools.product(*cands):
        keys.append(torch.where(xo & yo & zo & valid, (zi * Hm + yi) * Wm + xi, torch.full_like(xi, -1)))
    N = x["pix_to_face"].shape[0]
    return torch.stack(keys, 1), torch.arange(N).repeat_interleave(x["pix_to_face"][0].numel())


def reach(x, mode):
    """[(image, span, steps, distinct faces, distinct in-map texels)] per wave span of sample_uv_bwd_kernel."""
    N = x["pix_to_face"].shape[0]
    HWK = x["pix_to_face"][0].numel()
    span = span_of(HWK)
    keys, _ = footprint(x, mode)
    keys = keys.view(N, HWK, -1)
    f = x["pix_to_face"].reshape(N, HWK)
    F = x["face_uvs"].shape[0]
    out = []
    for n in range(N):
        for s, b in enumerate(range(0, HWK, span)):
            fs, ks = f[n, b:b + span], keys[n, b:b + span]
            faces = fs[(fs >= 0) & (fs < F)].unique().numel()
            out.append((n, s, _ceil_div(min(span, HWK - b), LANES), faces, ks[ks >= 0].unique().numel()))
    return out


def flushes_mid_span(x, mode):
    """Does every span of at least two steps hold more distinct faces and texels than a table keeps before it empties itself?"""
    return all(faces > UV_SLOTS - RESERVE and texels > TEXEL_SLOTS - RESERVE for _, _, steps, faces, texels in reach(x, mode) if steps >= 2)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _bary(gen, n):
    b = torch.rand(n, 3, generator=gen) + 0.02
    return b / b.sum(-1, keepdim=True)


def face_blocks(F):
    """{block: (first, count)}: `inside` faces, then `lattice`, `outside` and eight `far` ones"""
    far, lat, out = 8, max(4, F // 9), max(4, F // 8)
    inside = F - far - lat - out
    assert inside >= 1, F
    return {"inside": (0, inside), "lattice": (inside, lat), "outside": (inside + lat, out), "far": (F - far, far)}


def inputs(gen, shape, F, map_size, C, mode, classes=CLASSES, M=None, L=None, one_face=False):
    """Seeded fragments on the CPU -> {pix_to_face (N,H,W,K) i64, bary (N,H,W,K,3), face_uvs (F,3,2), maps (N,Hm,Wm,C) or (N,M,Hm,Wm,C),
    grad_texels (N,H,W,K,C), classes (N,H,W) indices into CLASSES} and, with M, maps_ids (N, L / N) i64: every map used, entry 0 -- the
    id every background sample reads -- the last map.  `classes` other than `general` take the rows of class_rows.  Faces are shared
    by the images, as packed face indices are not; the gate groups them per image all the same."""
    N, H, W, K = shape
    Hm, Wm = map_size
    align, pad, samp = mode
    blocks = face_blocks(F)
    fu = torch.rand(F, 3, 2, generator=gen)
    b0, cnt = blocks["lattice"]
    fu[b0:b0 + cnt] = torch.randint(0, 17, (cnt, 3, 2), generator=gen).float() / 16.0
    fu[b0, 0] = torch.tensor([0.5, 0.5])  # the switch of torch.lerp, the centre of the map
    fu[b0, 1] = torch.tensor([0.0, 1.0])
    fu[b0, 2] = torch.tensor([1.0, 0.0])
    b0, cnt = blocks["outside"]
    for j in range(cnt):  # one coordinate outside [0, 1] by up to 0.3 at all three vertices, the other anywhere in [-0.3, 1.3]
        band = torch.rand(3, generator=gen) * 0.29 + 0.005
        other = torch.rand(3, generator=gen) * 1.6 - 0.3
        side = band + 1.0 if j & 2 else -band
        fu[b0 + j] = torch.stack([side, other] if j & 1 else [other, side], -1)
    b0, cnt = blocks["far"]
    for j, (u, v) in enumerate([(5.0, None), (None, -5.0), (-5.0, 5.0), (1e6, None), (None, 1e6), (-1e6, None), (None, -1e6), (-1e6, 1e6)]):
        near = torch.rand(3, 2, generator=gen)
        if u is not None:
            near[:, 0] = u + near[:, 0] * 0.25
        if v is not None:
            near[:, 1] = v + near[:, 1] * 0.25
        fu[b0 + j] = near

    p2f = torch.randint(0, blocks["inside"][1], (N, H, W, K), generator=gen)
    bary = _bary(gen, N * H * W * K).view(N, H, W, K, 3)
    cmap = torch.zeros(N, H, W, dtype=torch.int64)
    for name, rows in class_rows(H, classes).items():
        R = len(rows)
        if name == "outside":
            b0, cnt = blocks["outside"]
            face = torch.randint(b0, b0 + cnt, (N, R, W, K), generator=gen)
            far = torch.randint(F - 8, F, (N, R, W, K), generator=gen)
            pick = (torch.arange(W * K).view(W, K) % 8 == 3).expand(N, R, W, K)
            p2f[:, rows] = torch.where(pick, far, face)
        elif name == "lattice":
            b0, cnt = blocks["lattice"]
            p2f[:, rows] = torch.randint(b0, b0 + cnt, (N, R, W, K), generator=gen)
            p2f[:, rows[0], :3, 0] = b0
            corner = torch.randint(0, 3, (N, R, W, K), generator=gen)
            corner[:, 0, :3, 0] = torch.arange(3)
            bary[:, rows] = TF.one_hot(corner, 3).float()
        elif name == "run":
            face = torch.empty(N, R, W, K, dtype=torch.int64)
            for n, r, k in itertools.product(range(N), range(R), range(K)):
                w = 0
                while w < W:
                    length = int(torch.randint(1, 201, (1,), generator=gen))
                    face[n, r, w:w + length, k] = int(torch.randint(0, blocks["inside"][1], (1,), generator=gen))
                    w += length
            p2f[:, rows] = face
        elif name == "background":
            p2f[:, rows] = -1
            bary[:, rows] = -1.0
        cmap[:, rows] = CLASSES.index(name)
    if one_face:  # image 0: face 0 on every sample; image 1: background only
        assert N == 2 and classes == ("general",)
        p2f[0], p2f[1], bary[1], cmap[1] = 0, -1, -1.0, CLASSES.index("background")
    x = {"pix_to_face": p2f.contiguous(), "bary": bary.contiguous(), "face_uvs": fu.contiguous(), "classes": cmap}
    if M is None:
        x["maps"] = torch.rand(N, Hm, Wm, C, generator=gen)
    else:
        assert M >= 2 and (M - 1) & (M - 2) == 0, "2 id / (M - 1) is exact only for M - 1 a power of two"
        L = F if L is None else L
        assert L % N == 0
        ids = torch.arange(L) % M
        ids = ids[torch.randperm(L, generator=gen)] if L else ids
        if L:
            ids[0] = M - 1
            assert ids.unique().numel() == M
        x["maps"] = torch.rand(N, M, Hm, Wm, C, generator=gen)
        x["maps_ids"] = ids.view(N, L // N)
    # grad_texels are +-[0.5, 1] in multiples of 1 / 128, and 1 / PILE_SCALE of that on the samples that pile onto a few
    # texels: the background ones (all of an image add into the same one to four texels, 256 of them in SHAPE) and the class `outside`
    # (border padding clamps them onto the edge and corner texels, 20 and more to a corner).  Why: the map gradient is a scatter sum
    # whose order the GPU changes from run to run (atomics), while the bound is ONE draw of the same rounding, chain(float32)'s.  The
    # highest binade of grad_maps holds a few texels only -- the piles, and whichever texel drew 20 to 40 samples -- so MARGIN x the
    # largest of their few errors against the largest of a few others has a tail: with normal deviates as grad_texels, on the GPU, the per-sample
    # atomics of channel 4 at C = 5 came to 1.19 of the bound (align, zeros, nearest, image 2) while the per-wave sums of channels
    # 0 to 3 stayed below 0.2; with the piles at 1 / 16 one cell (C = 8, noalign, border, nearest) still moved from 0.24 to 0.77 between
    # two runs of the same code, and float32 sums in 60 random orders on the CPU reached 1.0 to 2.0 of it in one cell or another
    # whatever the faces' layout.  All of these are nearest-mode cells, where a term is grad_texels itself.  With multiples of 1 / 2048
    # every nearest-mode sum is exact in any order (fewer than 2^13 terms of at most 1 in absolute value) and is held to one ulp of the
    # largest entry; the bilinear sums (weight x grad_texels, four times as many terms of a quarter of the size) round as before and
    # stayed below 0.40 of their bounds in both of those runs.  A lost contribution of any kind is still 1e4 bounds large (MUTANTS).
    piled = (p2f < 0) | (cmap == CLASSES.index("outside"))[..., None]
    size = torch.round((torch.rand(N, H, W, K, C, generator=gen) * 0.5 + 0.5) * 128.0) / 128.0  # [0.5, 1]: one binade (see SEEDS)
    deviates = size * (torch.randint(0, 2, (N, H, W, K, C), generator=gen) * 2 - 1).float()
    x["grad_texels"] = deviates * torch.where(piled, 1.0 / PILE_SCALE, 1.0)[..., None]

    # redraw until the conditions hold
    free = ((cmap != CLASSES.index("lattice")) & (cmap != CLASSES.index("background")))[..., None].expand(N, H, W, K).reshape(-1)

    def unsettled():
        uv = _uv64(x)
        ok = _axis_settled(_index64(uv[:, 0], Wm, align, False), Wm, align, pad == "border", samp == "nearest")
        ok &= _axis_settled(_index64(uv[:, 1], Hm, align, True), Hm, align, pad == "border", samp == "nearest")
        return free & ~ok

    flat = x["bary"].view(-1, 3)
    for _ in range(200):
        bad = unsettled()
        if not bool(bad.any()):
            break
        flat[bad] = _bary(gen, int(bad.sum()))
    assert not bool(unsettled().any()), "a sample stays within TOL of a discontinuity"
    for name in classes:
        assert bool((cmap == CLASSES.index(name)).any()), name
    return x


_CASES = {}


def case(kind, *args):
    """-> (x, chain32, chain64) of a case of tests/test_gpu_texture_edges.py, built once per process and shared: treat it as read-only.

      ("main", C, mode)        SHAPE, FACES faces, a MAP map, all five classes
      ("small", size, mode)    SMALL_SHAPE, 40 faces, C = 3, a map of SMALL_MAPS
      ("lattice", size, mode)  SMALL_SHAPE with every row of class `lattice`, C = 3
      ("one_face", C, mode)    two images of 4096 + 1 samples: face 0 everywhere (its last wave span is one lane wide), background only
      ("multi", M, C, mode)    SHAPE, maps_ids for 288 of the 300 faces: the last twelve (outside / far ones) read zero"""
    key = (kind,) + args
    if key not in _CASES:
        mode = args[-1]
        gen = torch.Generator().manual_seed(SEEDS[kind] + 97 * MODES.index(mode) + sum(int(v) for a in args[:-1] for v in (a if isinstance(a, tuple) else (a,))))
        if kind == "main":
            x = inputs(gen, SHAPE, FACES, MAP, args[0], mode)
        elif kind == "small":
            x = inputs(gen, SMALL_SHAPE, 40, args[0], 3, mode)
        elif kind == "lattice":
            x = inputs(gen, SMALL_SHAPE, 40, args[0], 3, mode, classes=("general",))
            x = _all_lattice(gen, x)
        elif kind == "one_face":
            x = inputs(gen, (2, 1, 4097, 1), 40, MAP, args[0], mode, classes=("general",), one_face=True)
        elif kind == "multi":
            x = inputs(gen, SHAPE, FACES, (16, 20), args[1], mode, M=args[0], L=288)
        else:
            raise KeyError(kind)
        _CASES[key] = (x, chain(x, mode, torch.float32), chain(x, mode, torch.float64))
    return _CASES[key]


def _all_lattice(gen, x):
    """Every sample of x moved to the lattice faces with one-hot barycentrics."""
    F = x["face_uvs"].shape[0]
    b0, cnt = face_blocks(F)["lattice"]
    shape = x["pix_to_face"].shape
    x["pix_to_face"] = torch.randint(b0, b0 + cnt, shape, generator=gen)
    corner = torch.randint(0, 3, shape, generator=gen)
    x["pix_to_face"][:, 0, :3] = b0
    corner[:, 0, :3] = torch.arange(3)[:, None]
    x["bary"] = TF.one_hot(corner, 3).float()
    x["classes"] = torch.full(shape[:3], CLASSES.index("lattice"), dtype=torch.int64)
    return x


# ---- references ------------------------------------------------------------------------------------------------------------------
def _leaves(x, dtype, with_grad):
    return tuple(x[k].detach().to(dtype).clone().requires_grad_(with_grad) for k in ("face_uvs", "bary", "maps"))


def _pixel_uvs(x, fu, bary):
    """interpolate_face_attributes (renderer/mesh/utils.py): (N,H,W,K,2), background -- and faces that do not exist -- at 0"""
    p2f = x["pix_to_face"]
    F = fu.shape[0]
    face = (p2f >= 0) & (p2f < F)
    rows = fu[p2f.clamp(0, max(F - 1, 0))] if F else torch.zeros(p2f.shape + (3, 2), dtype=fu.dtype)
    uv = (bary[..., None] * rows).sum(-2)
    return torch.where(face[..., None], uv, torch.zeros((), dtype=fu.dtype))


def _finish(texels, x, leaves, with_grad):
    texels = texels * _valid(x).view(x["pix_to_face"].shape)[..., None].to(texels.dtype)
    res = {"texels": texels.detach()}
    if with_grad:
        fu, bary, maps = leaves
        texels.backward(x["grad_texels"].to(texels.dtype))
        grad = lambda t: torch.zeros_like(t) if t.grad is None else t.grad  # noqa: E731 -- nearest mode in restated(): no path at all
        res.update(grad_bary=grad(bary), grad_face_uvs=grad(fu), grad_maps=grad(maps))
    return res


def chain(x, mode, dtype, with_grad=True):
    """TexturesUV.sample_textures in `dtype` -> {texels} and, with_grad, the three gradients by torch autograd."""
    if "maps_ids" in x:
        return chain_multi(x, mode, dtype, with_grad)
    align, pad, samp = mode
    fu, bary, maps = leaves = _leaves(x, dtype, with_grad)
    N, H, W, K = x["pix_to_face"].shape
    _, Hm, Wm, C = maps.shape
    uv = _pixel_uvs(x, fu, bary).permute(0, 3, 1, 2, 4).reshape(N * K, H, W, 2)
    tm = maps.permute(0, 3, 1, 2)[None].expand(K, -1, -1, -1, -1).transpose(0, 1).reshape(N * K, C, Hm, Wm)
    grid = torch.lerp(uv.new_tensor([-1.0, 1.0]), uv.new_tensor([1.0, -1.0]), uv)
    t = TF.grid_sample(tm, grid, mode=samp, align_corners=align, padding_mode=pad)
    return _finish(t.reshape(N, K, C, H, W).permute(0, 3, 4, 1, 2), x, leaves, with_grad)


def chain_multi(x, mode, dtype, with_grad=True):
    """The maps_ids branch: maps (N,M,Hm,Wm,C) sampled as a volume, the map id normalised like a coordinate."""
    align, pad, samp = mode
    fu, bary, maps = leaves = _leaves(x, dtype, with_grad)
    p2f = x["pix_to_face"]
    M = maps.shape[1]
    zid = (2.0 * _map_id(x).view(p2f.shape + (1,)).float() / float(M - 1)) - 1
    uv = _pixel_uvs(x, fu, bary).permute(0, 3, 1, 2, 4)
    grid = torch.lerp(uv.new_tensor([-1.0, 1.0]), uv.new_tensor([1.0, -1.0]), uv)
    uvm = torch.cat((grid, zid.to(dtype).permute(0, 3, 1, 2, 4)), dim=4)
    t = TF.grid_sample(maps.permute(0, 4, 1, 2, 3), uvm, mode=samp, align_corners=align, padding_mode=pad)
    return _finish(t.permute(0, 3, 4, 2, 1), x, leaves, with_grad)


def kernel_order(x, mode):
    """The C oracle: float32 per sample in the kernels' order, scatter sums in double."""
    from oracle import oracle as orc

    kw = mode_kw(mode)
    a = (x["pix_to_face"], x["bary"], x["face_uvs"], x["maps"])
    if "maps_ids" in x:
        tex = orc.sample_uv_multi(*a, x["maps_ids"], **kw)
        gb, gfu, gm = orc.sample_uv_multi_backward(x["grad_texels"], *a, x["maps_ids"], **kw)
    else:
        tex = orc.sample_uv(*a, **kw)
        gb, gfu, gm = orc.sample_uv_backward(x["grad_texels"], *a, **kw)
    return {"texels": tex, "grad_bary": gb, "grad_face_uvs": gfu, "grad_maps": gm}


def restated(x, mode, mutant=None, dtype=torch.float32):
    """The sampler in explicit torch ops -> the four QUANTITIES.  mutant: one of MUTANTS, a structural error planted into it."""
    assert mutant is None or mutant in MUTANTS
    align, pad, samp = mode
    border, nearest = pad == "border", samp == "nearest"
    multi = "maps_ids" in x
    fu, bary, maps = leaves = _leaves(x, dtype, True)
    p2f = x["pix_to_face"]
    N, HWK = p2f.shape[0], p2f[0].numel()
    P = N * HWK
    F = fu.shape[0]
    f = p2f.reshape(-1)
    image = torch.arange(N).repeat_interleave(HWK)
    lost = torch.zeros(P, dtype=torch.bool)
    if mutant == "lost_step":
        first = LOST_STEP[0] * HWK + LOST_STEP[1] * LANES
        lost[first:first + LANES] = True
    rows = fu.double()[f.clamp(0, F - 1)].to(dtype)  # the scatter sums of the backward run in double, like the oracle's
    rows = torch.where(lost[:, None, None], rows.detach(), rows)
    uv = (bary.reshape(P, 3, 1) * rows).sum(1) * ((f >= 0) & (f < F))[:, None].to(dtype)
    grid = torch.lerp(uv.new_tensor([-1.0, 1.0]), uv.new_tensor([1.0, -1.0]), uv)

    def source_index(coord, size):
        pos = (coord + 1.0) / 2.0 * (size - 1) if align else ((coord + 1.0) * size - 1.0) / 2.0
        if not border:
            return pos
        clipped = pos.detach().clamp(0, size - 1)
        if mutant == "border_keeps_multiplier":
            return pos + (clipped - pos.detach())
        return torch.where((pos > 0) & (pos < size - 1), pos, clipped)

    vol = (maps if multi else maps[:, None]).double()
    M, Hm, Wm, C = vol.shape[1:]
    axes = [(source_index(grid[:, 0], Wm), Wm), (source_index(grid[:, 1], Hm), Hm)]
    if multi:
        gz = (2.0 * _map_id(x).to(dtype) / float(M - 1)) - 1
        iz = source_index(gz, M)
        axes.append((torch.round(iz) if mutant == "iz_rounded" else iz, M))
    else:
        axes.append((torch.zeros(P, dtype=dtype), 1))
    cands = []
    for k, (pos, size) in enumerate(axes):
        one = torch.ones(P, dtype=dtype)
        if nearest or (k == 2 and not multi):
            q = pos.detach()
            r = torch.where(q >= 0, torch.floor(q + 0.5), torch.ceil(q - 0.5)) if mutant == "half_away_from_zero" else torch.round(q)
            cands.append([(r.long(), one)])
        else:
            fl = torch.floor(pos.detach())
            cands.append([(fl.long(), fl + 1.0 - pos), (fl.long() + 1, pos - fl)])
    if mutant == "map_of_image_0":
        image = torch.zeros_like(image)
    frozen = lost | ((f < 0) if mutant == "background_map_grad_dropped" else torch.zeros(P, dtype=torch.bool))
    out = torch.zeros(P, C, dtype=dtype)
    for (zi, zw), (yi, yw), (xi, xw) in itertools.product(cands[2], cands[1], cands[0]):
        inside = (xi >= 0) & (xi < Wm) & (yi >= 0) & (yi < Hm) & (zi >= 0) & (zi < M)
        val = vol[image, zi.clamp(0, M - 1), yi.clamp(0, Hm - 1), xi.clamp(0, Wm - 1)].to(dtype)
        val = torch.where(frozen[:, None], val.detach(), val)
        out = out + torch.where(inside, xw * yw * zw, torch.zeros((), dtype=dtype))[:, None] * val
    return _finish(out.view(p2f.shape + (C,)), x, leaves, True)


# ---- the atlas -------------------------------------------------------------------------------------------------------------------
def atlas_cells(bary, R):
    """textures.py:600-614 -> (w_y, w_x) int64 as torch computes them, before indexing (no wrap, no range check)."""
    w01 = bary[..., :2]
    w_xy = (w01 * R).to(torch.int64).clamp(max=R - 1)
    below = (w01.sum(dim=-1) * R - w_xy.float().sum(dim=-1)) <= 1.0
    w_x, w_y = w_xy.unbind(-1)
    return torch.where(below, w_y, R - 1 - w_y), torch.where(below, w_x, R - 1 - w_x)


def atlas_chain(p2f, bary, atlas, grad_texels):
    """-> {texels (a gather), grad_atlas float64}; faces outside [0, F) read zero.  Every cell must be addressable."""
    F, R, _, C = atlas.shape
    face = (p2f >= 0) & (p2f < F)
    w_y, w_x = atlas_cells(torch.where(face[..., None], bary, torch.zeros_like(bary)), R)
    texels = atlas[p2f.clamp(0, F - 1), w_y, w_x] * face[..., None]
    ga = torch.zeros(F, R, R, C, dtype=torch.float64)
    ga.index_put_((p2f[face], w_y[face], w_x[face]), grad_texels[face].double(), accumulate=True)
    return {"texels": texels + 0.0, "grad_atlas": ga}


# ---- the gate --------------------------------------------------------------------------------------------------------------------
def touched(x, mode):
    """-> (faces (N, F) bool, texels bool of grad_maps' shape without C): what some sample of image n touches."""
    p2f = x["pix_to_face"]
    N, F = p2f.shape[0], x["face_uvs"].shape[0]
    f = p2f.reshape(N, -1)
    live = (f >= 0) & (f < F) & _valid(x).view(N, -1)
    faces = torch.zeros(N, F + 1, dtype=torch.bool)
    faces.scatter_(1, torch.where(live, f, torch.full_like(f, F)), True)
    keys, image = footprint(x, mode)
    per = x["maps"][0, ..., 0].numel()
    tex = torch.zeros(N, per + 1, dtype=torch.bool)
    flat = torch.where(keys >= 0, keys, torch.full_like(keys, per))
    tex[image[:, None].expand_as(flat).reshape(-1), flat.reshape(-1)] = True
    return faces[:, :F], tex[:, :per].view(x["maps"].shape[:-1])


def _judge(a, b, w, failures, show, label, q, group):
    if a.numel() == 0:
        return
    if not bool(torch.isfinite(w).all()):
        failures.append((q, group, float("nan"), float("nan")))
        show(f"GATE {label} {q:13s} {group:10s} the float64 chain is not finite: FAIL")
        return
    bound = max(MARGIN * float((b - w).abs().max()), ulp32(w.abs().max()))
    finite = bool(torch.isfinite(a).all())
    err = float((a - w).abs().max()) if finite else float("inf")
    ok = finite and err <= bound
    show(f"GATE {label} {q:13s} {group:10s} err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}{'' if ok else ' FAIL'}")
    if not ok:
        failures.append((q, group, err, bound))


def gate(got, chain32, chain64, x, mode, show=print, label=""):
    """The list of (quantity, group, err, bound) that `got` misses: empty when it passes.  One line per cell goes to `show`."""
    failures = []
    N = x["pix_to_face"].shape[0]
    t = {q: (got[q].detach().cpu().double(), chain32[q].detach().double(), chain64[q].detach().double()) for q in QUANTITIES}
    for q in QUANTITIES:
        assert t[q][0].shape == t[q][1].shape == t[q][2].shape, (q, [v.shape for v in t[q]])
    for q in ("texels", "grad_bary"):
        judged = 0
        for ci, cname in enumerate(CLASSES):
            sel = x["classes"] == ci
            judged += int(sel.sum()) * t[q][0][0, 0, 0].numel()
            _judge(*(v[sel] for v in t[q]), failures, show, label, q, cname)
        assert judged == t[q][0].numel(), (q, judged)  # no element is left out of every class
    faces, texels = touched(x, mode)
    for q, rows in (("grad_face_uvs", faces), ("grad_maps", texels)):
        a, b, w = t[q]
        for n in range(N):
            if q == "grad_maps":
                _judge(a[n][rows[n]], b[n][rows[n]], w[n][rows[n]], failures, show, label, q, f"image {n}")
            else:
                _judge(a[rows[n]], b[rows[n]], w[rows[n]], failures, show, label, q, f"image {n}")
        never = ~rows if q == "grad_maps" else ~rows.any(0)
        stray = int((a[never] != 0).sum()) + int((w[never] != 0).sum())
        show(f"GATE {label} {q:13s} untouched  {int(never.sum())} rows, {stray} entries not 0.0{' FAIL' if stray else ''}")
        if stray:
            failures.append((q, "untouched", float(a[never].abs().max()), 0.0))
    return failures


def old_gate(got, reference):
    """The gate these kernels had: allclose(atol = rtol = 1e-5) on the texels, allclose(rtol=1e-3, atol=2e-5 max(1, |ref|.max())) on
    every gradient, each over the whole tensor.  -> accepted?"""
    ok = True
    for q in QUANTITIES:
        a, r = got[q].detach().cpu().float(), reference[q].detach().float()
        ok &= torch.allclose(a, r, atol=1e-5, rtol=1e-5) if q == "texels" else torch.allclose(a, r, rtol=1e-3, atol=2e-5 * max(1.0, float(r.abs().max())))
    return bool(ok)
