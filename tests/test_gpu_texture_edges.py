"""The UV and atlas texture kernels (csrc/texture.hip, csrc/texture_multi.hip, csrc/atlas.hip) per mode, per channel width and at their
edges, against the float64 chain of tests/texture_case.py through its per-class gate (tests/test_cpu_texture_case.py shows on the CPU
that the gate is feasible for the oracle's restatement and what it rejects).

What selects a path:

    sampling_mode         the <NEAREST> instantiations of sample_uv_fwd_kernel / _bwd_kernel
    C <= 4                the map gradient through the texel table (kChunk, pitch 0, nlive = C); above: one atomic per sample and corner
    C > 4                 background channels 4.. take the per-sample road, 0..3 the per-wave sum
    > 64 faces, > 256     the uv table (128 slots) and the texel table (320 slots) empty themselves inside a wave span: the `main` cases,
    texels per span       asserted through texture_case.reach
    > 16384 * 1024        uvm_grid / atlas_grid cap the launch at 16384 workgroups: a fifth grid-stride round (test_long_launch_*)
    samples
The launch caps of the single-map kernels (65 535 workgroups x 1024 samples forward, 65 536 waves x 4096 samples backward) lie beyond
6.7e7 samples and are not run.
"""
import re
from collections import namedtuple

import pytest
import torch

import texture_case as tc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INVALID = -1  # P3D_ERR_INVALID_ARG
Frag = namedtuple("Frag", "pix_to_face bary_coords")
MODE_IDS = dict(argvalues=tc.MODES, ids=tc.mode_id)


def run(x, mode, wrap=None):
    """-> the four quantities of texture_case.QUANTITIES on the GPU, through the wrappers.  wrap: {name: f(tensor) -> the operand handed
    over}, for the strided-operand test."""
    import pytorch3d_amd as p3d

    wrap = wrap or {}
    w = lambda k, t: wrap[k](t) if k in wrap else t  # noqa: E731
    fu, b, mp = (x[k].to(DEV).detach().clone().requires_grad_(True) for k in ("face_uvs", "bary", "maps"))
    ids = x["maps_ids"].to(DEV) if "maps_ids" in x else None
    tex = p3d.sample_textures_uv(Frag(w("pix_to_face", x["pix_to_face"].to(DEV)), w("bary", b)), fu, w("maps", mp), maps_ids=ids,
                                 **tc.mode_kw(mode))
    tex.backward(w("grad_texels", x["grad_texels"].to(DEV)))
    torch.cuda.synchronize()
    return {"texels": tex.detach(), "grad_bary": b.grad, "grad_face_uvs": fu.grad, "grad_maps": mp.grad}


def _gated(kind, *args):
    x, c32, c64 = tc.case(kind, *args)
    mode = args[-1]
    got = run(x, mode)
    label = f"{kind} {' '.join(str(a) for a in args[:-1])} {tc.mode_id(mode)}"
    assert tc.gate(got, c32, c64, x, mode, label=label) == []
    return x, got, c64


@pytest.mark.parametrize("mode", **MODE_IDS)
@pytest.mark.parametrize("C", tc.CHANNELS)
def test_single_map_every_mode_and_channel_width(C, mode):
    """3 images of 24 x 64 x 2: one workgroup, four waves of twelve steps, in which both tables empty themselves; all five classes."""
    x, _, _ = _gated("main", C, mode)
    assert tc.flushes_mid_span(x, mode)


@pytest.mark.parametrize("mode", **MODE_IDS)
@pytest.mark.parametrize("size", tc.SMALL_MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_maps(size, mode):
    """Hm = 1 or Wm = 1: with align_corners the multiplier is (size - 1) / 2 = 0 and every index 0."""
    _gated("small", size, mode)


@pytest.mark.parametrize("mode", **MODE_IDS)
@pytest.mark.parametrize("size", tc.LATTICE_MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_lattice_only_image(size, mode):
    """Every sample on a tie, an integer index, a clamp equality or u = 0.5.  Nearest-mode texels are gathers: bit for bit."""
    _, got, c64 = _gated("lattice", size, mode)
    if mode[2] == "nearest":
        assert torch.equal(got["texels"].cpu(), c64["texels"].float())


@pytest.mark.parametrize("mode", **MODE_IDS)
@pytest.mark.parametrize("C", [3, 5])
def test_one_face_over_an_image_and_an_all_background_image(C, mode):
    """4096 + 1 samples per image: two waves, the second span ends one lane into its last step.  Image 0: every sample on face 0 (the
    tables merge all lanes of a step); image 1: background only (the per-wave sum, `t == 0` never true; C = 5: channel 4 per sample)."""
    x, got, _ = _gated("one_face", C, mode)
    assert tc.span_of(4097) * 4 >= 4097 > tc.span_of(4097) * 3 and (4097 - tc.span_of(4097) * 3) % 64 == 1
    assert bool((got["grad_face_uvs"][1:] == 0).all()) and bool((got["grad_bary"][1] == 0).all())


@pytest.mark.parametrize("mode", **MODE_IDS)
@pytest.mark.parametrize("M,C", tc.MULTI)
def test_multi_map_every_mode(M, C, mode):
    """ids cover every map, 0 and M - 1; 288 ids for 300 faces (the others read zero); every image has background rows, which read
    the map of face 0: the last one.  With align_corners=False the ids 0 and M - 1 sit half a map outside the volume."""
    x, got, _ = _gated("multi", M, C, mode)
    ids = x["maps_ids"].reshape(-1)
    assert int(ids[0]) == M - 1 and ids.unique().numel() == M and ids.numel() < x["face_uvs"].shape[0]
    no_id = (x["pix_to_face"] >= ids.numel())
    assert bool(no_id.any()) and bool((got["texels"].cpu()[no_id] == 0).all()) and bool((got["grad_bary"].cpu()[no_id] == 0).all())


@pytest.mark.parametrize("mode", [tc.MODES[0], tc.MODES[7]], ids=tc.mode_id)
def test_multi_map_without_ids(mode):
    """L = 0: every sample, the background included, reads zero; no gradient anywhere."""
    x = dict(tc.case("multi", 3, 3, mode)[0])
    x["maps_ids"] = x["maps_ids"][:, :0]
    got = run(x, mode)
    for q, t in got.items():
        assert bool((t == 0).all()), q


def test_pix_to_face_beyond_the_face_count_reads_zero():
    """pix_to_face == F and F + 7 on a few samples of a `general` row: zeros there, every other sample as before bit for bit, the
    scatter gradients within the gate of the chain on the same input (the chain masks such samples)."""
    mode = (True, "border", "bilinear")
    base, _, _ = tc.case("main", 3, mode)
    before = run(base, mode)
    x = {k: v.clone() for k, v in base.items()}
    F = x["face_uvs"].shape[0]
    assert int(x["classes"][0, 0, 0]) == 0
    x["pix_to_face"][:, 0, 3:9, 0] = F
    x["pix_to_face"][:, 0, 20:23, 1] = F + 7
    hit = x["pix_to_face"] >= F
    for m in tc.MODES:
        got = run(x, m)
        assert bool((got["texels"].cpu()[hit] == 0).all()) and bool((got["grad_bary"].cpu()[hit] == 0).all()), m
        if m == mode:
            assert torch.equal(got["texels"].cpu()[~hit], before["texels"].cpu()[~hit])
            assert torch.equal(got["grad_bary"].cpu()[~hit], before["grad_bary"].cpu()[~hit])
            assert tc.gate(got, tc.chain(x, m, torch.float32), tc.chain(x, m, torch.float64), x, m, label="beyond F") == []


# ---- the C entries ---------------------------------------------------------------------------------------------------------------
def _status(entry, *args):
    """The status an entry returns through _lib.call (0 when it does not raise)."""
    from pytorch3d_amd import _lib

    try:
        _lib.call(entry, "test", DEV, *args)
    except RuntimeError as e:
        m = re.search(r"\(p3d error (-?\d+)\)", str(e))
        assert m, str(e)
        return int(m.group(1))
    return 0


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _atlas_inputs(gen, P, F, R, C):
    p2f = torch.randint(-1, F + 1, (1, 1, P, 1), generator=gen)  # F itself: no such face
    b = torch.rand(1, 1, P, 1, 2, generator=gen) * 1.2 - 0.1
    b[0, 0, :8, 0] = torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [0.5, 0.5], [-0.05, 0.3], [0.25, 0.75], [1.0, 1.0], [0.999, 0.0]])
    bary = torch.cat([b, 1.0 - b.sum(-1, keepdim=True)], -1).contiguous()
    return p2f, bary, torch.rand(F, R, R, C, generator=gen) + 0.5


@pytest.mark.parametrize("mode", [tc.MODES[0], tc.MODES[5]], ids=tc.mode_id)
def test_every_output_element_is_written(mode):
    """The six entries through _lib.call into buffers that hold NaN: texels and grad_bary equal what the wrappers return, the scatter
    gradients are finite, within the wrappers' own results' gate and exactly zero where no sample touches them."""
    import pytorch3d_amd as p3d

    align, pad, samp = int(mode[0]), {"zeros": 0, "border": 1}[mode[1]], {"bilinear": 0, "nearest": 1}[mode[2]]
    for kind, args in (("small", ((2, 2), mode)), ("multi", (3, 3, mode))):
        x, c32, c64 = tc.case(kind, *args)
        N, H, W, K = x["pix_to_face"].shape
        p2f, b, fu, mp, g = (x[k].to(DEV) for k in ("pix_to_face", "bary", "face_uvs", "maps", "grad_texels"))
        F, C = fu.shape[0], mp.shape[-1]
        Hm, Wm = mp.shape[-3], mp.shape[-2]
        tex, gb, gfu, gm = _nan(N, H, W, K, C), _nan(N, H, W, K, 3), _nan(F, 3, 2), _nan(*mp.shape)
        if kind == "multi":
            ids = x["maps_ids"].to(DEV).reshape(-1)
            head = (ids, ids.numel(), N, H, W, K, F, mp.shape[1], Hm, Wm, C, align, pad, samp)
            assert _status("p3d_sample_uv_multi_forward", p2f, b, fu, mp, *head, tex) == 0
            assert _status("p3d_sample_uv_multi_backward", g, p2f, b, fu, mp, *head, gb, gfu, gm) == 0
        else:
            head = (N, H, W, K, F, Hm, Wm, C, align, pad, samp)
            assert _status("p3d_sample_uv_forward", p2f, b, fu, mp, *head, tex) == 0
            assert _status("p3d_sample_uv_backward", g, p2f, b, fu, mp, *head, gb, gfu, gm) == 0
        torch.cuda.synchronize()
        want = run(x, mode)
        assert torch.equal(tex, want["texels"]) and torch.equal(gb, want["grad_bary"]), kind
        raw = {"texels": tex, "grad_bary": gb, "grad_face_uvs": gfu, "grad_maps": gm}
        assert tc.gate(raw, c32, c64, x, mode, label=f"raw {kind}") == []  # finite, and 0.0 where untouched
    gen = torch.Generator().manual_seed(77)
    P, F, R, C = 1000, 9, 3, 3
    p2f, bary, atlas = _atlas_inputs(gen, P, F, R, C)
    p2f[p2f == 4] = 5  # face 4: never sampled
    g = torch.randn(1, 1, P, 1, C, generator=gen)
    tex, ga = _nan(1, 1, P, 1, C), _nan(F, R, R, C)
    assert _status("p3d_sample_atlas_forward", p2f.to(DEV), bary.to(DEV), atlas.to(DEV), P, F, R, C, tex) == 0
    assert _status("p3d_sample_atlas_backward", g.to(DEV), p2f.to(DEV), bary.to(DEV), P, F, R, C, ga) == 0
    torch.cuda.synchronize()
    want = tc.atlas_chain(p2f, bary, atlas, g)
    assert torch.equal(tex.cpu(), want["texels"])
    assert bool(torch.isfinite(ga).all()) and bool((ga[4] == 0).all()) and bool((ga.cpu()[want["grad_atlas"] == 0] == 0).all())
    a = p3d.sample_textures_atlas(Frag(p2f.to(DEV), bary.to(DEV)), atlas.to(DEV))
    assert torch.equal(a, tex)


def test_argument_checks_of_the_c_entries():
    """M < 2, Hm < 1, an unknown padding or sampling mode and N > 65535: P3D_ERR_INVALID_ARG and no launch (the outputs keep their NaN)."""
    N, H, W, K, F, M, Hm, Wm, C = 1, 2, 3, 1, 4, 2, 2, 2, 1
    p2f = torch.zeros(N, H, W, K, dtype=torch.int64, device=DEV)
    b, fu, g = torch.rand(N, H, W, K, 3, device=DEV), torch.rand(F, 3, 2, device=DEV), torch.rand(N, H, W, K, C, device=DEV)
    mp, ids = torch.rand(N, M, Hm, Wm, C, device=DEV), torch.zeros(F, dtype=torch.int64, device=DEV)
    tex, gb, gfu, gm = _nan(N, H, W, K, C), _nan(N, H, W, K, 3), _nan(F, 3, 2), _nan(N, M, Hm, Wm, C)

    def single(N=N, Hm=Hm, pad=0, samp=0):
        head = (N, H, W, K, F, Hm, Wm, C, 1, pad, samp)
        return [_status("p3d_sample_uv_forward", p2f, b, fu, mp, *head, tex), _status("p3d_sample_uv_backward", g, p2f, b, fu, mp, *head, gb, gfu, gm)]

    def multi(N=N, M=M, Hm=Hm, pad=0, samp=0):
        head = (ids, F, N, H, W, K, F, M, Hm, Wm, C, 1, pad, samp)
        return [_status("p3d_sample_uv_multi_forward", p2f, b, fu, mp, *head, tex),
                _status("p3d_sample_uv_multi_backward", g, p2f, b, fu, mp, *head, gb, gfu, gm)]

    refused = (single(Hm=0) + single(pad=2) + single(pad=-1) + single(samp=2) + single(N=65536)
               + multi(M=1) + multi(M=0) + multi(Hm=0) + multi(pad=2) + multi(samp=2) + multi(samp=-1) + multi(N=65536))
    assert refused == [INVALID] * len(refused), refused
    torch.cuda.synchronize()
    for t in (tex, gb, gfu, gm):
        assert bool(torch.isnan(t).all())
    assert single() == [0, 0] and multi() == [0, 0]  # the same arguments, valid: accepted
    torch.cuda.synchronize()


# ---- operands as they arrive -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [tc.MODES[2], tc.MODES[4]], ids=tc.mode_id)
def test_strided_operands_equal_contiguous_copies(mode):
    """maps permuted from (N, C, Hm, Wm), bary a [..., :3] slice of a 4-wide tensor, pix_to_face expanded over K, grad_texels permuted:
    the forward equals that of contiguous copies bit for bit, the backward passes the gate."""
    gen = torch.Generator().manual_seed(tc.SEED + 5)
    x1 = tc.inputs(gen, (2, 16, 16, 1), 40, (8, 12), 3, mode)
    K = 2
    x = dict(x1)
    x["pix_to_face"] = x1["pix_to_face"].expand(-1, -1, -1, K).contiguous()
    x["bary"] = x1["bary"].expand(-1, -1, -1, K, -1).contiguous()
    x["grad_texels"] = torch.randn(2, 16, 16, K, 3, generator=gen)
    wrap = {"pix_to_face": lambda t: t[..., :1].expand(-1, -1, -1, K),
            "bary": lambda t: torch.cat([t, torch.zeros_like(t[..., :1])], -1)[..., :3],
            "maps": lambda t: (t.permute(0, 3, 1, 2).contiguous() * 1.0).permute(0, 2, 3, 1),
            "grad_texels": lambda t: t.permute(0, 1, 2, 4, 3).contiguous().permute(0, 1, 2, 4, 3)}
    for k, f in wrap.items():
        assert not f(x[k].to(DEV)).is_contiguous(), k
    plain, strided = run(x, mode), run(x, mode, wrap)
    assert torch.equal(plain["texels"], strided["texels"])
    c32, c64 = tc.chain(x, mode, torch.float32), tc.chain(x, mode, torch.float64)
    assert tc.gate(strided, c32, c64, x, mode, label="strided") == []


@pytest.mark.parametrize("C", [3, 5])
def test_two_runs_of_one_backward(C):
    """grad_bary is written per sample: bit for bit.  grad_maps and grad_face_uvs are atomic sums: each run within the gate."""
    mode = (False, "zeros", "bilinear")
    x, c32, c64 = tc.case("main", C, mode)
    a, b = run(x, mode), run(x, mode)
    assert torch.equal(a["texels"], b["texels"]) and torch.equal(a["grad_bary"], b["grad_bary"])
    assert tc.gate(a, c32, c64, x, mode, label="run 1") == [] and tc.gate(b, c32, c64, x, mode, label="run 2") == []


# ---- long launches -----------------------------------------------------------------------------------------------------------------
# uvm_grid and atlas_grid launch ceil(samples / 1024) workgroups of 256 lanes, 16384 at the most: the grid-stride loops take four rounds
# at any size, and more only beyond 16384 * 1024 samples.  Two sizes: 16384 * 256 + 257 (4097 workgroups, the fourth round partly
# filled) and 16384 * 1024 + 257 (the cap: four full rounds, then one full workgroup and one lane of the next in round five).
BLOCK = 65536
LONG = {"4097-workgroups": 16384 * 256 + 256 + 1, "past-the-cap": 16384 * 1024 + 256 + 1}


def _tile(t, dim, big):
    """t (a block of BLOCK samples along `dim`) repeated to `big` samples, on the GPU"""
    idx = torch.arange(big, device=DEV) % BLOCK
    return t.to(DEV).index_select(dim, idx).contiguous()


@pytest.mark.parametrize("big", list(LONG.values()), ids=list(LONG))
def test_long_launch_multi_map(big):
    """sample_uvm_fwd_kernel / _bwd_kernel with N = K = C = 1, two 2 x 2 maps, F = 8 with ids for six.  The input is a block of 65 536
    samples repeated, and every figure in it is a short dyadic number -- one-hot barycentrics, vertex uvs k / 16, maps k / 4,
    align_corners (ix = u, iy = 1 - v, iz = id), grad_texels +-1 on two samples in every 4 x (number of repeats) and 0 elsewhere -- so
    that every term of every scatter sum is a multiple of 2^-8, at most 1 in absolute value, and fewer than 2^16 of them are not zero:
    every float32 sum is exact in any order (asserted below), and the results equal the float64 chain's bit for bit.  The chain runs on
    the block and on its first 257 samples; the scatter gradients of the full input are (repeats) x the block's + the head's."""
    mode = (True, "zeros", "bilinear")
    reps, rest = divmod(big, BLOCK)
    assert rest == 257
    gen = torch.Generator().manual_seed(tc.SEED + 64)
    F, M = 8, 2
    mod = 4 * reps
    at = torch.arange(BLOCK) % mod
    x0 = {"pix_to_face": torch.randint(-1, F, (1, 1, BLOCK, 1), generator=gen),
          "bary": torch.nn.functional.one_hot(torch.randint(0, 3, (1, 1, BLOCK, 1), generator=gen), 3).float(),
          "face_uvs": torch.randint(0, 17, (F, 3, 2), generator=gen).float() / 16.0,
          "maps": torch.randint(0, 5, (1, M, 2, 2, 1), generator=gen).float() / 4.0,
          "maps_ids": torch.tensor([[1, 0, 1, 1, 0, 0]]),
          "grad_texels": torch.where((at == 77) | (at == 256 % mod), torch.randint(0, 2, (BLOCK,), generator=gen).float() * 2 - 1,
                                     torch.zeros(BLOCK)).view(1, 1, BLOCK, 1, 1)}
    x0["pix_to_face"][0, 0, 77::mod, 0][1::3] = -1  # background samples that carry a gradient
    x0["pix_to_face"][0, 0, 77, 0], x0["pix_to_face"][0, 0, 256, 0] = 2, 3
    sliced = lambda v: v.dim() >= 4 and v.shape[2] == BLOCK  # noqa: E731
    head = {k: (v[:, :, :257].contiguous() if sliced(v) else v) for k, v in x0.items()}
    full64, head64 = tc.chain(x0, mode, torch.float64), tc.chain(head, mode, torch.float64)
    nonzero = int((x0["grad_texels"] != 0).sum()) * reps + int((head["grad_texels"] != 0).sum())
    # a term of grad_maps is weight x grad_texel, a multiple of 2^-8 with |term| <= 1; one of grad_face_uvs is (a difference of two map
    # values) x weight, a multiple of 2^-6 with |term| <= 1: sums of fewer than 2^16 such terms stay below 2^24 units of 2^-8
    assert nonzero < 2 ** 16 and int((head["grad_texels"] != 0).sum()) >= 2 and float(head["grad_texels"][0, 0, 256]) != 0
    for q, unit in (("texels", 1024), ("grad_bary", 1024), ("grad_face_uvs", 64), ("grad_maps", 256)):
        assert torch.equal((full64[q] * unit).round(), full64[q] * unit), q
    x = {k: (_tile(v, 2, big) if sliced(v) else v.to(DEV)) for k, v in x0.items()}
    got = run(x, mode)
    idx = torch.arange(big) % BLOCK
    for q in ("texels", "grad_bary"):
        assert torch.equal(got[q].cpu()[0, 0], full64[q].float()[0, 0][idx]), q  # every sample of every round
    for q in ("grad_face_uvs", "grad_maps"):
        want = full64[q] * reps + head64[q]
        assert bool(want.abs().max() > 0) and bool((head64[q] != 0).any()), q
        assert torch.equal(got[q].cpu().double(), want), (q, got[q].cpu().double() - want)


@pytest.mark.parametrize("big", list(LONG.values()), ids=list(LONG))
def test_long_launch_atlas(big):
    """atlas_fwd_kernel / atlas_bwd_kernel (the C = 1 instantiations), R = 2, F = 8: the forward is a gather, compared bit for bit on every
    sample; grad_texels are -1, 0 and 1 on every fourth sample, so every atomic sum is an integer below 2^24, exact in any order, and
    equals the float64 sum: (repeats) x the block's + that of its first 257 samples."""
    import pytorch3d_amd as p3d

    reps, rest = divmod(big, BLOCK)
    assert rest == 257 and big // 4 + 1 < 2 ** 24
    gen = torch.Generator().manual_seed(tc.SEED + 65)
    F, R, C = 8, 2, 1
    p2f, bary, atlas = _atlas_inputs(gen, BLOCK, F, R, C)
    g = torch.randint(-1, 2, (1, 1, BLOCK, 1, C), generator=gen).float() * (torch.arange(BLOCK) % 4 == 0).view(1, 1, BLOCK, 1, 1)
    p2f[0, 0, 256, 0], g[0, 0, 256, 0, 0] = 3, 1.0  # the lone lane of the last workgroup carries a gradient
    block = tc.atlas_chain(p2f, bary, atlas, g)
    head = tc.atlas_chain(p2f[:, :, :257], bary[:, :, :257], atlas, g[:, :, :257])
    at = atlas.to(DEV).requires_grad_(True)
    tex = p3d.sample_textures_atlas(Frag(_tile(p2f, 2, big), _tile(bary, 2, big)), at)
    tex.backward(_tile(g, 2, big))
    torch.cuda.synchronize()
    idx = torch.arange(big) % BLOCK
    assert torch.equal(tex.detach().cpu()[0, 0], block["texels"][0, 0][idx])
    want = block["grad_atlas"] * reps + head["grad_atlas"]
    assert bool((head["grad_atlas"] != 0).any())
    assert torch.equal(at.grad.cpu().double(), want)
