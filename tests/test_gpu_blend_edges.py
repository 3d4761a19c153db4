"""The RGB blend kernels of csrc/blend.hip (sigmoid_alpha_blend, softmax_rgb_blend, hard_rgb_blend) per capacity, per branch and at
their edges, against the float64 chain of tests/blend_case.py through its per-class gate (tests/test_cpu_blend_case.py shows on the
CPU that the gate is feasible for the kernels' order of operations and what it rejects).

K -> kernel (blend_capacity / P3D_BLEND_DISPATCH; sigmoid_alpha_{fwd,bwd} and softmax_blend_{fwd,bwd} alike):

    K = 1 -> <1>     2 -> <2>     3, 4 -> <4>     5, 7, 8 -> <8>     9, 16 -> <16>     31, 32 -> <32>
    33, 64, 150 -> sigmoid_alpha_*_generic, softmax_blend_generic<false / true>

K = 2, 4, 8, 16, 32 take the 16-byte row loaders (pix_to_face from K = 2, float and colour rows from K = 4), the others the scalar ones
with the padded tail.  test_every_capacity gates each of them for both operators, forward and backward.
"""
import re

import pytest
import torch

import blend_case as bc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INVALID = -1  # P3D_ERR_INVALID_ARG


class Frag:
    def __init__(self, pix_to_face, zbuf, dists):
        self.pix_to_face, self.zbuf, self.dists = pix_to_face, zbuf, dists


def _plane(v):
    return torch.tensor(v, dtype=torch.float32, device=DEV) if isinstance(v, (tuple, list)) else v


def run_softmax(x, sigma, gamma, bg, znear, zfar, grad_out):
    """-> the four quantities of blend_case.QUANTITIES, on the GPU"""
    import pytorch3d_amd as p3d

    c, d, z = (x[k].to(DEV).detach().clone().requires_grad_(True) for k in ("colors", "dists", "zbuf"))
    img = p3d.softmax_rgb_blend(c, Frag(x["pix_to_face"].to(DEV), z, d), p3d.BlendParams(sigma, gamma, bg), znear=_plane(znear),
                                zfar=_plane(zfar))
    img.backward(grad_out.to(DEV))
    torch.cuda.synchronize()
    return {"out": img.detach(), "grad_colors": c.grad, "grad_dists": d.grad, "grad_zbuf": z.grad}


def run_sigmoid(x, sigma, grad_alphas):
    from pytorch3d_amd import _C

    d, p2f = x["dists"].to(DEV), x["pix_to_face"].to(DEV)
    alphas = _C.sigmoid_alpha_blend(d, p2f, sigma)
    gd = _C.sigmoid_alpha_blend_backward(grad_alphas.to(DEV), alphas, d, p2f, sigma)
    torch.cuda.synchronize()
    return {"out": alphas, "grad_dists": gd}


def run_hard(x, bg, grad_out):
    import pytorch3d_amd as p3d

    c = x["colors"].to(DEV).detach().clone().requires_grad_(True)
    img = p3d.hard_rgb_blend(c, Frag(x["pix_to_face"].to(DEV), None, None), p3d.BlendParams(background_color=bg))
    img.backward(grad_out.to(DEV))
    torch.cuda.synchronize()
    return {"out": img.detach(), "grad_colors": c.grad}


def _softmax_args(x, sigma, gamma, bg, zn, zf):
    return (x["colors"], x["pix_to_face"], x["dists"], x["zbuf"], sigma, gamma, bg, zn, zf)


def _check_sigmoid_and_hard(x, sigma, bg, grad_out, label):
    got = run_sigmoid(x, sigma, grad_out[..., 3])
    c32 = bc.sigmoid_chain(x["pix_to_face"], x["dists"], sigma, torch.float32, grad_out[..., 3])
    c64 = bc.sigmoid_chain(x["pix_to_face"], x["dists"], sigma, torch.float64, grad_out[..., 3])
    assert bc.gate(got, c32, c64, x["classes"], label=label + " sigmoid") == []
    hard, want = run_hard(x, bg, grad_out), bc.hard_chain(x["colors"], x["pix_to_face"], bg, grad_out)
    assert torch.equal(hard["out"].cpu(), want["out"]) and torch.equal(hard["grad_colors"].cpu(), want["grad_colors"])


@pytest.mark.parametrize("pattern", bc.PATTERNS)
@pytest.mark.parametrize("K", bc.CAPACITIES)
def test_every_capacity(K, pattern):
    """Per-image planes as tensors, all five pixel classes (four at K = 1), both gammas; the same inputs as the CPU feasibility test."""
    N, H, W = bc.SHAPE
    gen = torch.Generator().manual_seed(bc.SEED + 10 * K + bc.PATTERNS.index(pattern))
    x = bc.inputs(gen, N, H, W, K, bc.SIGMA, pattern, zfar=bc.ZFAR)
    grad_out = torch.randn(N, H, W, 4, generator=gen)
    for gamma in bc.GAMMAS:
        args = _softmax_args(x, bc.SIGMA, gamma, bc.BG, bc.ZNEAR, bc.ZFAR)
        c32, c64 = bc.chain(*args, torch.float32, grad_out), bc.chain(*args, torch.float64, grad_out)
        got = run_softmax(x, bc.SIGMA, gamma, bc.BG, bc.ZNEAR, bc.ZFAR, grad_out)
        assert bc.gate(got, c32, c64, x["classes"], label=f"K={K} {pattern} gamma={gamma}") == []
    _check_sigmoid_and_hard(x, bc.SIGMA, bc.BG, grad_out, f"K={K} {pattern}")


@pytest.mark.parametrize("K", [2, 8, 33])
def test_default_parameters(K):
    """BlendParams() -- sigma = gamma = 1e-4 -- with the scalar planes 1 / 100.  (z_inv - z_inv_max) / gamma amplifies rounding by 1e4:
    the bound is MARGIN x whatever the float32 chain itself misses on this input (printed per cell, of the order 1e-3 on the image
    as test_softmax_rgb_blend_at_bench_size_vs_dense_torch describes)."""
    import pytorch3d_amd as p3d

    N, H, W = bc.SHAPE
    bp = p3d.BlendParams()
    gen = torch.Generator().manual_seed(bc.SEED + 10 * K)
    x = bc.inputs(gen, N, H, W, K, bp.sigma, "prefix", zfar=100.0)
    grad_out = torch.randn(N, H, W, 4, generator=gen)
    args = _softmax_args(x, bp.sigma, bp.gamma, bp.background_color, 1.0, 100.0)
    c32, c64 = bc.chain(*args, torch.float32, grad_out), bc.chain(*args, torch.float64, grad_out)
    got = run_softmax(x, bp.sigma, bp.gamma, bp.background_color, 1.0, 100.0, grad_out)
    assert bc.gate(got, c32, c64, x["classes"], label=f"K={K} BlendParams()") == []
    _check_sigmoid_and_hard(x, bp.sigma, bp.background_color, grad_out, f"K={K} BlendParams()")


@pytest.mark.parametrize("gamma", bc.GAMMAS)
def test_register_and_generic_kernels_agree(gamma):
    """Fragments at K = 32 (the <32> kernels) and the same padded to K = 33 with one empty slot (the generic kernels): both add the
    same terms in the same order and the pad contributes w = 0 and a factor 1 - p = 1, so the images are equal bit for bit."""
    N, H, W = bc.SHAPE
    gen = torch.Generator().manual_seed(3233)
    x = bc.inputs(gen, N, H, W, 32, bc.SIGMA, "holes", zfar=bc.ZFAR)
    grad_out = torch.randn(N, H, W, 4, generator=gen)
    pad = lambda t, v: torch.cat([t, torch.full_like(t[..., :1], v)], dim=3)  # noqa: E731
    y = {"colors": torch.cat([x["colors"], torch.rand(N, H, W, 1, 3, generator=gen)], dim=3), "pix_to_face": pad(x["pix_to_face"], -1),
         "dists": pad(x["dists"], -1.0), "zbuf": pad(x["zbuf"], -1.0), "classes": x["classes"]}
    a = run_softmax(x, bc.SIGMA, gamma, bc.BG, bc.ZNEAR, bc.ZFAR, grad_out)
    b = run_softmax(y, bc.SIGMA, gamma, bc.BG, bc.ZNEAR, bc.ZFAR, grad_out)
    differ = (a["out"] != b["out"]).any(-1)
    print("pixels whose images differ:", int(differ.sum()), "largest difference", float((a["out"] - b["out"]).abs().max()))
    assert torch.equal(a["out"], b["out"])
    args = _softmax_args(y, bc.SIGMA, gamma, bc.BG, bc.ZNEAR, bc.ZFAR)
    c32, c64 = bc.chain(*args, torch.float32, grad_out), bc.chain(*args, torch.float64, grad_out)
    assert bc.gate(b, c32, c64, y["classes"], label=f"K=32+1 gamma={gamma}") == []
    for q in ("grad_colors", "grad_dists", "grad_zbuf"):
        assert bool((b[q][:, :, :, 32] == 0).all()), q  # the padded slot
    sa, sb = run_sigmoid(x, bc.SIGMA, grad_out[..., 3]), run_sigmoid(y, bc.SIGMA, grad_out[..., 3])
    assert torch.equal(sa["out"], sb["out"]) and torch.equal(sa["grad_dists"], sb["grad_dists"][..., :32])
    assert bool((sb["grad_dists"][..., 32] == 0).all())


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


def _raw_all(x, sigma, gamma, bg, zn_t, zf_t, grad_out, alphas):
    """Every RGB blend entry once, through _lib.call, into buffers that hold NaN -> {name: tensor}; all statuses are P3D_OK."""
    N, H, W, K = x["pix_to_face"].shape
    c, p2f, d, z = (x[k].to(DEV) for k in ("colors", "pix_to_face", "dists", "zbuf"))
    g = grad_out.to(DEV)
    ga = g[..., 3].contiguous()
    r = {"softmax_out": _nan(N, H, W, 4), "softmax_gc": _nan(N, H, W, K, 3), "softmax_gd": _nan(N, H, W, K), "softmax_gz": _nan(N, H, W, K),
         "sigmoid_out": _nan(N, H, W), "sigmoid_gd": _nan(N, H, W, K), "hard_out": _nan(N, H, W, 4), "hard_gc": _nan(N, H, W, K, 3)}
    assert _status("p3d_softmax_rgb_blend_forward", c, p2f, d, z, sigma, gamma, bg, 0.0, 0.0, zn_t, zf_t, N, H * W, K, r["softmax_out"]) == 0
    assert _status("p3d_softmax_rgb_blend_backward", g, c, p2f, d, z, sigma, gamma, bg, 0.0, 0.0, zn_t, zf_t, N, H * W, K, r["softmax_gc"],
                   r["softmax_gd"], r["softmax_gz"]) == 0
    assert _status("p3d_sigmoid_alpha_blend_forward", d, p2f, sigma, N * H * W, K, r["sigmoid_out"]) == 0
    assert _status("p3d_sigmoid_alpha_blend_backward", ga, alphas, d, p2f, sigma, N * H * W, K, r["sigmoid_gd"]) == 0
    assert _status("p3d_hard_rgb_blend_forward", c, p2f, bg, N * H * W, K, r["hard_out"]) == 0
    assert _status("p3d_hard_rgb_blend_backward", g, p2f, N * H * W, K, r["hard_gc"]) == 0
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("K", [2, 5, 8, 33])
def test_every_output_element_is_written(K):
    """Raw calls into buffers pre-filled with NaN, on images with empty pixels (the early-exit rows of softmax_blend_bwd_kernel
    among them): equal to what the wrappers return, no NaN left."""
    N, H, W = bc.SHAPE
    gen = torch.Generator().manual_seed(50 + K)
    x = bc.inputs(gen, N, H, W, K, bc.SIGMA, "prefix", zfar=bc.ZFAR)
    assert bool((x["pix_to_face"] < 0).all(-1).any())
    grad_out = torch.randn(N, H, W, 4, generator=gen)
    sm = run_softmax(x, bc.SIGMA, 0.05, bc.BG, bc.ZNEAR, bc.ZFAR, grad_out)
    sg, hd = run_sigmoid(x, bc.SIGMA, grad_out[..., 3]), run_hard(x, bc.BG, grad_out)
    r = _raw_all(x, bc.SIGMA, 0.05, bc.BG, _plane(bc.ZNEAR), _plane(bc.ZFAR), grad_out, sg["out"])
    want = {"softmax_out": sm["out"], "softmax_gc": sm["grad_colors"], "softmax_gd": sm["grad_dists"], "softmax_gz": sm["grad_zbuf"],
            "sigmoid_out": sg["out"], "sigmoid_gd": sg["grad_dists"], "hard_out": hd["out"], "hard_gc": hd["grad_colors"]}
    for name, t in r.items():
        assert not bool(torch.isnan(t).any()), name
        assert torch.equal(t, want[name]), name


@pytest.mark.parametrize("K", [2, 5, 33])
def test_equal_planes_follow_the_reference_chain(K):
    """zfar == znear in image 0, not in image 1.  The reference evaluates 0 / 0 * 0 there; the kernels' early exit for pixels
    without a face is guarded by zf != zn so that they do the same: the non-finite pattern of every quantity equals the one of
    chain(float32) on every pixel of both images, and image 1 is finite."""
    N, H, W = 2, 13, 11
    gen = torch.Generator().manual_seed(90 + K)
    x = bc.inputs(gen, N, H, W, K, bc.SIGMA, "prefix", zfar=(5.0, 10.0), classes=("general", "empty"))
    grad_out = torch.randn(N, H, W, 4, generator=gen)
    zn, zf = (5.0, 1.0), (5.0, 10.0)
    got = run_softmax(x, bc.SIGMA, 0.05, bc.BG, zn, zf, grad_out)
    want = bc.chain(*_softmax_args(x, bc.SIGMA, 0.05, bc.BG, zn, zf), torch.float32, grad_out)
    empty = (x["pix_to_face"] < 0).all(-1)
    assert bool(empty[0].any()) and bool(empty[1].any())
    for q in bc.QUANTITIES:
        a, b = torch.isfinite(got[q].cpu()), torch.isfinite(want[q])
        print(K, q, "non-finite entries: kernel", int((~a).sum()), "chain", int((~b).sum()))
        assert torch.equal(a, b), q
        assert not bool(torch.isfinite(got[q][0].cpu())[empty[0]].all()), q  # image 0 did not take the early exit
    for q in bc.QUANTITIES:
        assert bool(torch.isfinite(got[q][1]).all()), q
    assert torch.equal(got["out"][1][empty[1].to(DEV)].cpu(), torch.tensor(bc.BG + (0.0,)).expand(int(empty[1].sum()), 4))


def test_second_grid_stride_round():
    """blend_grid() caps a launch at 16384 workgroups of 256 lanes; 16384 * 256 + 257 pixels is the smallest launch that puts a
    partial workgroup into the second round of `i += gridDim.x * kBlendBlock`.  A block of 4099 pixels at K = 1 with every class
    that exists there is tiled to that size as one image; pixels are independent, so pixel i equals pixel i mod 4099 bit for bit,
    and the first block goes through the gate.  The generic kernels share the loop header and are not run at this size: their
    inputs alone would be 3.9 GB at K = 33."""
    P0, K, sigma, gamma = 4099, 1, bc.SIGMA, 0.05
    npix = 16384 * 256 + 257
    gen = torch.Generator().manual_seed(4099)
    zn, zf = (1.0,), (10.0,)
    x0 = bc.inputs(gen, 1, P0, 1, K, sigma, "prefix", zfar=zf)
    assert {bc.CLASSES[i] for i in x0["classes"].unique().tolist()} == {"general", "beyond", "saturated", "empty"}
    g0 = torch.randn(1, P0, 1, 4, generator=gen)
    idx = torch.arange(npix, device=DEV) % P0
    tile = lambda t: t.to(DEV)[0][idx].unsqueeze(0).contiguous()  # noqa: E731
    x = {k: tile(x0[k]) for k in ("colors", "pix_to_face", "dists", "zbuf")}
    grad_out = tile(g0)
    sm, sg, hd = run_softmax(x, sigma, gamma, bc.BG, zn, zf, grad_out), run_sigmoid(x, sigma, grad_out[..., 3]), run_hard(x, bc.BG, grad_out)
    for name, res in (("softmax", sm), ("sigmoid", sg), ("hard", hd)):
        for q, t in res.items():
            assert t.shape[1] == npix
            assert torch.equal(t[0], t[0, :P0][idx]), (name, q)
    first = lambda res: {q: t[:, :P0] for q, t in res.items()}  # noqa: E731
    args = _softmax_args(x0, sigma, gamma, bc.BG, zn, zf)
    assert bc.gate(first(sm), bc.chain(*args, torch.float32, g0), bc.chain(*args, torch.float64, g0), x0["classes"], label="round 2 softmax") == []
    c32, c64 = (bc.sigmoid_chain(x0["pix_to_face"], x0["dists"], sigma, dt, g0[..., 3]) for dt in (torch.float32, torch.float64))
    assert bc.gate(first(sg), c32, c64, x0["classes"], label="round 2 sigmoid") == []
    want = bc.hard_chain(x0["colors"], x0["pix_to_face"], bc.BG, g0)
    assert torch.equal(hd["out"][:, :P0].cpu(), want["out"]) and torch.equal(hd["grad_colors"][:, :P0].cpu(), want["grad_colors"])


@pytest.mark.parametrize("K", [8, 33])
def test_three_runs_one_on_a_side_stream_give_identical_bits(K):
    """The kernels contain no atomics."""
    N, H, W = bc.SHAPE
    gen = torch.Generator().manual_seed(60 + K)
    x = bc.inputs(gen, N, H, W, K, bc.SIGMA, "holes", zfar=bc.ZFAR)
    grad_out = torch.randn(N, H, W, 4, generator=gen)

    def once():
        res = {}
        for name, r in (("softmax", run_softmax(x, bc.SIGMA, 0.05, bc.BG, bc.ZNEAR, bc.ZFAR, grad_out)),
                        ("sigmoid", run_sigmoid(x, bc.SIGMA, grad_out[..., 3])), ("hard", run_hard(x, bc.BG, grad_out))):
            res.update({name + "/" + q: t for q, t in r.items()})
        return res

    a, b = once(), once()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c = once()
    side.synchronize()
    for q in a:
        assert torch.equal(a[q], b[q]) and torch.equal(a[q], c[q]), q


def test_argument_checks_at_the_c_abi():
    """Negative npix / K and a null pointer with K > 0: P3D_ERR_INVALID_ARG, nothing written.  K = 0: the backwards are P3D_OK without
    a launch, the forwards P3D_OK and write alpha 0 respectively the background, hard_rgb_blend (K >= 1) refuses."""
    N, H, W, K = 1, 4, 5, 3
    gen = torch.Generator().manual_seed(1)
    x = bc.inputs(gen, N, 13, W, K, bc.SIGMA, "full")
    c, p2f, d, z = (x[k][:, :H].contiguous().to(DEV) for k in ("colors", "pix_to_face", "dists", "zbuf"))
    g, ga, al = torch.randn(N, H, W, 4, device=DEV), torch.randn(N, H, W, device=DEV), torch.rand(N, H, W, device=DEV)
    P = N * H * W
    out4, out1, gc, gd, gz = _nan(N, H, W, 4), _nan(N, H, W), _nan(N, H, W, K, 3), _nan(N, H, W, K), _nan(N, H, W, K)
    bg = bc.BG
    sm_f = lambda c=c, p2f=p2f, d=d, z=z, N=N, P=H * W, K=K, out=out4: _status(  # noqa: E731
        "p3d_softmax_rgb_blend_forward", c, p2f, d, z, 2e-4, 0.05, bg, 1.0, 10.0, None, None, N, P, K, out)
    sm_b = lambda g=g, c=c, p2f=p2f, d=d, z=z, N=N, P=H * W, K=K, gc=gc, gd=gd, gz=gz: _status(  # noqa: E731
        "p3d_softmax_rgb_blend_backward", g, c, p2f, d, z, 2e-4, 0.05, bg, 1.0, 10.0, None, None, N, P, K, gc, gd, gz)
    sg_f = lambda d=d, p2f=p2f, P=P, K=K, out=out1: _status("p3d_sigmoid_alpha_blend_forward", d, p2f, 2e-4, P, K, out)  # noqa: E731
    sg_b = lambda ga=ga, al=al, d=d, p2f=p2f, P=P, K=K, gd=gd: _status(  # noqa: E731
        "p3d_sigmoid_alpha_blend_backward", ga, al, d, p2f, 2e-4, P, K, gd)
    hd_f = lambda c=c, p2f=p2f, P=P, K=K, out=out4: _status("p3d_hard_rgb_blend_forward", c, p2f, bg, P, K, out)  # noqa: E731
    hd_b = lambda g=g, p2f=p2f, P=P, K=K, gc=gc: _status("p3d_hard_rgb_blend_backward", g, p2f, P, K, gc)  # noqa: E731
    refused = [sm_f(N=-1), sm_f(P=-1), sm_f(K=-1), sm_b(N=-1), sm_b(P=-1), sm_b(K=-1), sg_f(P=-1), sg_f(K=-1), sg_b(P=-1), sg_b(K=-1),
               hd_f(P=-1), hd_f(K=-1), hd_b(P=-1), hd_b(K=-1), hd_f(K=0), hd_b(K=0),
               sm_f(c=None), sm_f(p2f=None), sm_f(d=None), sm_f(z=None), sm_f(out=None),
               sm_b(g=None), sm_b(c=None), sm_b(p2f=None), sm_b(d=None), sm_b(z=None), sm_b(gc=None), sm_b(gd=None), sm_b(gz=None),
               sg_f(d=None), sg_f(p2f=None), sg_f(out=None), sg_b(ga=None), sg_b(al=None), sg_b(d=None), sg_b(p2f=None), sg_b(gd=None),
               hd_f(c=None), hd_f(p2f=None), hd_f(out=None), hd_b(g=None), hd_b(p2f=None), hd_b(gc=None)]
    assert refused == [INVALID] * len(refused), refused
    assert sm_b(K=0) == 0 and sg_b(K=0) == 0
    torch.cuda.synchronize()
    for t in (out4, out1, gc, gd, gz):
        assert bool(torch.isnan(t).all())  # none of the above launched a kernel
    assert sm_f(K=0) == 0 and sg_f(K=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(out4.cpu(), torch.tensor(bg + (0.0,)).expand(N, H, W, 4)) and bool((out1 == 0).all())


# ---- alignment -----------------------------------------------------------------------------------------------------------------
def _offset_view(t):
    """A contiguous view of `t`'s values that starts one element into its storage: 4 or 8 bytes off a 16-byte boundary, and
    .contiguous() returns it as it is."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.storage_offset() == 1 and v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("K", [4, 2])
def test_views_at_a_storage_offset_equal_aligned_copies(K):
    """All five blend operators, forward and backward, with every tensor operand (the incoming gradient included) a contiguous view
    one element into its storage: the wrappers copy such an operand, so the results equal those of aligned tensors bit for bit and
    no misaligned 16-byte access is launched.  K = 4: float and colour rows; K = 2: pix_to_face rows."""
    import pytorch3d_amd as p3d

    N, H, W = bc.SHAPE
    gen = torch.Generator().manual_seed(40 + K)
    x = bc.inputs(gen, N, H, W, K, bc.SIGMA, "holes", zfar=bc.ZFAR)
    grad_out = torch.randn(N, H, W, 4, generator=gen).to(DEV)
    g1 = grad_out[..., :1].contiguous()
    bp = p3d.BlendParams(bc.SIGMA, 0.05, bc.BG)
    zn, zf = _plane(bc.ZNEAR), _plane(bc.ZFAR)

    def ops(wrap):
        p2f = wrap(x["pix_to_face"].to(DEV))
        leaf = lambda k: wrap(x[k].to(DEV)).requires_grad_(True)  # noqa: E731
        res = {}
        c, d, z = leaf("colors"), leaf("dists"), leaf("zbuf")
        img = p3d.softmax_rgb_blend(c, Frag(p2f, z, d), bp, znear=zn, zfar=zf)
        img.backward(wrap(grad_out))
        res.update(softmax=img.detach(), softmax_gc=c.grad, softmax_gd=d.grad, softmax_gz=z.grad)
        c, d = leaf("colors"), leaf("dists")
        img = p3d.sigmoid_alpha_blend(c, Frag(p2f, None, d), bp)
        img.backward(wrap(grad_out))
        res.update(sigmoid=img.detach(), sigmoid_gc=c.grad, sigmoid_gd=d.grad)
        c = leaf("colors")
        img = p3d.hard_rgb_blend(c, Frag(p2f, None, None), bp)
        img.backward(wrap(grad_out))
        res.update(hard=img.detach(), hard_gc=c.grad)
        d, z = leaf("dists"), leaf("zbuf")
        img = p3d.soft_depth_blend(Frag(p2f, z, d), bp, zfar=10.0)
        img.backward(wrap(g1))
        res.update(soft_depth=img.detach(), soft_depth_gd=d.grad, soft_depth_gz=z.grad)
        z = leaf("zbuf")
        img = p3d.hard_depth_blend(Frag(p2f, z, None), zfar=10.0)
        img.backward(wrap(g1))
        res.update(hard_depth=img.detach(), hard_depth_gz=z.grad)
        torch.cuda.synchronize()
        return res

    aligned, offset = ops(lambda t: t.detach().clone()), ops(_offset_view)
    for name, t in aligned.items():
        assert t.data_ptr() % 16 == 0 and torch.equal(t, offset[name]), name


@pytest.mark.parametrize("K", [4, 2])
def test_offset_pointers_are_refused_at_the_c_abi(K):
    """The address of every row base the kernels would move in 16-byte units, and of the RGBA images of the softmax entries, shifted by
    one element: P3D_ERR_INVALID_ARG before any launch (the outputs keep their NaN).  Only the refusal is exercised: no misaligned
    access is made."""
    N, H, W = 1, 3, 5
    gen = torch.Generator().manual_seed(70 + K)
    x = bc.inputs(gen, N, 13, W, K, bc.SIGMA, "full")
    # one element of slack behind every tensor, so that a shifted address would still lie inside its allocation
    room = lambda t: torch.cat([t.reshape(-1), t.reshape(-1)[:1]])  # noqa: E731
    c, p2f, d, z = (room(x[k][:, :H].contiguous().to(DEV)) for k in ("colors", "pix_to_face", "dists", "zbuf"))
    g, ga, al = room(torch.randn(N, H, W, 4, device=DEV)), torch.randn(N * H * W, device=DEV), torch.rand(N * H * W, device=DEV)
    P = N * H * W
    out4, out1, gc, gd, gz = _nan(P * 4 + 1), _nan(P), _nan(P * K * 3 + 1), _nan(P * K + 1), _nan(P * K + 1)
    bg = bc.BG
    A = {"c": c, "p2f": p2f, "d": d, "z": z, "g": g, "out4": out4, "gc": gc, "gd": gd, "gz": gz}

    def shifted(which):
        a = {k: t.data_ptr() for k, t in A.items()}
        for k in a:
            assert a[k] % 16 == 0
        if which is not None:
            a[which] += A[which].element_size()
        return a

    entries = {
        "p3d_softmax_rgb_blend_forward": (lambda a: (a["c"], a["p2f"], a["d"], a["z"], 2e-4, 0.05, bg, 1.0, 10.0, None, None, N, H * W, K, a["out4"]),
                                          ("p2f", "out4") + (("c", "d", "z") if K % 4 == 0 else ())),
        "p3d_softmax_rgb_blend_backward": (lambda a: (a["g"], a["c"], a["p2f"], a["d"], a["z"], 2e-4, 0.05, bg, 1.0, 10.0, None, None, N, H * W, K,
                                                      a["gc"], a["gd"], a["gz"]),
                                           ("p2f", "g") + (("c", "d", "z", "gc", "gd", "gz") if K % 4 == 0 else ())),
        "p3d_sigmoid_alpha_blend_forward": (lambda a: (a["d"], a["p2f"], 2e-4, P, K, out1), ("p2f",) + (("d",) if K % 4 == 0 else ())),
        "p3d_sigmoid_alpha_blend_backward": (lambda a: (ga, al, a["d"], a["p2f"], 2e-4, P, K, a["gd"]),
                                             ("p2f",) + (("d", "gd") if K % 4 == 0 else ())),
        "p3d_hard_rgb_blend_forward": (lambda a: (a["c"], a["p2f"], bg, P, K, a["out4"]), ("out4",)),
    }
    for entry, (args, which) in entries.items():
        for w in which:
            assert _status(entry, *args(shifted(w))) == INVALID, (entry, w)
    torch.cuda.synchronize()
    for t in (out4, out1, gc, gd, gz):
        assert bool(torch.isnan(t).all())
    # and the same addresses unshifted are accepted
    for entry, (args, _) in entries.items():
        assert _status(entry, *args(shifted(None))) == 0, entry
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out4[:P * 4]).any()) and not bool(torch.isnan(gc[:P * K * 3]).any())
