"""Inputs, references and the gate of the RGB blend kernels (csrc/blend.hip: sigmoid_alpha_blend, softmax_rgb_blend, hard_rgb_blend);
the yardstick of tests/test_gpu_blend_edges.py.  tests/test_cpu_blend_case.py ties it to the reference's recorded results and shows,
without a GPU, that the gate is feasible for the kernels' own order of operations and rejects four structural mutants of it.

References, every one in torch on the CPU:

    chain(..., dtype)          softmax_rgb_blend as the reference states it (renderer/blending.py:147-244), gradients by torch autograd;
                               float64 is the yardstick, float32 the reference chain's own arithmetic
    sigmoid_chain(..., dtype)  sigmoid_alpha_blend as the reference's kernel states it (sigmoid_alpha_blend.cu:57-66) with its closed-form
                               backward (:146-160); the float32 flavour keeps the doubles its literals promote to, like sig_prob in blend.hip
    hard_chain(...)            hard_rgb_blend (blending.py:54-88): copies, compared with torch.equal
    kernel_order(...)          float32, the arithmetic of softmax_blend_fwd_kernel / _bwd_kernel and of softmax_blend_generic in their own
                               order: sequential slot sums, inv_denom, prefix / suffix products, the explicit backward formulas

Gate.  For every quantity (out, grad_colors, grad_dists, grad_zbuf) and every pixel class, over all elements of the class:

    max |got - chain64|  <=  max(MARGIN * max |chain32 - chain64|, ulp32(max |chain64|))

and `got` is finite wherever chain64 is.  Every pixel belongs to exactly one class; a class whose float64 figures are not finite fails.
"""
import torch

import depth_restatement as dr
from box3d_case import MARGIN
from mesh_refine_case import ulp32

EPS = 1e-10
CLASSES = ("general", "tie", "beyond", "saturated", "empty")
QUANTITIES = ("out", "grad_colors", "grad_dists", "grad_zbuf")
MUTANTS = ("planes_of_image_0", "no_delta_in_G_zmax", "others_by_division", "last_slot_left_out")

# the cases of tests/test_gpu_blend_edges.py::test_every_capacity
CAPACITIES = (1, 2, 3, 4, 5, 7, 8, 9, 16, 31, 32, 33, 64, 150)
PATTERNS = ("prefix", "holes", "full")
GAMMAS = (0.05, 0.5)
SHAPE = (3, 13, 11)
SIGMA = 2e-4
ZNEAR = (1.0, 0.5, 2.0)
ZFAR = (10.0, 8.0, 12.0)
BG = (0.2, 0.4, 0.6)
# A pixel keeps at most LIVE_SLOTS slots near an edge, at positions drawn per pixel among its K; its other valid slots lie 20 to 40
# sigma outside their face (p <= 2e-9: valid, walked by every loop, without weight), so every slot index is live in some pixel.
# Why: the kernels add a pixel's slots one after the other and round once per live slot, torch's blocked sum in chain(float32)
# rounds about 1.5 ulp whatever K is, so err / bound grows with the live slots.  kernel_order, all cells of test_every_capacity,
# largest err / bound over 18 seeds and torch's three CPU code paths (ATEN_CPU_CAPABILITY=default, avx2, avx512 -- the bound is
# chain(float32)'s own error and moves with the CPU's summation order): 150 live slots 1.1 to 1.5 on `out` and grad_zbuf (not
# feasible); 32 live 0.79 to 1.40; 16 live 0.70 to 1.01; 8 live no better (a class is one row of 33 pixels per image, and the
# largest of 99 errors against 4 x the largest of 99 others keeps such a tail).  So the seed is part of the input: SEED is one
# where kernel_order stays below 0.75 of every bound on all three code paths.  Case (K, pattern) draws from SEED + 10 K + index
# of the pattern.
SEED = 800
LIVE_SLOTS = 16


def _per_image(v, N):
    """znear / zfar as N Python floats"""
    if torch.is_tensor(v):
        v = v.reshape(-1).tolist()
    elif not isinstance(v, (tuple, list)):
        v = [float(v)]
    v = [float(x) for x in v]
    return v * N if len(v) == 1 else v


def class_rows(H, classes):
    """{class: rows of the image it takes}: special class j takes the rows r with r % (2 m + 5) == 2 j + 1, m special classes --
    one row each at H = 13, every 13th row of a taller image; `general` keeps the rest."""
    special = [c for c in classes if c != "general"]
    stride = 2 * len(special) + 5
    rows = {c: [r for r in range(H) if r % stride == 2 * j + 1] for j, c in enumerate(special)}
    for c, r in rows.items():
        assert r, f"an image of {H} rows has no row for class `{c}`"
    return rows


def _thin(gen, d, sigma):
    """dists (..., K) with all but LIVE_SLOTS slots of every pixel, at positions drawn per pixel, moved 20 to 40 sigma outside"""
    K = d.shape[-1]
    if K <= LIVE_SLOTS:
        return d
    rank = torch.argsort(torch.rand(d.shape, generator=gen), dim=-1)
    far = (torch.rand(d.shape, generator=gen) * 20.0 + 20.0) * sigma
    return torch.where(rank < LIVE_SLOTS, d, far)


def inputs(gen, N, H, W, K, sigma, pattern="prefix", zfar=100.0, classes=CLASSES):
    """Seeded fragments on the CPU: {colors (N,H,W,K,3) f32, pix_to_face i64, zbuf f32, dists f32 (N,H,W,K), classes (N,H,W) i64 holding
    indices into CLASSES}.  depth_restatement.depth_inputs draws the image in `pattern`; then whole pixel rows (class_rows) are
    overwritten, the same rows in every image, so that each class of `classes` covers at least one image row of every image:

      tie        every slot valid, zbuf ascending, slot 1 equal to slot 0 (needs K >= 2)
      beyond     every slot valid, every depth greater than that image's zfar
      saturated  every slot valid, slot 0 at dists = +200 sigma (expf overflows, p = 0), slot 1 and, with K >= 3, slot 2 at -200 sigma
                 (p = 1 exactly: one respectively two zero factors in the products of 1 - p)
      empty      no face: -1 in pix_to_face, zbuf and dists, as the rasterizer leaves empty slots

    Their other dists are uniform in (-3 sigma, 6 sigma).  Above K = LIVE_SLOTS every pixel of every class is thinned (_thin).  zfar: one number or one per image."""
    classes = tuple(c for c in classes if not (c == "tie" and K < 2))
    p2f, z, d = dr.depth_inputs(gen, N, H, W, K, sigma, pattern)
    d = torch.where(p2f >= 0, _thin(gen, d, sigma), d)
    colors = torch.rand(N, H, W, K, 3, generator=gen)
    far = torch.tensor(_per_image(zfar, N)).view(N, 1, 1)
    cmap = torch.zeros(N, H, W, dtype=torch.int64)
    for name, rows in class_rows(H, classes).items():
        R = len(rows)
        face = torch.randint(0, 50, (N, R, W, K), generator=gen)
        zz = torch.sort(torch.rand(N, R, W, K, generator=gen) * 3.0 + 0.8, dim=-1).values
        dd = (torch.rand(N, R, W, K, generator=gen) * 9.0 - 3.0) * sigma
        dd = _thin(gen, dd, sigma)
        if name == "tie":
            zz[..., 1] = zz[..., 0]
        elif name == "beyond":
            zz = zz - 0.3 + far.unsqueeze(-1)  # 0.5 .. 3.5 behind the far plane
        elif name == "saturated":
            dd[..., 0] = 200.0 * sigma
            dd[..., 1:3] = -200.0 * sigma
        elif name == "empty":
            face.fill_(-1)
            zz.fill_(-1.0)
            dd.fill_(-1.0)
        p2f[:, rows], z[:, rows], d[:, rows] = face, zz, dd
        cmap[:, rows] = CLASSES.index(name)
    return {"colors": colors, "pix_to_face": p2f.contiguous(), "zbuf": z.contiguous(), "dists": d.contiguous(), "classes": cmap}


# ---- softmax_rgb_blend ----------------------------------------------------------------------------------------------------------
def chain(colors, p2f, dists, zbuf, sigma, gamma, bg, znear, zfar, dtype, grad_out=None):
    """blending.py:147-244 in `dtype` -> {out (N,H,W,4)} and, with grad_out, {grad_colors, grad_dists, grad_zbuf} by torch autograd.
    znear / zfar: a number, or a tensor / sequence with one entry per image."""
    c, d, z = (t.detach().to(dtype).clone().requires_grad_(grad_out is not None) for t in (colors, dists, zbuf))

    def plane(v):
        if torch.is_tensor(v) or isinstance(v, (tuple, list)):
            return torch.as_tensor(v, dtype=torch.float32).to(dtype).reshape(-1)[:, None, None, None]
        return float(v)

    zf, zn = plane(zfar), plane(znear)
    background = torch.tensor([float(x) for x in bg], dtype=torch.float32).to(dtype)
    mask = p2f >= 0
    prob_map = torch.sigmoid(-d / sigma) * mask
    alpha = torch.prod(1.0 - prob_map, dim=-1)
    z_inv = (zf - z) / (zf - zn) * mask
    z_inv_max = torch.max(z_inv, dim=-1).values[..., None].clamp(min=EPS)
    weights_num = prob_map * torch.exp((z_inv - z_inv_max) / gamma)
    delta = torch.exp((EPS - z_inv_max) / gamma).clamp(min=EPS)
    denom = weights_num.sum(dim=-1)[..., None] + delta
    weighted_colors = (weights_num[..., None] * c).sum(dim=-2)
    rgb = (weighted_colors + delta * background) / denom
    out = torch.cat([rgb, (1.0 - alpha)[..., None]], dim=-1)
    res = {"out": out.detach()}
    if grad_out is not None:
        out.backward(grad_out.to(dtype))
        res.update(grad_colors=c.grad, grad_dists=d.grad, grad_zbuf=z.grad)
    return res


def kernel_order(colors, p2f, dists, zbuf, sigma, gamma, bg, znear, zfar, grad_out, mutant=None):
    """float32: what csrc/blend.hip evaluates per pixel, in its order -- the register kernels for K <= 32, softmax_blend_generic above.
    (Not bit for bit: the device contracts a * b + c and has its own expf.)  -> the four QUANTITIES.
    mutant: one of MUTANTS, a structural error planted into that arithmetic."""
    assert mutant is None or mutant in MUTANTS
    f = torch.float32
    N, H, W, K = p2f.shape
    P = N * H * W
    generic = K > 32
    t = lambda v: torch.tensor(v, dtype=f)  # noqa: E731
    sig, gam, eps = t(sigma), t(gamma), t(EPS)
    bgt = torch.tensor([float(x) for x in bg], dtype=f)
    zn, zf = (torch.tensor(_per_image(v, N), dtype=f) for v in (znear, zfar))
    if mutant == "planes_of_image_0":
        zn, zf = zn[:1].expand(N), zf[:1].expand(N)
    zn, zf = (v.repeat_interleave(H * W) for v in (zn, zf))
    c, d, z, g = colors.reshape(P, K, 3).to(f), dists.reshape(P, K).to(f), zbuf.reshape(P, K).to(f), grad_out.reshape(P, 4).to(f)
    valid = p2f.reshape(P, K) >= 0
    Ks = K - 1 if mutant == "last_slot_left_out" else K  # slots taken into the slot sums

    m = valid.to(f)
    s = 1.0 / (1.0 + torch.exp(d / sig))
    p = s * m
    zi = (zf[:, None] - z) / (zf - zn)[:, None] * m
    zraw = torch.full((P,), float("-inf"), dtype=f)
    kstar = torch.zeros(P, dtype=torch.int64)
    for k in range(K):
        up = zi[:, k] > zraw
        zraw = torch.where(up, zi[:, k], zraw)
        kstar = torch.where(up, torch.full_like(kstar, k), kstar)
    z_clamped = zraw < eps
    zmax = torch.where(z_clamped, eps, zraw)
    delta = torch.exp((eps - zmax) / gam)
    d_clamped = delta < eps
    delta = torch.where(d_clamped, eps, delta)
    e = torch.exp((zi - zmax[:, None]) / gam)
    w = p * e
    denom = torch.zeros(P, dtype=f)
    for k in range(Ks):
        denom = denom + w[:, k]
    denom = denom + delta

    # forward
    alpha = torch.ones(P, dtype=f)
    r = torch.zeros(P, 3, dtype=f)
    for k in range(K):
        alpha = alpha * (1.0 - p[:, k])
        if k < Ks:
            r = r + w[:, k, None] * c[:, k]
    rgb = (r + delta[:, None] * bgt) / denom[:, None]
    out = torch.cat([rgb, (1.0 - alpha)[:, None]], dim=1)

    # backward
    inv_denom = 1.0 / denom
    if generic:
        rb = rgb
    else:
        rb = delta[:, None] * bgt
        for k in range(Ks):
            rb = rb + w[:, k, None] * c[:, k]
        rb = rb * inv_denom[:, None]

    def dot3(x):  # g.x * x0 + g.y * x1 + g.z * x2, left to right
        return g[:, 0] * x[:, 0] + g[:, 1] * x[:, 1] + g[:, 2] * x[:, 2]

    G_delta = dot3(bgt - rb) * inv_denom
    G_zmax = torch.where(d_clamped, torch.zeros(P, dtype=f), G_delta * (-delta / gam))
    if mutant == "no_delta_in_G_zmax":
        G_zmax = torch.zeros(P, dtype=f)
    Gw = torch.stack([dot3(c[:, k] - rb) * inv_denom for k in range(K)], dim=1)
    for k in range(Ks):
        G_zmax = G_zmax + Gw[:, k] * (-w[:, k] / gam)
    if generic:
        gc = g[:, None, :3] * w[:, :, None] * inv_denom[:, None, None]
    else:
        gc = g[:, None, :3] * (w * inv_denom[:, None])[:, :, None]
    one_minus = 1.0 - p
    if mutant == "others_by_division":
        others = alpha[:, None] / one_minus
    elif generic:
        others = torch.ones(P, K, dtype=f)
        not_self = ~torch.eye(K, dtype=torch.bool)
        for j in range(K):
            others = others * torch.where(not_self[j][None, :], one_minus[:, j, None], torch.ones((), dtype=f))
    else:
        pre = torch.ones(P, K, dtype=f)
        run = torch.ones(P, dtype=f)
        for k in range(K):
            pre[:, k] = run
            run = run * one_minus[:, k]
        others = torch.empty(P, K, dtype=f)
        run = torch.ones(P, dtype=f)
        for k in range(K - 1, -1, -1):
            others[:, k] = pre[:, k] * run
            run = run * one_minus[:, k]
    G_zi = Gw * w / gam
    at_max = (torch.arange(K)[None, :] == kstar[:, None]) & ~z_clamped[:, None]
    G_zi = torch.where(at_max, G_zi + G_zmax[:, None], G_zi)
    if generic:
        gz = G_zi * (-m / (zf - zn)[:, None])
    else:
        gz = G_zi * (-m * (1.0 / (zf - zn))[:, None])
    G_p = Gw * e + g[:, 3, None] * others
    gd = G_p * (-(1.0 / sig) * s * (1.0 - s) * m)

    if not generic:  # the early exit of the register kernels: a pixel without a face, unless the planes coincide
        leave = ~valid.any(-1) & (zf != zn)
        out = torch.where(leave[:, None], torch.cat([bgt, torch.zeros(1, dtype=f)])[None, :], out)
        zero = torch.zeros((), dtype=f)
        gc = torch.where(leave[:, None, None], zero, gc)
        gd = torch.where(leave[:, None], zero, gd)
        gz = torch.where(leave[:, None], zero, gz)
    return {"out": out.view(N, H, W, 4), "grad_colors": gc.view(N, H, W, K, 3), "grad_dists": gd.view(N, H, W, K),
            "grad_zbuf": gz.view(N, H, W, K)}


# ---- sigmoid_alpha_blend ---------------------------------------------------------------------------------------------------------
def _sig_prob(dists, sigma, dtype):
    """sigmoid_alpha_blend.cu:55-58.  float32: dist and exp(-dist / sigma) are floats, `1. / (1. + x)` a double rounded to float."""
    dist = -1.0 * dists.to(dtype)
    x = torch.exp(-dist / sigma)
    return (1.0 / (1.0 + x.double())).to(dtype)


def sigmoid_chain(p2f, dists, sigma, dtype, grad_alphas=None):
    """-> {out: alphas (N,H,W)} and, with grad_alphas, {grad_dists (N,H,W,K)} by the reference's closed form from its own alphas."""
    K = p2f.shape[3]
    valid = p2f >= 0
    prob = _sig_prob(dists, sigma, dtype)
    alpha = torch.ones(p2f.shape[:3], dtype=dtype)
    for k in range(K):  # alpha *= (1.0 - prob): a double product rounded to scalar_t, slot by slot, skipped for empty slots
        alpha = torch.where(valid[..., k], (alpha.double() * (1.0 - prob[..., k].double())).to(dtype), alpha)
    alphas = (1.0 - alpha.double()).to(dtype)
    res = {"out": alphas}
    if grad_alphas is not None:
        back = (1.0 - alphas.double()).to(dtype)  # const scalar_t alpha = 1.0 - alphas[n][yi][xi]
        g = grad_alphas.to(dtype).double()[..., None] * (-1.0 / float(sigma)) * prob.double() * back.double()[..., None]
        res["grad_dists"] = torch.where(valid, g.to(dtype), torch.zeros((), dtype=dtype))
    return res


# ---- hard_rgb_blend --------------------------------------------------------------------------------------------------------------
def hard_chain(colors, p2f, bg, grad_out=None):
    """blending.py:54-88 -> {out (N,H,W,4)} and, with grad_out, {grad_colors (N,H,W,K,3)}: copies only."""
    hit = p2f[..., 0] >= 0
    background = torch.tensor([float(x) for x in bg], dtype=colors.dtype)
    rgb = torch.where(hit[..., None], colors[..., 0, :], background)
    res = {"out": torch.cat([rgb, hit.to(colors.dtype)[..., None]], dim=-1)}
    if grad_out is not None:
        gc = torch.zeros_like(colors)
        gc[..., 0, :] = torch.where(hit[..., None], grad_out[..., :3], torch.zeros((), dtype=grad_out.dtype))
        res["grad_colors"] = gc
    return res


# ---- the gates -------------------------------------------------------------------------------------------------------------------
def gate(got, chain32, chain64, classes, show=print, label=""):
    """The list of (quantity, class, err, bound) that `got` misses: empty when it passes.  got / chain32 / chain64: {quantity: tensor},
    every quantity of chain64 is judged; classes: (N,H,W) indices into CLASSES.  One line per (quantity, class) goes to `show`."""
    assert int(classes.min()) >= 0 and int(classes.max()) < len(CLASSES)
    failures = []
    for q, w64 in chain64.items():
        a_all, b_all, w_all = got[q].detach().cpu().double(), chain32[q].detach().double(), w64.detach().double()
        assert a_all.shape == w_all.shape == b_all.shape, (q, a_all.shape, b_all.shape, w_all.shape)
        judged = 0
        for ci, cname in enumerate(CLASSES):
            sel = classes == ci
            if not bool(sel.any()):
                continue
            a, b, w = a_all[sel], b_all[sel], w_all[sel]
            judged += a.numel()
            if not bool(torch.isfinite(w).all()):
                failures.append((q, cname, float("nan"), float("nan")))
                show(f"{label} {q:11s} {cname:9s} the float64 chain is not finite: FAIL")
                continue
            own = (b - w).abs()
            own = own[torch.isfinite(own)]
            bound = max(MARGIN * (float(own.max()) if own.numel() else 0.0), ulp32(w.abs().max()))
            finite = bool(torch.isfinite(a).all())
            err = float((a - w).abs().max()) if finite else float("inf")
            ok = finite and err <= bound
            show(f"{label} {q:11s} {cname:9s} err {err:.3e} bound {bound:.3e}{'' if ok else ' FAIL'}")
            if not ok:
                failures.append((q, cname, err, bound))
        assert judged == a_all.numel(), (q, judged, a_all.numel())  # no element is left out of every class
    return failures


def old_gate(got, reference):
    """The gate these kernels had before: tests/test_gpu_blending.py's allclose(atol=1e-4 max(1, |ref|.max()), rtol=1e-3) on gradients
    (depth_restatement.grad_close) and atol = 1e-5 on the image, each over the whole tensor.  -> accepted?"""
    ok = True
    for q, r in reference.items():
        a = got[q].detach().cpu()
        ok &= torch.allclose(a, r.to(a.dtype), atol=1e-5, rtol=1e-5) if q == "out" else dr.grad_close(a, r)
    return bool(ok)
