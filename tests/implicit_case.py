"""Cases, inputs and gates of the implicit-rendering tests (tests/test_cpu_implicit.py, tests/test_gpu_implicit.py,
tests/shim_implicit_case.py) and of the generator of their fixture (tests/golden/make_golden_implicit.py -> golden/implicit_ref.npz).

Inputs are redrawn from seeds here; the fixture holds the reference's outputs only:
* sample_pdf: per case the output of the reference's compiled CPU operator.  Gate: bit-equal (NaN equal to NaN), every case.
* raymarching: per case the float64 outputs and autograd gradients of the reference's raymarching.py (the truth), and per quantity
  E_ref: the largest error of the reference's own float32 CPU run against that truth over all cases, relative to the case's largest
  |truth|.  Gate: |got - truth| <= 4 E_ref max|truth| per quantity and case (the project's convention; the factor covers the other
  product and sum order of a parallel scan against the same float32 roundings).  A case the reference's float32 run breaks (a
  non-finite value) is named in the fixture, left out of E_ref and gated like the others against the truth.

The sample_pdf cases hold every B in {1, 3, 257}, n_bins in {1, 2, 63, 64, 65} and S in {1, 5, 64, 129}: the full cross product at
B in {1, 3}, alternating det=True and random uniforms, and at B = 257 every n_bins once with S chosen so that every S occurs (a
fixture of the full product at B = 257 would pass the size limit of a committed file).  The raymarch cases hold every P in
{1, 2, 31, 32, 33, 63, 64, 65, 130} with every s in {1, 2, 5, P, P + 3}, C and the density kinds cycling, on 5 rays (P <= 33: several
rays share a wave) or 1, and further cases for the ray counts 64, 65 and 257, the leading shapes (2, 3, 4) and none, and 1.5.
"""
import functools
import itertools
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "implicit_ref.npz")
SEED = 20240611
QUANTITIES = ("features", "opacities", "weights", "grad_densities", "grad_features")
GATE_FACTOR = 4.0


def _gen(*key):
    return torch.Generator().manual_seed(SEED + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


# ---- sample_pdf -------------------------------------------------------------------------------------------------------------------
PDF_B, PDF_BINS, PDF_S = (1, 3, 257), (1, 2, 63, 64, 65), (1, 5, 64, 129)
SPECIAL_BINS = 9
LONG_BINS = 8192  # the first n_bins of the workspace form: asserted against the library's constants by the tests


def pdf_cases():
    """(id, kind, B, n_bins, S, det, eps)."""
    out = []
    for i, (B, n, S) in enumerate(itertools.product((1, 3), PDF_BINS, PDF_S)):
        out.append(("grid-B%d-n%d-S%d-%s" % (B, n, S, "det" if i % 2 == 0 else "rand"), "grid", B, n, S, i % 2 == 0, 1e-5))
    for n, S, det in ((1, 5, True), (2, 1, False), (63, 129, False), (64, 64, True), (65, 5, False)):
        out.append(("grid-B257-n%d-S%d-%s" % (n, S, "det" if det else "rand"), "grid", 257, n, S, det, 1e-5))
    out.append(("grid-B3-n63-S64-both-det", "grid", 3, 63, 64, True, 1e-5))
    out.append(("grid-B3-n64-S129-both-rand", "grid", 3, 64, 129, False, 1e-5))
    for det in (True, False):
        out.append(("special-%s" % ("det" if det else "rand"), "special", 8, SPECIAL_BINS, 33, det, 1e-5))
    out.append(("dyadic-eps0", "dyadic", 4, 8, 65, True, 0.0))
    out.append(("nan-row", "nan", 3, 5, 9, False, 1e-5))
    out.append(("long-row", "grid", 2, LONG_BINS, 5, False, 1e-5))
    return out


def pdf_inputs(case):
    """bins (B, n_bins + 1), weights (B, n_bins), uniforms (B, S) float32 CPU tensors of a case."""
    cid, kind, B, n, S, det, eps = case
    g = _gen(1, B, n, S, int(det), len(cid))
    bins = torch.cumsum(0.05 + torch.rand((B, n + 1), generator=g), 1) - 1.0
    weights = torch.rand((B, n), generator=g)
    u = torch.linspace(0.0, 1.0, S).expand(B, S).contiguous() if det else torch.rand((B, S), generator=g)
    if kind == "special":
        w = weights
        w[0, :3] = 0.0                      # a run of zeros at the start
        w[1, 3:6] = 0.0                     # in the middle
        w[2, -3:] = 0.0                     # at the end
        w[3, :] = 0.0                       # an all-zero row
        w[4, :] = 0.0
        w[4, 4] = 0.7                       # a single non-zero bin
        w[5, :] = w[5, :] * 1e-6            # every weight below eps
        w[6, ::2] = 3e-6                    # weights below eps between ordinary ones
        w[7, 0], w[7, -1] = 0.0, 0.0        # zeros at both ends
    elif kind == "dyadic":
        # eps = 0, weights and uniforms multiples of 1/64 with a total of 1 or 2: total * u equals partial sums exactly (the tie of lower_bound)
        weights = torch.tensor([[8, 8, 8, 8, 8, 8, 8, 8], [16, 0, 16, 0, 0, 16, 8, 8], [32, 16, 8, 4, 2, 1, 1, 0], [16, 16, 16, 16, 16, 16, 16, 16]],
                               dtype=torch.float32) / 64.0
        u = torch.linspace(0.0, 1.0, S).expand(B, S).contiguous()  # S = 65: multiples of 1/64
    elif kind == "nan":
        weights[1, 2] = float("nan")
        u[2, 4] = float("nan")
        u[1, 0] = float("nan")
    return bins.contiguous(), weights.contiguous(), u.contiguous(), eps


def pdf_numpy(bins, weights, u, eps, upper_bound=False, total_from_eps=False):
    """The operator's contract restated in numpy float32, sample by sample (slow: small cases).  The two switches are the mistakes
    tests/test_cpu_implicit.py holds the gate against: upper_bound in place of lower_bound, a total that starts at eps."""
    f = np.float32
    bins, weights, u = (np.asarray(t, dtype=f) for t in (bins, weights, u))
    B, n = weights.shape
    out = np.empty_like(u)
    eps = f(eps)
    with np.errstate(all="ignore"):
        for r in range(B):
            partial, total = np.empty(n, f), (eps if total_from_eps else f(0.0))
            for i in range(n):
                total = f(total + weights[r, i])
                partial[i] = total
            if not total_from_eps:
                total = f(total + eps)
            for j in range(u.shape[1]):
                v = f(total * u[r, j])
                first, length = 0, n - 1
                while length > 0:
                    half = length >> 1
                    mid = first + half
                    if (not (v < partial[mid])) if upper_bound else (partial[mid] < v):
                        first, length = mid + 1, length - half - 1
                    else:
                        length = half
                i = first
                if i > 0:
                    v = f(v - partial[i - 1])
                lo, hi, w = bins[r, i], bins[r, i + 1], weights[r, i]
                if v > w:
                    out[r, j] = hi
                elif w > eps:
                    out[r, j] = f(lo + f(f(v / w) * f(hi - lo)))
                else:
                    out[r, j] = lo
    return out


def same_bits(a, b):
    return bool(np.array_equal(np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32), equal_nan=True))


# ---- raymarching ------------------------------------------------------------------------------------------------------------------
RAY_P = (1, 2, 31, 32, 33, 63, 64, 65, 130)
KINDS = ("uniform", "zeros", "one1", "one2", "all1")


def _shifts(P):
    return (1, 2, 5, P, P + 3)


def ray_cases():
    """(id, lead shape, P, C, s, density kind, return_weights)."""
    out, i = [], 0
    for pi, P in enumerate(RAY_P):
        for si, s in enumerate(_shifts(P)):
            lead, C, kind = ((5,) if P <= 33 else (1,)), (1, 3, 4, 7)[(pi + si) % 4], KINDS[(2 * pi + si) % 5]
            out.append(("P%d-s%d-C%d-r%d-%s%s" % (P, s, C, lead[0], kind, "-w" if i % 3 == 0 else ""), lead, P, C, s, kind, i % 3 == 0))
            i += 1
    for lead, P, C, s, kind, rw in (((64,), 64, 1, 1, "uniform", True), ((65,), 33, 1, 2, "one1", False), ((257,), 2, 4, 1, "zeros", True),
                                    ((65,), 31, 1, 5, "one2", False), ((64,), 130, 1, 1, "one1", True), ((2, 3, 4), 32, 3, 1, "uniform", True),
                                    ((), 33, 3, 2, "one1", False), ((), 130, 4, 1, "uniform", True), ((5,), 64, 3, 1, "over", False),
                                    ((65,), 65, 1, 1, "all1", False), ((5,), 130, 7, 5, "one2", True)):
        out.append(("x-%s-P%d-s%d-C%d-%s%s" % ("x".join(map(str, lead)) or "none", P, s, C, kind, "-w" if rw else ""), lead, P, C, s, kind, rw))
    return out


def ray_inputs(case):
    """float32 CPU tensors: densities lead + (P, 1), features lead + (P, C), grad_out lead + (C + 1,) (not ones), grad_weights lead +
    (P,) or None; eps."""
    cid, lead, P, C, s, kind, rw = case
    g = _gen(2, P, C, s, KINDS.index(kind) if kind in KINDS else 9, int(rw), len(lead), sum(lead), len(cid))
    d = 0.02 + 0.9 * torch.rand(lead + (P,), generator=g)
    # (a third of the points opaque and the rest near 0, as on a NeRF ray: the transmission of 130 points stays far from underflow)
    d = d * (torch.rand(lead + (P,), generator=g) < 0.3) * 1.0 + 0.05 * d
    flat = d.reshape(-1, P)
    pick = torch.randint(0, P, (flat.shape[0], 2), generator=g)
    if P >= 2:
        pick[:, 1] = (pick[:, 0] + 1 + torch.randint(0, P - 1, (flat.shape[0],), generator=g)) % P  # a second, different point
    rows = torch.arange(flat.shape[0])
    if kind == "zeros":
        flat[rows, pick[:, 0]] = 0.0
        flat[rows, pick[:, 1]] = 0.0
        flat[:, 0] = 0.0
    elif kind == "one1":
        flat[rows, pick[:, 0]] = 1.0
    elif kind == "one2":
        flat[rows, pick[:, 0]] = 1.0
        flat[rows, pick[:, 1]] = 1.0
    elif kind == "all1":
        flat[:] = 1.0
    elif kind == "over":
        flat[rows, pick[:, 0]] = 1.5
    d = flat.reshape(lead + (P, 1)).contiguous()
    f = torch.randn(lead + (P, C), generator=g)
    g_out = torch.randn(lead + (C + 1,), generator=g)
    g_w = torch.randn(lead + (P,), generator=g) if rw else None
    return d, f, g_out, g_w, 1e-10


def run_ray(fn, case, device="cpu", dtype=torch.float32):
    """The five quantities of `fn(densities, features, eps, s, return_weights)` on a case as float64 numpy arrays (weights: None
    unless the case returns them).  fn returns out, or (out, weights)."""
    cid, lead, P, C, s, kind, rw = case
    d, f, g_out, g_w, eps = ray_inputs(case)
    d = d.to(device=device, dtype=dtype).requires_grad_(True)
    f = f.to(device=device, dtype=dtype).requires_grad_(True)
    res = fn(d, f, eps, s, rw)
    out, w = res if rw else (res, None)
    loss = (out * g_out.to(out)).sum()
    if rw:
        loss = loss + (w * g_w.to(w)).sum()
    gd, gf = torch.autograd.grad(loss, (d, f))
    np64 = lambda t: None if t is None else t.detach().double().cpu().numpy()
    return {"features": np64(out[..., :C]), "opacities": np64(out[..., C:]), "weights": np64(w), "grad_densities": np64(gd), "grad_features": np64(gf)}


def key(cid, name):
    return "%s/%s" % (cid, name)


@functools.lru_cache(maxsize=1)
def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def e_ref(quantity):
    return float(fixture()["E_ref/" + quantity])


def ray_errors(case, got):
    """{quantity: (error, gate)} of run_ray's result against the fixture's truth; error = max |got - truth| (inf where got is not
    finite), gate = 4 E_ref max |truth|."""
    fix, out = fixture(), {}
    for q in QUANTITIES:
        if got[q] is None:
            continue
        truth = fix[key(case[0], q)]
        assert truth.shape == got[q].shape, (case[0], q, truth.shape, got[q].shape)
        err = float(np.abs(got[q] - truth).max()) if np.isfinite(got[q]).all() else float("inf")
        out[q] = (err, GATE_FACTOR * e_ref(q) * float(np.abs(truth).max()))
    return out


def ray_failures(cases, fn, device="cpu", dtype=torch.float32, verbose=False):
    """[(case id, quantity, error, gate)] of everything beyond its gate."""
    bad = []
    for case in cases:
        for q, (err, gate) in ray_errors(case, run_ray(fn, case, device, dtype)).items():
            if verbose:
                print("%-40s %-15s error %.3e gate %.3e" % (case[0], q, err, gate))
            if not err <= gate:
                bad.append((case[0], q, err, gate))
    return bad
