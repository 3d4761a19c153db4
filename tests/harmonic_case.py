"""Cases, seeded inputs and gates for HarmonicEmbedding and the stratified ray depths (csrc/harmonic.hip), shared by
tests/golden/make_golden_harmonic.py (which records the reference), tests/test_cpu_harmonic.py and tests/test_gpu_harmonic.py.

The fixture tests/golden/harmonic_ref.npz holds outputs only; the inputs are redrawn here from seeds.  Every gate is measured
against the reference, never against the code under test:

* gate 1, the argument-exact gate (forward): the test forms a_s = fl(fl(x f) + c_s) in numpy float32 exactly as the contract
  (csrc/implicit_abi.h) and takes sin in float64 -- a truth without any argument rounding, so any other way of forming the argument
  shows.  E_sin is the largest error of the reference's own float32 CPU output against it over all cases; with diag_cov the same
  construction with the float32 exponent and exp in float64 is pooled as E_exp.  |got - truth| <= 4 max(E, E_device), E_device the
  same error of the torch chain on the device the test runs on (0 on the CPU).
* gate 2, the truth gate (forward and both gradients): the reference module in float64 with float64 autograd, recorded per case;
  E_ref[pool, quantity] is the largest error of the reference's float32 CPU run relative to the case's max |truth|, pooled over the
  cases of one argument class (small, octaves, scene, large, dyadic) crossed with logspace.  |got - truth| <= 4 E_ref max |truth|.
The 4 is the project's standing factor (implicit_case.py, volume_sampler_case.py).  Slots that are not finite in the truth (the
special-values case) are compared as positions and left out of every pool.
"""
import collections
import math
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "harmonic_ref.npz")
SEED = 20261021
GATE_FACTOR = 4.0
QUANTITIES = ("out", "grad_x", "grad_cov")
HALF_PI32 = np.float32(0.5 * math.pi)

Case = collections.namedtuple("Case", "id cls lead dim n append logspace omega cov freqs layout special")
_RANGE = {"small": 1.0, "octaves": 1.0, "scene": 4.0, "large": 1000.0, "dyadic": 4.0}
HAND_FREQUENCIES = (3.0, 0.25, 17.5, 1.0, 0.7, 40.0)  # non-monotone, not powers of two


def _case(cid, cls, lead, dim, n, append=True, logspace=True, omega=1.0, cov=None, freqs="module", layout="contiguous", special=False):
    return Case(cid, cls, tuple(lead), dim, n, append, logspace, omega, cov, freqs, layout, special)


def backward_tile_rows(W, consts):
    """Rows of one backward tile at the width W, by the header's constants (consts: pytorch3d_amd._lib)."""
    return min(consts.HARMONIC_BWD_ROWS, consts.HARMONIC_BWD_LDS_FLOATS // (W | 1))


def cases():
    out = []
    # rows around the forward's tile and the backward's tile at narrow rows (both 64: test_cpu_harmonic.py asserts it from the header)
    # (0 rows: the reference's own reshape(..., -1) refuses an empty input, so there is nothing to record; the tests check the shapes)
    for rows in (1, 2, 63, 64, 65, 257):
        out.append(_case(f"rows{rows}", "small", (rows,), 1, 1))
    # dim x n, both append settings
    for dim, n, rows, append in ((1, 4, 5, False), (2, 6, 5, True), (3, 10, 5, True), (4, 6, 3, False), (3, 6, 65, True), (3, 4, 7, True)):
        out.append(_case(f"small-d{dim}-n{n}-r{rows}-a{int(append)}", "small", (rows,), dim, n, append))
    # octaves: x in [-1, 1] with n = 16 and 33, whose arguments reach 2^15 and 2^32 -- a class of its own, or the float32 error of the
    # reference at these arguments (the sine of a number whose ulp is 512) would be the gate of every n = 4 case in [-1, 1] too.
    # W = 4 * 67 = 268 at 31 rows is one row above the backward's LDS-limited tile of 30
    for logspace in (True, False):
        for dim, n, rows, append in ((4, 16, 3, False), (4, 33, 31 if logspace else 2, True), (2, 33, 3, False), (1, 16, 5, True), (3, 33, 2, True),
                                     (2, 16, 4, False)):
            out.append(_case(f"octaves-{'log' if logspace else 'lin'}-d{dim}-n{n}-r{rows}-a{int(append)}", "octaves", (rows,), dim, n, append, logspace))
    # leading shapes and layouts
    out.append(_case("lead-none", "small", (), 3, 6))
    out.append(_case("lead-2-3-7", "small", (2, 3, 7), 2, 1))
    out.append(_case("transposed", "small", (9,), 3, 6, layout="transposed"))
    out.append(_case("slice", "small", (2, 5), 3, 4, layout="slice"))
    # omega_0 and linspace, the hand-made frequencies (pooled with the linear ones: neither is a power of two)
    for omega, name in ((0.1, "0.1"), (math.pi, "pi")):
        out.append(_case(f"small-omega{name}", "small", (5,), 3, 6, omega=omega))
        out.append(_case(f"small-lin-omega{name}", "small", (5,), 3, 6, logspace=False, omega=omega))
    for dim, n, append in ((1, 4, True), (2, 10, False), (3, 6, True), (4, 4, True)):
        out.append(_case(f"small-lin-d{dim}-n{n}-a{int(append)}", "small", (4,), dim, n, append, logspace=False))
    out.append(_case("hand", "small", (6,), 3, len(HAND_FREQUENCIES), logspace=False, freqs="hand"))
    out.append(_case("hand-cov", "small", (6,), 2, len(HAND_FREQUENCIES), logspace=False, freqs="hand", cov="cov"))
    # diag_cov in [0, 1e-2]; at n = 10 the top octaves' factors underflow to 0 (the generator asserts it)
    out.append(_case("cov-d3-n4", "small", (7,), 3, 4, cov="cov"))
    out.append(_case("cov-d2-n6-noappend", "small", (5,), 2, 6, False, cov="cov"))
    out.append(_case("cov-underflow", "small", (5,), 3, 10, cov="top"))
    out.append(_case("cov-lin", "small", (5,), 3, 6, logspace=False, cov="cov"))
    # scene: [-4, 4] with n = 10
    for i, (dim, rows, append, logspace, omega, cov) in enumerate((
            (3, 5, True, True, 1.0, None), (3, 2, False, True, 1.0, None), (1, 9, True, True, 0.1, None), (2, 5, True, True, math.pi, None),
            (4, 3, True, True, 1.0, None), (3, 4, True, True, 1.0, "cov"),
            (3, 5, True, False, 1.0, None), (3, 2, False, False, 1.0, None), (1, 9, True, False, 0.1, None), (2, 5, True, False, math.pi, None),
            (4, 3, True, False, 1.0, None), (3, 4, True, False, 1.0, "cov"))):
        out.append(_case(f"scene{i}", "scene", (rows,), dim, 10, append, logspace, omega, cov))
    # large: [-1000, 1000], where sinf's range reduction works
    for i, (dim, n, rows, append, logspace, omega) in enumerate((
            (3, 10, 5, True, True, 1.0), (1, 4, 9, False, True, 1.0), (2, 6, 5, True, True, math.pi), (4, 16, 2, True, True, 0.1),
            (3, 1, 7, True, True, 1.0), (3, 6, 3, False, True, 1.0),
            (3, 10, 5, True, False, 1.0), (1, 4, 9, False, False, 1.0), (2, 6, 5, True, False, math.pi), (4, 16, 2, True, False, 0.1),
            (3, 2, 7, True, False, 1.0), (3, 6, 3, False, False, 1.0))):
        out.append(_case(f"large{i}", "large", (rows,), dim, n, append, logspace, omega))
    # dyadic: multiples of 2^-6 with logspace and omega_0 = 1, every t exact
    for i, (dim, n, rows, append) in enumerate(((3, 10, 5, True), (1, 4, 9, False), (2, 6, 5, True), (4, 16, 2, True), (3, 1, 7, True), (3, 6, 3, False))):
        out.append(_case(f"dyadic{i}", "dyadic", (rows,), dim, n, append))
    # x = 0, -0.0, +-inf, NaN and a denormal in one row (dim = 6), an ordinary row next to it
    out.append(_case("special", "small", (2,), 6, 4, special=True))
    assert len({c.id for c in out}) == len(out)
    return out


def pool(case):
    return case.cls + ("-log" if case.logspace else "-lin")


def case_by_id(cid):
    return next(c for c in cases() if c.id == cid)


def width(case):
    return case.dim * (2 * case.n + int(case.append))


def frequencies(case):
    """The module's _frequencies buffer as the reference's constructor makes it, or the hand-made tensor."""
    if case.freqs == "hand":
        return torch.tensor(HAND_FREQUENCIES, dtype=torch.float32)
    if case.logspace:
        f = 2.0 ** torch.arange(case.n, dtype=torch.float32)
    else:
        f = torch.linspace(1.0, 2.0 ** (case.n - 1), case.n, dtype=torch.float32)
    return f * case.omega


def inputs(case, device="cpu", dtype=torch.float32):
    """(x, diag_cov or None, frequencies, grad into the output), drawn in float32 on the CPU from a seed by the case's position, then
    cast and moved; the layout of x (a transposed view, a channel slice) is made on the device."""
    g = torch.Generator().manual_seed(SEED + 131 * [c.id for c in cases()].index(case.id))
    shape = case.lead + (case.dim,)
    if case.cls == "dyadic":
        x = torch.randint(-256, 257, shape, generator=g).to(torch.float32) / 64.0
    else:
        x = (2.0 * torch.rand(shape, generator=g) - 1.0) * _RANGE[case.cls]
    if case.special:
        x[0] = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e-40])
    big = torch.rand(case.lead + (case.dim + 2,), generator=g) if case.layout == "slice" else None
    x = x.to(device=device, dtype=dtype)
    if case.layout == "transposed":
        x = x.t().contiguous().t()  # (rows, dim) with strides (1, rows)
        assert len(case.lead) == 1 and not x.is_contiguous()
    elif case.layout == "slice":
        big = big.to(device=device, dtype=dtype)
        big[..., 1:1 + case.dim] = x
        x = big[..., 1:1 + case.dim]
        assert not x.is_contiguous()
    cov = None
    if case.cov == "cov":
        cov = 1e-2 * torch.rand(shape, generator=g)
    elif case.cov == "top":
        cov = torch.full(shape, 1e-2)
    grad = torch.randn(case.lead + (width(case),), generator=g)
    move = lambda t: None if t is None else t.to(device=device, dtype=dtype)  # noqa: E731
    return x, move(cov), move(frequencies(case)), move(grad)


def run(fn, case, dtype=torch.float32, device="cpu", need=(True, True), inp=None):
    """fn(x, frequencies, diag_cov, append_input) on the case's inputs and the seeded gradient into its output: {quantity: float64
    numpy array or None} (grad_cov: None without diag_cov or where not needed)."""
    x, cov, f, g = inp if inp is not None else inputs(case, device, dtype)
    x = x.detach().requires_grad_(need[0])  # (detach keeps the strides)
    cov = None if cov is None else cov.detach().requires_grad_(need[1])
    out = fn(x, f, cov, case.append)
    leaves = [t for t in (x, cov) if t is not None and t.requires_grad]
    grads = iter(torch.autograd.grad(out, leaves, g) if leaves and out.numel() else [torch.zeros_like(t) for t in leaves])

    def np64(t):
        return None if t is None else t.detach().double().cpu().numpy()

    return {"out": np64(out), "grad_x": np64(next(grads) if need[0] else None),
            "grad_cov": np64(next(grads) if cov is not None and need[1] else None)}


def argument_truth(case, inp=None):
    """Gate 1's truth: sin in float64 of the float32 argument a_s = fl(fl(x f) + c_s), times exp in float64 of the float32 exponent
    fl(-0.5 fl(cov fl(f f))) with diag_cov; the trigonometric block only, shape lead + (2 dim n,)."""
    x, cov, f, _ = inp if inp is not None else inputs(case)
    x32, f32 = x.detach().cpu().numpy().astype(np.float32), f.cpu().numpy().astype(np.float32)
    t = x32[..., :, None] * f32  # (..., dim, n), float32
    a = t[..., None, :, :] + np.array([0.0, HALF_PI32], dtype=np.float32)[:, None, None]
    assert t.dtype == np.float32 and a.dtype == np.float32
    with np.errstate(invalid="ignore"):
        truth = np.sin(a.astype(np.float64))
    if cov is not None:
        exponent = np.float32(-0.5) * (cov.detach().cpu().numpy().astype(np.float32)[..., :, None] * (f32 * f32))
        assert exponent.dtype == np.float32
        truth = truth * np.exp(exponent.astype(np.float64))[..., None, :, :]
    return truth.reshape(case.lead + (-1,))


_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(FIXTURE) as z:
            _FIXTURE = {k: z[k] for k in z.files}
    return _FIXTURE


def key(cid, q):
    return f"{cid}/{q}"


def e_ref(case, q):
    return float(fixture()[f"E_ref/{pool(case)}/{q}"])


def argument_error(case, out, inp=None):
    """Largest |out - gate 1's truth| over the finite slots of the trigonometric block (0 for an empty case)."""
    truth = argument_truth(case, inp)
    got = out[..., :truth.shape[-1]]
    ok = np.isfinite(truth)
    return float(np.abs(got[ok] - truth[ok]).max()) if ok.any() else 0.0


def failures(case_list, fn, device="cpu", e_device=None, need=(True, True)):
    """Every miss of fn against the exact parts, gate 1 and gate 2 as a list of strings.  e_device: {"sin": .., "exp": ..} measured by
    the caller from the torch chain on `device`; None: 0, the CPU."""
    fix, bad = fixture(), []
    e_device = e_device or {"sin": 0.0, "exp": 0.0}
    for case in case_list:
        inp = inputs(case, device)
        got = run(fn, case, device=device, need=need, inp=inp)
        W, trig = width(case), 2 * case.dim * case.n
        if got["out"].shape != case.lead + (W,):
            bad.append(f"{case.id}: output shape {got['out'].shape}")
            continue
        if case.append and not torch.equal(torch.from_numpy(got["out"][..., trig:]).float().view(torch.int32),
                                           inp[0].detach().cpu().contiguous().view(torch.int32)):
            bad.append(f"{case.id}: the appended block is not x bit for bit")
        which = "exp" if case.cov else "sin"
        gate1 = GATE_FACTOR * max(float(fix["E_" + which]), e_device[which])
        err = argument_error(case, got["out"], inp)
        if not err <= gate1:
            bad.append(f"{case.id}: gate 1 ({which}) {err:.3e} > {gate1:.3e}")
        for q in QUANTITIES:
            if got[q] is None:
                continue
            truth = fix[key(case.id, q)]
            if got[q].shape != truth.shape:
                bad.append(f"{case.id}/{q}: shape {got[q].shape} != {truth.shape}")
                continue
            finite = np.isfinite(truth)
            if not (np.array_equal(np.isfinite(got[q]), finite) and np.array_equal(got[q][~finite], truth[~finite], equal_nan=True)):
                bad.append(f"{case.id}/{q}: the slots that are not finite differ from the reference's")
                continue
            if not finite.any():
                continue
            scale = float(np.abs(truth[finite]).max())
            err, gate = float(np.abs(got[q][finite] - truth[finite]).max()), GATE_FACTOR * e_ref(case, q) * scale
            if not err <= gate:
                bad.append(f"{case.id}/{q}: gate 2 {err:.3e} > {gate:.3e} (max |truth| {scale:.3e})")
    return bad


# ---- stratified depths -----------------------------------------------------------------------------------------------------------------
DepthCase = collections.namedtuple("DepthCase", "id n rows form edge")
# (n, rows): every n of 1, 2, 63, 64, 65, 150 and every rows of 1, 3, 257 at least once; 257 x 2 and 3 x 150 are more than one workgroup
_DEPTH_SIZES = ((1, 1), (1, 257), (2, 3), (2, 257), (63, 1), (63, 3), (64, 3), (64, 1), (65, 3), (65, 1), (150, 3), (150, 1), (150, 3))
DEPTH_FORMS = ("expand", "contiguous", "nonuniform")


def depth_cases():
    out = [DepthCase(f"depths-n{n}-r{rows}-{DEPTH_FORMS[i % 3]}", n, rows, DEPTH_FORMS[i % 3], False) for i, (n, rows) in enumerate(_DEPTH_SIZES)]
    # u of exactly 0 and of the largest float32 below 1 (rows alternate), through the reference's own arithmetic
    out += [DepthCase(f"depths-edge-n{n}-{form}", n, 4, form, True) for n, form in ((1, "expand"), (2, "contiguous"), (65, "expand"), (150, "nonuniform"))]
    return out


def depth_seed(case):
    return SEED + 7 * [c.id for c in depth_cases()].index(case.id)


def depth_centers(case, device="cpu"):
    """The centres (rows, n): a stride-0 expand of a linspace (what the ray samplers pass), the same contiguous, or sorted non-uniform."""
    g = torch.Generator().manual_seed(depth_seed(case) + 1)
    if case.form == "nonuniform":
        c = torch.sort(0.5 + 5.0 * torch.rand((case.rows, case.n), generator=g), dim=-1).values.to(device)
        return c
    line = torch.linspace(0.1, 3.0, case.n).to(device)
    c = line[None].expand(case.rows, case.n)
    assert case.rows == 1 or c.stride(0) == 0
    return c.contiguous() if case.form == "contiguous" else c


def edge_uniforms(case):
    u = torch.zeros((case.rows, case.n))
    u[1::2] = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    return u
