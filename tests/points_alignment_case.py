"""Cases and gates of iterative_closest_point / corresponding_points_alignment (tests/test_cpu_points_alignment.py,
tests/test_gpu_points_alignment.py, tests/golden/make_golden_points_alignment.py).

The yardstick is the reference's own pytorch3d/ops/points_alignment.py on the CPU, recorded in tests/golden/points_alignment_ref.npz:
per case the seed, a checksum of the inputs, the float64 run (R, T, s and, for ICP, rmse, Xt, the iteration count, the converged flag
and the neighbour index of every iteration) and the error of the reference's own float32 run against it, per quantity.

  gate      MARGIN x the LARGEST float32 error of the reference over the cases of a family, per quantity; an error is the largest
            absolute difference to the float64 run.  MARGIN = 4 covers a different but equally rounded summation order and solver
            (the project's standing margin).  Nothing is fixed in advance: the figures live in the fixture and `check` prints them.
  inputs    drawn by the CPU generator from the recorded seed and shaped by ELEMENTWISE float32 operations only (a matrix product
            rounds differently from one BLAS to the next); rotations are products of Pythagorean (cos, sin) pairs in Python floats.
  asserted by the generator (a seed that fails one is skipped, at most half of the tried seeds of a family):
            every iteration of the float64 run: the nearest and second-nearest DISTINCT distance of every live X point differ by
              MIN_GAP, relative.  A point moved by d changes a distance by at most d, and the runs compared here place a point within
              about 1e-6 of each other (R differs by some 5e-7 on points of norm 2), so at neighbour distances of 0.07 and above a
              gap of 3e-5 separates the two candidates in every run;
            the reference's float32 run has the float64 run's neighbours in every iteration, and its iteration count;
            converged cases: the last relative decrease is <= thr / 10 and the one before it >= 10 thr -- the count is no coin toss;
            sigma1 - sigma2 and sigma2 - sigma3 of the last covariance are >= SIGMA_GAP sigma1 (planar: only sigma1 - sigma2).
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "points_alignment_ref.npz")
MARGIN = 4.0
MIN_GAP = 3e-5
SIGMA_GAP = 1e-2
THR = 1e-6
SEED0 = 4100

# exact (cos, sin) pairs: 16.3, 22.6, 12.7, 10.4, 8.8, 36.9 degrees
PAIRS = ((24 / 25, 7 / 25), (12 / 13, 5 / 13), (40 / 41, 9 / 41), (60 / 61, 11 / 61), (84 / 85, 13 / 85), (4 / 5, 3 / 5))
ALIGN_QUANTITIES = ("R", "T", "s")
ICP_QUANTITIES = ("R", "T", "s", "rmse", "Xt")

# (family, variant, repetition).  The family is what a gate is taken over.
ALIGN_CASES = (
    ("rigid", "plain", 0), ("rigid", "plain", 1), ("rigid", "identity", 0), ("rigid", "rot180", 0),
    ("scale", "plain", 0), ("scale", "plain", 1),
    ("weights", "rand", 0), ("weights", "rand", 1), ("weights", "zero", 0),
    ("offset", "plain", 0), ("offset", "plain", 1),
    ("reflect", "fix", 0), ("reflect", "allow", 0), ("reflect", "fix", 1),
    ("planar", "tilted", 0), ("planar", "tilted", 1), ("planar", "exact", 0),
    ("ragged", "none", 0), ("ragged", "weights", 0), ("ragged", "none", 1),
)
ICP_CASES = (
    ("icp_rigid", "200x300", 0), ("icp_rigid", "200x300", 1), ("icp_rigid", "init", 0), ("icp_rigid", "maxiter", 0),
    ("icp_rigid", "thr1", 0),
    ("icp_scale", "130x70", 0), ("icp_scale", "130x70", 1),
    ("icp_ragged", "hetero", 0), ("icp_ragged", "hetero", 1), ("icp_ragged", "equalpad", 0),
)
UNCONVERGED = ("maxiter",)  # variants that stop at max_iterations
FREE_COUNT = ("maxiter", "thr1")  # variants whose iteration count is set by an argument, not by the decrease


def case_id(case):
    return "%s-%s-%d" % case


def key(kind, case, what):
    return "%s/%s/%s/%d/%s" % ((kind,) + tuple(case) + (what,))


_Z = None


def fixture():
    global _Z
    if _Z is None:
        with np.load(FIXTURE) as z:
            _Z = {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}
    return _Z


def seed_of(kind, case):
    return int(fixture()[key(kind, case, "seed")])


class Clouds:
    """What the two functions use of a Pointclouds: padded points, counts, and update_padded."""

    def __init__(self, points, lengths):
        self._points, self._lengths = points, lengths

    def points_padded(self):
        return self._points

    def num_points_per_cloud(self):
        return self._lengths

    def update_padded(self, new_points):
        return Clouds(new_points, self._lengths)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def rotation(kz, kx):
    """Rz(PAIRS[kz]) Rx(PAIRS[kx]) as nested Python floats: products and sums of exact rationals' doubles."""
    (cz, sz), (cx, sx) = PAIRS[kz % len(PAIRS)], PAIRS[kx % len(PAIRS)]
    rz = ((cz, -sz, 0.0), (sz, cz, 0.0), (0.0, 0.0, 1.0))
    rx = ((1.0, 0.0, 0.0), (0.0, cx, -sx), (0.0, sx, cx))
    return [[sum(rz[i][k] * rx[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def move(X, R, T, s):
    """s * (X R) + T on (P, 3) rows, elementwise float32 operations in a fixed order."""
    cols = [s * ((X[:, 0] * R[0][k] + X[:, 1] * R[1][k]) + X[:, 2] * R[2][k]) + T[k] for k in range(3)]
    return torch.stack(cols, 1)


def _blob(n, gen, scales=(1.0, 0.6, 0.3)):
    return torch.randn(n, 3, generator=gen) * torch.tensor(scales)


def _pad(clouds, P, gen, decoys):
    out = torch.zeros(len(clouds), P, 3)
    if decoys:
        out = torch.randn(len(clouds), P, 3, generator=gen) * 3.0  # what a masked row must not let through
    for n, c in enumerate(clouds):
        out[n, :c.shape[0]] = c
    return out


def align_inputs(case, seed=None):
    """dict(X, Y (3, P, 3) float32 or Clouds, weights or None, kwargs) of a corresponding_points_alignment case."""
    family, variant, rep = case
    seed = seed_of("align", case) if seed is None else seed
    gen = torch.Generator().manual_seed(seed)
    P, lengths = 130, None
    if family == "ragged":
        lengths = [130, 77, 5]
    Xs, Ys = [], []
    for n in range(3):
        m = P if lengths is None else lengths[n]
        x = _blob(m, gen)
        R, T, s = rotation(n + rep, n + 2 * rep + 1), (0.3 * (n + 1), -0.2, 0.1 * n), 1.0
        noise = 0.01 * torch.randn(m, 3, generator=gen)
        if family == "scale":
            s = (0.5, 1.75, 2.5)[n]
        if family == "offset":
            x = x + torch.tensor([100.0, -100.0, 100.0])
        if family == "planar":
            x = x * torch.tensor([1.0, 1.0, 0.0])
            noise = noise * torch.tensor([1.0, 1.0, 0.0])
            if variant == "exact":  # z = 0 in X and in Y: sigma3 is exactly 0 in every precision
                cz, sz = PAIRS[n]
                R = [[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]]
                T = (T[0], T[1], 0.0)
            else:
                x = move(x, rotation(n + 3, n + 4), (0.0, 0.0, 0.0), 1.0)
                noise = move(noise, rotation(n + 3, n + 4), (0.0, 0.0, 0.0), 1.0)
        if variant == "identity":
            y = x.clone()
        else:
            if variant == "rot180":
                R = [[-1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0]]
            src = x * torch.tensor([1.0, 1.0, -1.0]) if family == "reflect" else x
            y = move(src, R, T, s) + noise
        Xs.append(x), Ys.append(y)
    decoys = lengths is not None
    X, Y = _pad(Xs, P, gen, decoys), _pad(Ys, P, gen, decoys)
    weights = None
    if variant in ("rand", "weights", "zero"):
        weights = torch.rand(3, P, generator=gen) * 2.0
        if variant == "zero":
            weights[1] = 0.0
    kwargs = {"estimate_scale": family in ("scale", "weights"), "allow_reflection": variant == "allow"}
    out = {"X": X, "Y": Y, "weights": weights, "kwargs": kwargs, "lengths": None}
    if lengths is not None:
        out["lengths"] = torch.tensor(lengths, dtype=torch.int64)
    return out


def icp_inputs(case, seed=None):
    """dict(X (3, P1, 3), Y (3, P2, 3) float32, lengths1, lengths2 or None, init or None, kwargs) of an ICP case: Y an anisotropic blob,
    X noisy samples of it moved back by a rotation of 9 to 37 degrees, a shift and, for icp_scale, a scale."""
    family, variant, rep = case
    seed = seed_of("icp", case) if seed is None else seed
    gen = torch.Generator().manual_seed(seed)
    P1, P2 = (130, 70) if family == "icp_scale" else (200, 300)
    l1 = l2 = None
    if variant == "hetero":
        l1, l2 = [200, 150, 64], [300, 170, 90]
    if variant == "equalpad":
        l1 = l2 = [200, 190, 180]
    Xs, Ys = [], []
    for n in range(3):
        m1, m2 = (P1 if l1 is None else l1[n]), (P2 if l2 is None else l2[n])
        y = _blob(m2, gen)
        pick = torch.randint(0, m2, (m1,), generator=gen)
        x = y[pick] + 0.02 * torch.randn(m1, 3, generator=gen)
        s = (0.8, 1.25, 1.1)[n] if family == "icp_scale" else 1.0
        kz = (4, 3, 2)[n] if variant != "init" else (5, 1, 0)[n]  # small angles; `init` starts far and is helped by its transform
        x = move(x, rotation(kz + rep, 4 - rep), (0.05 * n, -0.03, 0.04), s)
        Xs.append(x), Ys.append(y)
    X = _pad(Xs, P1, gen, l1 is not None)
    Y = _pad(Ys, P2, gen, l2 is not None)
    if variant == "equalpad":  # the padded rows of X enter with weight one, each paired with Y[n, 0]: keep them where the clouds are
        for n in range(3):
            X[n, l1[n]:] = Xs[n][:P1 - l1[n]] * torch.tensor([1.0, -1.0, 1.0])
    init = None
    if variant == "init":  # the inverse of the rotation part, roughly: (R^T, 0, 1) per cloud
        Rs = []
        for n in range(3):
            R = rotation((5, 1, 0)[n] + rep, 4 - rep)
            Rs.append([[R[j][i] for j in range(3)] for i in range(3)])
        init = (torch.tensor(Rs, dtype=torch.float32), torch.zeros(3, 3), torch.ones(3))
    kwargs = {"estimate_scale": family == "icp_scale", "relative_rmse_thr": THR, "max_iterations": 100}
    if variant == "maxiter":
        kwargs["max_iterations"] = 3
    if variant == "thr1":
        kwargs["relative_rmse_thr"] = 1.5
    t64 = lambda v: None if v is None else torch.tensor(v, dtype=torch.int64)  # noqa: E731
    return {"X": X, "Y": Y, "lengths1": t64(l1), "lengths2": t64(l2), "init": init, "kwargs": kwargs}


def checksum(d):
    """A float64 sum over the inputs: a generator that draws other numbers than the recorded run shows here, not in a gate."""
    total = d["X"].double().sum() + 3.0 * d["Y"].double().sum()
    if d.get("weights") is not None:
        total = total + 7.0 * d["weights"].double().sum()
    return total


def to(d, device=None, dtype=None):
    """The inputs of a case as call arguments on a device / in a dtype: (X, Y) tensors or Clouds."""
    def t(v, floating=True):
        if v is None:
            return None
        return v.to(device=device, dtype=dtype if floating else None)

    X, Y = t(d["X"]), t(d["Y"])
    if d.get("lengths") is not None:
        n = t(d["lengths"], False)
        return Clouds(X, n), Clouds(Y, n)
    if d.get("lengths1") is not None:
        return Clouds(X, t(d["lengths1"], False)), Clouds(Y, t(d["lengths2"], False))
    return X, Y


def run_align(fn, case, device=None, dtype=None, seed=None):
    d = align_inputs(case, seed)
    X, Y = to(d, device, dtype)
    w = None if d["weights"] is None else d["weights"].to(device=device, dtype=dtype)
    return fn(X, Y, weights=w, **d["kwargs"])


def run_icp(fn, case, device=None, dtype=None, seed=None, **more):
    d = icp_inputs(case, seed)
    X, Y = to(d, device, dtype)
    init = None if d["init"] is None else tuple(t.to(device=device, dtype=dtype) for t in d["init"])
    return fn(X, Y, init_transform=init, **d["kwargs"], **more)


# ---- figures and gates ---------------------------------------------------------------------------------------------------------------
def _padded(x):
    return x.points_padded() if hasattr(x, "points_padded") else x


def align_values(out):
    return {"R": out[0], "T": out[1], "s": out[2]}


def icp_values(sol):
    return {"R": sol.RTs.R, "T": sol.RTs.T, "s": sol.RTs.s, "rmse": sol.rmse, "Xt": _padded(sol.Xt)}


def errors(values, truth):
    """{quantity: the largest absolute difference to the float64 run}; a NaN is an infinite error."""
    out = {}
    for q, v in values.items():
        e = (v.detach().cpu().double() - truth[q].double()).abs().max()
        out[q] = float("inf") if bool(torch.isnan(e)) else float(e)
    return out


def truth(kind, case):
    z = fixture()
    return {q: z[key(kind, case, q + "64")] for q in (ALIGN_QUANTITIES if kind == "align" else ICP_QUANTITIES)}


def gates(kind, family):
    """{quantity: MARGIN x the reference's largest float32 error over the family}."""
    z = fixture()
    names = ALIGN_QUANTITIES if kind == "align" else ICP_QUANTITIES
    cases = [c for c in (ALIGN_CASES if kind == "align" else ICP_CASES) if c[0] == family]
    worst = torch.stack([z[key(kind, c, "err32")] for c in cases]).max(0).values
    return {q: MARGIN * float(worst[k]) for k, q in enumerate(names)}


def check(kind, case, values, who=""):
    """Asserts every quantity within its family's gate; prints the figures first."""
    err, gate = errors(values, truth(kind, case)), gates(kind, case[0])
    print("%s %s %s:" % (who, kind, case_id(case)), ", ".join("%s %.3g (gate %.3g)" % (q, err[q], gate[q]) for q in err))
    bad = {q: (err[q], gate[q]) for q in err if not err[q] <= gate[q]}
    assert not bad, (case_id(case), bad)


def refused(kind, case, values):
    """Whether some quantity misses its gate (the wrong variants must)."""
    err, gate = errors(values, truth(kind, case)), gates(kind, case[0])
    return any(not err[q] <= gate[q] for q in err)


def check_inputs(kind, case):
    d = align_inputs(case) if kind == "align" else icp_inputs(case)
    want = float(fixture()[key(kind, case, "checksum")])
    assert float(checksum(d)) == want, "the inputs of %s are not the recorded run's" % case_id(case)
