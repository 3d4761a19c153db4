"""Cases, seeded inputs and gates of the VolumeSampler tests (csrc/volume_sample.hip; pytorch3d_amd/volume_sampler.py).

A case is steps 2 and 3 of the reference's VolumeSampler.forward on LOCAL rays: volumes (Nv, C, D, H, W), origins and directions
(N, R, 3), lengths (N, R, P), and a gradient into each output (not ones).  The fixture tests/golden/volume_sampler_ref.npz
(tests/golden/make_golden_volume_sampler.py) holds the float64 truth of the seven quantities of QUANTITIES per case, E_ref/<quantity>
-- the largest error of the reference's own float32 CPU VolumeSampler against that truth over all cases, relative to the case's
largest |truth| -- and, for the lattice cases, F.grid_sample's float32 CPU outputs.  Gate, per quantity and case:
|got - truth| <= 4 E_ref max|truth|.

Kinds of cases (the smallest shapes at which the kernels can go wrong):
  rays     seeded rays that enter and leave the grid through every face, over all eight (mode, padding, align_corners) combinations,
           P in (1, 2, 63, 64, 65, 130) -- below, at and beyond a backward chunk of 32 points and the 64 lanes of a wave --, the grids
           (3, 4, 5) (an axis mix-up shows), (1, 4, 5), (3, 1, 5), (3, 4, 1) (the align_corners multiplier is 0 on that axis) and
           (5, 5, 5) (S - 1 a power of two), Cd in (1, 2), Cf in (None, 1, 3, 4, 5), N in (1, 2); R = 257 once; one grid shared by N = 3
  edges    points exactly at -1 and +1, NaN, +-inf, and coordinates whose source index does not fit an int32 (1e10, 3e38), on every axis.
           Under BORDER padding the NaN slots hold -2.5 (a finite coordinate beyond the face) instead: there the reference does not
           agree with itself -- ATen's CPU grid_sampler_3d clamps with std::min(S - 1, std::max(c, 0)), which sends NaN to S - 1, its GPU
           kernel with fmin / fmax, which send it to 0 -- so no truth exists.  The contract (csrc/implicit_abi.h) is NaN -> 0, the GPU's
           answer and vert_align's; the tests hold the kernels to it by asking that NaN gives what -inf gives, which the truth does gate
  lattice  dyadic origins, directions, lengths and voxel values on the 5^3 grid: every product and sum is exact, points land on voxels
           and on half-way planes (nearest ties, weights of exactly 0 and 1); the forward is gated BIT-EQUAL to F.grid_sample
  collide  all points of four rays inside one voxel cell: the backward's atomics are heavily contended
  world    the local rays the reference's own step 1 made (recorded in the fixture with the world-to-local matrix) of seeded world
           rays and a 6 x 7 x 8 Volumes with a non-zero translation and voxel size: volume_sampler_forward as a whole
Condition (asserted by the generator, met by re-seeding inside inputs()): no sample lies within CLEARANCE index units of a lattice
plane, or of a half-integer plane in nearest mode, where float32 and float64 floor differently and the coordinate gradient jumps --
unless its source index is the SAME number in float32 and float64, so that both floor alike: the exact coordinates of the edges and
lattice cases, and every coordinate on an axis of one voxel under align_corners (index 0 times anything).  No sample of any case is
left ungated.
"""
import collections
import functools
import itertools
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "volume_sampler_ref.npz")
SEED = 20240923
QUANTITIES = ("rays_densities", "rays_features", "grad_densities", "grad_features", "grad_origins", "grad_directions", "grad_lengths")
GATE_FACTOR = 4.0
CLEARANCE = 1e-4
MODES = tuple(itertools.product(("bilinear", "nearest"), ("zeros", "border"), (True, False)))
GRIDS = ((3, 4, 5), (1, 4, 5), (3, 1, 5), (3, 4, 1), (5, 5, 5))
RAY_P = (1, 2, 63, 64, 65, 130)
FEATURE_DIMS = (None, 1, 3, 4, 5)
WORLD_GRID, WORLD_TRANSLATION, WORLD_VOXEL_SIZE = (6, 7, 8), (0.3, -0.2, 0.15), (0.4, 0.35, 0.3)

Case = collections.namedtuple("Case", "id kind grid Cd Cf N R P mode padding align shared")


def _mode_id(mode, padding, align):
    return "%s-%s-%s" % (mode[:3], padding[:3], "ac" if align else "na")


def cases():
    out = []
    for i, (mode, padding, align) in enumerate(MODES):
        for j, P in enumerate(RAY_P):
            grid, Cf, Cd = GRIDS[(i + j) % 5], FEATURE_DIMS[(i + 2 * j) % 5], 1 + (i + j) % 2
            N, R = (2, 5) if P <= 2 else (1, 3)
            out.append(Case("rays-%s-P%d-g%d%d%d-Cd%d-Cf%s-N%d" % ((_mode_id(mode, padding, align), P) + grid + (Cd, Cf, N)), "rays", grid, Cd, Cf, N,
                            R, P, mode, padding, align, False))
        out.append(Case("edges-" + _mode_id(mode, padding, align), "edges", (3, 4, 5), 1, 3, 1, 40, 1, mode, padding, align, False))
        out.append(Case("lattice-" + _mode_id(mode, padding, align), "lattice", (5, 5, 5), 1, 3, 1, 16, 4, mode, padding, align, False))
    out.append(Case("rays-R257", "rays", (3, 4, 5), 1, 3, 1, 257, 2, "bilinear", "zeros", True, False))
    out.append(Case("rays-shared-N3", "rays", (3, 4, 5), 2, 3, 3, 4, 5, "bilinear", "zeros", True, True))
    out.append(Case("rays-shared-N3-nearest", "rays", (3, 4, 5), 1, None, 3, 4, 5, "nearest", "border", False, True))
    out.append(Case("collide", "collide", (3, 4, 5), 2, 4, 1, 4, 64, "bilinear", "zeros", True, False))
    out.append(Case("world", "world", WORLD_GRID, 1, 3, 2, 8, 20, "bilinear", "zeros", True, False))
    return out


def case_by_id(cid):
    return next(c for c in cases() if c.id == cid)


def _gen(case, attempt):
    key = (case.kind, case.grid, case.Cd, case.Cf or 0, case.N, case.R, case.P, MODES.index((case.mode, case.padding, case.align)), len(case.id))
    flat = [len(key[0])] + list(key[1]) + list(key[2:])
    return torch.Generator().manual_seed(SEED + sum((i + 1) * 7919 * int(k) for i, k in enumerate(flat)) + 104729 * attempt)


def source_index(c, S, align):
    """ATen's un-normalised source index of coordinate c on an axis of S voxels, before any padding (c's dtype decides the precision)."""
    one, two = c.dtype.type(1), c.dtype.type(2)
    if align:
        return ((c + one) / two) * c.dtype.type(S - 1)
    return ((c + one) * c.dtype.type(S) - one) / two


def plane_clearance(case, origins, directions, lengths):
    """(distance of every sample's source index to the nearest lattice plane -- or half-integer plane in nearest mode --, whether
    the float32 and the float64 source index are the same number), both (N, R, P, 3); samples that are not finite or beyond an int32 are
    far from every plane."""
    o, d, l = (np.asarray(t, dtype=np.float32) for t in (origins, directions, lengths))
    with np.errstate(all="ignore"):
        p32 = o[:, :, None, :] + l[:, :, :, None] * d[:, :, None, :]
        p64 = o.astype(np.float64)[:, :, None, :] + l.astype(np.float64)[:, :, :, None] * d.astype(np.float64)[:, :, None, :]
        D, H, W = case.grid
        dist, same = np.empty(p64.shape), np.empty(p64.shape, dtype=bool)
        for a, S in enumerate((W, H, D)):
            i64, i32 = source_index(p64[..., a], S, case.align), source_index(p32[..., a], S, case.align)
            step = 0.5 if case.mode == "nearest" else 1.0
            far = ~np.isfinite(i64) | (np.abs(i64) >= 2.0e9)
            dist[..., a] = np.where(far, 1.0, np.abs(i64 / step - np.round(i64 / step)) * step)
            same[..., a] = far | (i32.astype(np.float64) == i64)
    return dist, same


def clear_of_planes(case, origins, directions, lengths):
    dist, same = plane_clearance(case, origins, directions, lengths)
    return bool(((dist >= CLEARANCE) | same).all())


EDGE_VALUES = (-1.0, 1.0, float("nan"), float("inf"), float("-inf"), 1e10, -1e10, 3e38)


def _rays(case, g):
    N, R, P = case.N, case.R, case.P
    if case.kind == "edges":  # ray r: EDGE_VALUES[r % 8] on axis (r // 8) % 3 (rays 24..39: on two axes), the rest inside; direction 0, length 1
        o = 1.8 * torch.rand((N, R, 3), generator=g) - 0.9
        values = tuple(-2.5 if case.padding == "border" and v != v else v for v in EDGE_VALUES)
        for r in range(R):
            o[:, r, (r // 8) % 3] = values[r % 8]
            if r >= 24:
                o[:, r, (r // 8 + 1) % 3] = values[(r * 3 + 1) % 8]
        return o, torch.zeros((N, R, 3)), torch.ones((N, R, P))
    if case.kind == "lattice":  # multiples of 1/4: the source index is a multiple of 1/2 (align_corners) or of 1/8
        o = torch.randint(-6, 7, (N, R, 3), generator=g).float() / 4
        d = torch.randint(-2, 3, (N, R, 3), generator=g).float() / 4
        return o, d, torch.randint(0, 4, (N, R, P), generator=g).float()
    if case.kind == "collide":  # every point inside the cell of index (2.5, 1.5, 0.5) + small offsets: grid (3, 4, 5), align_corners
        centre = torch.tensor([0.27, 0.03, -0.46])
        o = centre + 0.02 * (torch.rand((N, R, 3), generator=g) - 0.5)
        d = 0.02 * (torch.rand((N, R, 3), generator=g) - 0.5)
        return o, d, torch.sort(torch.rand((N, R, P), generator=g), dim=-1).values
    # rays: from a sphere of radius 1.6 around the grid towards a point inside it; lengths up to 3.4, so that the far end is outside again
    start = torch.randn((N, R, 3), generator=g)
    start = 1.6 * start / start.norm(dim=-1, keepdim=True)
    aim = 1.2 * torch.rand((N, R, 3), generator=g) - 0.6
    d = (aim - start) / (aim - start).norm(dim=-1, keepdim=True)
    lengths = torch.sort(3.4 * torch.rand((N, R, P), generator=g), dim=-1).values
    return start, d, lengths


def world_rays():
    """(origins, directions, lengths) of the world case in WORLD coordinates, float32."""
    g = torch.Generator().manual_seed(SEED + 5)
    N, R, P = 2, 8, 20
    start = torch.randn((N, R, 3), generator=g)
    start = 2.2 * start / start.norm(dim=-1, keepdim=True) + torch.tensor(WORLD_TRANSLATION)
    aim = 0.8 * torch.rand((N, R, 3), generator=g) - 0.4
    d = (aim - start) / (aim - start).norm(dim=-1, keepdim=True)
    return start, d, torch.sort(0.8 + 3.0 * torch.rand((N, R, P), generator=g), dim=-1).values


def inputs(case, local_rays=None):
    """float32 CPU tensors of a case: densities, features (or None), origins, directions, lengths, grad_d, grad_f (or None).  The world
    case's local rays come from the fixture (the reference's step 1 made them) unless the generator hands them in."""
    D, H, W = case.grid
    Nv = 1 if case.shared else case.N
    for attempt in range(1000):
        g = _gen(case, attempt)
        if case.kind == "world":
            o, d = local_rays if local_rays is not None else (torch.from_numpy(fixture()["world/origins_local"]), torch.from_numpy(fixture()["world/directions_local"]))
            l = world_rays()[2]
        else:
            o, d, l = _rays(case, g)
        if clear_of_planes(case, o, d, l):
            break
        assert case.kind not in ("world", "edges", "lattice"), case.id  # (nothing to re-seed there)
    else:
        raise AssertionError(case.id)
    if case.kind == "lattice":
        dens = torch.randint(-32, 33, (Nv, case.Cd, D, H, W), generator=g).float() / 8
        feats = torch.randint(-32, 33, (Nv, case.Cf, D, H, W), generator=g).float() / 8
        g_d = torch.randint(-8, 9, (case.N, case.R, case.P, case.Cd), generator=g).float() / 4
        g_f = torch.randint(-8, 9, (case.N, case.R, case.P, case.Cf), generator=g).float() / 4
        return dens, feats, o, d, l, g_d, g_f
    dens = torch.rand((Nv, case.Cd, D, H, W), generator=g)
    feats = None if case.Cf is None else torch.randn((Nv, case.Cf, D, H, W), generator=g)
    g_d = torch.randn((case.N, case.R, case.P, case.Cd), generator=g)
    g_f = None if case.Cf is None else torch.randn((case.N, case.R, case.P, case.Cf), generator=g)
    return dens, feats, o, d, l, g_d, g_f


def run(fn, case, device="cpu", dtype=torch.float32, inp=None):
    """The seven quantities of fn(densities, features, origins, directions, lengths, sample_mode=, padding_mode=, align_corners=) ->
    (rays_densities, rays_features) on a case as float64 numpy arrays (None: the case has no features)."""
    inp = inputs(case) if inp is None else inp
    dens, feats, o, d, l, g_d, g_f = (None if t is None else t.to(device=device, dtype=dtype) for t in inp)
    leaves = [t.requires_grad_(True) for t in (dens, feats, o, d, l) if t is not None]
    rd, rf = fn(dens, feats, o, d, l, sample_mode=case.mode, padding_mode=case.padding, align_corners=case.align)
    loss = (rd * g_d).sum() + ((rf * g_f).sum() if feats is not None else 0.0)
    grads = iter(torch.autograd.grad(loss, leaves, allow_unused=True))
    gd = next(grads)
    gf = next(grads) if feats is not None else None
    go, gdir, gl = next(grads), next(grads), next(grads)

    def np64(t, like=None):
        if t is None:
            t = torch.zeros_like(like)
        return t.detach().double().cpu().numpy()

    return {"rays_densities": np64(rd), "rays_features": np64(rf) if feats is not None else None, "grad_densities": np64(gd, dens),
            "grad_features": np64(gf, feats) if feats is not None else None, "grad_origins": np64(go, o), "grad_directions": np64(gdir, d),
            "grad_lengths": np64(gl, l)}


def key(cid, name):
    return "%s/%s" % (cid, name)


@functools.lru_cache(maxsize=1)
def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def e_ref(quantity):
    return float(fixture()["E_ref/" + quantity])


def errors(case, got):
    """{quantity: (error, gate)} against the fixture's truth; error = max |got - truth| (inf where got is not finite or of another
    shape), gate = 4 E_ref max |truth|."""
    fix, out = fixture(), {}
    for q in QUANTITIES:
        if got[q] is None:
            continue
        truth = fix[key(case.id, q)]
        g = np.asarray(got[q], dtype=np.float64)
        err = float(np.abs(g - truth).max()) if g.shape == truth.shape and np.isfinite(g).all() else float("inf")
        if truth.size == 0:
            err = 0.0 if g.shape == truth.shape else float("inf")
        out[q] = (err, GATE_FACTOR * e_ref(q) * (float(np.abs(truth).max()) if truth.size else 0.0))
    return out


def failures(cases_, fn, device="cpu", dtype=torch.float32, verbose=False, quantities=QUANTITIES):
    """[(case id, quantity, error, gate)] of everything beyond its gate."""
    bad = []
    for case in cases_:
        for q, (err, gate) in errors(case, run(fn, case, device, dtype)).items():
            if verbose:
                print("%-60s %-16s error %.3e gate %.3e" % (case.id, q, err, gate))
            if q in quantities and not err <= gate:
                bad.append((case.id, q, err, gate))
    return bad


def same_bits(a, b):
    return bool(np.array_equal(np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32), equal_nan=True))


# ---- the world case's stand-in for a Volumes object: the recorded world-to-local matrix behind the reference's method names ----------
class MatrixTransform:
    """Transform3d's transform_points (points @ matrix in homogeneous row vectors, divided by w) over a fixed (N, 4, 4) matrix."""

    def __init__(self, matrix):
        self._matrix = matrix

    def get_matrix(self):
        return self._matrix

    def transform_points(self, points):
        batch = torch.cat([points, torch.ones_like(points[..., :1])], dim=2)
        out = torch.bmm(batch, self._matrix.expand(points.shape[0], 4, 4))
        return out[..., :3] / out[..., 3:]


class MatrixVolumes:
    def __init__(self, densities, features, matrix, align_corners=True):
        self._densities, self._features, self._matrix, self._align = densities, features, matrix, align_corners

    def densities(self):
        return self._densities

    def features(self):
        return self._features

    def get_align_corners(self):
        return self._align

    def get_world_to_local_coords_transform(self):
        return MatrixTransform(self._matrix)

    def world_to_local_coords(self, points):
        shape = points.shape
        return self.get_world_to_local_coords_transform().transform_points(points.view(shape[0], -1, 3)).view(shape)


RayBundle = collections.namedtuple("RayBundle", "origins directions lengths xys")


def nan_equals_minus_inf_under_border(fn, device="cpu"):
    """[(case id, quantity)] where fn, on a border edges case, answers a NaN coordinate otherwise than the same case with -inf in its
    place (bit for bit, over all seven quantities): the contract's NaN -> 0 (see the header)."""
    bad = []
    for case in (c for c in cases() if c.kind == "edges" and c.padding == "border"):
        inp = list(inputs(case))
        with_inf, with_nan = inp[2].clone(), inp[2].clone()
        with_inf[inp[2] == -2.5] = float("-inf")
        with_nan[inp[2] == -2.5] = float("nan")
        assert int((inp[2] == -2.5).sum()) >= 3
        a = run(fn, case, device, inp=inp[:2] + [with_inf] + inp[3:])
        b = run(fn, case, device, inp=inp[:2] + [with_nan] + inp[3:])
        bad += [(case.id, q) for q in QUANTITIES if a[q] is not None and not np.array_equal(a[q], b[q])]
    return bad
