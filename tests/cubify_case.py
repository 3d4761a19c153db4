"""Shared cases of the cubify tests: the cases of tests/golden/cubify_ref.npz (recorded by tests/golden/make_golden_cubify.py from the
reference's own CPU `pytorch3d.ops.cubify`), its loader, the inputs' builders, an independent nested-loop restatement of the contract
in plain Python / numpy (`restate`), and the one comparison every implementation -- the restatement, the torch formulation, the
kernels, deliberately wrong variants -- is judged by: `misses`, which is torch.equal on every tensor, with shapes and dtypes.  No
tolerance anywhere: the contract is integers and exactly specified float32 arithmetic.  No test collects this file.

A case is a name; inputs(name) gives (voxels (N, D, H, W), thresh, feats or None, align) as the fixture holds them.  Families:
  g<NDHW>_<align>_p<density>   random grids (2,3,4,5), (3,2,2,2), (2,5,3,2), (1,4,4,4) x the three aligns x densities 0.3 and 0.7
  feats_center                 (2,3,4,5) with feats (2,3,3,4,5), align "center": the TexturesAtlas values
  some_empty                   5 x (2,3,3), meshes 0, 2 and 4 without an occupied voxel
  all_empty                    3 x (2,3,2), nothing occupied: every list entry is an empty 1-D tensor
  solid3                       the solid 3^3 block: 56 vertices (the 8 interior lattice points are dropped), 108 faces
  checker                      2 x (4,4,4) 3-D checkerboards of either parity: every voxel exposes all six sides, diagonal cubes share vertices
  thresh07                     values float32(0.7), the float32 below it, NaN, +-inf and others with thresh = 0.7 (a double above float32(0.7))
The fixture holds per case <name>/voxels, thresh, align (and feats), and the reference's outputs packed: <name>/verts, faces, nv, nf
(per-mesh sizes), ndim (1 where the reference returned 1-D empties) and tex (F, K) where it returned textures.
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "cubify_ref.npz")

GRIDS = {"g2345": (2, 3, 4, 5), "g3222": (3, 2, 2, 2), "g2532": (2, 5, 3, 2), "g1444": (1, 4, 4, 4)}
ALIGNS = ("topleft", "corner", "center")
DENSITIES = (0.3, 0.7)
# (dh, dw, dd) of the directions -x +y -z -y +x +z, and the corners c = 4x + 2y + z of their two triangles each
DIRECTIONS = ((0, -1, 0), (1, 0, 0), (0, 0, -1), (-1, 0, 0), (0, 1, 0), (0, 0, 1))
TRIANGLES = ((0, 1, 2), (1, 3, 2), (2, 3, 6), (3, 7, 6), (0, 2, 6), (0, 6, 4), (0, 5, 1), (0, 4, 5), (6, 7, 5), (6, 5, 4), (1, 7, 3), (1, 5, 7))


def cases():
    names = ["%s_%s_p%d" % (g, a, round(10 * p)) for g in GRIDS for a in ALIGNS for p in DENSITIES]
    return names + ["feats_center", "some_empty", "all_empty", "solid3", "checker", "thresh07"]


def _gen(name):
    return torch.Generator().manual_seed(1000 + cases().index(name))


def random_voxels(shape, density, gen):
    """(voxels, thresh): uniform values, occupied with probability `density`."""
    return torch.rand(shape, generator=gen), 1.0 - density


def checkerboard(shape, parity=0):
    n, d, h, w = torch.meshgrid(*[torch.arange(s) for s in shape], indexing="ij")
    return (((d + h + w + n + parity) % 2) == 0).float()


def ball(shape):
    """Occupancy 1 inside the ball inscribed in the grid, 0 outside."""
    N, D, H, W = shape
    d, h, w = torch.meshgrid(*[(torch.arange(s) + 0.5) / s * 2 - 1 for s in (D, H, W)], indexing="ij")
    return ((d * d + h * h + w * w) <= 1.0).float()[None].expand(N, D, H, W).contiguous()


def build_inputs(name):
    """What the recorder stores as the case's inputs (tests read them from the fixture, not from here)."""
    gen = _gen(name)
    if name[:5] in GRIDS:
        grid, align, p = name.split("_")
        voxels, thresh = random_voxels(GRIDS[grid], int(p[1:]) / 10.0, gen)
        return voxels, thresh, None, align
    if name == "feats_center":
        voxels, thresh = random_voxels((2, 3, 4, 5), 0.5, gen)
        return voxels, thresh, torch.rand((2, 3, 3, 4, 5), generator=gen), "center"
    if name == "some_empty":
        voxels, thresh = random_voxels((5, 2, 3, 3), 0.5, gen)
        voxels[0::2] *= 0.25  # below the threshold
        return voxels, thresh, None, "topleft"
    if name == "all_empty":
        return torch.zeros((3, 2, 3, 2)), 0.5, None, "corner"
    if name == "solid3":
        return torch.ones((1, 3, 3, 3)), 0.5, None, "topleft"
    if name == "checker":
        return checkerboard((2, 4, 4, 4)), 0.5, None, "center"
    if name == "thresh07":
        at = torch.tensor(0.7, dtype=torch.float32)
        values = torch.stack([at, torch.nextafter(at, torch.tensor(0.0)), torch.tensor(float("nan")), torch.tensor(float("inf")),
                              torch.tensor(float("-inf")), torch.tensor(0.9), torch.tensor(0.1), torch.nextafter(at, torch.tensor(1.0))])
        return values[torch.randint(0, 8, (2, 3, 3, 4), generator=gen)], 0.7, None, "topleft"
    raise KeyError(name)


_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(FIXTURE) as z:
            _FIXTURE = {k: z[k] for k in z.files}
    return _FIXTURE


def inputs(name, device="cpu"):
    f = fixture()
    feats = torch.from_numpy(f[name + "/feats"]).to(device) if name + "/feats" in f else None
    return torch.from_numpy(f[name + "/voxels"]).to(device), float(f[name + "/thresh"]), feats, str(f[name + "/align"])


def split(verts, faces, nv, nf, tex=None):
    """Packed tensors and per-mesh sizes -> (verts list, faces list, tex list or None), as the reference's lists are."""
    nv, nf = [int(x) for x in nv], [int(x) for x in nf]
    return list(verts.split(nv, 0)), list(faces.split(nf, 0)), None if tex is None else list(tex.split(nf, 0))


def expected(name):
    """The reference's recorded lists of the case."""
    f = fixture()
    one_d = int(f[name + "/ndim"]) == 1
    verts, faces = torch.from_numpy(f[name + "/verts"]), torch.from_numpy(f[name + "/faces"])
    if one_d:
        verts, faces = verts.reshape(0), faces.reshape(0)
    tex = torch.from_numpy(f[name + "/tex"]).reshape(faces.shape[0], 1, 1, -1) if name + "/tex" in f else None
    return split(verts, faces, f[name + "/nv"], f[name + "/nf"], tex)


def axis_value(i, size, align):
    t = np.float32(i)
    if align == "center":
        t = np.float32(t - np.float32(0.5))
    t = np.float32(t * np.float32(2.0))
    t = np.float32(t / np.float32(size - (0.0 if align == "corner" else 1.0)))
    return np.float32(t - np.float32(1.0))


def restate(voxels, thresh, feats=None, align="topleft"):
    """The contract in nested loops over numpy arrays -> (verts list, faces list, tex list or None) of torch tensors."""
    if align not in ALIGNS:
        raise ValueError("Align mode must be one of (topleft, corner, center).")
    vox = voxels.detach().cpu().numpy()
    N, D, H, W = vox.shape
    level = vox.dtype.type(thresh)
    fts = feats.detach().cpu().numpy() if feats is not None and align == "center" else None

    def occupied(n, h, w, d):
        return 0 <= h < H and 0 <= w < W and 0 <= d < D and bool(vox[n, d, h, w] >= level)  # NaN: False

    all_faces, all_tex = [], []
    for n in range(N):
        faces, tex = [], []
        for h in range(H):
            for w in range(W):
                for d in range(D):
                    if not occupied(n, h, w, d):
                        continue
                    for k, (dh, dw, dd) in enumerate(DIRECTIONS):
                        if occupied(n, h + dh, w + dw, d + dd):
                            continue
                        for tri in TRIANGLES[2 * k:2 * k + 2]:
                            faces.append([((h + ((c >> 1) & 1)) * (W + 1) + w + ((c >> 2) & 1)) * (D + 1) + d + (c & 1) for c in tri])
                            if fts is not None:
                                tex.append(fts[n, :, d, h, w])
        all_faces.append(faces)
        all_tex.append(tex)
    if not any(all_faces):
        return [torch.zeros(0)] * N, [torch.zeros(0, dtype=torch.int64)] * N, None
    verts_list, faces_list, tex_list = [], [], []
    for faces, tex in zip(all_faces, all_tex):
        kept = sorted({g for f in faces for g in f})
        rank = {g: r for r, g in enumerate(kept)}
        verts = np.zeros((len(kept), 3), np.float32)
        for r, g in enumerate(kept):
            z, t = g % (D + 1), g // (D + 1)
            x, y = t % (W + 1), t // (W + 1)
            verts[r] = (axis_value(x, W, align), axis_value(y, H, align), axis_value(z, D, align))
        verts_list.append(torch.from_numpy(verts))
        faces_list.append(torch.tensor([[rank[g] for g in f] for f in faces], dtype=torch.int64).reshape(-1, 3))
        if fts is not None:
            tex_list.append(torch.from_numpy(np.array(tex, dtype=fts.dtype).reshape(len(tex), 1, 1, fts.shape[1])))
    return verts_list, faces_list, tex_list if fts is not None else None


def lists_of(packed):
    """cubify_packed's 5-tuple -> the three lists."""
    verts, faces, nv, nf, tex = packed
    return split(verts, faces, nv.tolist(), nf.tolist(), tex)


def misses(got, want, what=""):
    """Every difference between two (verts list, faces list, tex list or None): lengths, shapes, dtypes, then torch.equal."""
    out = []
    for kind, g, w in zip(("verts", "faces", "tex"), got, want):
        if (g is None) != (w is None):
            out.append("%s %s: %s against %s" % (what, kind, "None" if g is None else "a list", "None" if w is None else "a list"))
            continue
        if g is None:
            continue
        if len(g) != len(w):
            out.append("%s %s: %d meshes against %d" % (what, kind, len(g), len(w)))
            continue
        for i, (a, b) in enumerate(zip(g, w)):
            a = a.detach().cpu()
            if a.shape != b.shape or a.dtype != b.dtype:
                out.append("%s %s[%d]: %s %s against %s %s" % (what, kind, i, a.dtype, tuple(a.shape), b.dtype, tuple(b.shape)))
            elif not torch.equal(a, b):
                out.append("%s %s[%d]: %d entries differ" % (what, kind, i, int((a != b).sum())))
    return out


def failures(fn, names=None, device="cpu"):
    """misses of fn(voxels, thresh, feats, align) -> three lists, against the fixture, over the named cases (default: all)."""
    out = []
    for name in names or cases():
        voxels, thresh, feats, align = inputs(name, device)
        out += misses(fn(voxels, thresh, feats, align), expected(name), name)
    return out
